"""The exact-scan kernels by name: one case per top-1 / top-K / store row of kScanTable (csrc/fir_capi.hip) and how a public call
reaches it, plus the rows other test modules own. Plain Python, no GPU: tests/test_scan_forms_table.py checks both lists against the
source, tests/test_gpu_scan_forms.py runs every case and asserts the name in the dispatch record.

How a case is reached (top1_dev, topk_dev, range_dev, select_scan):
  * a pinned queries_per_pass keeps the call on the scan (no matrix cores, no chi-square / KL candidate lists) and is the largest
    query tile; a batch is cut into whole tiles of the largest power of two that fits, so a batch of exactly `batch` queries ends
    -- and a top-K or store call consists of -- launches of the `batch`-query tile: the dispatch record then names it;
  * one-query tiles take the few-tiles form (query staged in LDS, 16 chunks per load group) while the gallery has at most
    4 * CUs tiles; the generic one-query rows need more than that (size "many"); top-K has no few-tiles form;
  * whole-chunk L2 top-1 ranges (start and end multiples of 4) with 8 or 16 queries take the hand-scheduled kernels, so the generic
    8-query L2 top-1 row is reached only by a ragged range; 16 queries per pass exist only there and only while the tile fits
    64 KiB of LDS; rows beyond 144 KiB of tile (d > 4604) take the scalar-operand kernel;
  * chi-square / KL rows are launched with their plain-range twin (metric + 2) on the same grid: which of the two does the pass is
    decided on the device, the record names the full-sequence row.
The table states size classes, never row counts: the GPU test derives "many" from the device's CU count."""
from collections import namedtuple

L2, CHI2, KL = 0, 1, 2
TOP1, TOPK, STORE = "search_top1", "search_topk", "range_distances"
EPI = {TOP1: 0, TOPK: 1, STORE: 2}
FEW, MANY = "few tiles", "more than 4 * cus tiles"
ANY, WHOLE, RAGGED = "any range", "whole chunks", "ragged ranges"

# name: the dispatch record's kernel; twin: the plain-range row launched next to it (chi-square / KL) or None; qpp: the pinned
# queries_per_pass; batch: the whole-tile batch size; size: the gallery's size class; chunks: the feature ranges that reach it; d: row length
Case = namedtuple("Case", "name twin entry metric qpp batch size chunks d")


def k_scan(qb, metric, epi, ldsq=0):
    return "fir::k_scan<%d, %d, %d, %d, 8, %d, %d>" % (qb, metric, 16 if ldsq else 8, epi, 4 if metric < 3 else 3, ldsq)


def _case(entry, metric, qb, size, ldsq=0, chunks=ANY):
    twin = k_scan(qb, metric + 2, EPI[entry], ldsq) if metric != L2 else None
    return Case(k_scan(qb, metric, EPI[entry], ldsq), twin, entry, metric, qb, qb, size, chunks, 100)


L2_LDS_8 = "fir::k_scan_l2_lds<1, 8, 4, false>"
L2_LDS_16 = "fir::k_scan_l2_lds<2, 4, 3, false, 2>"
L2_FAST_8 = "fir::k_scan_l2_fast<1, 8, 4>"


def _cases():
    out = []
    for m in (L2, CHI2, KL):
        # top-1: the generic tiles, the few-tiles form
        out.append(_case(TOP1, m, 1, MANY))
        out.append(_case(TOP1, m, 2, FEW))
        out.append(_case(TOP1, m, 4, FEW))
        out.append(_case(TOP1, m, 8, FEW, chunks=RAGGED if m == L2 else ANY))
        out.append(_case(TOP1, m, 1, FEW, ldsq=1))
        # top-K: 2 * KMAX registers per query, 4 queries at most; no few-tiles form
        for qb in (1, 2, 4):
            out.append(_case(TOPK, m, qb, FEW))
        # store
        out.append(_case(STORE, m, 1, MANY))
        for qb in (2, 4, 8):
            out.append(_case(STORE, m, qb, FEW))
        out.append(_case(STORE, m, 1, FEW, ldsq=1))
    # the hand-scheduled L2 top-1 kernels
    out.append(Case(L2_LDS_8, None, TOP1, L2, 8, 8, FEW, WHOLE, 100))
    out.append(Case(L2_LDS_16, None, TOP1, L2, 16, 16, FEW, WHOLE, 100))
    out.append(Case(L2_FAST_8, None, TOP1, L2, 8, 8, FEW, WHOLE, 4800))
    return out


CASES = _cases()

# the generic one-query other-class rows: asserted by tests/test_gpu_other_class.py over more than 4 * cus tiles
OTHER_CLASS_GENERIC_ONE = [k_scan(1, m, 6) for m in (L2, CHI2, KL)]


def k_scan_subranges(qbt, metric):
    return "fir::k_scan_subranges<%d, %d, 8, 4>" % (qbt, metric)


# the sub-range scans behind the staged three-way-decision drivers: asserted by name and slot by slot by tests/test_gpu_subrange_scans.py
SUBRANGE_ROWS = [k_scan_subranges(qbt, m) for qbt in (1, 2, 4, 8) for m in (L2, CHI2, KL)]


def _exempt():
    ex = {}
    nom = "append / nomination scans: tests/test_gpu_nomination_scans.py"
    ex["fir::k_scan_l2_lds<1, 8, 4, true>"] = nom
    for m in (6, 7):
        ex["fir::k_scan<8, %d, 8, 0, 8, 3>" % m] = nom
        ex["fir::k_nominate<%d, 2, 8, 3>" % m] = nom
    for m in range(6):
        ex["fir::k_scan<8, %d, 8, 3, 8, %d>" % (m, 4 if m < 3 else 3)] = nom
    for name in SUBRANGE_ROWS:
        ex[name] = "k_scan_subranges, read through the library's internal entries: tests/test_gpu_subrange_scans.py"
    for m in range(5):
        wps = 4 if m < 3 else 3
        ex[k_scan(8, m, 5)] = "class minimum: tests/test_gpu_class_rank.py, tests/test_gpu_gallery_handle.py"
        ex[k_scan(1, m, 6, ldsq=1)] = "other-class few-tiles form: tests/test_gpu_other_class.py"
        for qb in (1, 2, 4, 8):
            ex[k_scan(qb, m, 6)] = "other-class %s: tests/test_gpu_other_class.py" % ("generic one-query rows" if qb == 1 else "multi-query tiles")
            for epi in (0, 2):
                ex["fir::k_scan<%d, %d, 8, %d, 8, %d, 0, 1>" % (qb, m, epi, wps)] = "masked: tests/test_gpu_masked_search.py"
        ex["fir::k_scan<8, %d, 8, 5, 8, %d, 0, 1>" % (m, wps)] = "masked: tests/test_gpu_masked_search.py"
    return ex


EXEMPT = _exempt()


def covered_names():
    """Every kScanTable row this table answers for: the named rows and their plain-range twins."""
    return {c.name for c in CASES} | {c.twin for c in CASES if c.twin}
