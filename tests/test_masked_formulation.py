"""The masked searches without a GPU: masked_ref, the numpy restatement the device tests grade against, pinned to the oracle the way
the contract states it -- "the answer of a handle freshly created over the selected rows in their order, every returned row mapped
back to its index in the full gallery": the oracle's first-minimum search, its top-K and a per-class first minimum run over the
COMPACTED rows, their indices mapped through np.flatnonzero(mask), must give masked_ref's keys over the full distance matrix. Then
the mask layout: pack_row_mask against an explicit bit loop, FIR_MASK_WORDS read from the header."""
import os
import re

import numpy as np
import pytest

import knn_select_ref as ks
import masked_ref as ref
import synth

F32 = np.float32
I32 = np.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def masks_of(n, seed):
    r = synth.splitmix64(np.arange(n, dtype=np.uint64), seed)
    yield "half", (r & np.uint64(1)).astype(bool)
    yield "alternating", (np.arange(n) % 2 == 0)
    yield "all", np.ones(n, bool)
    yield "none", np.zeros(n, bool)
    one = np.zeros(n, bool)
    one[n - 1] = True
    yield "last row", one
    gaps = np.ones(n, bool)
    gaps[64:128] = False                       # a whole word of zeros between two others
    gaps[192:] = False                         # ... and the last, part-full word
    yield "zero words", gaps


@pytest.mark.parametrize("metric", (0, 1, 2))
@pytest.mark.parametrize("seed", (13, 17))
def test_masked_ref_is_the_oracle_over_the_compacted_rows(oracle, seed, metric):
    n, d, nq, classes = 257, 64, 5, 9
    rows = synth.make_gallery(seed, n, d, metric)
    rows[200] = rows[3]                        # ties across the mask's edge
    rows[77] = rows[3]
    labels = (synth.splitmix64(np.arange(n, dtype=np.uint64), seed + 1) % np.uint64(classes)).astype(I32)
    q, _ = synth.make_queries(seed + 2, rows, nq, metric)
    q[0] = rows[3]
    for start, end in ((0, d), (3, 61)):
        dist = np.stack([oracle.all_distances(rows, qq, start, end, metric) for qq in q])
        for name, take in masks_of(n, seed + 3):
            sel = np.flatnonzero(take)
            sub, sub_labels = np.ascontiguousarray(rows[sel]), labels[sel]
            want1 = ref.top1_keys(dist, take)
            want8 = ref.knn_keys(dist, take, 8)
            wantc, wantcc = ref.class_keys(dist, take, labels, classes, 5)
            for i in range(nq):
                tag = (seed, metric, start, end, name, i)
                if sel.shape[0] == 0:
                    assert want1[i] == ref.KEY_NONE and (want8[i] == ref.KEY_NONE).all() and (wantcc[i] == -1).all(), tag
                    continue
                # first minimum (db_features.cpp:329-332) over the compacted rows
                bi, bd = oracle.recognize_bf(sub, q[i], start, end, metric)
                got1 = ks.all_keys(np.array([bd], F32), 0)[0] & np.uint64(0xFFFFFFFF00000000) | np.uint64(bi) if bi >= 0 else ref.KEY_NONE
                assert ref.map_back(np.array([got1], np.uint64), sel)[0] == want1[i], tag
                # top-K over the compacted rows
                kk = min(8, sel.shape[0])
                ti, td = oracle.topk(sub, q[i], start, end, kk, metric)
                gotk = (ks.orderable(td).astype(np.uint64) << np.uint64(32)) | ti.astype(np.uint64)
                assert np.array_equal(ref.map_back(gotk, sel), want8[i, :kk]), tag
                assert (want8[i, kk:] == ref.KEY_NONE).all(), tag
                # class ranking: per class the first minimum of the compacted rows' oracle distances, then ascending
                dsub = oracle.all_distances(sub, q[i], start, end, metric)
                assert np.array_equal(dsub.view(np.uint32), dist[i, sel].view(np.uint32)), tag
                best = {}
                for j, v in enumerate(dsub):
                    c = int(sub_labels[j])
                    if v < F32(100000.0) and (c not in best or v < best[c][0]):
                        best[c] = (v, j)
                top = sorted((v, j, c) for c, (v, j) in best.items())[:5]
                gotc = np.array([(int(ks.orderable(F32(v))) << 32) | j for v, j, _ in top], np.uint64)
                assert np.array_equal(ref.map_back(gotc, sel), wantc[i, :len(top)]), tag
                assert [c for _, _, c in top] == wantcc[i, :len(top)].tolist() and (wantcc[i, len(top):] == -1).all(), tag


def test_hand_made_rows_nan_cutoff_offset_and_counts():
    row = np.array([3.0, 1.0, 1.0, np.nan, 100000.0, 0.5, -0.0, 0.0, 2.0e5], F32)
    take = np.array([1, 1, 1, 1, 1, 0, 0, 1, 1], bool)
    for off in (0, 1 << 20):
        assert ks.unpack(ref.top1_keys(row, take, off))[0][0] == 7 + off         # rows 5 and 6 are masked out
        assert ks.unpack(ref.knn_keys(row, take, 6, off))[0][0].tolist() == [7 + off, 1 + off, 2 + off, 0 + off, -1, -1]
    # NaN, the cut-off and anything above never qualify, inside the mask or not
    only = np.zeros(9, bool)
    only[[3, 4, 8]] = True
    assert ref.top1_keys(row, only)[0] == ref.KEY_NONE
    cnt, keys = ref.radius_keys(row, take, [2.0], 2)
    assert cnt.tolist() == [3] and ks.unpack(keys)[0][0].tolist() == [7, 1]       # the count is not capped
    cnt, keys = ref.radius_keys(row, take, [np.inf], 0)
    assert cnt.tolist() == [4] and keys.shape == (1, 0)
    assert ref.radius_keys(row, np.zeros(9, bool), [np.inf], 3)[0].tolist() == [0]
    # a class whose only rows are masked out does not appear; labels outside [0, num_classes) take no part
    labels = np.array([0, 1, 1, 2, 2, 3, 3, 7, -1], I32)
    kc, cc = ref.class_keys(row, take, labels, 4, 4)
    assert cc[0].tolist() == [1, 0, -1, -1] and ks.unpack(kc)[0][0].tolist() == [1, 0, -1, -1]
    # the all-ones mask is the unmasked restatement
    assert np.array_equal(ref.knn_keys(row, np.ones(9, bool), 9)[0], ks.expected_keys(row, 9))
    # an empty gallery
    assert ref.top1_keys(np.zeros((2, 0), F32), np.zeros(0, bool)).tolist() == [ref.KEY_NONE] * 2


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_pack_row_mask_against_the_bit_loop(fir, n):
    for seed in (1, 2):
        take = (synth.splitmix64(np.arange(n, dtype=np.uint64), seed + n) & np.uint64(1)).astype(bool)
        for t in (take, np.ones(n, bool), np.zeros(n, bool)):
            got = fir.pack_row_mask(t)
            assert got.dtype == np.uint64 and got.shape == (ref.mask_words(n),) and got.flags["C_CONTIGUOUS"]
            assert np.array_equal(got, ref.pack_bits(t)), (n, seed)
            assert np.array_equal(ref.unpack_bits(got, n), t)
    full = fir.pack_row_mask(np.ones(n, bool))
    if n % 64:
        assert int(full[-1]) == (1 << (n % 64)) - 1                             # the bits past n are zero
    assert fir.mask_words(n) == ref.mask_words(n)
    assert fir.pack_row_mask(np.zeros(0, bool)).shape == (0,)


def test_mask_words_macro_and_declarations():
    header = open(os.path.join(ROOT, "include", "fir_amd.h")).read()
    m = re.search(r"#define\s+FIR_MASK_WORDS\(n\)\s+(.+)", header)
    assert m, "FIR_MASK_WORDS is not defined"
    body = m.group(1).strip()
    assert re.fullmatch(r"[\(\)n\s\d\+/]+", body), body                           # integer arithmetic on n only: safe to evaluate
    for n in (0, 1, 63, 64, 65, 128, 129, (1 << 31) - 1):
        assert eval(body.replace("/", "//"), {"n": n}) == (n + 63) // 64 == ref.mask_words(n), n


def test_bound_and_declared_symbols(fir):
    sigs = {name: args for name, _, args in fir.capi.SYMBOLS}
    names = (("fir_search_top1_masked", 8), ("fir_search_top1_masked_keys_dev", 8), ("fir_search_knn_masked", 9), ("fir_search_knn_masked_keys_dev", 9),
             ("fir_search_radius_masked", 11), ("fir_search_radius_masked_keys_dev", 11), ("fir_search_top_classes_masked", 11),
             ("fir_search_top_classes_masked_keys_dev", 11), ("fir_gallery_mask_of_classes", 5), ("fir_gallery_mask_of_classes_dev", 6))
    header = open(os.path.join(ROOT, "include", "fir_amd.h")).read()
    for name, nargs in names:
        assert name in sigs and len(sigs[name]) == nargs, name
        assert hasattr(fir.lib(), name)
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, name
        if name.startswith("fir_search"):                                         # the mask directly after end_pos
            assert re.search(r"int32_t\s+end_pos\s*,\s*const\s+uint64_t\s*\*\s*(d_)?mask\s*,", decl.group(1)), name
    for meth in ("search_top1_masked", "search_top1_masked_keys_dev", "search_knn_masked", "search_knn_masked_keys_dev", "search_radius_masked",
                 "search_radius_masked_keys_dev", "search_top_classes_masked", "search_top_classes_masked_keys_dev", "mask_of_classes",
                 "mask_of_classes_dev"):
        assert callable(getattr(fir.Gallery, meth)), meth
