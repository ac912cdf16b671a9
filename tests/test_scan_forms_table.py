"""tests/scan_forms.py against the source: every row of kScanTable (csrc/fir_capi.hip) is either a case of the table -- the GPU
module tests/test_gpu_scan_forms.py then runs it and asserts its name -- or exempt with a reason, and neither list names a row
that no longer exists. The names are derived from the source itself: the FIR_ROW macros and the table are cut out of fir_capi.hip,
expanded by the host C preprocessor, and each row's adjacent string literals are joined as the compiler joins them."""
import os
import re
import shutil
import subprocess

import scan_forms as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "fast-image-recognition_amd", "csrc", "fir_capi.hip")


def source_rows():
    text = open(SRC).read()
    a = text.index("#define FIR_ROW")
    b = text.index("};", text.index("kScanTable[] = {", a)) + 2
    cc = next(c for c in ("cc", "gcc", "clang") if shutil.which(c))
    out = subprocess.run([cc, "-E", "-P", "-x", "c", "-"], input=text[a:b], capture_output=True, text=True, check=True).stdout
    names = ["".join(re.findall(r'"([^"]*)"', run)) for run in re.findall(r'(?:"[^"]*"\s*)+', out)]
    assert names and all(n.startswith("fir::k_") and n.endswith(">") for n in names), names[:5]
    return names


def test_the_names_are_spelled_as_the_dispatch_record_spells_them():
    rows = source_rows()
    assert len(rows) == len(set(rows)), sorted(r for r in rows if rows.count(r) > 1)
    assert "fir::k_scan<4, 2, 8, 0, 8, 4, 0>" in rows and "fir::k_scan_l2_lds<2, 4, 3, false, 2>" in rows


def test_every_row_is_a_case_or_exempt_and_every_name_is_a_row():
    rows = set(source_rows())
    cases = sf.covered_names()
    exempt = set(sf.EXEMPT)
    assert not (cases & exempt), sorted(cases & exempt)
    assert rows - cases - exempt == set(), "rows of kScanTable no test answers for: %s" % sorted(rows - cases - exempt)
    assert cases - rows == set(), "cases that name no row of kScanTable: %s" % sorted(cases - rows)
    assert exempt - rows == set(), "exemptions that name no row of kScanTable: %s" % sorted(exempt - rows)
    assert all(sf.EXEMPT[n] for n in exempt)
    assert set(sf.OTHER_CLASS_GENERIC_ONE) <= exempt
    assert len(sf.SUBRANGE_ROWS) == 12 == len(set(sf.SUBRANGE_ROWS))
    assert set(sf.SUBRANGE_ROWS) == {r for r in rows if r.startswith("fir::k_scan_subranges<")}, "SUBRANGE_ROWS is not the source's k_scan_subranges rows"
    assert set(sf.SUBRANGE_ROWS) <= exempt and all("tests/test_gpu_subrange_scans.py" in sf.EXEMPT[n] for n in sf.SUBRANGE_ROWS)


def test_the_table_is_well_formed():
    names = [c.name for c in sf.CASES]
    assert len(names) == len(set(names))
    for c in sf.CASES:
        assert c.entry in sf.EPI and c.metric in (sf.L2, sf.CHI2, sf.KL) and c.size in (sf.FEW, sf.MANY) and c.chunks in (sf.ANY, sf.WHOLE, sf.RAGGED)
        assert c.qpp in (1, 2, 4, 8, 16) and c.batch == c.qpp
        assert (c.twin is None) == (c.metric == sf.L2)
        # top-K over 65 536 rows or more takes the candidate lists whatever the tuning: its rows stay on the small galleries
        assert not (c.entry == sf.TOPK and c.size == sf.MANY)
    # 12 + 3 + 3 top-1 rows, 9 top-K rows, 12 + 3 store rows
    assert len(sf.CASES) == 42 and len(sf.covered_names()) == 42 + 26
