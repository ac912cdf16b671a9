"""csrc/fir_search_request.h without a GPU: tests/search_request_main.cpp, a stand-alone program built with the address and
undefined-behaviour sanitizers, prints for every kind of search, qb in {0, 1, 2, 3, 1024} and k in {0 (radius only), 1, 8, 9,
1024} what the request says -- slots per query, key words, count words, the status element's index, the bytes of radii behind the
queries -- and checks the offset view at(q0) itself (every pointer advanced by q0 * k, q0 and q0; NULL stays NULL). Here the printed
numbers are held to the formulas the gallery, matrix-core and shard code spelled out by hand before the request type existed.
Nothing is loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, SELECT, RADIUS, CLASSES = range(4)
QBS = (0, 1, 2, 3, 1024)
KS = (0, 1, 8, 9, 1024)


def test_sizes_and_layouts_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "search_request_main")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]      # (clang links them statically by itself)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    *static, os.path.join(ROOT, "tests", "search_request_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[-2:] == ["ok", ""], out[-3:]
    got = {}
    for line in out[:-2]:
        kind, qb, k, *rest = (int(w) for w in line.split())
        assert (kind, qb, k) not in got
        got[kind, qb, k] = tuple(rest)
    want = {}
    for kind in (ROWS, SELECT, RADIUS, CLASSES):
        for qb in QBS:
            for k in KS:
                if k == 0 and kind != RADIUS:
                    continue
                per = qb * k                                                 # the parent's formulas
                counts = (qb + 1) // 2 if kind == RADIUS else 0
                radii = (qb + (qb & 1)) * 4 if kind == RADIUS else 0
                want[kind, qb, k] = (k, per, counts, per + counts, radii)
    assert len(want) == 4 * 5 * 4 + 5
    assert got == want, sorted(set(got.items()) ^ set(want.items()))[:8]
