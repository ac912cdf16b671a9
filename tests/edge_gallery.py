"""The edge gallery of tests/test_gpu_scan_forms.py (its docstring says what every plant is for), shared with
tests/test_gpu_subrange_scans.py. Plain numpy, no GPU."""
import collections
import functools

import numpy as np

import synth

L2 = 0
F32 = np.float32
NQ = 17
R0 = 133

Gal = collections.namedtuple("Gal", "rows q metric n d key")      # key: names the gallery in the cache of oracle values


def mix(a, b, metric):
    return synth.normalise((F32(0.9) * a + F32(0.1) * b)[None, :], metric)[0]


@functools.lru_cache(maxsize=None)
def edge_gallery(metric, n, d=100, nq=NQ, variant="edges"):
    rows = synth.make_gallery(9100 + metric, n, d, metric)
    q, _ = synth.make_queries(9200 + metric, rows, nq, metric)
    for r in (R0 + 64, R0 + 256, R0 + 768, n - 2):
        rows[r] = rows[R0]
    q[0] = rows[R0]
    q[1] = mix(rows[n - 1], rows[7], metric)
    q[2] = mix(rows[0], rows[11], metric)
    rows[620] = rows[300]
    rows[620, 5] = np.nextafter(rows[620, 5], F32(1))
    rows[620, 70] = np.nextafter(rows[620, 70], F32(0))
    q[3] = mix(rows[300], rows[13], metric)
    q[4] = rows[451]
    q[4, 6] = rows[452, 6]
    if metric == L2:
        q[5] = mix(rows[210], rows[17], metric)
        rows[200:232] *= F32(1.0e7)
    if metric == L2 or variant != "edges":
        rows[451, 6] = np.nan
    if metric == L2:
        rows[450] = np.nan
    if variant != "edges":
        rows[500, 17] = F32(1e-41)                      # a denormal: outside the plain range of the division sequence
    if variant == "nan row":
        rows[960] = np.nan                              # chi-square / KL: every term skipped, distance 0 to every query
    rows.setflags(write=False)
    q.setflags(write=False)
    return Gal(rows, q, metric, n, d, ("edge", metric, n, d, nq, variant))
