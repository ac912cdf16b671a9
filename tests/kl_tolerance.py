"""The one tolerance the scan tests grant: KL, whose device logf is not glibc's. Shared by test_gpu_fuzz.py and
test_gpu_scan_forms.py so that neither can drift from the other. L2 and chi-square have none: they are compared bit for bit."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def kl_bound(qv, rows, start, end):
    """How far two faithful evaluations of the KL arm (db_features.cpp:33-36) may differ when their logf differ by a
    few ulp: the terms l*log(2l/s) and r*log(2r/s) have opposite signs and nearly cancel for similar vectors, so the
    bound scales with the sum of their MAGNITUDES, not with the distance itself. Per row."""
    l = qv[start:end].astype(np.float64)[None, :]
    r = np.atleast_2d(rows)[:, start:end].astype(np.float64)
    s = l + r
    with np.errstate(divide="ignore", invalid="ignore"):
        tl = np.where((s > 0) & (l > 0), np.abs(l * np.log(2 * l / s)), 0.0)
        tr = np.where((s > 0) & (r > 0), np.abs(r * np.log(2 * r / s)), 0.0)
    return 4 * 6e-8 * (tl + tr).sum(axis=1) / (end - start)
