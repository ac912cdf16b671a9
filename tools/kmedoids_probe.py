"""Time of fir_cls_kmedoids against the device and ABI part of the per-class path it replaces in
PNNwithClusteringClassifier::train.

    (a) one fir_cls_kmedoids call on a handle over all classes (K = 5, steps = 0, automatic scratch);
    (b) per class: fir_cls_create over the class's rows, fir_cls_distance_sums of the class against itself (the n x n
        table to the host), fir_cls_destroy -- what the per-class path asks of the device and the ABI. Its 100 assign /
        update rounds on the host are NOT included, so (b) is a lower bound of that path.

    shapes: 101 classes x 30 rows x 256 features (the reference's Caltech-101 split), 8 classes x 2 000 rows x 256
    one warm-up of each, then the median (min .. max) of --reps host-clock times around the synchronous calls, the two
    alternating; the kernels' event times of one (a) call (fir_cls_profile_*) and the steps computed per class.

    python tools/kmedoids_probe.py [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

fir = ge.load_package()
K = 5


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return f"{np.median(ts):9.3f} ms ({ts.min():.3f} .. {ts.max():.3f})"


def shape(classes, per_class, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.random((classes, d))
    cls = np.repeat(np.arange(classes), per_class).astype(np.int32)
    rows = rng.random((classes * per_class, d)) + 0.5 * centres[cls]
    rows /= np.sqrt((rows * rows).sum(axis=1))[:, None]
    zero = np.zeros(d)
    one = np.zeros(per_class, np.int32)

    def per_class_path():
        for i in range(classes):
            r = rows[i * per_class:(i + 1) * per_class]
            with fir.ClsModel(r, one, 1, zero, 0) as m:
                m.distance_sums(r)

    with fir.ClsModel(rows, cls, classes, zero, 0) as model:
        new = lambda: model.kmedoids(K)
        _, count, run = new()
        per_class_path()
        ta, tb = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); new(); t1 = time.perf_counter(); per_class_path(); t2 = time.perf_counter()
            ta.append(t1 - t0); tb.append(t2 - t1)
        model.profile_enable(True)
        new()
        ms, _, _ = model.profile_read()
        model.profile_enable(False)
    print(f"--- {classes} classes x {per_class} rows x {d}, K = {K}", flush=True)
    print(f"(a) fir_cls_kmedoids                         {stats(ta)}")
    print(f"(b) per class create + distance_sums + close {stats(tb)}   (b)/(a) {np.median(tb) / np.median(ta):.2f}")
    print("    event times of one (a) call, in launch order (k_kmed_pairs, k_kmed_iterate per group), ms: " + " ".join(f"{v:.3f}" for v in ms))
    print(f"    steps computed per class: min {run.min()} median {int(np.median(run))} max {run.max()}; medoids per class {count.min()} .. {count.max()}", flush=True)


shape(101, 30, 256, 1)
shape(8, 2000, 256, 2)
