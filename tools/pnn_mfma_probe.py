#!/usr/bin/env python3
"""PNN batches on the float64 matrix cores (fir_cls_set_pnn_mfma, csrc/fir_cls_pnn_mfma.h) against the scan, at scale.

    (a) --ubench PATH: the sustained v_mfma_f64_16x16x4_f64 rate and the clock held, from tools/ubench_mfma_f64.hip built to PATH
        (hipcc --offload-arch=gfx950 -O3 -o ubench_mfma_f64 tools/ubench_mfma_f64.hip). It runs as a child process before this one
        touches the device, and its lines are passed through.
    (b) 1 000 000 x 512 float64 training rows in HBM, 101 classes (rows = class centre + 0.004 noise, as bench.py's K3 block draws
        them), --batches queries per call. Per batch size one warm-up call of either form, then --reps times alternately
            "scan"    the exact scan: the routing threshold is put above the batch (fir_cls_set_pnn_mfma(c, 2^30) -- what a fresh
                      handle and the parent commit run; 0 would also free the row norms, and the next routed call would pay for them)
            "routed"  fir_cls_set_pnn_mfma(c, 1)
        on the same handle, host pointers in, scores and classes out. Per form: wall time per call and the device time of the
        bracketed launches (fir_cls_profile_read), median and range over the repeats; for the routed form the share of the
        matrix-core pass, of k_cls_pnn (exp and class sums) and of the band kernel in the device time and in the call, the queries the
        scan answered after all, and the largest relative score difference against the scan.

        --rows 500000 --d 1024 measures the 16-queries-per-read kernel (640 < d <= 1280) at the same 4.1 GB.

    python tools/pnn_mfma_probe.py [--ubench ./ubench_mfma_f64] [--batches 64,512,4096] [--reps 5] [--rows 1000000] [--d 512]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--ubench", default="")
ap.add_argument("--batches", default="64,512,4096")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=512)
ap.add_argument("--classes", type=int, default=101)
args = ap.parse_args()

if args.ubench:
    print("# (a) " + args.ubench, flush=True)
    subprocess.run([args.ubench], check=True)
    sys.stdout.flush()

import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

fir = ge.load_package()
dev = torch.device("cuda", 0)
n, d, ncls = args.rows, args.d, args.classes
batches = [int(b) for b in args.batches.split(",")]
g = torch.Generator(device=dev)
g.manual_seed(31337)
centres = torch.rand((ncls, d), generator=g, device=dev, dtype=torch.float64)
tcls = (torch.arange(n, device=dev) * ncls // n).to(torch.int64)
tr = torch.empty((n, d), device=dev, dtype=torch.float64)
step = 125_000
for lo in range(0, n, step):
    hi = min(n, lo + step)
    tr[lo:hi] = centres[tcls[lo:hi]] + 0.004 * torch.randn((hi - lo, d), generator=g, device=dev, dtype=torch.float64)
avg = tr.mean(dim=0).cpu().numpy()
pick = torch.randint(0, ncls, (max(batches),), generator=g, device=dev)
queries = (centres[pick] + 0.004 * torch.randn((max(batches), d), generator=g, device=dev, dtype=torch.float64)).cpu().numpy()
torch.cuda.synchronize()
m = fir.ClsModel(None, tcls.to(torch.int32).cpu().numpy(), ncls, avg, 0, dev_ptr=tr.data_ptr(), nt=n, d=d)
del tr
torch.cuda.empty_cache()
m.profile_enable(True)


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):9.3f} ({v.min():.3f}..{v.max():.3f})"


print(f"# (b) {n} x {d} float64 ({n * d * 8 / 1e9:.1f} GB), {ncls} classes, reps {args.reps}; ms: median (min..max)", flush=True)
for qb in batches:
    q = queries[:qb]
    m.set_pnn_mfma(1 << 30)
    scan_cls, scan_sc = m.pnn_predict(q)
    m.set_pnn_mfma(1)
    mm_cls, mm_sc = m.pnn_predict(q)
    m.profile_read()
    wall = {"scan": [], "routed": []}
    devt = {"scan": [], "routed": []}
    parts = {"mfma": [], "pnn": [], "band": []}
    s0 = m.pnn_stats()
    kernels = {}
    for _ in range(args.reps):
        for form, mode in (("scan", 1 << 30), ("routed", 1)):
            m.set_pnn_mfma(mode)
            t0 = time.perf_counter()
            m.pnn_predict(q)
            wall[form].append((time.perf_counter() - t0) * 1e3)
            ms, _, kname = m.profile_read()
            kernels[form] = kname if len(ms) else "no bracketed launch: this d runs the scan outside its LDS-tile kernels"
            devt[form].append(float(ms.sum()))
            if form == "routed":                      # three pairs per internal batch: the pass, k_cls_pnn, the band kernel
                assert len(ms) % 3 == 0, len(ms)
                for i, key in enumerate(("mfma", "pnn", "band")):
                    parts[key].append(float(ms[i::3].sum()))
    s1 = m.pnn_stats()
    rel = float(np.max(np.abs(mm_sc - scan_sc) / np.maximum(np.abs(scan_sc), 1e-300)))
    print(f"queries {qb}: classes equal {bool(np.array_equal(mm_cls, scan_cls))}, planted class found {float(np.mean(mm_cls == pick[:qb].cpu().numpy())):.3f}, "
          f"largest relative score difference to the scan {rel:.3e}, answered by the scan after all "
          f"{(s1['exact_scan_queries_of_them'] - s0['exact_scan_queries_of_them']) // args.reps} of {qb}")
    print(f"  scan    wall ms/call {spread(wall['scan'])}   scan kernels ms {spread(devt['scan'])}   [{kernels['scan']}]")
    print(f"  routed  wall ms/call {spread(wall['routed'])}   bracketed kernels ms {spread(devt['routed'])}   [{kernels['routed']}]")
    print(f"          matrix-core pass ms {spread(parts['mfma'])}   k_cls_pnn ms {spread(parts['pnn'])}   k_cls_pnn_band ms {spread(parts['band'])}")
    wm, dm = np.median(wall["routed"]), np.median(devt["routed"])
    print(f"          share of the bracketed device time: pass {np.median(parts['mfma']) / dm:.3f}, k_cls_pnn {np.median(parts['pnn']) / dm:.3f}, band {np.median(parts['band']) / dm:.4f};"
          f" of the call: pass {np.median(parts['mfma']) / wm:.3f}, k_cls_pnn {np.median(parts['pnn']) / wm:.3f}, band {np.median(parts['band']) / wm:.4f}")
    tf = 2.0 * n * d * qb / (np.median(parts["mfma"]) * 1e-3) / 1e12
    print(f"          pass: {tf:.2f} TFLOP/s of dot products; queries/s scan {qb / np.median(wall['scan']) * 1e3:.0f}, routed {qb / wm * 1e3:.0f}; "
          f"wall ratio scan/routed {np.median(wall['scan']) / wm:.2f}", flush=True)
m.close()
