"""The K nearest distinct classes of a large batch: the matrix-core form (fir_gemm_search_top_classes_keys_dev) against the exact
class-minimum scan (fir_search_top_classes_keys_dev, the only form before it), same process, same gallery, device pointers.

    gallery: --rows x --dim (1M x 512), rows / 10 identities of 10 images (centre * (1 + 0.3 noise), normalised), K = 5;
             "class-major": the images of an identity are consecutive rows, "permuted": the same rows in random order
    batches: 128, 1 024, 4 096 and 32 768 queries per call (images of random identities drawn the same way)
    per case one warm-up call of each form, then --reps timed calls of each, ALTERNATING (host clock around call + device
    synchronise); the table gives the median queries/s of both forms and their ratio, the queries the matrix-core form left to
    the exact scan (fir_gemm_stats_ex), and -- from one more call through the audit build with FIR_GEMM_DEBUG_COUNTS, which
    synchronises and reports the LAST super-batch of the call -- appended rows per query (mean, max), lists that overflowed and
    the device time of that super-batch's three phases between events: the sample bound (with the query preparation), the fp16
    append pass, the re-rank. --sample-div: FIR_GEMM_CLASS_SAMPLE_DIV for every state (rows sampled = max(16384, n K / div)).

    python tools/class_rank_gemm_bench.py [--reps 3] [--rows 1000000] [--dim 512] [--batches 128,1024,4096,32768] [--sample-div 64]
"""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--batches", default="128,1024,4096,32768")
ap.add_argument("--sample-div", type=int, default=0)
ap.add_argument("--no-audit", action="store_true", help="skip the audit-build call (appended rows, phases)")
args = ap.parse_args()
if args.sample_div:
    os.environ["FIR_GEMM_CLASS_SAMPLE_DIV"] = str(args.sample_div)

fir = ge.load_package()
dev = torch.device("cuda", 0)
K, PER = 5, 10
n, d = args.rows, args.dim
nc = n // PER
batches = [int(b) for b in args.batches.split(",")]


def images(centres, who, gen):
    x = centres[who] * (1 + 0.3 * (torch.rand((who.numel(), d), generator=gen, device=dev) - 0.5))
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


gen = torch.Generator(device=dev).manual_seed(5)
centres = torch.rand((nc, d), generator=gen, device=dev)
labels_major = torch.arange(n, device=dev, dtype=torch.int64) // PER
rows_major = images(centres, labels_major, gen)
queries = images(centres, torch.randint(0, nc, (max(batches),), generator=gen, device=dev), gen)
perm = torch.randperm(n, generator=gen, device=dev)


def stderr_of(fn):
    """what fn() writes to file descriptor 2 (the library prints there)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


print(f"# {n} x {d}, {nc} classes, K = {K}, reps = {args.reps}, sample div = {args.sample_div or 64}; device: {fir.device_info(0)}")
print("# labelling     queries   scan q/s   matrix q/s   ratio  uncertified")
print("#   audit ...: appended rows per query mean, max, lists overflowed | sample bound ms, append pass ms, re-rank ms (the call's last super-batch)")
for name in ("class-major", "permuted"):
    rows = rows_major if name == "class-major" else rows_major[perm].contiguous()
    labels = (labels_major if name == "class-major" else labels_major[perm]).to(torch.int32)
    h_rows, h_labels = rows.cpu().numpy(), labels.cpu().numpy()
    with fir.Gallery(h_rows, h_labels, 0, 0) as g, fir.GemmSearch(g, 2) as m:
        g.set_large_batch_mfma(0)                                   # the baseline is the scan form, whatever the batch
        for qb in batches:
            q = queries[:qb]
            out = [(torch.zeros(qb * K, dtype=torch.int64, device=dev), torch.zeros(qb * K, dtype=torch.int32, device=dev)) for _ in range(2)]
            scan = lambda: g.search_top_classes_keys_dev(q.data_ptr(), qb, nc, K, out[0][0].data_ptr(), out[0][1].data_ptr())
            gemm = lambda: m.search_top_classes_keys_dev(q.data_ptr(), qb, nc, K, out[1][0].data_ptr(), out[1][1].data_ptr())
            timed(scan), timed(gemm)                                  # warm-up (scratch, kernel loading)
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), (name, qb)
            before = m.stats()["fallback_queries"]
            ts, tg = [], []
            for _ in range(args.reps):
                ts.append(timed(scan))
                tg.append(timed(gemm))
            unc = (m.stats()["fallback_queries"] - before) // args.reps
            rs, rg = qb / np.median(ts), qb / np.median(tg)
            print(f"{name:12s} {qb:9d} {rs:10.0f} {rg:12.0f} {rg / rs:7.2f} {unc:12d}   # ms per call: scan {min(ts) * 1e3:.2f}..{max(ts) * 1e3:.2f}, "
                  f"matrix cores {min(tg) * 1e3:.2f}..{max(tg) * 1e3:.2f}", flush=True)
    if args.no_audit:
        continue
    # the audit build's report: its own handles on the same data
    aud = ge.load_package(audit=True)
    os.environ["FIR_GEMM_DEBUG_COUNTS"] = "1"
    with aud.Gallery(h_rows, h_labels, 0, 0) as g, aud.GemmSearch(g, 2) as m:
        for qb in batches:
            q = queries[:qb]
            keys, cls = torch.zeros(qb * K, dtype=torch.int64, device=dev), torch.zeros(qb * K, dtype=torch.int32, device=dev)
            call = lambda: m.search_top_classes_keys_dev(q.data_ptr(), qb, nc, K, keys.data_ptr(), cls.data_ptr())
            call()
            text = stderr_of(call)
            r = re.search(r"last super-batch of (\d+)\): mean ([\d.]+), max (\d+);.*?(\d+) uncertified; (\d+) lists overflowed; preparation ([\d.]+) ms, "
                          r"full passes ([\d.]+) ms, re-rank ([\d.]+) ms", text)
            if r:
                print(f"#   audit {name:12s} {qb:7d} | {float(r.group(2)):13.1f} {int(r.group(3)):6d} {int(r.group(5)):11d} | {float(r.group(6)):8.3f} "
                      f"{float(r.group(7)):8.3f} {float(r.group(8)):11.3f}  ({r.group(1)} queries, {r.group(4)} uncertified)", flush=True)
            else:
                print(f"#   audit {name} {qb}: no report: {text!r}", flush=True)
    del os.environ["FIR_GEMM_DEBUG_COUNTS"]
