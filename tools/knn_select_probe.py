"""fir_search_knn_keys_dev on one GPU, 1M x 512 and 100 000 x 512, L2, qb in {8, 256}, k in {8, 16, 64, 256, 1024}: the whole call by
HIP events on the caller's stream; its store pass and its select each by the library's own event pairs (fir_profile_enable: one pair
around every tile's store pass, one around its select, summed over the call's tiles, in runs of their own); FIR_KNN_SELECT_BLOCKS=1
times the one-workgroup-per-query select the same way. Yardsticks: fir_range_distances_dev alone and the top-K scan at k = 8.
profiles/knn_select.txt is this script's output."""
import os
import sys
import statistics

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

fir = ge.load_package()
DEV = torch.device("cuda", 0)
OUT = sys.argv[1] if len(sys.argv) > 1 else None      # the table is printed; a path as first argument gets a copy
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


def unit(n, d, seed):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    x = torch.rand((n, d), generator=gen, device=DEV)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def timed(fn, stream, inner, windows=5, warm=2):
    """median / min ms per call over `windows` event windows of `inner` back-to-back calls"""
    for _ in range(warm):
        fn()
    stream.synchronize()
    res = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(inner):
            fn()
        e1.record(stream)
        e1.synchronize()
        res.append(e0.elapsed_time(e1) / inner)
    return statistics.median(res), min(res)


def split(g, call, st, reps):
    """(store ms, select ms) per call from the library's event pairs: median over `reps` profiled calls"""
    g.profile_enable(True)
    call()
    st.synchronize()
    g.profile_read()
    store, select = [], []
    for _ in range(reps):
        call()
        st.synchronize()
        ms, _ = g.profile_read()
        assert ms.shape[0] % 2 == 0 and ms.shape[0] > 0
        store.append(float(ms[0::2].sum()))
        select.append(float(ms[1::2].sum()))
    g.profile_enable(False)
    return statistics.median(store), statistics.median(select)


def main():
    d = 512
    st = torch.cuda.Stream(device=DEV)
    sp = st.cuda_stream
    say("fir_search_knn_keys_dev on " + str(fir.device_info(0)))
    say("L2, d = 512, unit rows; ms per call = median of 5 event windows (min in brackets); large-batch matrix cores off")
    say("store / select (events): the library's event pairs around every tile's store pass and select, summed per call, median of 5 calls")
    for n in (1_000_000, 100_000):
        rows = unit(n, d, 1)
        g = fir.Gallery(dev_ptr=rows.data_ptr(), n=n, d=d, metric=fir.METRIC_L2)
        g.set_large_batch_mfma(0)
        del rows
        for qb in (8, 256):
            inner = 8 if qb == 8 else 2
            q = unit(qb, d, 2 + qb)
            dist = torch.empty(qb * n, dtype=torch.float32, device=DEV)
            keys = torch.empty(qb * 1024, dtype=torch.int64, device=DEV)
            keys2 = torch.empty(qb * 1024, dtype=torch.int64, device=DEV)
            torch.cuda.synchronize()
            say()
            say(f"n = {n}, qb = {qb}")
            t_store = timed(lambda: g.range_distances_dev(q.data_ptr(), qb, dist.data_ptr(), stream=sp), st, inner)
            say(f"  store pass alone (fir_range_distances_dev)          {t_store[0]:9.3f} ms  [{t_store[1]:.3f}]")
            t_top = timed(lambda: g.search_topk_keys_dev(q.data_ptr(), qb, 8, keys2.data_ptr(), stream=sp), st, inner)
            say(f"  fir_search_topk_keys_dev k=8, default dispatch     {t_top[0]:9.3f} ms  [{t_top[1]:.3f}]")

            def reglist():
                for q0 in range(0, qb, 4):
                    g.search_topk_keys_dev(q.data_ptr() + q0 * d * 4, 4, 8, keys2.data_ptr() + q0 * 8 * 8, stream=sp)

            t_reg = timed(reglist, st, inner)
            say(f"  register-list top-K scan k=8 (calls of 4 queries)  {t_reg[0]:9.3f} ms  [{t_reg[1]:.3f}]")
            say("     k   knn call    store (events)  select (events)  select share   call / register-list   one-workgroup select (events)")
            for k in (8, 16, 64, 256, 1024):
                os.environ.pop("FIR_KNN_SELECT_BLOCKS", None)
                t = timed(lambda: g.search_knn_keys_dev(q.data_ptr(), qb, k, keys.data_ptr(), stream=sp), st, inner)
                call = lambda: g.search_knn_keys_dev(q.data_ptr(), qb, k, keys.data_ptr(), stream=sp)  # noqa: E731
                sto, sel = split(g, call, st, 5)
                one = ""
                if qb == 8:
                    os.environ["FIR_KNN_SELECT_BLOCKS"] = "1"
                    one = f"{split(g, call, st, 3)[1]:9.3f} ms"
                    os.environ.pop("FIR_KNN_SELECT_BLOCKS", None)
                say(f"  {k:4d}  {t[0]:9.3f} ms  {sto:9.3f} ms    {sel:9.3f} ms     {100 * sel / (sto + sel):6.1f} %        {t[0] / t_reg[0]:6.2f} x              {one}")
                if k == 8:      # same keys as the scan, at the size timed
                    g.search_knn_keys_dev(q.data_ptr(), qb, 8, keys.data_ptr(), stream=sp)
                    g.search_topk_keys_dev(q.data_ptr(), qb, 8, keys2.data_ptr(), stream=sp)
                    st.synchronize()
                    same = torch.equal(keys[: qb * 8], keys2[: qb * 8])
                    say(f"        keys of the k = 8 call equal fir_search_topk_keys_dev's: {same}")
            del dist, keys, keys2
        g.close()
        torch.cuda.empty_cache()


main()
