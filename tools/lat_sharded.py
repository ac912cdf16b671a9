#!/usr/bin/env python3
"""Median host time of small fir_sharded_search_top1 calls (host pointers) on one device cut into logical shards: the call
where the frame around the exchange -- the growth check, the fan-out over the devices, the status element, the bounded wait,
the verdict -- is all of the cost. usage: python tools/lat_sharded.py [rows] [dim] [queries] [shards]"""
import gc
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

fir = ge.load_package()
n, d, qb, spd = (int(sys.argv[i]) if len(sys.argv) > i else v for i, v in ((1, 4099), (2, 128), (3, 8), (4, 8)))
rng = np.random.default_rng(1)
rows = rng.random((n, d), dtype=np.float32)
q = rng.random((qb, d), dtype=np.float32)
s = fir.ShardedGallery(rows, None, 0, devices=[0], shards_per_device=spd)
for _ in range(200):
    s.search_top1(q)
gc.disable()
ts = []
for _ in range(2000):
    t0 = time.perf_counter()
    s.search_top1(q)
    ts.append(time.perf_counter() - t0)
ts = np.array(ts) * 1e6
print("%d x %d in %d shards, %d queries: median %.1f us  p10 %.1f  p90 %.1f" % (n, d, spd, qb, np.median(ts), np.percentile(ts, 10), np.percentile(ts, 90)))
