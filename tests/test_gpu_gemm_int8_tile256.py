"""The 256-query tile of the int8 nomination pass -- k_gemm_proxy_f16x<3, 0, 0, 0, 8, I8 = 1, QH = 2>, reported as
"k_gemm_proxy_i8x<3, 0> (256-query tile)": a workgroup holds two pairs' queries in LDS and walks every row block's two 256-feature
units once per tile half, into the same accumulators. A launch of two pairs or more over 257..512 features takes it; a one-pair
launch (the odd pair of a call) and the second-chance rounds keep the 128-query kernels.

Every case asserts the exact scan's keys bit for bit, which form the dispatch names, and that neither counter (second pass, exact
device scan) moved. What is new in the kernel is where a row block's sums are looked at -- half 0's between the halves, half 1's in
the next block's first step, the last block's behind the loop, a straddling block's row by row in both places, a wave's first block
on a walk of its own -- so winners are planted in each of those places for queries of both halves, and the lists themselves are held
to tests/test_gpu_gemm_int8_nominations.py's float64 assertions through the new form and, switched off, through the old one."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_f16_form as form
import gemm_nomination_cases as cases
from test_gemm_int8_formulation import I8Form, descending_fixture
from test_gpu_gemm_int8_nominations import _report, _set_int8, check_i8_lists
from test_gpu_gemm_nominations import _dev, _exact, nominations

pytestmark = pytest.mark.gpu

TILE = "k_gemm_proxy_i8x<3, 0> (256-query tile)"
OLD = "k_gemm_proxy_i8x<3, 0>"
N_WALK, QB_WALK = cases.N_MULTI, cases.QB_MULTI          # 20 037 rows x 2 048 queries: eight tiles share 32 row ranges


def _set_tile(fir, m, mode):
    fn = C.CDLL(fir.lib_path()).fir_gemm_set_int8_tile_
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_int32]
    fn(m._h, mode)


def run(fir, rows, q, tile=None, lists=False):
    """one int8 top-1 call of a matrix-core state on device rows; -> keys, the exact scan's keys, dispatch, counters, (lists)"""
    n, d = rows.shape
    qb = q.shape[0]
    rows_t, q_t = _dev(rows), _dev(q)
    keys = torch.empty(qb, dtype=torch.int64, device=q_t.device)
    with fir.Gallery(dev_ptr=rows_t.data_ptr(), n=n, d=d, metric=0, device=0) as g:
        with fir.GemmSearch(g, 2) as m:
            _set_int8(fir, m, 1)
            if tile is not None:
                _set_tile(fir, m, tile)
            m.search_top1_keys_dev(q_t.data_ptr(), qb, keys.data_ptr())
            torch.cuda.synchronize()
            disp = g.last_dispatch()
            st = m.stats()
            ex = nominations(fir, m, 0) if lists else None
        want = _exact(g, dict(entry="top", k=1, end=0), q_t, qb)
    return keys, want, disp, st, ex


def assert_answered(keys, want, disp, st, name):
    if name == TILE:
        assert TILE in disp["kernel"], disp
    else:
        assert OLD in disp["kernel"] and "256-query" not in disp["kernel"], disp
    assert torch.equal(keys, want)
    assert st["second_pass_queries"] == 0 and st["fallback_queries"] == 0, st


def winners_of(fir, keys):
    return fir.keys_unpack(keys.cpu().numpy().view(np.uint64))[0]


@pytest.mark.parametrize("d", [512, 300, 257])
def test_walk(fir, d):
    """Eight tiles, every wave takes several row blocks from the hand-out; 300 and 257 features: padding inside the second unit.
    random_data's plants: query 5 is row 11, which the last row copies (the lower row wins), query 6 the row before the last."""
    rows, q = cases.random_data(N_WALK, d, QB_WALK)
    keys, want, disp, st, _ = run(fir, rows, q)
    assert_answered(keys, want, disp, st, TILE)
    idx = winners_of(fir, keys)
    assert idx[5] == 11 and idx[6] == N_WALK - 2
    assert disp["queries_per_pass"] == 2048 and disp["grid"][1] == 1, disp


def test_planted_winners_in_every_place_a_block_is_checked(fir):
    """Queries of both tile halves (index < 128 and >= 128 inside the 256-query tile), each an exact copy of a row that lies in: a
    wave's first row block (walked twice: observed, then checked -- for several waves of one range, whatever the grid), a block in
    the middle of a walk, the last full row block (625: only the code behind the loop checks half 1's sums of a wave's last block),
    the straddling block (626: five rows)."""
    rows, q = cases.random_data(N_WALK, 512, QB_WALK)
    rows, q = rows.copy(), q.copy()
    places = [0, 3 * 32 + 9, 96 * 32 + 3, 99 * 32 + 20, 101 * 32 + 31, 313 * 32 + 17, 625 * 32 + 10, 625 * 32 + 31, 626 * 32 + 1, 626 * 32 + 3]
    slots = []
    for i, r in enumerate(places):
        for tile, inside in ((0, 40 + i), (0, 128 + 7 + i), (3, 250 - i), (7, 100 - i), (7, 128 + 16 * (i % 8) + i)):
            slots.append((tile * 256 + inside, r))
    assert len({s for s, _ in slots}) == len(slots)
    for s, r in slots:
        q[s] = rows[r]
    keys, want, disp, st, _ = run(fir, rows, q)
    assert_answered(keys, want, disp, st, TILE)
    idx = winners_of(fir, keys)
    for s, r in slots:
        assert idx[s] == r, (s, r, int(idx[s]))
    assert idx[5] == 11 and idx[6] == N_WALK - 2


@pytest.mark.parametrize("n,qb,launches", [(N_WALK, 256, 1), (N_WALK, 300, 2), (32 * 7 + 5, 256, 1), (20, 256, 1), (8192 * 3 + 37, 384, 2)])
def test_ragged_ends(fir, n, qb, launches):
    """256 queries: one tile. 300: a two-pair launch in the new form and a one-pair launch in the old one, in one call (384: the
    third pair is full). 229 rows: a short last block, waves past the end. 20 rows: not one full block, T stays +inf."""
    rows, q = cases.random_data(n, 512, qb)
    keys, want, disp, st, _ = run(fir, rows, q)
    assert_answered(keys, want, disp, st, TILE)
    assert disp["grid"][1] == launches and disp["queries_per_pass"] == 256, disp      # (grid[1]: full-pass launches of the super-batch)
    idx = winners_of(fir, keys)
    assert idx[5] == 11 and idx[6] == n - 2


@pytest.mark.parametrize("tile,name", [(1, TILE), (0, OLD)], ids=["tile256", "tile128"])
@pytest.mark.parametrize("data", ["top1-d512", "near-duplicates"])
def test_lists_and_bounds(fir, data, tile, name):
    """check_i8_lists (soundness, completeness, every row inside one window of the smallest proxy listed, tau from both sides) through
    the new form, and through the old one at sixteen pairs per launch, which still answers odd pairs and second rounds."""
    rows, q = cases.near_duplicate_data() if data == "near-duplicates" else cases.random_data(N_WALK, 512, QB_WALK)
    keys, want, disp, st, ex = run(fir, rows, q, tile=tile, lists=True)
    assert_answered(keys, want, disp, st, name)
    assert len(ex["counts"]) == q.shape[0]
    figs = check_i8_lists(I8Form(rows), q, ex, adaptive=True, label=f"{data} {name}")
    _report(f"{data} tile={tile}", disp["kernel"], figs, st)


def test_every_list_overflows_through_the_eight_slot_stage(fir_audit, monkeypatch):
    """descending_fixture with FIR_GEMM_ADAPT_DBG=3 (audit build: every workgroup keeps its own bound): each workgroup of the one tile
    appends its whole range -- eight staged slots per query, everything else directly -- every list overflows, and the int8
    second-chance rounds answer every query (nothing is left to the exact device scan)."""
    rows, q = descending_fixture()
    n, qb = rows.shape[0], q.shape[0]
    monkeypatch.setenv("FIR_GEMM_ADAPT_DBG", "3")
    keys, want, disp, st, ex = run(fir_audit, rows, q, lists=True)
    assert TILE in disp["kernel"], disp
    over = ex["counts"] > form.K_LIST_CAP
    print(f"TILE256 OVERFLOW: first counts {int(ex['counts'].min())}/{int(ex['counts'].max())}, overflowed {int(over.sum())} of {qb}, {st}")
    assert over.sum() > 128, ex["counts"]
    assert st["second_pass_queries"] == int(over.sum()) and st["fallback_queries"] == 0, (st, int(over.sum()))
    assert torch.equal(keys, want)
    assert np.all(winners_of(fir_audit, keys) == n - 1)
