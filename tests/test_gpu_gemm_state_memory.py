"""What a matrix-core state says it holds (fir_gemm_memory_bytes_, the part of fir_gallery_memory_bytes callers cap HBM with) against
what its calls must have allocated: the candidate lists follow the batches seen in whole 128-query pairs and two sets, the few-query
call adds its proxies, the int8 copy its fragments and per-row / per-query words, a repeated call and a recreated state move nothing,
and an f32 state reports the sample buffer its first call allocates. Every call's keys are the exact scan's.

One 20 000 x 96 gallery; the sizes below are the library's constants (fir_gemm.hip): kListCap = 4096 entries of 8 bytes per query and a
4-byte count, kPasses * kQT = 8192 queries per scratch set, kScQueries = 128 per second-chance round, kMinSampleRows = 8192."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

N, D, QB = 20000, 96, 1024
K_LIST_CAP, K_SET_QUERIES, K_SC_QUERIES, K_MIN_SAMPLE_ROWS = 4096, 8192, 128, 8192


def _memory(fir, m):
    fn = C.CDLL(fir.lib_path()).fir_gemm_memory_bytes_
    fn.restype = None
    fn.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 3
    f, r, s = C.c_int64(), C.c_int64(), C.c_int64()
    fn(m._h, C.byref(f), C.byref(r), C.byref(s))
    return {"fragments": f.value, "rowmajor": r.value, "scratch": s.value}


def _set_int8(fir, m, mode):
    fn = C.CDLL(fir.lib_path()).fir_gemm_set_int8_
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_int32]
    fn(m._h, mode)


@pytest.fixture(scope="module")
def world(fir):
    """the gallery, the queries on the device and the exact scan's keys of all of them (computed once, never written again)"""
    rows = synth.make_gallery(97, N, D, 0)
    q, _ = synth.make_queries(97, rows, QB, 0)
    g = fir.Gallery(rows, None, 0, 0)
    g.set_large_batch_mfma(0)
    q_t = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(torch.device("cuda", 0))
    want = torch.empty(QB, dtype=torch.int64, device=q_t.device)
    torch.cuda.synchronize()                            # (the library's streams do not wait for torch's)
    g.search_top1_keys_dev(q_t.data_ptr(), QB, want.data_ptr())
    torch.cuda.synchronize()
    assert g.last_dispatch()["path"] == "scan"
    yield {"g": g, "q": q_t, "want": want.cpu().numpy()}
    g.close()


def _call(fir, m, world, qb, few=False):
    """one call of the first qb queries; its keys are the exact scan's; -> the state's report after it"""
    keys = torch.zeros(qb, dtype=torch.int64, device=world["q"].device)
    torch.cuda.synchronize()
    (m.search_few_keys_dev if few else m.search_top1_keys_dev)(world["q"].data_ptr(), qb, keys.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(keys.cpu().numpy(), world["want"][:qb]), (qb, few)
    return _memory(fir, m)


def test_fp16_state_reports_what_its_calls_allocate(fir, world):
    n = N
    with fir.GemmSearch(world["g"], fir.GemmSearch.F16) as m:
        created = _memory(fir, m)
        assert created["fragments"] == ((n + 31) // 32) * ((D + 127) // 128 * 8) * 1024, created       # one-KiB pieces: 32 rows x 16 features of fp16
        # lists growth: sized by the batch seen, in whole 128-query pairs, times two sets
        small = _call(fir, m, world, 128)
        assert _call(fir, m, world, 128) == small
        large = _call(fir, m, world, 1024)
        print("GEMM STATE MEMORY fp16: created", created, "| 128 queries", small, "| 1024 queries", large)
        assert large["scratch"] - small["scratch"] == 2 * (1024 - 128) * (K_LIST_CAP * 8 + 4), (small, large)
        assert (large["fragments"], large["rowmajor"]) == (small["fragments"], small["rowmajor"]) == (created["fragments"], created["rowmajor"])
        assert _call(fir, m, world, 1024) == large
        # the few-query call: the proxies of the 4-query form
        few = _call(fir, m, world, 3, few=True)
        assert few == dict(large, scratch=large["scratch"] + 4 * n * 4), (large, few)
        assert _call(fir, m, world, 3, few=True) == few
        # the int8 copy: its fragments; the centred rows' norms, the column means, four parameters, eabs of two sets and of the round
        assert _call(fir, m, world, 64) == few
        _set_int8(fir, m, 1)
        i8 = _call(fir, m, world, 64)
        dk8 = 8
        print("GEMM STATE MEMORY fp16: few", few, "| int8", i8)
        assert i8["fragments"] - few["fragments"] == ((n + 31) // 32) * dk8 * 1024, (few, i8)
        assert i8["scratch"] - few["scratch"] == n * 4 + (D // 4) * 16 + 32 + 2 * K_SET_QUERIES * 4 + K_SC_QUERIES * 4, (few, i8)
        assert i8["rowmajor"] == few["rowmajor"]
        assert _call(fir, m, world, 64) == i8
    # destroy and recreate: the fresh state reports what the first one did right after creation
    with fir.GemmSearch(world["g"], fir.GemmSearch.F16) as m2:
        assert _memory(fir, m2) == created


def test_f32_state_reports_its_sample_buffer(fir, world):
    """every sampled proxy of a super-batch, allocated by the first call: kPasses * kQT * sample_rows floats"""
    sample_rows = min(N, max(K_MIN_SAMPLE_ROWS, N // 64))
    with fir.GemmSearch(world["g"], fir.GemmSearch.F32) as m:
        created = _memory(fir, m)
        after = _call(fir, m, world, 64)
        print("GEMM STATE MEMORY f32: created", created, "| 64 queries", after)
        assert after["scratch"] >= K_SET_QUERIES * sample_rows * 4, (created, after)
        assert _call(fir, m, world, 64) == after
