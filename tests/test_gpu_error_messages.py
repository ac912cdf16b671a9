"""What fir_last_error() says after a bad-argument call into each of the library's seven translation units: the
texts are the ones the argument checks have always produced, and a later failure replaces an earlier one's text.
Argument checks only: nothing here faults or fails a launch."""
import ctypes

import numpy as np
import pytest

import golden_cases as gc

pytestmark = pytest.mark.gpu

ERR_ARG = -1        # FIR_ERR_ARG, include/fir_amd.h


@pytest.fixture(scope="module")
def handles(fir):
    """A 70 x 256 gallery with 5 classes and an 8 x 4 float64 training set."""
    rows, cls, q, ncls = gc.twd_case(seed=7, n=70, d=256, n_classes=5)
    x = np.random.default_rng(3).random((8, 4))
    lab = np.array([0, 0, 0, 1, 1, 1, 2, 2], np.int32)
    with fir.Gallery(rows, cls, gc.L2, 0) as g, fir.ClsModel(x, lab, 3, x.mean(0), 0) as m:
        yield {"g": g, "m": m, "rows": rows, "cls": cls, "q": q[:2], "ncls": ncls, "x": x, "lab": lab}


def unsorted_fpnn(fir, h):
    lab = h["lab"].copy()
    lab[6] = 0
    return fir.Fpnn(h["x"], lab, 3, h["x"].mean(0), h["x"].std(0), 1.0, 0)


def short_twd_report(fir, h):
    info = fir.capi.TwdDispatchInfo()
    info.struct_bytes = 4
    fir.capi._check(fir.lib().fir_twd_last_dispatch(h["g"]._h, ctypes.byref(info)))


# (translation unit, the failing call, the message its argument check writes)
CASES = [
    ("fir_capi.hip", lambda fir, h: h["g"].search_topk(h["q"], 9), "k=9 outside [1,8]"),
    ("fir_cls.hip", lambda fir, h: h["m"].knn_predict(h["x"][:2], 0), "k=0 outside [1,8]"),
    ("fir_twd.hip", lambda fir, h: h["g"].twd_conventional(h["q"], h["ncls"], 3, 0.5, 64), "type 3 outside [0,2]"),
    ("fir_twd.hip", lambda fir, h: h["g"].twd_proposed(h["q"], 48, 0.7), "reduced_features_count=48 must divide 256"),
    ("fir_twd.hip", lambda fir, h: h["g"].twd_proposed(h["q"], 256, 0.7), "reduced_features_count=256 outside (0,256)"),
    ("fir_gemm.hip", lambda fir, h: fir.GemmSearch(h["g"], precision=7), "bad precision 7"),
    ("fir_dem.hip", lambda fir, h: h["g"].dem_pivot_table(0, 0), "n_pivots=0 must be positive"),
    ("fir_dem.hip", lambda fir, h: h["g"].rows_distances(h["q"], np.zeros((2, 3), np.int32), 5, 3), "feature range [5,3) outside [0,256)"),
    ("fir_fpnn.hip", unsorted_fpnn, "train_class must be non-decreasing in [0,3) (row 6)"),
    ("fir_shard.hip", lambda fir, h: fir.ShardedGallery(h["rows"], h["cls"], gc.L2, devices=(0, 0)),
     "device 0 listed twice (use shards_per_device for logical shards)"),
    ("fir_twd.hip", short_twd_report, "fir_twd_dispatch_info.struct_bytes = 4"),
]


def message_of(fir, call, h):
    with pytest.raises(fir.FirError) as e:
        call(fir, h)
    assert e.value.code == ERR_ARG
    prefix = f"fir_amd error {ERR_ARG}: "
    assert str(e.value).startswith(prefix)
    return str(e.value)[len(prefix):]


@pytest.mark.parametrize("unit,call,message", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_argument_error_text(fir, handles, unit, call, message):
    assert message_of(fir, call, handles) == message


def test_later_failure_replaces_earlier_text(fir, handles):
    """Every translation unit writes the one buffer fir_last_error() reads: whichever failed last is what it says,
    also when the earlier text was the longer one."""
    order = [CASES[9], CASES[2], CASES[7], CASES[1], CASES[3], CASES[0]]
    for _, call, message in order:
        assert message_of(fir, call, handles) == message
    assert fir.lib().fir_last_error().decode() == order[-1][2]
