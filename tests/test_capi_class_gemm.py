"""fir_gemm_search_top_classes_keys_dev is part of the C ABI: both libraries export it and capi binds it with the header's signature
(state, queries, qb, num_classes, k, keys, classes, stream)."""
import ctypes

NAME = "fir_gemm_search_top_classes_keys_dev"


def test_both_libraries_export_the_symbol(fir, fir_audit):
    for pkg in (fir, fir_audit):
        assert hasattr(ctypes.CDLL(pkg.lib_path()), NAME), pkg.lib_path()


def test_capi_declares_the_header_signature(fir):
    decl = [s for s in fir.capi.SYMBOLS if s[0] == NAME]
    assert len(decl) == 1
    _, res, args = decl[0]
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert res is ctypes.c_int and list(args) == [vp, vp, i32, i32, i32, vp, vp, vp]
    assert hasattr(fir.GemmSearch, "search_top_classes_keys_dev")
    fn = getattr(fir.lib(), NAME)
    assert list(fn.argtypes) == list(args) and fn.restype is res
