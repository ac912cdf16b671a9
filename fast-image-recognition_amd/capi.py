"""ctypes binding of include/fir_amd.h (plumbing only: argument marshalling, error mapping)."""
import ctypes as C
import os

import numpy as np

METRIC_L2, METRIC_CHI2, METRIC_KL = 0, 1, 2
KEY_NONE = 0xFFFFFFFFFFFFFFFF

_HERE = os.path.dirname(os.path.abspath(__file__))


_LIB_FILE = "libfir_amd.so"       # __graft_entry__.load_package(audit=True) points its own copy of this module at libfir_amd_audit.so


def lib_path():
    # FIR_AMD_LIB: an alternative build of the same library (kernel-variant experiments in tools/)
    return os.environ.get("FIR_AMD_LIB") or os.path.join(_HERE, _LIB_FILE)


class FirError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fir_amd error {code}: {msg}")
        self.code = code


# Every symbol include/fir_amd.h declares: (name, restype, argtypes).
_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_u64p = C.POINTER(C.c_uint64)
_vp = C.c_void_p
SYMBOLS = [
    ("fir_last_error", C.c_char_p, []),
    ("fir_version", C.c_int, []),
    ("fir_device_count", C.c_int, []),
    ("fir_device_info", C.c_int, [C.c_int32, C.c_char_p, C.c_int32, _i32p, _i64p]),
    ("fir_device_peak_hbm_gbs", C.c_int, [C.c_int32, C.POINTER(C.c_double)]),
    ("fir_gallery_create", C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    ("fir_gallery_create_dev", C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, C.POINTER(_vp)]),
    ("fir_gallery_destroy", C.c_int, [_vp]),
    ("fir_gallery_info", C.c_int, [_vp, _i64p, _i32p, _i32p, _i32p]),
    ("fir_gallery_set_metric", C.c_int, [_vp, C.c_int32]),
    ("fir_gallery_set_row_offset", C.c_int, [_vp, C.c_int64]),
    ("fir_gallery_reserve", C.c_int, [_vp, C.c_int64]),
    ("fir_gallery_capacity", C.c_int, [_vp, _i64p]),
    ("fir_gallery_append", C.c_int, [_vp, _vp, C.c_int64, _vp]),
    ("fir_gallery_append_dev", C.c_int, [_vp, _vp, C.c_int64, _vp, _vp]),
    ("fir_gallery_set_rows", C.c_int, [_vp, _vp, C.c_int32, _vp, _vp]),
    ("fir_gallery_remove_rows", C.c_int, [_vp, _vp, C.c_int32, _vp]),
    ("fir_gallery_remove_plan", C.c_int, [C.c_int64, _vp, C.c_int32, _vp]),
    ("fir_gallery_read_rows", C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp]),
    ("fir_gallery_set_large_batch_mfma", C.c_int, [_vp, C.c_int32]),
    ("fir_gallery_set_int8_nomination", C.c_int, [_vp, C.c_int32]),
    ("fir_feature_distance", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p]),
    ("fir_search_top1", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_search_top1_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_keys_unpack", C.c_int, [_vp, C.c_int32, _vp, _vp]),
    ("fir_key_pack", C.c_uint64, [C.c_float, C.c_int32]),
    ("fir_gallery_classes_of", C.c_int, [_vp, _vp, C.c_int32, _vp]),
    ("fir_search_topk", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_search_topk_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_search_knn", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_search_knn_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_search_radius", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    ("fir_search_radius_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    ("fir_search_top1_other_class", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("fir_search_top1_other_class_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("fir_search_top1_masked", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("fir_search_top1_masked_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("fir_search_knn_masked", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp]),
    ("fir_search_knn_masked_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp]),
    ("fir_search_radius_masked", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp]),
    ("fir_search_radius_masked_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp]),
    ("fir_search_top_classes_masked", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("fir_search_top_classes_masked_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("fir_gallery_mask_of_classes", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, _vp]),
    ("fir_gallery_mask_of_classes_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_gallery_rows_of_mask", C.c_int, [_vp, _vp, _vp, C.c_int64, _i64p]),
    ("fir_gallery_rows_of_mask_dev", C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, _vp]),
    ("fir_gallery_gather_rows_dev", C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp]),
    ("fir_gallery_create_from_rows", C.c_int, [_vp, _vp, C.c_int64, C.POINTER(_vp)]),
    ("fir_gallery_create_from_rows_dev", C.c_int, [_vp, _vp, C.c_int64, _vp, C.POINTER(_vp)]),
    ("fir_gallery_create_subset", C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    ("fir_gallery_create_subset_dev", C.c_int, [_vp, _vp, _vp, C.POINTER(_vp)]),
    ("fir_gallery_origin_rows", C.c_int, [_vp, C.c_int64, C.c_int64, _vp]),
    ("fir_keys_to_origin_dev", C.c_int, [_vp, _vp, C.c_int64, _vp]),
    ("fir_keys_map_rows", C.c_int, [_vp, C.c_int64, _vp, C.c_int64, C.c_int64]),
    ("fir_gallery_other_class_keys_dev", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_gallery_other_class", C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_gallery_far_threshold", C.c_int, [_vp, C.c_int32, C.c_int32, C.c_float, _vp, _vp, _vp, _vp]),
    ("fir_search_top_classes", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("fir_search_top_classes_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("fir_class_keys_merge", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_range_distances", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp]),
    ("fir_range_distances_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_twd_conventional", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, _vp, _vp]),
    ("fir_twd_proposed", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_double, _vp, _vp, _vp]),
    ("fir_twd_last_dispatch", C.c_int, [_vp, _vp]),
    ("fir_twd_last_mfma", C.c_int, [_vp, _vp]),
    ("fir_cls_create", C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, C.POINTER(_vp)]),
    ("fir_cls_create_dev", C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, C.POINTER(_vp)]),
    ("fir_cls_destroy", C.c_int, [_vp]),
    ("fir_cls_create_sharded", C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, _vp, _vp, C.c_int32, _vp, C.POINTER(_vp)]),
    ("fir_cls_sharded_destroy", C.c_int, [_vp]),
    ("fir_cls_sharded_pnn_predict", C.c_int, [_vp, _vp, C.c_int32, C.c_double, _vp, _vp]),
    ("fir_cls_sharded_knn_predict", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, _vp]),
    ("fir_cls_set_total_training_size", C.c_int, [_vp, C.c_int64]),
    ("fir_cls_kmedoids", C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp]),
    ("fir_cls_distance_sums", C.c_int, [_vp, _vp, C.c_int32, _vp]),
    ("fir_cls_pnn_predict", C.c_int, [_vp, _vp, C.c_int32, C.c_double, _vp, _vp]),
    ("fir_cls_pnn_predict_seq", C.c_int, [_vp, _vp, C.c_int32, C.c_double, _vp, _vp]),
    ("fir_cls_knn_predict", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, _vp]),
    ("fir_cls_set_knn_mfma", C.c_int, [_vp, C.c_int32]),
    ("fir_cls_knn_stats", C.c_int, [_vp, _i64p, _i64p]),
    ("fir_cls_set_pnn_mfma", C.c_int, [_vp, C.c_int32]),
    ("fir_cls_pnn_stats", C.c_int, [_vp, _i64p, _i64p]),
    ("fir_cls_last_dispatch", C.c_int, [_vp, C.c_char_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("fir_cls_knn_class_nearest", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, _vp]),
    ("fir_gemm_create", C.c_int, [_vp, C.POINTER(_vp)]),
    ("fir_gemm_create_ex", C.c_int, [_vp, C.c_int32, C.POINTER(_vp)]),
    ("fir_gemm_destroy", C.c_int, [_vp]),
    ("fir_gemm_create_range", C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    ("fir_gemm_search_top1_keys_dev", C.c_int, [_vp, _vp, C.c_int32, _vp, _vp]),
    ("fir_gemm_search_topk_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_gemm_search_top_classes_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("fir_gemm_search_knn_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_gemm_search_radius_keys_dev", C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    ("fir_gemm_search_few_keys_dev", C.c_int, [_vp, _vp, C.c_int32, _vp, _vp]),
    ("fir_gemm_stats", C.c_int, [_vp, _i64p, _i64p]),
    ("fir_gemm_stats_ex", C.c_int, [_vp, _i64p]),
    ("fir_gemm_uncertified_notes", C.c_int, [_vp, _f32p, _i32p]),
    ("fir_gallery_mfma_uncertified_notes", C.c_int, [_vp, _f32p, _i32p]),
    ("fir_dem_pivot_table", C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _i32p]),
    ("fir_dem_create", C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    ("fir_dem_destroy", C.c_int, [_vp]),
    ("fir_dem_info", C.c_int, [_vp, _i32p, _i32p, _i32p, _i64p]),
    ("fir_dem_get", C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("fir_dem_likelihoods", C.c_int, [_vp, _vp, C.c_int32, _vp, _vp]),
    ("fir_dem_recognize", C.c_int, [_vp, _vp, C.c_int32, C.c_float, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    ("fir_dem_recognize_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_float, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fir_rows_distances", C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, _vp]),
    ("fir_fpnn_train", C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, _vp, _vp, C.c_double, C.c_int32, C.POINTER(_vp)]),
    ("fir_fpnn_destroy", C.c_int, [_vp]),
    ("fir_fpnn_info", C.c_int, [_vp, _i32p, _i32p, _i32p]),
    ("fir_fpnn_get_model", C.c_int, [_vp, _vp]),
    ("fir_fpnn_predict", C.c_int, [_vp, _vp, C.c_int32, _vp, _vp]),
    ("fir_fpnn_predict_seq", C.c_int, [_vp, _vp, C.c_int32, C.c_float, _vp, _vp]),
    ("fir_comm_unique_id", C.c_int, [_vp]),
    ("fir_gallery_create_sharded", C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, C.POINTER(_vp)]),
    ("fir_gallery_create_sharded_ex", C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, _vp, C.POINTER(_vp)]),
    ("fir_sharded_destroy", C.c_int, [_vp]),
    ("fir_sharded_info", C.c_int, [_vp, _i64p, _i32p, _i32p, _i32p, _i32p, _i32p]),
    ("fir_sharded_shard", C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i64p, _i64p]),
    ("fir_sharded_set_metric", C.c_int, [_vp, C.c_int32]),
    ("fir_sharded_search_top1", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_sharded_search_topk", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_sharded_search_knn", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_sharded_search_top1_other_class", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("fir_sharded_search_radius", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    ("fir_sharded_classify_top1", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    ("fir_sharded_search_top1_keys_dev", C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    ("fir_sharded_sync", C.c_int, [_vp]),
    ("fir_sharded_profile_enable", C.c_int, [_vp, C.c_int32]),
    ("fir_sharded_profile_read", C.c_int, [_vp, _vp, C.c_int32, _i32p]),
    ("fir_profile_enable", C.c_int, [_vp, C.c_int32]),
    ("fir_profile_read", C.c_int, [_vp, _vp, C.c_int32, _i32p, C.POINTER(C.c_double)]),
    ("fir_gallery_last_dispatch", C.c_int, [_vp, _vp]),
    ("fir_gallery_sync", C.c_int, [_vp]),
    ("fir_gallery_set_tuning", C.c_int, [_vp, C.c_int32, C.c_int32]),
    ("fir_gallery_value_range", C.c_int, [_vp, _i32p, _i32p]),
    ("fir_gallery_get_tuning", C.c_int, [_vp, _i32p, _i32p, _i32p]),
    ("fir_cls_profile_enable", C.c_int, [_vp, C.c_int32]),
    ("fir_cls_profile_read", C.c_int, [_vp, _vp, C.c_int32, _i32p, C.POINTER(C.c_double), C.c_char_p, C.c_int32]),
    ("fir_gallery_mfma_stats", C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fir_gallery_mfma_stats_ex", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("fir_gallery_memory_bytes", C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fir_gallery_set_shadow_copies", C.c_int, [_vp, C.c_int32]),
    ("fir_gallery_feature_stats", C.c_int, [_vp, _vp, _i64p, _vp, _vp, _vp, _vp]),
    ("fir_gallery_scatter", C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64p]),
    ("fir_projection_create", C.c_int, [_vp, C.c_int32, C.c_int32, _vp, C.c_int32, C.POINTER(_vp)]),
    ("fir_projection_destroy", C.c_int, [_vp]),
    ("fir_projection_info", C.c_int, [_vp, _i32p, _i32p, _i32p]),
    ("fir_projection_apply", C.c_int, [_vp, _vp, C.c_int64, _vp]),
    ("fir_projection_apply_dev", C.c_int, [_vp, _vp, C.c_int64, _vp, _vp]),
    ("fir_gallery_create_projected", C.c_int, [_vp, _vp, C.POINTER(_vp)]),
]

_lib = None


def lib():
    """Load libfir_amd.so (once). Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise FirError(-100, f"{p} not built (run __graft_entry__.build())")
        L = C.CDLL(p)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise FirError(rc, lib().fir_last_error().decode(errors="replace"))


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(_vp)


def device_count():
    return lib().fir_device_count()


def device_info(device=0):
    name = C.create_string_buffer(64)
    cus = C.c_int32()
    hbm = C.c_int64()
    _check(lib().fir_device_info(device, name, 64, C.byref(cus), C.byref(hbm)))
    return {"arch": name.value.decode(), "cus": cus.value, "hbm_bytes": hbm.value}


def device_peak_hbm_gbs(device=0):
    v = C.c_double()
    _check(lib().fir_device_peak_hbm_gbs(device, C.byref(v)))
    return v.value


def feature_distance(lhs, rhs, start=0, end=None, metric=METRIC_L2, device=0):
    lhs, pl = _f32(lhs)
    rhs, pr = _f32(rhs)
    if end is None:
        end = lhs.size
    out = C.c_float()
    _check(lib().fir_feature_distance(pl, pr, lhs.size, start, end, metric, device, C.byref(out)))
    return np.float32(out.value)


def key_pack(dist, idx):
    return int(lib().fir_key_pack(float(dist), int(idx)))


def keys_unpack(keys):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    idx = np.empty(keys.shape, np.int32)
    dist = np.empty(keys.shape, np.float32)
    _check(lib().fir_keys_unpack(keys.ctypes.data_as(_vp), keys.size, idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
    return idx, dist


def class_keys_merge(keys, classes, k):
    """keys[parts, qb, k] / classes[parts, qb, k] of search_top_classes_keys_dev over row shards -> (keys[qb, k], classes[qb, k])
    of the whole gallery (fir_class_keys_merge: per class the smallest key, then the k smallest)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    classes = np.ascontiguousarray(classes, dtype=np.int32)
    if keys.ndim != 3 or keys.shape != classes.shape or keys.shape[2] != k:
        raise ValueError("keys and classes must both be [parts, qb, k]")
    parts, qb, _ = keys.shape
    keys_out = np.empty((qb, k), np.uint64)
    classes_out = np.empty((qb, k), np.int32)
    _check(lib().fir_class_keys_merge(keys.ctypes.data_as(_vp), classes.ctypes.data_as(_vp), parts, qb, k, keys_out.ctypes.data_as(_vp),
                                      classes_out.ctypes.data_as(_vp)))
    return keys_out, classes_out


def mask_words(n):
    """FIR_MASK_WORDS(n): the 64-bit words of a row mask over n rows."""
    return (int(n) + 63) // 64


def pack_row_mask(take):
    """bool[n] -> uint64[FIR_MASK_WORDS(n)]: row r takes part iff bit r & 63 of word r >> 6 is set; the bits past n are zero."""
    take = np.asarray(take).astype(bool).reshape(-1)
    bits = np.zeros(mask_words(take.size) * 64, np.uint8)
    bits[:take.size] = take
    return np.ascontiguousarray(np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64))


def keys_map_rows(keys, row_map, row_add=0):
    """fir_keys_map_rows on a copy: every key's low word r becomes uint32(row_map[r] + row_add), the distance bits and FIR_KEY_NONE
    stay. Pure host code. Raises FirError when a low word is at or beyond len(row_map)."""
    out = np.array(keys, dtype=np.uint64, order="C", copy=True)
    row_map = np.ascontiguousarray(row_map, dtype=np.int32).reshape(-1)
    _check(lib().fir_keys_map_rows(out.ctypes.data_as(_vp) if out.size else None, out.size, row_map.ctypes.data_as(_vp) if row_map.size else None,
                                   row_map.size, int(row_add)))
    return out


def remove_plan(n, row_idx):
    """fir_gallery_remove_rows' rule as pure integer work on the host (fir_gallery_remove_plan): moved_from[m], the former row
    now sitting at row_idx[i], -1 where row_idx[i] >= n - m. Raises FirError on an index outside [0, n) or a duplicate."""
    row_idx = np.ascontiguousarray(row_idx, dtype=np.int32).reshape(-1)
    moved = np.empty(row_idx.size, np.int32)
    _check(lib().fir_gallery_remove_plan(int(n), row_idx.ctypes.data_as(_vp), row_idx.size, moved.ctypes.data_as(_vp)))
    return moved


class DispatchInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("path", C.c_int32), ("kernel", C.c_char * 160), ("launches", C.c_int32), ("grid_x", C.c_int32),
                ("grid_y", C.c_int32), ("block", C.c_int32), ("lds_bytes", C.c_int32), ("vgprs", C.c_int32), ("queries_per_pass", C.c_int32),
                ("bytes_per_launch", C.c_double), ("flops_per_launch", C.c_double), ("warmup_calls_left", C.c_int32), ("reserved", C.c_int32),
                ("knobs", C.c_char * 160)]


class TwdDispatchInfo(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("classifier", C.c_int32), ("planned_fused", C.c_int32), ("tiles_per_wave", C.c_int32),
                ("workgroups_per_query", C.c_int32), ("queries_per_launch", C.c_int32), ("fused_launches", C.c_int32),
                ("fused_gave_up", C.c_int32), ("staged_batches", C.c_int32), ("reserved", C.c_int32), ("kernel", C.c_char * 160)]


SHADOW_NONE, SHADOW_FP16, SHADOW_ALL = 0, 1, 2


class Gallery:
    """Owns one fir_gallery handle. Host arrays in, host arrays out, unless the *_dev methods
    are used with raw device pointers (ints, e.g. torch.Tensor.data_ptr())."""

    def __init__(self, rows=None, class_no=None, metric=METRIC_L2, device=0, *, dev_ptr=None, n=None, d=None,
                 dev_class_ptr=None, stream=None):
        self._h = _vp()
        if dev_ptr is not None:
            _check(lib().fir_gallery_create_dev(_vp(dev_ptr), n, d, _vp(dev_class_ptr) if dev_class_ptr else None, metric,
                                                device, _vp(stream) if stream else None, C.byref(self._h)))
            self.n, self.d = int(n), int(d)
        else:
            rows = np.ascontiguousarray(rows, dtype=np.float32)
            if rows.ndim != 2:
                raise ValueError("rows must be [n, d]")
            cls_p = None
            if class_no is not None:
                class_no = np.ascontiguousarray(class_no, dtype=np.int32)
                cls_p = class_no.ctypes.data_as(_vp)
            _check(lib().fir_gallery_create(rows.ctypes.data_as(_vp), rows.shape[0], rows.shape[1], cls_p, metric, device,
                                            C.byref(self._h)))
            self.n, self.d = rows.shape
        self.device = device

    def close(self):
        if self._h:
            lib().fir_gallery_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_metric(self, metric):
        _check(lib().fir_gallery_set_metric(self._h, metric))

    def set_row_offset(self, off):
        _check(lib().fir_gallery_set_row_offset(self._h, off))

    # ---- in-place updates (include/fir_amd.h); self.n follows the handle ----
    def _follow(self):
        n = C.c_int64()
        _check(lib().fir_gallery_info(self._h, C.byref(n), None, None, None))
        self.n = int(n.value)

    def reserve(self, rows):
        _check(lib().fir_gallery_reserve(self._h, int(rows)))

    def capacity(self):
        rows = C.c_int64()
        _check(lib().fir_gallery_capacity(self._h, C.byref(rows)))
        return int(rows.value)

    def append(self, rows, class_no=None):
        """rows[m, d] (class_no[m] on a labelled handle) become gallery rows n .. n + m - 1."""
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.d)
        cls_p = None
        if class_no is not None:
            class_no = np.ascontiguousarray(class_no, dtype=np.int32).reshape(-1)
            if class_no.size != rows.shape[0]:
                raise ValueError("class_no must have one entry per row")
            cls_p = class_no.ctypes.data_as(_vp)
        _check(lib().fir_gallery_append(self._h, rows.ctypes.data_as(_vp), rows.shape[0], cls_p))
        self._follow()

    def append_dev(self, rows_ptr, m, class_ptr=None, stream=None):
        """The same from device memory (raw pointers), asynchronous on `stream`."""
        _check(lib().fir_gallery_append_dev(self._h, _vp(rows_ptr), int(m), _vp(class_ptr) if class_ptr else None, _vp(stream) if stream else None))
        self._follow()

    def set_rows(self, row_idx, new_rows, class_no=None):
        """Rows row_idx (local, distinct) take the values new_rows[m, d]; class_no None keeps their labels."""
        row_idx = np.ascontiguousarray(row_idx, dtype=np.int32).reshape(-1)
        new_rows = np.ascontiguousarray(new_rows, dtype=np.float32).reshape(-1, self.d)
        if new_rows.shape[0] != row_idx.size:
            raise ValueError("new_rows must have one row per index")
        cls_p = None
        if class_no is not None:
            class_no = np.ascontiguousarray(class_no, dtype=np.int32).reshape(-1)
            if class_no.size != row_idx.size:
                raise ValueError("class_no must have one entry per index")
            cls_p = class_no.ctypes.data_as(_vp)
        _check(lib().fir_gallery_set_rows(self._h, row_idx.ctypes.data_as(_vp), row_idx.size, new_rows.ctypes.data_as(_vp), cls_p))

    def remove_rows(self, row_idx):
        """Swap-remove of the rows row_idx (local, distinct); returns moved_from[m] (see remove_plan)."""
        row_idx = np.ascontiguousarray(row_idx, dtype=np.int32).reshape(-1)
        moved = np.empty(row_idx.size, np.int32)
        _check(lib().fir_gallery_remove_rows(self._h, row_idx.ctypes.data_as(_vp), row_idx.size, moved.ctypes.data_as(_vp)))
        self._follow()
        return moved

    def read_rows(self, row0=0, m=None, with_classes=False):
        """Rows row0 .. row0 + m - 1 (m None: to the end) as [m, d] float32; with_classes: (rows, class_no[m])."""
        self._follow()
        m = self.n - row0 if m is None else int(m)
        rows = np.empty((max(m, 0), self.d), np.float32)
        cls = np.empty(max(m, 0), np.int32) if with_classes else None
        _check(lib().fir_gallery_read_rows(self._h, int(row0), m, rows.ctypes.data_as(_vp), cls.ctypes.data_as(_vp) if with_classes else None))
        return (rows, cls) if with_classes else rows

    def set_large_batch_mfma(self, min_queries):
        _check(lib().fir_gallery_set_large_batch_mfma(self._h, min_queries))

    def set_int8_nomination(self, mode):
        """-1: the library's rule, 0: never, 1: every eligible large L2 top-1 call nominates on the int8 matrix cores"""
        _check(lib().fir_gallery_set_int8_nomination(self._h, mode))

    def set_shadow_copies(self, mode):
        _check(lib().fir_gallery_set_shadow_copies(self._h, mode))

    def mfma_stats(self):
        """passes queued; queries whose first certificate did not hold (second matrix-core pass); queries the exact device scan answered"""
        o = (C.c_int64 * 3)()
        _check(lib().fir_gallery_mfma_stats_ex(self._h, o))
        return {"passes": o[0], "second_pass_queries": o[1], "fallback_queries": o[2]}

    def uncertified_notes(self):
        """the first (up to 8) queries whose first certificate did not hold: [list entries asked for, bound, smallest stored proxy, |q|^2]"""
        o, c = (C.c_float * 32)(), C.c_int32()
        _check(lib().fir_gallery_mfma_uncertified_notes(self._h, o, C.byref(c)))
        return [[float(o[4 * i + j]) for j in range(4)] for i in range(c.value)]

    def memory_bytes(self):
        t, f, r, sc = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _check(lib().fir_gallery_memory_bytes(self._h, C.byref(t), C.byref(f), C.byref(r), C.byref(sc)))
        return {"tiled": t.value, "fp16_fragments": f.value, "rowmajor_shadow": r.value, "scratch": sc.value}

    def value_range(self):
        """(every gallery value in the plain range, every query value of the last search too) -- chi-square / KL scans
        use the short division sequence when both hold (include/fir_amd.h)."""
        a, b = C.c_int32(), C.c_int32()
        _check(lib().fir_gallery_value_range(self._h, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    def set_tuning(self, queries_per_pass=0, waves=0):
        _check(lib().fir_gallery_set_tuning(self._h, queries_per_pass, waves))

    def get_tuning(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().fir_gallery_get_tuning(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"queries_per_pass": a.value, "waves": b.value, "max_waves": c.value}

    def search_top1(self, queries, start=0, end=0):
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        idx = np.empty(q.shape[0], np.int32)
        dist = np.empty(q.shape[0], np.float32)
        _check(lib().fir_search_top1(self._h, pq, q.shape[0], start, end, idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
        return idx, dist

    def search_top1_keys_dev(self, q_ptr, qb, keys_ptr, start=0, end=0, stream=None):
        _check(lib().fir_search_top1_keys_dev(self._h, _vp(q_ptr), qb, start, end, _vp(keys_ptr), _vp(stream) if stream else None))

    def search_topk(self, queries, k, start=0, end=0):
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.float32)
        _check(lib().fir_search_topk(self._h, pq, q.shape[0], start, end, k, idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
        return idx, dist

    def search_topk_keys_dev(self, q_ptr, qb, k, keys_ptr, start=0, end=0, stream=None):
        _check(lib().fir_search_topk_keys_dev(self._h, _vp(q_ptr), qb, start, end, k, _vp(keys_ptr), _vp(stream) if stream else None))

    def search_knn(self, queries, k, start=0, end=0):
        """The k nearest rows of each query for 1 <= k <= 1024: (idx, dist), each [qb, k], ascending by (distance, row);
        unused slots -1 / 100000."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.float32)
        _check(lib().fir_search_knn(self._h, pq, q.shape[0], start, end, k, idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
        return idx, dist

    def search_knn_keys_dev(self, q_ptr, qb, k, keys_ptr, start=0, end=0, stream=None):
        _check(lib().fir_search_knn_keys_dev(self._h, _vp(q_ptr), qb, start, end, k, _vp(keys_ptr), _vp(stream) if stream else None))

    def search_radius(self, queries, radius, max_results, start=0, end=0):
        """Every row closer than radius (a scalar, or one per query) to each query: (count, idx, dist). count [qb] is exact
        however large; idx / dist [qb, max_results] hold the min(count, max_results) nearest of them ascending by (distance,
        row), unused slots -1 / 100000. max_results = 0: counts only, idx and dist are None."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        qb = q.shape[0]
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (qb,)))
        count = np.empty(qb, np.int32)
        idx = np.empty((qb, max_results), np.int32) if max_results != 0 else None
        dist = np.empty((qb, max_results), np.float32) if max_results != 0 else None
        _check(lib().fir_search_radius(self._h, pq, qb, start, end, r.ctypes.data_as(_vp), max_results, count.ctypes.data_as(_vp),
                                       idx.ctypes.data_as(_vp) if idx is not None else None,
                                       dist.ctypes.data_as(_vp) if dist is not None else None))
        return count, idx, dist

    def search_radius_keys_dev(self, q_ptr, qb, radius_ptr, max_results, count_ptr, keys_ptr, start=0, end=0, stream=None):
        _check(lib().fir_search_radius_keys_dev(self._h, _vp(q_ptr), qb, start, end, _vp(radius_ptr), max_results, _vp(count_ptr),
                                                _vp(keys_ptr) if keys_ptr else None, _vp(stream) if stream else None))

    def search_top1_other_class(self, queries, exclude_class, start=0, end=0):
        """The nearest row of each query among the rows whose class differs from exclude_class (a scalar, or one per query; any
        int32): (idx, dist), each [qb]; -1 / 100000 where no row qualifies."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        qb = q.shape[0]
        ex = np.ascontiguousarray(np.broadcast_to(np.asarray(exclude_class, np.int32).reshape(-1), (qb,)))
        idx = np.empty(qb, np.int32)
        dist = np.empty(qb, np.float32)
        _check(lib().fir_search_top1_other_class(self._h, pq, qb, start, end, ex.ctypes.data_as(_vp), idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
        return idx, dist

    def search_top1_other_class_keys_dev(self, q_ptr, qb, exclude_ptr, keys_ptr, start=0, end=0, stream=None):
        _check(lib().fir_search_top1_other_class_keys_dev(self._h, _vp(q_ptr), qb, start, end, _vp(exclude_ptr) if exclude_ptr else None,
                                                          _vp(keys_ptr) if keys_ptr else None, _vp(stream) if stream else None))

    # ---- searches over a subset of the rows (include/fir_amd.h). mask: bool[n], or the packed uint64 words of pack_row_mask ----
    def _mask(self, mask):
        if mask is None:
            return None, None
        m = np.asarray(mask)
        if m.dtype == np.bool_:
            if m.size != self.n:
                raise ValueError(f"a bool mask over {self.n} rows has {self.n} entries, got {m.size}")
            m = pack_row_mask(m)
        else:
            m = np.ascontiguousarray(m, dtype=np.uint64).reshape(-1)
        if m.size != mask_words(self.n):
            raise ValueError(f"a packed mask over {self.n} rows has {mask_words(self.n)} words, got {m.size}")
        return m, m.ctypes.data_as(_vp)

    def search_top1_masked(self, queries, mask, start=0, end=0):
        """search_top1 over the rows of the mask: (idx, dist), each [qb]; -1 / 100000 where no row qualifies."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        m, pm = self._mask(mask)
        idx = np.empty(q.shape[0], np.int32)
        dist = np.empty(q.shape[0], np.float32)
        _check(lib().fir_search_top1_masked(self._h, pq, q.shape[0], start, end, pm, idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
        return idx, dist

    def search_top1_masked_keys_dev(self, q_ptr, qb, mask_ptr, keys_ptr, start=0, end=0, stream=None):
        _check(lib().fir_search_top1_masked_keys_dev(self._h, _vp(q_ptr), qb, start, end, _vp(mask_ptr) if mask_ptr else None,
                                                     _vp(keys_ptr) if keys_ptr else None, _vp(stream) if stream else None))

    def search_knn_masked(self, queries, mask, k, start=0, end=0):
        """search_knn over the rows of the mask: (idx, dist), each [qb, k]."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        m, pm = self._mask(mask)
        idx = np.empty((q.shape[0], max(k, 0)), np.int32)
        dist = np.empty((q.shape[0], max(k, 0)), np.float32)
        _check(lib().fir_search_knn_masked(self._h, pq, q.shape[0], start, end, pm, k, idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
        return idx, dist

    def search_knn_masked_keys_dev(self, q_ptr, qb, mask_ptr, k, keys_ptr, start=0, end=0, stream=None):
        _check(lib().fir_search_knn_masked_keys_dev(self._h, _vp(q_ptr), qb, start, end, _vp(mask_ptr) if mask_ptr else None, k,
                                                    _vp(keys_ptr) if keys_ptr else None, _vp(stream) if stream else None))

    def search_radius_masked(self, queries, mask, radius, max_results, start=0, end=0):
        """search_radius over the rows of the mask: (count, idx, dist); the counts count masked-in rows only."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        qb = q.shape[0]
        m, pm = self._mask(mask)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (qb,)))
        count = np.empty(qb, np.int32)
        idx = np.empty((qb, max_results), np.int32) if max_results > 0 else None
        dist = np.empty((qb, max_results), np.float32) if max_results > 0 else None
        _check(lib().fir_search_radius_masked(self._h, pq, qb, start, end, pm, r.ctypes.data_as(_vp), max_results, count.ctypes.data_as(_vp),
                                              idx.ctypes.data_as(_vp) if idx is not None else None,
                                              dist.ctypes.data_as(_vp) if dist is not None else None))
        return count, idx, dist

    def search_radius_masked_keys_dev(self, q_ptr, qb, mask_ptr, radius_ptr, max_results, count_ptr, keys_ptr, start=0, end=0, stream=None):
        _check(lib().fir_search_radius_masked_keys_dev(self._h, _vp(q_ptr), qb, start, end, _vp(mask_ptr) if mask_ptr else None, _vp(radius_ptr),
                                                       max_results, _vp(count_ptr), _vp(keys_ptr) if keys_ptr else None,
                                                       _vp(stream) if stream else None))

    def search_top_classes_masked(self, queries, mask, num_classes, k, start=0, end=0):
        """search_top_classes over the rows of the mask: (classes, idx, dist), each [qb, k]; a class with no masked-in row does not appear."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        m, pm = self._mask(mask)
        cls = np.empty((q.shape[0], max(k, 0)), np.int32)
        idx = np.empty((q.shape[0], max(k, 0)), np.int32)
        dist = np.empty((q.shape[0], max(k, 0)), np.float32)
        _check(lib().fir_search_top_classes_masked(self._h, pq, q.shape[0], start, end, pm, num_classes, k, cls.ctypes.data_as(_vp),
                                                   idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
        return cls, idx, dist

    def search_top_classes_masked_keys_dev(self, q_ptr, qb, mask_ptr, num_classes, k, keys_ptr, classes_ptr, start=0, end=0, stream=None):
        _check(lib().fir_search_top_classes_masked_keys_dev(self._h, _vp(q_ptr), qb, start, end, _vp(mask_ptr) if mask_ptr else None, num_classes, k,
                                                            _vp(keys_ptr) if keys_ptr else None, _vp(classes_ptr) if classes_ptr else None,
                                                            _vp(stream) if stream else None))

    def mask_of_classes(self, classes, invert=False):
        """The packed mask of the rows whose class is (invert: is not) one of `classes` (any int32 values, any order): uint64[FIR_MASK_WORDS(n)]."""
        c = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1)
        out = np.zeros(mask_words(self.n), np.uint64)
        _check(lib().fir_gallery_mask_of_classes(self._h, c.ctypes.data_as(_vp) if c.size else None, c.size, 1 if invert else 0,
                                                 out.ctypes.data_as(_vp) if out.size else None))
        return out

    def mask_of_classes_dev(self, classes_ptr, m, mask_ptr, invert=False, stream=None):
        """... on the device: classes_ptr -> m ascending int32 (duplicates allowed), mask_ptr -> FIR_MASK_WORDS(n) words; asynchronous."""
        _check(lib().fir_gallery_mask_of_classes_dev(self._h, _vp(classes_ptr) if classes_ptr else None, m, 1 if invert else 0,
                                                     _vp(mask_ptr) if mask_ptr else None, _vp(stream) if stream else None))

    # ---- device-side subsets (include/fir_amd.h): compact by mask or row list, map back ----
    @classmethod
    def _adopt(cls, handle, device):
        """A Gallery over a handle the library created (fir_gallery_create_subset ...): it owns it from here on."""
        g = cls.__new__(cls)
        g._h = handle
        g.device = device
        n, d = C.c_int64(), C.c_int32()
        _check(lib().fir_gallery_info(handle, C.byref(n), C.byref(d), None, None))
        g.n, g.d = int(n.value), int(d.value)
        return g

    def rows_of_mask(self, mask, cap=None):
        """(count, rows): the exact number of rows the mask selects and the first min(count, cap) of them, ascending int32 (cap None:
        all of them; cap 0: the count-only call)."""
        m, pm = self._mask(mask)
        cap = self.n if cap is None else int(cap)
        rows = np.empty(max(cap, 0), np.int32)
        count = C.c_int64()
        _check(lib().fir_gallery_rows_of_mask(self._h, pm, rows.ctypes.data_as(_vp) if cap > 0 else None, cap, C.byref(count)))
        return int(count.value), rows[:min(int(count.value), max(cap, 0))]

    def rows_of_mask_dev(self, mask_ptr, rows_ptr, cap, count_ptr, stream=None):
        """... on the device: mask_ptr -> FIR_MASK_WORDS(n) words, rows_ptr -> cap int32, count_ptr -> one int64; asynchronous."""
        _check(lib().fir_gallery_rows_of_mask_dev(self._h, _vp(mask_ptr) if mask_ptr else None, _vp(rows_ptr) if rows_ptr else None, int(cap),
                                                  _vp(count_ptr) if count_ptr else None, _vp(stream) if stream else None))

    def gather_rows_dev(self, idx_ptr, m, rows_ptr, class_ptr=None, stream=None):
        """rows_ptr[m, d] (class_ptr[m]) <- rows idx_ptr[0 .. m) of the gallery, row-major, on the device; asynchronous."""
        _check(lib().fir_gallery_gather_rows_dev(self._h, _vp(idx_ptr) if idx_ptr else None, int(m), _vp(rows_ptr) if rows_ptr else None,
                                                 _vp(class_ptr) if class_ptr else None, _vp(stream) if stream else None))

    def subset(self, mask=None, *, mask_ptr=None, stream=None):
        """A new Gallery holding the rows the mask selects, ascending (mask: bool[n] or packed words; mask_ptr: device words)."""
        h = _vp()
        if mask_ptr is not None:
            _check(lib().fir_gallery_create_subset_dev(self._h, _vp(mask_ptr) if mask_ptr else None, _vp(stream) if stream else None, C.byref(h)))
        else:
            m, pm = self._mask(mask)
            _check(lib().fir_gallery_create_subset(self._h, pm, C.byref(h)))
        return Gallery._adopt(h, self.device)

    def from_rows(self, rows=None, *, rows_ptr=None, m=None, stream=None):
        """A new Gallery holding rows `rows` of this one in that order, repeats allowed (rows_ptr / m: a device list of int32)."""
        h = _vp()
        if rows_ptr is not None:
            _check(lib().fir_gallery_create_from_rows_dev(self._h, _vp(rows_ptr) if rows_ptr else None, int(m), _vp(stream) if stream else None, C.byref(h)))
        else:
            r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
            _check(lib().fir_gallery_create_from_rows(self._h, r.ctypes.data_as(_vp) if r.size else None, r.size, C.byref(h)))
        return Gallery._adopt(h, self.device)

    def origin_rows(self, row0=0, m=None):
        """The source's LOCAL rows of this subset's rows [row0, row0 + m) (m None: to the end of the row list): int32[m]."""
        if m is None:
            self._follow()
            m = self.n - row0
        out = np.empty(max(int(m), 0), np.int32)
        _check(lib().fir_gallery_origin_rows(self._h, int(row0), int(m), out.ctypes.data_as(_vp) if out.size else None))
        return out

    def keys_to_origin_dev(self, keys_ptr, count, stream=None):
        """Device keys of a search over this subset -> keys over its source, in place; asynchronous."""
        _check(lib().fir_keys_to_origin_dev(self._h, _vp(keys_ptr) if keys_ptr else None, int(count), _vp(stream) if stream else None))

    # ---- linear projection / PCA (include/fir_amd.h) ----
    def feature_stats(self, mask=None):
        """(count, min, max, avg, std) of the rows the mask selects (None: every row), float64[d] each: split_train_test's statistics."""
        m, pm = self._mask(mask)
        count = C.c_int64()
        out = np.empty((4, self.d), np.float64)
        _check(lib().fir_gallery_feature_stats(self._h, pm, C.byref(count), *(out[i].ctypes.data_as(_vp) for i in range(4))))
        return int(count.value), out[0], out[1], out[2], out[3]

    def scatter(self, mask=None, center=None):
        """(S, mean, count): S[d, d] = sum over the selected rows of (x - c)(x - c)^T in float64, c = center or, for None, their mean
        (returned as `mean`; with a center it is the center itself)."""
        m, pm = self._mask(mask)
        pc = None
        if center is not None:
            center = np.ascontiguousarray(center, dtype=np.float64).reshape(-1)
            if center.size != self.d:
                raise ValueError(f"center must have {self.d} entries")
            pc = center.ctypes.data_as(_vp)
        s = np.empty((self.d, self.d), np.float64)
        mean = np.empty(self.d, np.float64)
        count = C.c_int64()
        _check(lib().fir_gallery_scatter(self._h, pm, pc, s.ctypes.data_as(_vp), mean.ctypes.data_as(_vp), C.byref(count)))
        return s, mean, int(count.value)

    def projected(self, projection):
        """A new Gallery: every row mapped by `projection` (a Projection), labels, metric and row offset carried."""
        h = _vp()
        _check(lib().fir_gallery_create_projected(self._h, projection._h, C.byref(h)))
        return Gallery._adopt(h, self.device)

    def other_class(self, start=0, end=0):
        """Every row of the gallery against the gallery with its own class excluded (row i is the query): (idx, dist), each [n];
        -1 / 100000 for a row that has no row of another class."""
        idx = np.empty(self.n, np.int32)
        dist = np.empty(self.n, np.float32)
        _check(lib().fir_gallery_other_class(self._h, start, end, idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
        return idx, dist

    def other_class_keys_dev(self, row0, m, keys_ptr, start=0, end=0, stream=None):
        _check(lib().fir_gallery_other_class_keys_dev(self._h, row0, m, start, end, _vp(keys_ptr) if keys_ptr else None, _vp(stream) if stream else None))

    def far_threshold(self, false_accept_rate, start=0, end=0):
        """The reference's getThreshold over the distances of other_class(): (threshold, min_dist, max_dist, rows_counted)."""
        thr, lo, hi = C.c_float(), C.c_float(), C.c_float()
        cnt = C.c_int64()
        _check(lib().fir_gallery_far_threshold(self._h, start, end, false_accept_rate, C.byref(thr), C.byref(lo), C.byref(hi), C.byref(cnt)))
        return np.float32(thr.value), np.float32(lo.value), np.float32(hi.value), int(cnt.value)

    def search_top_classes(self, queries, num_classes, k, start=0, end=0):
        """The k nearest distinct classes of each query: (classes, idx, dist), each [qb, k]; unused slots -1 / -1 / 100000."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        cls = np.empty((q.shape[0], k), np.int32)
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.float32)
        _check(lib().fir_search_top_classes(self._h, pq, q.shape[0], start, end, num_classes, k, cls.ctypes.data_as(_vp), idx.ctypes.data_as(_vp),
                                            dist.ctypes.data_as(_vp)))
        return cls, idx, dist

    def search_top_classes_keys_dev(self, q_ptr, qb, num_classes, k, keys_ptr, classes_ptr, start=0, end=0, stream=None):
        _check(lib().fir_search_top_classes_keys_dev(self._h, _vp(q_ptr), qb, start, end, num_classes, k, _vp(keys_ptr), _vp(classes_ptr),
                                                     _vp(stream) if stream else None))

    def range_distances(self, queries, start=0, end=0):
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        out = np.empty((q.shape[0], self.n), np.float32)
        _check(lib().fir_range_distances(self._h, pq, q.shape[0], start, end, out.ctypes.data_as(_vp)))
        return out

    def rows_distances(self, queries, rows, start=0, end=0):
        """out[q][k] = distance(query q, gallery row rows[q][k]) (fir_rows_distances)."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        rows = np.ascontiguousarray(rows, np.int32).reshape(q.shape[0], -1)
        out = np.empty(rows.shape, np.float32)
        _check(lib().fir_rows_distances(self._h, pq, q.shape[0], rows.ctypes.data_as(_vp), rows.shape[1], start, end, out.ctypes.data_as(_vp)))
        return out

    def dem_pivot_table(self, first_pivot, n_pivots, want_table=True):
        """DirectedEnumeration's PIVOT build (ann.cpp:302-331): (pivots, table or None, min_other, n_built)."""
        piv = np.empty(n_pivots, np.int32)
        mo = np.empty(n_pivots, np.float32)
        table = np.empty((n_pivots, self.n), np.float32) if want_table else None
        built = C.c_int32()
        _check(lib().fir_dem_pivot_table(self._h, first_pivot, n_pivots, piv.ctypes.data_as(_vp),
                                         table.ctypes.data_as(_vp) if want_table else None, mo.ctypes.data_as(_vp), C.byref(built)))
        return piv, table, mo, built.value

    def range_distances_dev(self, q_ptr, qb, out_ptr, start=0, end=0, stream=None):
        _check(lib().fir_range_distances_dev(self._h, _vp(q_ptr), qb, start, end, _vp(out_ptr), _vp(stream) if stream else None))

    def twd_conventional(self, queries, num_classes, typ, threshold, reduced_features_count=64):
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        cls = np.empty(q.shape[0], np.int32)
        unrel = np.empty(q.shape[0], np.int32)
        _check(lib().fir_twd_conventional(self._h, pq, q.shape[0], num_classes, typ, threshold, reduced_features_count,
                                          cls.ctypes.data_as(_vp), unrel.ctypes.data_as(_vp)))
        return cls, unrel

    def twd_proposed(self, queries, reduced_features_count, threshold):
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        cls = np.empty(q.shape[0], np.int32)
        unrel = np.empty(q.shape[0], np.int32)
        chunks = np.empty(q.shape[0], np.int32)
        _check(lib().fir_twd_proposed(self._h, pq, q.shape[0], reduced_features_count, threshold, cls.ctypes.data_as(_vp),
                                      unrel.ctypes.data_as(_vp), chunks.ctypes.data_as(_vp)))
        return cls, unrel, chunks

    def twd_last_dispatch(self):
        """Which form answered the most recent twd_conventional / twd_proposed call on this handle (fir_twd_last_dispatch): a host-side
        record, reading it does not touch the device."""
        o = TwdDispatchInfo()
        o.struct_bytes = C.sizeof(TwdDispatchInfo)
        _check(lib().fir_twd_last_dispatch(self._h, C.byref(o)))
        return {"classifier": {0: "conventional", 1: "proposed"}.get(o.classifier), "planned_fused": o.planned_fused,
                "tiles_per_wave": o.tiles_per_wave, "workgroups_per_query": o.workgroups_per_query, "queries_per_launch": o.queries_per_launch,
                "fused_launches": o.fused_launches, "fused_gave_up": o.fused_gave_up, "staged_batches": o.staged_batches,
                "kernel": o.kernel.decode()}

    def twd_last_mfma(self):
        """What the most recent twd_conventional call on this handle did with the matrix cores (fir_twd_last_mfma): six host-side counters,
        all zero when the call was not routed."""
        o = (C.c_int64 * 6)()
        _check(lib().fir_twd_last_mfma(self._h, o))
        return {"queries": o[0], "reliable": o[1], "second_stage": o[2], "band": o[3], "uncertified": o[4], "class_scan": o[5]}

    def classes_of(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        out = np.empty(idx.shape, np.int32)
        _check(lib().fir_gallery_classes_of(self._h, idx.ctypes.data_as(_vp), idx.size, out.ctypes.data_as(_vp)))
        return out

    def profile_enable(self, on=True):
        _check(lib().fir_profile_enable(self._h, 1 if on else 0))

    def profile_read(self, cap=65536):
        ms = np.empty(cap, np.float32)
        cnt = C.c_int32()
        nbytes = C.c_double()
        _check(lib().fir_profile_read(self._h, ms.ctypes.data_as(_vp), cap, C.byref(cnt), C.byref(nbytes)))
        return ms[: min(cnt.value, cap)].copy(), nbytes.value

    def sync(self):
        _check(lib().fir_gallery_sync(self._h))

    def last_dispatch(self):
        """The dominant kernel of the most recent top-1 search as the library launched it (fir_gallery_last_dispatch)."""
        o = DispatchInfo()
        o.struct_bytes = C.sizeof(DispatchInfo)
        _check(lib().fir_gallery_last_dispatch(self._h, C.byref(o)))
        return {"path": "mfma" if o.path == 1 else "scan", "kernel": o.kernel.decode(), "launches": o.launches, "grid": [o.grid_x, o.grid_y],
                "block": o.block, "lds_bytes": o.lds_bytes, "vgprs": o.vgprs, "queries_per_pass": o.queries_per_pass,
                "bytes_per_launch": o.bytes_per_launch, "flops_per_launch": o.flops_per_launch, "warmup_calls_left": o.warmup_calls_left,
                "knobs": o.knobs.decode()}


COMM_ID_BYTES = 128


class Projection:
    """Owns one fir_projection handle: y = f32(W x - W c) for basis W [p, d] (rows = eigenvectors) and center c [d] (None: zeros)."""

    def __init__(self, basis, center=None, device=0):
        basis = np.ascontiguousarray(basis, dtype=np.float64)
        if basis.ndim != 2:
            raise ValueError("basis must be [p, d]")
        pc = None
        if center is not None:
            center = np.ascontiguousarray(center, dtype=np.float64).reshape(-1)
            if center.size != basis.shape[1]:
                raise ValueError(f"center must have {basis.shape[1]} entries")
            pc = center.ctypes.data_as(_vp)
        self._h = _vp()
        _check(lib().fir_projection_create(basis.ctypes.data_as(_vp), basis.shape[0], basis.shape[1], pc, device, C.byref(self._h)))
        self.p, self.d = basis.shape
        self.device = device

    def close(self):
        if self._h:
            lib().fir_projection_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        p, d, dev = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().fir_projection_info(self._h, C.byref(p), C.byref(d), C.byref(dev)))
        return int(p.value), int(d.value), int(dev.value)

    def apply(self, rows):
        """rows[m, d] -> float32[m, p], through host memory."""
        q, pq = _f32(rows)
        q = q.reshape(-1, self.d)
        out = np.empty((q.shape[0], self.p), np.float32)
        _check(lib().fir_projection_apply(self._h, pq if q.size else None, q.shape[0], out.ctypes.data_as(_vp) if out.size else None))
        return out

    def apply_dev(self, rows_ptr, m, out_ptr, stream=None):
        """rows_ptr -> m x d float32 on the device, out_ptr -> m x p float32; asynchronous."""
        _check(lib().fir_projection_apply_dev(self._h, _vp(rows_ptr) if rows_ptr else None, int(m), _vp(out_ptr) if out_ptr else None,
                                              _vp(stream) if stream else None))


def comm_unique_id():
    """RCCL unique id (bytes) made by process 0 of a multi-process sharded gallery; hand it to the other processes."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().fir_comm_unique_id(buf))
    return buf.raw


class ShardOpts(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("shards_per_device", C.c_int32), ("first_global_row", C.c_int64), ("comm_id", _vp),
                ("proc_rank", C.c_int32), ("nprocs", C.c_int32), ("rows_on_device", C.c_int32), ("reserved", C.c_int32), ("total_rows", C.c_int64),
                ("timeout_ms", C.c_int32), ("fail_shard", C.c_int32), ("fail_step", C.c_int32), ("reserved2", C.c_int32)]


class _BorrowedGallery(Gallery):
    """A shard's fir_gallery handle, owned by the ShardedGallery it came from."""

    def __init__(self, handle, n, d, device):  # noqa: super().__init__ not called on purpose
        self._h = handle
        self.n, self.d, self.device = n, d, device

    def close(self):
        self._h = _vp()


class ShardedGallery:
    """Owns one fir_sharded handle: a gallery split by rows over `devices` (x shards_per_device logical shards each);
    the ranks' keys are reduced by RCCL inside the library (include/fir_amd.h)."""

    def __init__(self, rows=None, class_no=None, metric=METRIC_L2, devices=(0,), shards_per_device=1, *, first_global_row=0,
                 comm_id=None, proc_rank=0, nprocs=1, dev_ptr=None, n=None, d=None, dev_class_ptr=None, timeout_ms=0, fail_shard=0,
                 fail_step=0):
        self._h = _vp()
        devs = np.ascontiguousarray(list(devices), dtype=np.int32)
        o = ShardOpts()
        o.struct_bytes = C.sizeof(ShardOpts)
        o.shards_per_device = shards_per_device
        o.first_global_row = first_global_row
        self._id = C.create_string_buffer(comm_id, COMM_ID_BYTES) if comm_id is not None else None
        o.comm_id = C.cast(self._id, _vp) if self._id is not None else None
        o.proc_rank, o.nprocs = proc_rank, nprocs
        o.timeout_ms, o.fail_shard, o.fail_step = timeout_ms, fail_shard, fail_step
        if dev_ptr is not None:
            o.rows_on_device = 1
            rp, cp = _vp(dev_ptr), (_vp(dev_class_ptr) if dev_class_ptr else None)
            self.n, self.d = int(n), int(d)
        else:
            rows = np.ascontiguousarray(rows, dtype=np.float32)
            if rows.ndim != 2:
                raise ValueError("rows must be [n, d]")
            self.n, self.d = rows.shape
            rp = rows.ctypes.data_as(_vp)
            cp = None
            if class_no is not None:
                class_no = np.ascontiguousarray(class_no, dtype=np.int32)
                cp = class_no.ctypes.data_as(_vp)
        _check(lib().fir_gallery_create_sharded_ex(rp, self.n, self.d, cp, metric, devs.ctypes.data_as(_vp), devs.size, C.byref(o),
                                                   C.byref(self._h)))
        self.devices = [int(v) for v in devs]

    def close(self):
        if self._h:
            lib().fir_sharded_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        n, d, nd, ns, nr, fr = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().fir_sharded_info(self._h, C.byref(n), C.byref(d), C.byref(nd), C.byref(ns), C.byref(nr), C.byref(fr)))
        return {"n_local": n.value, "d": d.value, "ndev": nd.value, "nshards": ns.value, "nranks": nr.value, "first_rank": fr.value}

    def shard(self, i):
        """(borrowed Gallery or None, first global row, rows) of local shard i."""
        g, lo, rows = _vp(), C.c_int64(), C.c_int64()
        _check(lib().fir_sharded_shard(self._h, i, C.byref(g), C.byref(lo), C.byref(rows)))
        return (_BorrowedGallery(g, rows.value, self.d, None) if g else None), lo.value, rows.value

    def set_metric(self, metric):
        _check(lib().fir_sharded_set_metric(self._h, metric))

    def search_top1(self, queries, start=0, end=0):
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        idx = np.empty(q.shape[0], np.int32)
        dist = np.empty(q.shape[0], np.float32)
        _check(lib().fir_sharded_search_top1(self._h, pq, q.shape[0], start, end, idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
        return idx, dist

    def search_topk(self, queries, k, start=0, end=0):
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.float32)
        _check(lib().fir_sharded_search_topk(self._h, pq, q.shape[0], start, end, k, idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
        return idx, dist

    def search_knn(self, queries, k, start=0, end=0):
        """Gallery.search_knn over the shards: global row indices, the unsharded handle's keys."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.float32)
        _check(lib().fir_sharded_search_knn(self._h, pq, q.shape[0], start, end, k, idx.ctypes.data_as(_vp), dist.ctypes.data_as(_vp)))
        return idx, dist

    def search_top1_other_class(self, queries, exclude_class, start=0, end=0):
        """Gallery.search_top1_other_class over the shards: global row indices, the unsharded handle's keys."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        qb = q.shape[0]
        ex = np.ascontiguousarray(np.broadcast_to(np.asarray(exclude_class, np.int32).reshape(-1), (qb,)))
        idx = np.empty(qb, np.int32)
        dist = np.empty(qb, np.float32)
        _check(lib().fir_sharded_search_top1_other_class(self._h, pq, qb, start, end, ex.ctypes.data_as(_vp), idx.ctypes.data_as(_vp),
                                                         dist.ctypes.data_as(_vp)))
        return idx, dist

    def search_radius(self, queries, radius, max_results, start=0, end=0):
        """Gallery.search_radius over the shards: global row indices, the unsharded handle's counts and keys."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        qb = q.shape[0]
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (qb,)))
        count = np.empty(qb, np.int32)
        idx = np.empty((qb, max_results), np.int32) if max_results != 0 else None
        dist = np.empty((qb, max_results), np.float32) if max_results != 0 else None
        _check(lib().fir_sharded_search_radius(self._h, pq, qb, start, end, r.ctypes.data_as(_vp), max_results, count.ctypes.data_as(_vp),
                                               idx.ctypes.data_as(_vp) if idx is not None else None,
                                               dist.ctypes.data_as(_vp) if dist is not None else None))
        return count, idx, dist

    def classify_top1(self, queries, start=0, end=0):
        q, pq = _f32(queries)
        q = q.reshape(-1, self.d)
        cls = np.empty(q.shape[0], np.int32)
        idx = np.empty(q.shape[0], np.int32)
        dist = np.empty(q.shape[0], np.float32)
        _check(lib().fir_sharded_classify_top1(self._h, pq, q.shape[0], start, end, cls.ctypes.data_as(_vp), idx.ctypes.data_as(_vp),
                                               dist.ctypes.data_as(_vp)))
        return cls, idx, dist

    def search_top1_keys_dev(self, q_ptr, qb, keys_ptr, start=0, end=0, stream=None):
        _check(lib().fir_sharded_search_top1_keys_dev(self._h, _vp(q_ptr), qb, start, end, _vp(keys_ptr), _vp(stream) if stream else None))

    def sync(self):
        _check(lib().fir_sharded_sync(self._h))

    def profile_enable(self, on=True):
        _check(lib().fir_sharded_profile_enable(self._h, 1 if on else 0))

    def profile_read(self, cap=65536):
        ms = np.empty(cap, np.float32)
        cnt = C.c_int32()
        _check(lib().fir_sharded_profile_read(self._h, ms.ctypes.data_as(_vp), cap, C.byref(cnt)))
        return ms[: min(cnt.value, cap)].copy()


class GemmSearch:
    """Large-batch L2 top-1 through the matrix cores (fir_gemm_*): same answers as Gallery.search_top1."""

    F32, BF16_SPLIT, F16 = 0, 1, 2

    def __init__(self, gallery, precision=2, end=0):
        self._g = gallery           # keeps the gallery alive
        self._h = _vp()
        _check(lib().fir_gemm_create_range(gallery._h, precision, end, C.byref(self._h)))   # end: a feature prefix [0, end), 0 = whole rows

    def close(self):
        if self._h:
            lib().fir_gemm_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def search_top1_keys_dev(self, q_ptr, qb, keys_ptr, stream=None):
        _check(lib().fir_gemm_search_top1_keys_dev(self._h, _vp(q_ptr), qb, _vp(keys_ptr), _vp(stream) if stream else None))

    def search_few_keys_dev(self, q_ptr, qb, keys_ptr, stream=None):
        _check(lib().fir_gemm_search_few_keys_dev(self._h, _vp(q_ptr), qb, _vp(keys_ptr), _vp(stream) if stream else None))

    def search_topk_keys_dev(self, q_ptr, qb, k, keys_ptr, stream=None):
        _check(lib().fir_gemm_search_topk_keys_dev(self._h, _vp(q_ptr), qb, k, _vp(keys_ptr), _vp(stream) if stream else None))

    def search_top_classes_keys_dev(self, q_ptr, qb, num_classes, k, keys_ptr, classes_ptr, stream=None):
        """Gallery.search_top_classes_keys_dev's keys and classes through the matrix cores; synchronises `stream` once."""
        _check(lib().fir_gemm_search_top_classes_keys_dev(self._h, _vp(q_ptr), qb, num_classes, k, _vp(keys_ptr), _vp(classes_ptr),
                                                          _vp(stream) if stream else None))

    def search_knn_keys_dev(self, q_ptr, qb, k, keys_ptr, stream=None):
        """Gallery.search_knn_keys_dev's keys for k <= GEMM_KNN_MAX through the matrix cores; k > 8 synchronises `stream` once."""
        _check(lib().fir_gemm_search_knn_keys_dev(self._h, _vp(q_ptr), qb, k, _vp(keys_ptr), _vp(stream) if stream else None))

    def search_radius_keys_dev(self, q_ptr, qb, radius_ptr, max_results, count_ptr, keys_ptr, stream=None):
        """Gallery.search_radius_keys_dev's counts and keys for max_results <= GEMM_KNN_MAX through the matrix cores; synchronises
        `stream` once."""
        _check(lib().fir_gemm_search_radius_keys_dev(self._h, _vp(q_ptr), qb, _vp(radius_ptr), max_results, _vp(count_ptr),
                                                     _vp(keys_ptr) if keys_ptr else None, _vp(stream) if stream else None))

    def stats(self):
        o = (C.c_int64 * 3)()
        _check(lib().fir_gemm_stats_ex(self._h, o))
        return {"passes": o[0], "second_pass_queries": o[1], "fallback_queries": o[2]}


class Dem:
    """DirectedEnumeration's device state (fir_dem_*): pivot table + kept pivots, likelihoods at query time."""

    def __init__(self, gallery, first_pivot, n_pivots):
        self._g = gallery
        self._h = _vp()
        _check(lib().fir_dem_create(gallery._h, first_pivot, n_pivots, C.byref(self._h)))
        a, b, c, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib().fir_dem_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        self.n_pivots, self.n_built, self.n_used, self.n = a.value, b.value, c.value, n.value

    def close(self):
        if self._h:
            lib().fir_dem_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get(self, want_table=True):
        piv = np.empty(self.n_pivots, np.int32)
        mo = np.empty(self.n_pivots, np.float32)
        table = np.empty((self.n_used, self.n), np.float32) if want_table else None
        order = np.empty(self.n, np.int32)
        _check(lib().fir_dem_get(self._h, piv.ctypes.data_as(_vp), mo.ctypes.data_as(_vp),
                                 table.ctypes.data_as(_vp) if want_table else None, order.ctypes.data_as(_vp)))
        return piv, mo, table, order

    def likelihoods(self, queries, want_lik=True):
        q, pq = _f32(queries)
        q = q.reshape(-1, self._g.d)
        pd = np.empty((q.shape[0], self.n_used), np.float32)
        lik = np.empty((q.shape[0], self.n), np.float32) if want_lik else None
        _check(lib().fir_dem_likelihoods(self._h, pq, q.shape[0], pd.ctypes.data_as(_vp), lik.ctypes.data_as(_vp) if want_lik else None))
        return pd, lik

    def recognize(self, queries, threshold, image_count=0):
        """DirectedEnumeration::recognize for every query in one call -> (row, dist, found, calc, tie)."""
        q, pq = _f32(queries)
        qb = q.reshape(-1, self._g.d).shape[0]
        row, found, calc, tie = (np.empty(qb, np.int32) for _ in range(4))
        dist = np.empty(qb, np.float32)
        _check(lib().fir_dem_recognize(self._h, pq, qb, threshold, image_count, *(a.ctypes.data_as(_vp) for a in (row, dist, found, calc, tie))))
        return row, dist, found, calc, tie

    def recognize_dev(self, q_ptr, qb, threshold, image_count, row_ptr, dist_ptr, found_ptr, calc_ptr, tie_ptr, stream=None):
        _check(lib().fir_dem_recognize_dev(self._h, _vp(q_ptr), qb, threshold, image_count, *(_vp(p) if p else None for p in
                                           (row_ptr, dist_ptr, found_ptr, calc_ptr, tie_ptr)), _vp(stream) if stream else None))


class Fpnn:
    """FPNNClassifier (classification.cpp:618-791): trained trigonometric-series model on the device."""

    def __init__(self, train_rows, train_class, num_classes, avg, sd, scale=1.0, device=0):
        rows = np.ascontiguousarray(train_rows, np.float64)
        cls = np.ascontiguousarray(train_class, np.int32)
        avg = np.ascontiguousarray(avg, np.float64)
        sd = np.ascontiguousarray(sd, np.float64)
        self.d, self.num_classes = rows.shape[1], num_classes
        self._h = _vp()
        _check(lib().fir_fpnn_train(rows.ctypes.data_as(_vp), rows.shape[0], self.d, cls.ctypes.data_as(_vp), num_classes,
                                    avg.ctypes.data_as(_vp), sd.ctypes.data_as(_vp), scale, device, C.byref(self._h)))
        j = C.c_int32()
        _check(lib().fir_fpnn_info(self._h, C.byref(j), None, None))
        self.J = j.value

    def close(self):
        if self._h:
            lib().fir_fpnn_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def model(self):
        a = np.empty(self.d * self.num_classes * (2 * self.J + 1), np.float64)
        _check(lib().fir_fpnn_get_model(self._h, a.ctypes.data_as(_vp)))
        return a

    def predict(self, queries):
        q = np.ascontiguousarray(queries, np.float64).reshape(-1, self.d)
        best = np.empty(q.shape[0], np.int32)
        outs = np.empty((q.shape[0], self.num_classes), np.float32)
        _check(lib().fir_fpnn_predict(self._h, q.ctypes.data_as(_vp), q.shape[0], best.ctypes.data_as(_vp), outs.ctypes.data_as(_vp)))
        return best, outs

    def predict_seq(self, queries, output_ratio=0.9):
        q = np.ascontiguousarray(queries, np.float64).reshape(-1, self.d)
        best = np.empty(q.shape[0], np.int32)
        chunks = np.empty(q.shape[0], np.int32)
        _check(lib().fir_fpnn_predict_seq(self._h, q.ctypes.data_as(_vp), q.shape[0], output_ratio, best.ctypes.data_as(_vp),
                                          chunks.ctypes.data_as(_vp)))
        return best, chunks


class ClsModel:
    """Owns one fir_cls handle: the training set of the double-precision kNN / PNN classifiers
    (qt_cpp/classification.cpp:116-226) in the reference's class-major scan order."""

    def __init__(self, train_rows, train_class, num_classes, avg, device=0, *, dev_ptr=None, nt=None, d=None):
        tc = np.ascontiguousarray(train_class, dtype=np.int32)
        av = np.ascontiguousarray(avg, dtype=np.float64)
        self._h = _vp()
        self.num_classes = int(num_classes)
        if dev_ptr is not None:          # rows already in the device's memory (float64, row-major)
            self.nt, self.d = int(nt), int(d)
            _check(lib().fir_cls_create_dev(_vp(dev_ptr), self.nt, self.d, tc.ctypes.data_as(_vp), num_classes, av.ctypes.data_as(_vp), device,
                                            C.byref(self._h)))
            return
        tr = np.ascontiguousarray(train_rows, dtype=np.float64)
        self.nt, self.d = tr.shape
        _check(lib().fir_cls_create(tr.ctypes.data_as(_vp), tr.shape[0], tr.shape[1], tc.ctypes.data_as(_vp), num_classes,
                                    av.ctypes.data_as(_vp), device, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().fir_cls_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _q(self, queries):
        q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, self.d)
        return q, q.ctypes.data_as(_vp)

    def profile_enable(self, on=True):
        _check(lib().fir_cls_profile_enable(self._h, 1 if on else 0))

    def profile_read(self, cap=4096):
        ms = np.empty(cap, np.float32)
        cnt, nb = C.c_int32(), C.c_double()
        name = C.create_string_buffer(64)
        _check(lib().fir_cls_profile_read(self._h, ms.ctypes.data_as(_vp), cap, C.byref(cnt), C.byref(nb), name, 64))
        return ms[: min(cnt.value, cap)].copy(), nb.value, name.value.decode()

    def set_total_training_size(self, total):
        _check(lib().fir_cls_set_total_training_size(self._h, int(total)))

    def kmedoids(self, num_clusters, steps=0, scratch_bytes=0):
        """k-medoids inside every class (PNNwithClusteringClassifier::train): rows[num_classes, num_clusters] = positions in
        train_rows of the live medoids in cluster order (-1 padded), their count and the steps computed per class."""
        rows = np.empty((self.num_classes, max(int(num_clusters), 0)), np.int32)
        count = np.empty(self.num_classes, np.int32)
        steps_run = np.empty(self.num_classes, np.int32)
        _check(lib().fir_cls_kmedoids(self._h, int(num_clusters), int(steps), int(scratch_bytes), rows.ctypes.data_as(_vp),
                                      count.ctypes.data_as(_vp), steps_run.ctypes.data_as(_vp)))
        return rows, count, steps_run

    def distance_sums(self, queries):
        q, pq = self._q(queries)
        out = np.empty((q.shape[0], self.nt), np.float64)
        _check(lib().fir_cls_distance_sums(self._h, pq, q.shape[0], out.ctypes.data_as(_vp)))
        return out

    def pnn_predict(self, queries, var=0.0):
        q, pq = self._q(queries)
        scores = np.empty((q.shape[0], self.num_classes), np.float64)
        best = np.empty(q.shape[0], np.int32)
        _check(lib().fir_cls_pnn_predict(self._h, pq, q.shape[0], var, scores.ctypes.data_as(_vp), best.ctypes.data_as(_vp)))
        return best, scores

    def pnn_predict_seq(self, queries, var=0.0):
        q, pq = self._q(queries)
        best = np.empty(q.shape[0], np.int32)
        chunks = np.empty(q.shape[0], np.int32)
        _check(lib().fir_cls_pnn_predict_seq(self._h, pq, q.shape[0], var, best.ctypes.data_as(_vp), chunks.ctypes.data_as(_vp)))
        return best, chunks

    def set_knn_mfma(self, min_queries):
        _check(lib().fir_cls_set_knn_mfma(self._h, min_queries))

    def knn_stats(self):
        a, b = C.c_int64(), C.c_int64()
        _check(lib().fir_cls_knn_stats(self._h, C.byref(a), C.byref(b)))
        return {"matrix_core_queries": a.value, "exact_scan_queries_of_them": b.value}

    def set_pnn_mfma(self, min_queries):
        _check(lib().fir_cls_set_pnn_mfma(self._h, min_queries))

    def pnn_stats(self):
        a, b = C.c_int64(), C.c_int64()
        _check(lib().fir_cls_pnn_stats(self._h, C.byref(a), C.byref(b)))
        return {"matrix_core_queries": a.value, "exact_scan_queries_of_them": b.value}

    def last_dispatch(self):
        buf = C.create_string_buffer(96)
        nb, fl = C.c_double(), C.c_double()
        _check(lib().fir_cls_last_dispatch(self._h, buf, 96, C.byref(nb), C.byref(fl)))
        return {"kernel": buf.value.decode(), "bytes_per_launch": nb.value, "flops_per_launch": fl.value}

    def knn_class_nearest(self, queries, k):
        """[qb, num_classes, k] smallest mean distances per class among the rows held (sharded kNN vote)."""
        q, pq = self._q(queries)
        out = np.empty((q.shape[0], self.num_classes, k), np.float64)
        _check(lib().fir_cls_knn_class_nearest(self._h, pq, q.shape[0], k, out.ctypes.data_as(_vp)))
        return out

    def knn_predict(self, queries, k):
        q, pq = self._q(queries)
        best = np.empty(q.shape[0], np.int32)
        _check(lib().fir_cls_knn_predict(self._h, pq, q.shape[0], k, best.ctypes.data_as(_vp)))
        return best


class ShardedClsModel:
    """Owns one fir_cls_sharded handle: the PNN training set split by rows over `devices` (x shards_per_device), class
    scores added across shards on the device and across ranks by RCCL (ncclAllReduce(ncclSum, ncclDouble))."""

    def __init__(self, train_rows, train_class, num_classes, avg, devices=(0,), shards_per_device=1, *, timeout_ms=0, fail_shard=0, fail_step=0):
        tr = np.ascontiguousarray(train_rows, dtype=np.float64)
        tc = np.ascontiguousarray(train_class, dtype=np.int32)
        av = np.ascontiguousarray(avg, dtype=np.float64)
        devs = np.ascontiguousarray(list(devices), dtype=np.int32)
        o = ShardOpts()
        o.struct_bytes = C.sizeof(ShardOpts)
        o.shards_per_device = shards_per_device
        o.timeout_ms, o.fail_shard, o.fail_step = timeout_ms, fail_shard, fail_step
        self._h = _vp()
        self.nt, self.d = tr.shape
        self.num_classes = int(num_classes)
        _check(lib().fir_cls_create_sharded(tr.ctypes.data_as(_vp), tr.shape[0], tr.shape[1], tc.ctypes.data_as(_vp), num_classes, av.ctypes.data_as(_vp),
                                            devs.ctypes.data_as(_vp), devs.size, C.byref(o), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().fir_cls_sharded_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def pnn_predict(self, queries, var=0.0):
        q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, self.d)
        scores = np.empty((q.shape[0], self.num_classes), np.float64)
        best = np.empty(q.shape[0], np.int32)
        _check(lib().fir_cls_sharded_pnn_predict(self._h, q.ctypes.data_as(_vp), q.shape[0], var, scores.ctypes.data_as(_vp), best.ctypes.data_as(_vp)))
        return best, scores

    def knn_predict(self, queries, k):
        q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, self.d)
        best = np.empty(q.shape[0], np.int32)
        _check(lib().fir_cls_sharded_knn_predict(self._h, q.ctypes.data_as(_vp), q.shape[0], k, best.ctypes.data_as(_vp)))
        return best
