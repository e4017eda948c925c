"""ctypes binding of liblkhip.so (the C ABI in include/lkhip.h).

No CPU fallback exists anywhere in this package: if the library is missing or there is no GPU the
first compute call raises.  numpy arrays in -> numpy arrays out (host-pointer entry points); the
``*_dev`` variants take raw device pointers (ints) for callers that already hold data in HBM
(bench.py / batch.py pass ``torch.Tensor.data_ptr()``).
"""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LK_LIB_PATH") or os.path.join(_HERE, "liblkhip.so")   # LK_LIB_PATH: A/B builds of the library

LK_OK, LK_EINVAL, LK_ENOMEM, LK_EHIP = 0, 1, 2, 3
NORM = {"standard": 0, "psd": 1, "lk_amplitude": 2, "lk_psd": 3}
BLS_FIELDS = ("power", "depth", "depth_err", "duration", "transit_time", "depth_snr", "log_likelihood")

_c_dp = ctypes.POINTER(ctypes.c_double)
_c_ip = ctypes.POINTER(ctypes.c_int64)
_vp = ctypes.c_void_p
_c_u8p = ctypes.POINTER(ctypes.c_uint8)
_c_i32p = ctypes.POINTER(ctypes.c_int32)
CUBE_MASK_MAX_NPIX = 4096      # LK_CUBE_MASK_MAX_NPIX (include/lkhip.h): pixels per cutout of lk_cube_threshold_mask_batch_dev
_c_fp = ctypes.POINTER(ctypes.c_float)

# (name, restype, argtypes) for EVERY symbol include/lkhip.h declares — tests/test_capi_symbols.py checks the list
SIGNATURES = [
    ("lk_version", ctypes.c_int, []),
    ("lk_last_error", ctypes.c_char_p, []),
    ("lk_device_count", ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    ("lk_init", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    ("lk_destroy", None, [_vp]),
    ("lk_set_host_chunk_mb", ctypes.c_int, [_vp, ctypes.c_int]),
    ("lk_bls_max_period", ctypes.c_int, [_c_dp, ctypes.c_int, ctypes.c_int, _c_dp]),
    ("lk_bls_set_ordered_histogram", ctypes.c_int, [_vp, ctypes.c_int]),
    ("lk_pld_set_eig_tolerance", ctypes.c_int, [_vp, ctypes.c_double]),
    ("lk_workspace_bytes", ctypes.c_int64, [_vp]),
    ("lk_synchronize", ctypes.c_int, [_vp]),
    ("lk_ls_power_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp]),
    ("lk_ls_power_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    ("lk_ls_chi2_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp]),
    ("lk_ls_chi2_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    ("lk_ls_fastchi2_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_dp, ctypes.c_int, _c_dp]),
    ("lk_ls_fastchi2_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp]),
    ("lk_ls_fast_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, _c_dp, ctypes.c_int, _c_dp]),
    ("lk_ls_fast_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp]),
    ("lk_ls_fast_peaks_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, _c_dp, ctypes.c_int, _c_dp, _c_dp, _c_ip]),
    ("lk_ls_fast_peaks_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("lk_ls_fast_peaks_lc_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, _c_dp, ctypes.c_int, _c_dp, _c_dp, _c_ip]),
    ("lk_dev_alloc", ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.c_size_t]),
    ("lk_dev_free", ctypes.c_int, [_vp, _vp]),
    ("lk_stream_create", ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    ("lk_stream_destroy", ctypes.c_int, [_vp, _vp]),
    ("lk_stream_synchronize", ctypes.c_int, [_vp, _vp]),
    ("lk_memcpy_h2d", ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp]),
    ("lk_memcpy_d2h", ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp]),
    ("lk_memcpy_d2d", ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp]),
    ("lk_flatten_apply_batch_dev", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_ls_fast_peaks_lc_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("lk_rebase_times_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp]),
    ("lk_segment_probe_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, _vp, _c_ip, _c_ip, _vp]),
    ("lk_bls_prepare_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_compact_columns_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_ip, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp]),
    ("lk_gather_f64_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, _c_dp, _vp]),
    ("lk_bls_stats_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_ip, _c_dp, _c_i32p, _c_i32p, _c_i32p, _c_dp, _c_dp]),
    ("lk_bls_stats_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _c_dp, _c_dp, _c_dp, _c_ip, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_ls_model_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp,
      _c_dp, _c_dp]),
    ("lk_ls_model_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _c_dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp,
      _vp]),
    ("lk_ls_model_eval_batch", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, ctypes.c_int, _c_dp, _c_dp, _c_dp]),
    ("lk_ls_model_eval_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, _c_dp, _c_dp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("lk_shader_clock_mhz", ctypes.c_int, [_vp, ctypes.c_double, _c_dp]),
    ("lk_host_alloc", ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_size_t]),
    ("lk_host_free", ctypes.c_int, [_vp]),
    ("lk_fold_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, ctypes.c_double, _c_dp, ctypes.c_int, ctypes.c_int,
      ctypes.POINTER(_c_dp), ctypes.POINTER(_c_dp), _c_dp, _c_ip]),
    ("lk_fold_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _c_dp, _c_dp, ctypes.c_double, _c_dp, ctypes.c_int, ctypes.c_int,
      ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _vp]),
    ("lk_pg_logmedian_batch", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int64, _c_dp, ctypes.c_int, _c_i32p, _c_i32p, _c_i32p, _c_i32p, ctypes.c_double,
      _c_dp]),
    ("lk_pg_logmedian_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int64, _vp, ctypes.c_int, _c_i32p, _c_i32p, _c_i32p, _c_i32p, ctypes.c_double, _vp,
      _vp]),
    ("lk_pg_boxsmooth_batch", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp, ctypes.c_int, _c_dp]),
    ("lk_pg_boxsmooth_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int64, _vp, _c_dp, ctypes.c_int, _vp, _vp]),
    ("lk_pg_acf2d_batch", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int64, _c_dp, ctypes.c_int, _c_i32p, ctypes.c_int, _c_dp, _c_dp]),
    ("lk_pg_acf2d_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int64, _vp, ctypes.c_int, _c_i32p, ctypes.c_int, _vp, _vp, _vp]),
    ("lk_pg_snr_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, _vp, _vp, _vp, _vp]),
    ("lk_pg_acf_metric_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int64, _vp, ctypes.c_int, _c_i32p, ctypes.c_int, _vp, _vp]),
    ("lk_pg_numax_pick_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, _c_dp, ctypes.c_int, _vp, _vp, _vp]),
    ("lk_pg_deltanu_batch", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int64, _c_dp, _c_i32p, _c_i32p, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int, _c_dp, _c_i32p,
      _c_i32p, _c_i32p, _c_i32p, _c_dp]),
    ("lk_pg_deltanu_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int64, _vp, _c_i32p, _c_i32p, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int, _vp, _vp, _vp, _vp,
      _vp, _vp, _vp]),
    ("lk_sigma_clip_batch",ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _c_dp, ctypes.c_double, ctypes.c_int, _c_u8p]),
    ("lk_sigma_clip_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, ctypes.c_double, ctypes.c_int, _vp, _vp]),
    ("lk_outlier_mask_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, _c_u8p]),
    ("lk_outlier_mask_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _vp]),
    ("lk_select_columns_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, ctypes.c_int, ctypes.c_int, _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _c_ip, _vp]),
    ("lk_cdpp_batch", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _c_dp, _c_u8p, ctypes.c_int, _c_dp]),
    ("lk_cdpp_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, _vp, ctypes.c_int, _vp, _vp]),
    ("lk_fill_gaps_plan_batch", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_i32p, _c_dp, _c_i32p, _c_ip]),
    ("lk_fill_gaps_plan_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _vp, _vp, _c_ip, _vp]),
    ("lk_fill_gaps_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_ip, _c_dp, _c_dp, _c_dp, _c_i32p, _c_i32p, _c_dp, _c_i32p, _c_dp, _c_dp, ctypes.c_uint64,
      ctypes.c_int64, ctypes.c_int64, _c_dp, _c_dp, _c_dp, _c_i32p, _c_i32p, _c_u8p]),
    ("lk_fill_gaps_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_ip, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, ctypes.c_int64,
      ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_gather_segments_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_ip, ctypes.c_int64, ctypes.c_int, _c_i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp]),
    ("lk_ingest_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_ip, _c_dp]),
    ("lk_ingest_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _c_ip, _vp, _vp]),
    ("lk_fits_unpack_batch", ctypes.c_int, [_vp, ctypes.c_int, _c_u8p, _c_ip, _c_i32p, _c_ip, _c_dp, _c_dp, _c_dp, _c_i32p, _c_ip]),
    ("lk_fits_unpack_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _vp, _c_ip, _c_i32p, _c_ip, _vp, _vp, _vp, _vp, _c_ip, _vp]),
    ("lk_fits_unpack_cube", ctypes.c_int, [_vp, _c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _c_i32p, ctypes.c_int, _c_dp,
                                            _c_i32p, ctypes.POINTER(ctypes.c_float), _c_ip]),
    ("lk_fits_unpack_cube_dev", ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _c_i32p, ctypes.c_int, _vp,
                                                _vp, _vp, _c_ip, _vp]),
    ("lk_transit_mask_batch", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _c_dp, _c_i32p, _c_dp, _c_dp, _c_dp, _c_u8p]),
    ("lk_transit_mask_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, _c_i32p, _c_dp, _c_dp, _c_dp, _vp, _vp]),
    ("lk_bin_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_ip, _c_dp, _c_dp, ctypes.c_int64, ctypes.c_double, _c_u8p, _c_dp,
      _c_dp, _c_dp]),
    ("lk_bin_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _c_ip, _c_dp, _c_dp, ctypes.c_int64, ctypes.c_double, _c_u8p, _vp, _vp, _vp,
      _vp]),
    ("lk_fold_bin_plan_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int, ctypes.c_double, _c_dp, ctypes.c_int, _c_dp,
      _c_dp]),
    ("lk_fold_bin_plan_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _c_dp, _c_dp, ctypes.c_int, ctypes.c_double, _c_dp, ctypes.c_int, _c_dp, _c_dp,
      _vp]),
    ("lk_fold_cycle_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, _vp, _c_dp, _c_dp, _c_dp, _vp, _vp, _vp, _vp]),
    ("lk_phase_bin_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_u8p, ctypes.c_int, _vp, _vp,
      _vp, _vp, _vp]),
    ("lk_fold_bin_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_double, _c_dp, ctypes.c_int, _c_dp, _c_dp,
      ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_i32p]),
    ("lk_fold_bin_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _c_dp, _c_dp, ctypes.c_double, _c_dp, ctypes.c_int, _c_dp, _c_dp, ctypes.c_int,
      _c_ip, _c_dp, _c_dp, _c_dp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_river_plan_batch", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int, _c_dp]),
    ("lk_river_plan_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _c_dp, _c_dp, ctypes.c_int, _c_dp, _vp]),
    ("lk_river_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int, _c_i32p, _c_i32p, _c_ip, _c_dp, _c_dp,
      _c_i32p, _c_i32p]),
    ("lk_river_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _c_dp, _c_dp, _c_dp, ctypes.c_int, _c_i32p, _c_i32p, _c_ip, _c_dp, _vp, _vp, _vp,
      _vp]),
    ("lk_argmax_batch", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp, _c_ip]),
    ("lk_argmax_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, _vp, _vp, _vp, _vp]),
    ("lk_bls_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int64, _c_dp, ctypes.c_int, ctypes.c_int,
      ctypes.c_int, _c_dp]),
    ("lk_bls_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _c_dp, _vp, ctypes.c_int64, _c_dp, ctypes.c_int, ctypes.c_int,
      ctypes.c_int, _vp, _vp]),
    ("lk_regress_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_u8p, _c_dp, _c_dp, ctypes.c_double,
      ctypes.c_int, _c_dp, _c_dp, _c_u8p]),
    ("lk_regress_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_int, _vp,
      _vp, _vp, _vp]),
    ("lk_regress_cov_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_u8p, _c_dp, _c_dp, ctypes.c_double,
      ctypes.c_int, _c_dp, _c_dp, _c_u8p, _c_dp]),
    ("lk_regress_cov_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_int, _vp,
      _vp, _vp, _vp, _vp]),
    ("lk_regress_shared_batch", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_u8p, _c_dp, _c_dp, ctypes.c_double,
      ctypes.c_int, _c_dp, _c_dp, _c_u8p, _c_dp]),
    ("lk_regress_shared_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_int, _vp,
      _vp, _vp, _vp, _vp]),
    ("lk_ridge_prior_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_double, _vp, _vp, _vp]),
    ("lk_ridge_prior_alphas_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    ("lk_regress_shared_rows_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_i32p, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_u8p, _c_dp, _c_dp, ctypes.c_double,
      ctypes.c_int, _c_dp, _c_dp, _c_u8p, _c_dp]),
    ("lk_regress_shared_rows_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_int,
      _vp, _vp, _vp, _vp, _vp]),
    ("lk_align_rows_batch", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _c_i32p, ctypes.c_int, _c_i32p, _c_i32p, _c_i32p]),
    ("lk_align_rows_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("lk_ridge_prior_rows_batch", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, ctypes.c_int, _c_dp, ctypes.c_double, _c_dp, _c_dp]),
    ("lk_ridge_prior_rows_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, ctypes.c_int, _vp, ctypes.c_double, _vp, _vp, _vp]),
    ("lk_ridge_prior_rows_alphas_batch", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_dp]),
    ("lk_ridge_prior_rows_alphas_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    ("lk_fits_cadenceno_batch", ctypes.c_int, [_vp, ctypes.c_int, _c_u8p, _c_ip, _c_i32p, _c_i32p, _c_ip, _c_ip, _c_i32p]),
    ("lk_fits_cadenceno_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _vp, _c_ip, _c_i32p, _c_i32p, _c_ip, _c_ip, _vp, _vp]),
    ("lk_subtract_f64_dev", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp]),
    ("lk_pchip_interp_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp, _c_u8p, ctypes.c_int, ctypes.c_int, _c_dp, _c_u8p]),
    ("lk_pchip_interp_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    ("lk_underfit_neighbors_batch", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, _c_dp, ctypes.c_int, _c_i32p, ctypes.c_int, _c_i32p, _c_dp, _c_dp]),
    ("lk_underfit_neighbors_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("lk_underfit_rows_bytes", ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    ("lk_underfit_rows_prepare_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int64, _vp]),
    ("lk_underfit_against_rows_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("lk_underfit_grid_neighbors_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_i32p, ctypes.c_int, _c_dp, _c_u8p, ctypes.c_int, _c_i32p, _c_dp, _c_i32p, _c_dp]),
    ("lk_underfit_grid_neighbors_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    ("lk_underfit_grid_rows_bytes", ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    ("lk_underfit_grid_rows_prepare_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int64, _vp]),
    ("lk_underfit_grid_against_rows_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    ("lk_overfit_scratch_bytes", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
      ctypes.POINTER(ctypes.c_int)]),
    ("lk_overfit_metric_batch", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp, _c_dp, _c_dp, ctypes.c_int, _c_i32p, ctypes.c_double, ctypes.c_double,
      ctypes.c_int64, ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _c_dp]),
    ("lk_overfit_metric_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
      ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp]),
    ("lk_overfit_scratch_rows_bytes", ctypes.c_int,
     [ctypes.c_int, _c_ip, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]),
    ("lk_overfit_metric_rows_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, _c_i32p, _c_ip, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
      ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _c_dp]),
    ("lk_overfit_metric_rows_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _vp, _vp, _c_ip, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
      ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp]),
    ("lk_overfit_session_rows_bytes", ctypes.c_int,
     [ctypes.c_int, _c_ip, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]),
    ("lk_overfit_session_begin_rows_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _c_ip, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
      ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, _vp, ctypes.c_int64, _vp]),
    ("lk_overfit_session_eval_rows_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _c_ip, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int, _vp,
      ctypes.c_int64, _vp, _vp]),
    ("lk_overfit_session_bytes", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
      ctypes.POINTER(ctypes.c_int)]),
    ("lk_overfit_session_begin_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
      ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, _vp, ctypes.c_int64, _vp]),
    ("lk_overfit_session_eval_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
      ctypes.c_int, _vp, ctypes.c_int64, _vp, _vp]),
    ("lk_overfit_noise_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, _vp, _vp]),
    ("lk_savgol_trend_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
      ctypes.c_double, _c_dp, _c_u8p]),
    ("lk_savgol_trend_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
      ctypes.c_double, _vp, _vp, _vp]),
    ("lk_savgol_design", ctypes.c_int, [ctypes.c_int, ctypes.c_int, _c_dp, _c_dp]),
    ("lk_pld_design_width", ctypes.c_int, [ctypes.c_int] * 5),
    ("lk_pld_design_batch", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_fp, _c_fp, _c_fp, _c_dp, _c_dp, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp]),
    ("lk_pld_design_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    ("lk_pld_correct_batch", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_fp, _c_fp, _c_fp, _c_dp, _c_dp, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp, _c_u8p,
      ctypes.c_double, ctypes.c_int, _c_dp, _c_dp, _c_u8p, _c_dp]),
    ("lk_pld_correct_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp,
      ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_pld_correct_ragged_batch", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_fp, _c_fp, _c_fp, _c_dp, _c_dp, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp, _c_u8p,
      ctypes.c_double, ctypes.c_int, _c_dp, _c_dp, _c_u8p, _c_dp, _c_i32p, _c_i32p]),
    ("lk_pld_correct_ragged_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp,
      ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_cube_threshold_mask_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double,
      ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("lk_pld_gather_ragged_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _vp,
      ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _c_i32p, _c_dp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
      _c_i32p, _vp]),
    ("lk_cube_aperture_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _c_ip, _c_ip, _vp]),
    ("lk_cube_median_image_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("lk_pld_gather_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _c_i32p,
      ctypes.c_int, ctypes.c_int, _c_i32p, ctypes.c_int, ctypes.c_int, _c_i32p, _c_dp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
      _c_i32p, _vp]),
    ("lk_pca_batch", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp]),
    ("lk_pca_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    ("lk_spline_basis_batch", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp, ctypes.c_int, ctypes.c_int, _c_dp]),
    ("lk_spline_basis_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    ("lk_standardize_batch", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp]),
    ("lk_standardize_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    ("lk_cube_centroids_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double,
      _vp, _vp, _vp]),
    ("lk_cube_centroids_quadratic_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double,
      _vp, _vp, _vp, _vp]),
    ("lk_image_centroids_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int,
      _vp, _vp, _vp, _vp]),
    ("lk_cube_diffimage_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _c_dp, _c_dp, _c_dp, ctypes.c_double, ctypes.c_double,
      ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_diffimage_offsets_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_cube_ampimage_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _c_dp, ctypes.c_int, _c_dp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
      _vp, _vp]),
    ("lk_ampimage_offsets_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_cube_pixel_ls_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _c_dp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_dp, _vp, _vp,
      _vp, _vp, _vp, _vp]),
    ("lk_cube_psf_photometry_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp,
      _c_dp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, _c_i32p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_cube_prf_photometry_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp,
      _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_i32p, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int,
      _c_i32p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_cube_psf_fit_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp,
      _c_dp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
      ctypes.c_int, _c_i32p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_cube_prf_fit_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp,
      _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_i32p, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double,
      ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, _c_i32p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
      _vp, _vp, _vp, _vp, _vp]),
    ("lk_cube_psf_width_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp,
      _c_dp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
      ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_cube_psf_positions_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _c_dp, _c_dp,
      _c_dp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
      ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("lk_cube_background_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    ("lk_cube_subtract_rows_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("lk_sff_scratch_bytes", ctypes.c_int,
     [ctypes.c_int, _c_ip, _c_i32p, _c_i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
      ctypes.POINTER(ctypes.c_int)]),
    ("lk_sff_arclength_batch", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_i32p]),
    ("lk_sff_arclength_batch_dev", ctypes.c_int, [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _vp, _vp]),
    ("lk_sff_design_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _vp, _c_i32p, _c_i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp,
      _vp, _vp, _vp, _vp, _vp]),
    ("lk_sff_correct_batch", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_u8p, _c_i32p, _c_i32p, ctypes.c_int, ctypes.c_int,
      ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp, _c_u8p, _c_i32p, _c_dp, _c_dp,
      _c_dp, _c_dp, ctypes.c_int]),
    ("lk_sff_correct_batch_dev", ctypes.c_int,
     [_vp, ctypes.c_int, _c_ip, _vp, _vp, _vp, _vp, _vp, _vp, _c_i32p, _c_i32p, ctypes.c_int, ctypes.c_int, ctypes.c_double,
      ctypes.c_int, ctypes.c_double, ctypes.c_int, _vp, ctypes.c_int64, _vp, _vp, _vp, _c_i32p, _vp, _vp, _vp, _vp, ctypes.c_int,
      _vp]),
]

_lib = None


class LkHipError(RuntimeError):
    """HIP runtime failure inside liblkhip.so (LK_EHIP)."""


def load_library(path=None):
    """dlopen liblkhip.so and type every entry point.  Raises OSError if it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise OSError(
            "%s not found: build it first (python -c 'import __graft_entry__ as g; g.build()' or "
            "make -C lightkurve_amd/csrc).  lightkurve_amd has no CPU fallback." % path)
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(path)
    for name, restype, argtypes in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's); if
    liblkhip.so pulls in /opt/rocm's copy first and torch is imported LATER, torch ends up on a second runtime and sees
    no GPU (round 1's import-order trap).  So when torch is installed but not imported yet, its bundled runtime is
    loaded first with RTLD_GLOBAL: liblkhip.so's DT_NEEDED libamdhip64.so.7 then resolves to that already-loaded
    object, and a later `import torch` reuses it — the situation bench.py (torch first) has always been in.
    LK_NO_TORCH_HIP=1 disables this (e.g. to force /opt/rocm's runtime)."""
    import sys
    if "torch" in sys.modules or os.environ.get("LK_NO_TORCH_HIP") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        libdir = os.path.join(os.path.dirname(spec.origin), "lib")
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            cand = os.path.join(libdir, name)
            if os.path.exists(cand):
                ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except Exception:      # never fatal: fall back to the plain load
        pass


def _check(rc):
    if rc == LK_OK:
        return
    msg = (_lib.lk_last_error() or b"").decode("utf-8", "replace")
    if rc == LK_EINVAL:
        raise ValueError(msg)
    if rc == LK_ENOMEM:
        raise MemoryError(msg)
    raise LkHipError(msg)


class Handle:
    """One lk_handle = one GPU.  Created lazily per device id and cached."""

    _cache = {}

    def __init__(self, device=0):
        lib = load_library()
        self._h = _vp()
        _check(lib.lk_init(int(device), ctypes.byref(self._h)))
        self.device = int(device)

    @classmethod
    def get(cls, device=0):
        device = int(device)
        if device not in cls._cache:
            cls._cache[device] = cls(device)
        return cls._cache[device]

    def close(self):
        if self._h:
            _lib.lk_destroy(self._h)
            self._h = _vp()

    def synchronize(self):
        _check(_lib.lk_synchronize(self._h))

    def workspace_bytes(self):
        return int(_lib.lk_workspace_bytes(self._h))

    def bls_set_ordered_histogram(self, on):
        """Force (True) the atomic-free BLS histogram — the form the library falls back to by itself on a device whose LDS
        ds_add_f64 is not lane-ordered; False returns to the automatic choice."""
        _check(_lib.lk_bls_set_ordered_histogram(self._h, int(bool(on))))

    def pld_set_eig_tolerance(self, tol):
        """Stop of the subspace iteration behind the PLD design matrices' PCA blocks (relative residual; 0 = the default 1e-7)."""
        _check(_lib.lk_pld_set_eig_tolerance(self._h, float(tol)))

    def set_host_chunk_mb(self, mb):
        """MiB of spectra per chunk of the pinned host pipeline behind ls_fast_batch / ls_fast_peaks_batch (default 64, or
        LK_HOST_CHUNK_MB when the handle was created)."""
        _check(_lib.lk_set_host_chunk_mb(self._h, int(mb)))


def device_count():
    lib = load_library()
    n = ctypes.c_int(0)
    rc = lib.lk_device_count(ctypes.byref(n))
    return n.value if rc == LK_OK else 0


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a, typ=_c_dp):
    return a.ctypes.data_as(typ) if a is not None else None


def _offsets(n_off, total):
    n_off = np.ascontiguousarray(n_off, dtype=np.int64)
    if n_off.ndim != 1 or n_off.size < 1 or n_off[0] != 0 or n_off[-1] != total or np.any(np.diff(n_off) < 0):
        raise ValueError("n_off must be non-decreasing prefix offsets starting at 0 and ending at len(t)")
    return n_off


# --------------------------------------------------------------------------------------------- Lomb-Scargle
MAX_NTERMS = 8  # LK_MAX_NTERMS in include/lkhip.h (5..8: exact sums for both 'chi2' and 'fastchi2')


def ls_power_batch(t, y, n_off, dy=None, frequency=None, f0=0.0, df=0.0, M=None, fit_mean=True,
                   center_data=True, normalization="psd", scale=None, device=0, nterms=1):
    """Exact GLS power for B ragged targets -> float64[B, M].

    ``t`` relative times [d], ``y`` flux, ``dy`` errors or None (uniform weights), concatenated over
    targets with prefix offsets ``n_off``.  Either ``frequency`` (any 1-D array, 1/d) or the regular grid
    ``f0 + df*arange(M)`` (the fast kernel).  ``nterms`` > 1: astropy's multi-term ``chi2`` periodogram."""
    if not 1 <= int(nterms) <= MAX_NTERMS:
        raise ValueError("nterms must be between 1 and %d on the HIP path (got %r)" % (MAX_NTERMS, nterms))
    h = Handle.get(device)
    t, y = _f64(t), _f64(y)
    n_off = _offsets(n_off, t.size)
    if y.shape != t.shape:
        raise ValueError("t and y must have the same length")
    dy = None if dy is None else _f64(np.broadcast_to(dy, t.shape))
    B = n_off.size - 1
    if frequency is not None:
        frequency = _f64(frequency).ravel()
        M = frequency.size
    M = int(M)
    scale = None if scale is None else _f64(np.broadcast_to(scale, (B,)))
    power = result_empty((B, M))
    _check(_lib.lk_ls_chi2_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(y), _ptr(dy), _ptr(frequency),
                                 float(f0), float(df), M, int(nterms), int(bool(fit_mean)), int(bool(center_data)),
                                 NORM[normalization], _ptr(scale), _ptr(power)))
    return power


def ls_power_batch_dev(handle, B, n_off_host, t_ptr, y_ptr, dy_ptr, freq_ptr, f0, df, M, fit_mean, center_data,
                       normalization, scale_ptr, power_ptr, stream=0, nterms=1):
    """Device-pointer variant (ints from tensor.data_ptr()); enqueues on ``stream`` and returns."""
    n_off_host = np.ascontiguousarray(n_off_host, dtype=np.int64)
    _check(_lib.lk_ls_chi2_batch_dev(handle._h, int(B), _ptr(n_off_host, _c_ip), _vp(t_ptr), _vp(y_ptr),
                                     _vp(dy_ptr or None), _vp(freq_ptr or None), float(f0), float(df), int(M),
                                     int(nterms), int(bool(fit_mean)), int(bool(center_data)), NORM[normalization],
                                     _vp(scale_ptr or None), _vp(power_ptr), _vp(stream or None)))


def ls_fast_batch(t, y, n_off, dy=None, f0=0.0, df=0.0, M=0, fit_mean=True, center_data=True, normalization="psd",
                  scale=None, oversampling=5, device=0, nterms=1):
    """The reference's default ``ls_method="fast"`` (extirpolation + FFT) for B ragged targets on the regular grid
    ``f0 + df*arange(M)`` -> float64[B, M].  ``nterms`` > 1: its multi-term sibling ``"fastchi2"``."""
    if not 1 <= int(nterms) <= MAX_NTERMS:
        raise ValueError("nterms must be between 1 and %d on the HIP path (got %r)" % (MAX_NTERMS, nterms))
    h = Handle.get(device)
    t, y = _f64(t), _f64(y)
    n_off = _offsets(n_off, t.size)
    if y.shape != t.shape:
        raise ValueError("t and y must have the same length")
    dy = None if dy is None else _f64(np.broadcast_to(dy, t.shape))
    B, M = n_off.size - 1, int(M)
    scale = None if scale is None else _f64(np.broadcast_to(scale, (B,)))
    power = result_empty((B, M))
    _check(_lib.lk_ls_fastchi2_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(y), _ptr(dy), float(f0), float(df), M,
                                     int(nterms), int(bool(fit_mean)), int(bool(center_data)), NORM[normalization],
                                     _ptr(scale), int(oversampling), _ptr(power)))
    return power


def ls_fast_batch_dev(handle, B, n_off_host, t_ptr, y_ptr, dy_ptr, f0, df, M, fit_mean, center_data, normalization,
                      scale_ptr, oversampling, power_ptr, stream=0):
    n_off_host = np.ascontiguousarray(n_off_host, dtype=np.int64)
    _check(_lib.lk_ls_fast_batch_dev(handle._h, int(B), _ptr(n_off_host, _c_ip), _vp(t_ptr), _vp(y_ptr),
                                     _vp(dy_ptr or None), float(f0), float(df), int(M), int(bool(fit_mean)),
                                     int(bool(center_data)), NORM[normalization], _vp(scale_ptr or None),
                                     int(oversampling), _vp(power_ptr), _vp(stream or None)))


def ls_fast_peaks_batch_dev(handle, B, n_off_host, t_ptr, y_ptr, dy_ptr, f0, df, M, fit_mean, center_data,
                            normalization, scale_ptr, oversampling, power_ptr, max_ptr, arg_ptr, stream=0):
    """lk_ls_fast_peaks_batch_dev: ls_method='fast' + per-target (nanmax, nanargmax), all device pointers."""
    n_off_host = np.ascontiguousarray(n_off_host, dtype=np.int64)
    _check(_lib.lk_ls_fast_peaks_batch_dev(handle._h, int(B), _ptr(n_off_host, _c_ip), _vp(t_ptr), _vp(y_ptr),
                                           _vp(dy_ptr or None), float(f0), float(df), int(M), int(bool(fit_mean)),
                                           int(bool(center_data)), NORM[normalization], _vp(scale_ptr or None),
                                           int(oversampling), _vp(power_ptr), _vp(max_ptr or None), _vp(arg_ptr or None),
                                           _vp(stream or None)))


def pinned_empty(shape, dtype=np.float64):
    """numpy array over page-locked host memory (lk_host_alloc): the host-pointer entry points DMA such buffers
    directly instead of staging them.  Freed when the array (and every view of it) is garbage collected."""
    import weakref
    load_library()
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    ptr = _vp()
    _check(_lib.lk_host_alloc(ctypes.byref(ptr), max(nbytes, 1)))
    buf = (ctypes.c_char * max(nbytes, 1)).from_address(ptr.value)
    weakref.finalize(buf, _lib.lk_host_free, _vp(ptr.value))
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)


_POOL = {}
_POOL_LOCK = threading.Lock()


def pinned_pool(key, count, dtype=np.float64):
    """float64[count] view of a page-locked staging buffer that is kept (and only ever grown) per ``key`` AND per calling
    thread: the packing step of the batch front end writes the concatenated light curves here so that the host-pointer
    entry points DMA them without the runtime's pageable staging.  The contents are valid until the next request for the
    same key from the same thread (ctypes releases the GIL inside lk_* calls: two threads packing into one buffer would
    overwrite each other's batch while its DMA is in flight — ADVICE r5)."""
    dtype = np.dtype(dtype)
    count = int(count)
    key = (threading.get_ident(), key)
    with _POOL_LOCK:
        buf = _POOL.get(key)
        if buf is None or buf.nbytes < count * dtype.itemsize:
            _POOL.pop(key, None)
            cap = max(count * dtype.itemsize + (count * dtype.itemsize >> 3), 1 << 16)
            buf = _POOL[key] = pinned_empty(cap, np.uint8)
    return buf[: count * dtype.itemsize].view(dtype)


def release_pinned_pool():
    """Free the page-locked staging buffers of every thread and the idle blocks of the result pool."""
    with _POOL_LOCK:
        _POOL.clear()
    if _RESULT_POOL is not None:
        _RESULT_POOL.release()


# Recycled RESULT memory.  A fresh 160-MB / 800-MB numpy result costs more in first-touch page faults (10 / 50 ms) than its
# transfer from the device (3 / 15 ms), so large results are placed in page-locked blocks that are kept for the next call.
# Ownership is numpy's own: every array handed out is built over a fresh LEASE object (its ``base`` chain ends there), and a
# block returns to the free list only when that lease is garbage collected — i.e. exactly when numpy would have freed the
# memory of an ordinary array: after the array, all its views and every memoryview / buffer export of it are gone.  (Rounds
# 4-5 looked at ``sys.getrefcount`` of a shared root array instead, which a buffer export does not raise — VERDICT r5 #8.)
# Idle blocks are capped (LK_RESULT_POOL_MB, default 2048: beyond it a returned block is freed at once);
# ``release_pinned_pool()`` frees them all; LK_RESULT_POOL=0 turns the recycling off (plain ``np.empty``).
_RESULT_POOL_MIN_BYTES = 1 << 22


class _ResultPool(object):
    def __init__(self, alloc, free, idle_limit_bytes):
        self._alloc, self._free, self.idle_limit = alloc, free, int(idle_limit_bytes)
        self.idle = []                   # (capacity, address) of blocks nobody holds
        self.lock = threading.Lock()
        self.leased = 0                  # blocks currently out (diagnostics / tests)

    def idle_bytes(self):
        with self.lock:
            return sum(c for c, _ in self.idle)

    def take(self, need):
        """(capacity, address) of a block of at least ``need`` bytes: the smallest idle one that is not wastefully large,
        else a new allocation."""
        with self.lock:
            fit = [i for i, (c, _) in enumerate(self.idle) if need <= c <= 2 * need + (1 << 20)]
            if fit:
                self.leased += 1
                return self.idle.pop(min(fit, key=lambda i: self.idle[i][0]))
        cap = need + (need >> 4)
        addr = self._alloc(cap)
        with self.lock:
            self.leased += 1
        return cap, addr

    def give(self, cap, addr):
        with self.lock:
            self.leased -= 1
            keep = sum(c for c, _ in self.idle) + cap <= self.idle_limit
            if keep:
                self.idle.append((cap, addr))
        if not keep:
            self._free(addr)

    def release(self):
        with self.lock:
            items, self.idle = self.idle, []
        for _c, addr in items:
            self._free(addr)

    def empty(self, shape, dtype):
        import weakref
        need = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        cap, addr = self.take(need)
        lease = (ctypes.c_char * cap).from_address(addr)              # does not own the memory; the finalizer returns it
        weakref.finalize(lease, self.give, cap, addr)
        return np.frombuffer(lease, dtype=dtype, count=need // dtype.itemsize).reshape(shape)


_RESULT_POOL = None
_RESULT_POOL_INIT = threading.Lock()


def _pinned_alloc(nbytes):
    ptr = _vp()
    _check(_lib.lk_host_alloc(ctypes.byref(ptr), max(int(nbytes), 1)))
    return ptr.value


def _pinned_free(addr):
    _lib.lk_host_free(_vp(addr))


def _result_pool():
    global _RESULT_POOL
    with _RESULT_POOL_INIT:
        if _RESULT_POOL is None:
            load_library()
            try:
                mb = int(os.environ.get("LK_RESULT_POOL_MB", "2048"))
            except ValueError:
                mb = 2048
            _RESULT_POOL = _ResultPool(_pinned_alloc, _pinned_free, max(mb, 0) << 20)
    return _RESULT_POOL


def result_empty(shape, dtype=np.float64):
    """Uninitialised array for a large result of a batch call (``np.empty`` semantics).  Results of 4 MB and more live in
    page-locked memory that is RECYCLED: once the array and everything that views or exports it has been garbage collected,
    the next large result may be placed at the same address.  An address obtained through ``arr.ctypes.data`` is valid for
    as long as ``arr`` (or a view of it) is alive — as for any numpy array.  LK_RESULT_POOL=0: plain ``np.empty``."""
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    dtype = np.dtype(dtype)
    need = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    if need < _RESULT_POOL_MIN_BYTES or os.environ.get("LK_RESULT_POOL", "1") == "0":
        return np.empty(shape, dtype=dtype)
    try:
        return _result_pool().empty(shape, dtype)
    except (OSError, RuntimeError, MemoryError):          # no library / no GPU runtime / pinned memory exhausted
        return np.empty(shape, dtype=dtype)


def ls_fast_peaks_batch(t, y, n_off, dy=None, f0=0.0, df=0.0, M=0, fit_mean=True, center_data=True,
                        normalization="psd", scale=None, oversampling=5, device=0, out=None, want_power=True,
                        want_peaks=True, absolute_time=False):
    """ls_method='fast' for B ragged targets through the pipelined host-pointer entry point.
    Returns (power[B, M] or None, max_power[B] or None, argmax[B] or None).  ``out``: preallocated float64[B, M]
    (e.g. from ``pinned_empty``) to receive the spectra; ``want_power=False`` keeps the spectra on the device and
    returns only the per-target peaks (Periodogram.max_power / nanargmax).  ``absolute_time``: ``t`` holds the light
    curves' own (absolute) times and each is rebased to ``t - t[first]`` on the device (lk_ls_fast_peaks_lc_batch)."""
    h = Handle.get(device)
    t, y = _f64(t), _f64(y)
    n_off = _offsets(n_off, t.size)
    if y.shape != t.shape:
        raise ValueError("t and y must have the same length")
    dy = None if dy is None else _f64(np.broadcast_to(dy, t.shape))
    B, M = n_off.size - 1, int(M)
    scale = None if scale is None else _f64(np.broadcast_to(scale, (B,)))
    power = None
    if want_power:
        power = out if out is not None else result_empty((B, M))
        if power.shape != (B, M) or power.dtype != np.float64 or not power.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of shape (B, M)")
    if not want_power and not want_peaks:
        raise ValueError("nothing requested")
    mx = np.empty(B, dtype=np.float64) if want_peaks else None
    am = np.empty(B, dtype=np.int64) if want_peaks else None
    entry = _lib.lk_ls_fast_peaks_lc_batch if absolute_time else _lib.lk_ls_fast_peaks_batch
    _check(entry(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(y), _ptr(dy), float(f0), float(df), M,
                 int(bool(fit_mean)), int(bool(center_data)), NORM[normalization], _ptr(scale),
                 int(oversampling), _ptr(power), _ptr(mx), _ptr(am, _c_ip)))
    return power, mx, am


# --------------------------------------------------------------------------------------------- Periodogram.smooth
def pg_logmedian_batch(power, win_lo, win_hi, klo, khi, corr=(8.0 / 9.0) ** 3, device=0):
    """Moving nanmedian in log-frequency windows for B periodograms on one grid (power float64[B, M]); the window
    tables come from ``periodogram._logmedian_windows`` -> float64[B, M]."""
    h = Handle.get(device)
    power = np.ascontiguousarray(np.atleast_2d(power), dtype=np.float64)
    B, M = power.shape
    tabs = [np.ascontiguousarray(a, dtype=np.int32) for a in (win_lo, win_hi, klo, khi)]
    if tabs[0].shape != tabs[1].shape or tabs[2].shape != (M,) or tabs[3].shape != (M,):
        raise ValueError("window tables do not match the grid")
    out = np.empty_like(power)
    _check(_lib.lk_pg_logmedian_batch(h._h, B, M, _ptr(power), int(tabs[0].size), _ptr(tabs[0], _c_i32p),
                                      _ptr(tabs[1], _c_i32p), _ptr(tabs[2], _c_i32p), _ptr(tabs[3], _c_i32p),
                                      float(corr), _ptr(out)))
    return out


def pg_boxsmooth_batch(power, kernel, device=0):
    """astropy.convolution.convolve(power[b], kernel) (boundary='fill', normalised, NaN-interpolating) for every row."""
    h = Handle.get(device)
    power = np.ascontiguousarray(np.atleast_2d(power), dtype=np.float64)
    B, M = power.shape
    taps = np.ascontiguousarray(np.asarray(kernel, dtype=np.float64)[::-1])
    out = np.empty_like(power)
    _check(_lib.lk_pg_boxsmooth_batch(h._h, B, M, _ptr(power), _ptr(taps), int(taps.size), _ptr(out)))
    return out


def pg_acf2d_batch(power, win_start, W, device=0):
    """Windowed autocorrelations of B periodograms on one grid (power float64[B, M]): for every window start the ACF of
    the W mean-subtracted samples and the mean collapsed correlation.  Returns (acf2d[B, n_win, W], metric[B, n_win])."""
    h = Handle.get(device)
    power = np.ascontiguousarray(np.atleast_2d(power), dtype=np.float64)
    B, M = power.shape
    ws = np.ascontiguousarray(win_start, dtype=np.int32).ravel()
    W = int(W)
    if ws.size and (ws.min() < 0 or int(ws.max()) + W > M):
        raise ValueError("a window reaches outside the spectrum")
    acf = np.empty((B, ws.size, W), dtype=np.float64)
    met = np.empty((B, ws.size), dtype=np.float64)
    _check(_lib.lk_pg_acf2d_batch(h._h, B, M, _ptr(power), int(ws.size), _ptr(ws, _c_i32p), W, _ptr(acf), _ptr(met)))
    return acf, met


def _deltanu_tables(plan, B):
    """The six per-target HOST tables of ``lk_pg_deltanu_batch`` from ``seismology._deltanu_plan``'s dict (kept alive by the
    caller for the call) and the widest selection."""
    tabs = [np.ascontiguousarray(plan[k], dtype=np.int32) for k in ("start", "width")]
    tabs += [np.ascontiguousarray(plan[k], dtype=np.float64) for k in ("deltanu_emp", "distance", "step", "stop")]
    if any(t.shape != (B,) for t in tabs):
        raise ValueError("the deltanu plan does not match the batch")
    return tabs, int(np.max(plan["sel_len"], initial=0))


def pg_deltanu_batch(power, plan, want_acf=False, device=0):
    """``estimate_deltanu_acf2d`` for B periodograms on one grid (power float64[B, M]), each with its own window from
    ``seismology._deltanu_plan`` -> dict of ``deltanu`` float64[B], ``n_peaks`` / ``status`` / ``sel_lo`` / ``sel_len`` int32[B]
    and, with ``want_acf``, ``acf`` float64[B, max_sel] (the rescaled ACF on the selected lags, NaN behind them)."""
    h = Handle.get(device)
    power = np.ascontiguousarray(np.atleast_2d(power), dtype=np.float64)
    B, M = power.shape
    tabs, max_sel = _deltanu_tables(plan, B)
    out = dict(deltanu=np.empty(B), n_peaks=np.empty(B, dtype=np.int32), status=np.empty(B, dtype=np.int32),
               sel_lo=np.empty(B, dtype=np.int32), sel_len=np.empty(B, dtype=np.int32))
    if want_acf:
        out["acf"] = np.empty((B, max_sel))
    _check(_lib.lk_pg_deltanu_batch(h._h, B, M, _ptr(power), _ptr(tabs[0], _c_i32p), _ptr(tabs[1], _c_i32p), _ptr(tabs[2]),
                                    _ptr(tabs[3]), _ptr(tabs[4]), _ptr(tabs[5]), max_sel, _ptr(out["deltanu"]),
                                    _ptr(out["n_peaks"], _c_i32p), _ptr(out["status"], _c_i32p), _ptr(out["sel_lo"], _c_i32p),
                                    _ptr(out["sel_len"], _c_i32p), _ptr(out.get("acf"))))
    return out


def argmax_batch(x, device=0):
    """Row-wise (nanmax, nanargmax) of float64[B, M]; first maximum wins; all-NaN row -> (nan, -1)."""
    h = Handle.get(device)
    x = _f64(x)
    if x.ndim != 2:
        raise ValueError("x must be 2-D")
    B, M = x.shape
    mx = np.empty(B, dtype=np.float64)
    am = np.empty(B, dtype=np.int64)
    _check(_lib.lk_argmax_batch(h._h, B, M, _ptr(x), _ptr(mx), _ptr(am, _c_ip)))
    return mx, am


def argmax_batch_dev(handle, B, M, x_ptr, max_ptr, arg_ptr, stream=0):
    _check(_lib.lk_argmax_batch_dev(handle._h, int(B), int(M), _vp(x_ptr), _vp(max_ptr), _vp(arg_ptr),
                                    _vp(stream or None)))


# --------------------------------------------------------------------------------------------- fold
def fold_batch(t, n_off, period, epoch_time, epoch_phase=0.0, wrap_phase=None, normalize_phase=False, columns=(),
               device=0):
    """LightCurve.fold for B ragged targets: returns (phase, order, [columns gathered into phase order]).
    ``period`` / ``epoch_time`` / ``wrap_phase``: scalars or one value per target; ``wrap_phase`` defaults to
    period/2 (0.5 with ``normalize_phase``), like astropy.  ``order`` indexes cadences relative to their target."""
    h = Handle.get(device)
    t = _f64(t)
    n_off = _offsets(n_off, t.size)
    B = n_off.size - 1
    period = _f64(np.broadcast_to(np.asarray(period, dtype=np.float64), (B,)))
    epoch_time = _f64(np.broadcast_to(np.asarray(epoch_time, dtype=np.float64), (B,)))
    if wrap_phase is None:
        wrap_phase = np.full(B, 0.5) if normalize_phase else period / 2.0
    wrap_phase = _f64(np.broadcast_to(np.asarray(wrap_phase, dtype=np.float64), (B,)))
    if not np.all(np.isfinite(period)) or np.any(period == 0):
        raise ValueError("period must be finite and non-zero")
    cols = [_f64(c) for c in columns]
    for c in cols:
        if c.shape != t.shape:
            raise ValueError("every column must have the length of t")
    outs = [np.empty_like(t) for _ in cols]
    arr_t = _c_dp * max(len(cols), 1)
    cin = arr_t(*[_ptr(c) for c in cols]) if cols else arr_t()
    cout = arr_t(*[_ptr(o) for o in outs]) if cols else arr_t()
    phase = np.empty_like(t)
    order = np.empty(t.size, dtype=np.int64)
    _check(_lib.lk_fold_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(period), _ptr(epoch_time), float(epoch_phase),
                              _ptr(wrap_phase), int(bool(normalize_phase)), len(cols), cin, cout, _ptr(phase),
                              _ptr(order, _c_ip)))
    return phase, order, outs


def fold_bin_batch(t, flux, n_off, period, flux_err=None, epoch_time=None, epoch_phase=0.0, wrap_phase=None,
                   normalize_phase=False, time_bin_size=None, time_bin_start=None, n_bins=None, bins=None,
                   aggregate_func="mean", which="all", device=0):
    """``lc.fold(period, epoch_time, ...).bin(...)`` for B ragged targets on host arrays, fused: no sort and no folded copy
    (``lk_fold_bin_plan_batch`` + ``lk_fold_bin_batch``).  Arguments as ``DeviceLightCurveBatch.fold_bin``.  Returns
    dict(phase, flux, flux_err, count, bin_off): target b's bins are ``[bin_off[b]:bin_off[b + 1]]``."""
    from . import foldbin
    aggregate_func, which_code = foldbin.check_bin_arguments(time_bin_size, n_bins, bins, aggregate_func, which)
    if aggregate_func != "mean":
        raise ValueError("the fused fold_bin supports aggregate_func='mean' only: use fold(...).bin(aggregate_func='median')")
    h = Handle.get(device)
    t, flux = _f64(t), _f64(flux)
    n_off = _offsets(n_off, t.size)
    B = n_off.size - 1
    err = None if flux_err is None else _f64(np.broadcast_to(flux_err, t.shape))
    period = _f64(np.broadcast_to(np.asarray(period, dtype=np.float64), (B,)))
    if not np.all(np.isfinite(period)) or np.any(period == 0):
        raise ValueError("period must be finite and non-zero")
    epoch_given = epoch_time is not None
    if epoch_time is None:
        epoch_time = t[np.minimum(n_off[:-1], max(t.size - 1, 0))] if t.size else np.zeros(B)
    epoch_time = _f64(np.broadcast_to(np.asarray(epoch_time, dtype=np.float64), (B,)))
    if wrap_phase is None:
        wrap_phase = np.full(B, 0.5) if normalize_phase else period / 2.0
    wrap_phase = _f64(np.broadcast_to(np.asarray(wrap_phase, dtype=np.float64), (B,)))
    cfrom = foldbin.count_from(time_bin_start, bins, B)
    plan = np.zeros(max(B, 1) * foldbin.NPLAN, dtype=np.float64)
    _check(_lib.lk_fold_bin_plan_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(flux), _ptr(err), _ptr(period), _ptr(epoch_time),
                                       int(epoch_given), float(epoch_phase), _ptr(wrap_phase), int(bool(normalize_phase)),
                                       _ptr(cfrom), _ptr(plan)))
    lay = foldbin.phase_bin_layout(np.diff(n_off), plan[:B * foldbin.NPLAN], time_bin_size, time_bin_start, n_bins, bins)
    cyc_epoch = epoch_time if epoch_given else _f64(plan[:B * foldbin.NPLAN].reshape(B, foldbin.NPLAN)[:, 0])
    nbt = int(lay["bin_off"][-1])
    po, fo, eo = (np.full(nbt, np.nan, dtype=np.float64) for _ in range(3))
    co = np.zeros(nbt, dtype=np.int32)
    _check(_lib.lk_fold_bin_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(flux), _ptr(err), _ptr(period), _ptr(epoch_time),
                                  float(epoch_phase), _ptr(wrap_phase), int(bool(normalize_phase)), _ptr(cyc_epoch), _ptr(plan),
                                  which_code, _ptr(lay["bin_off"], _c_ip), _ptr(lay["start"]), _ptr(lay["size_sec"]),
                                  _ptr(lay["edges"]), _ptr(po), _ptr(fo), _ptr(eo), _ptr(co, _c_i32p)))
    return dict(phase=po, flux=fo, flux_err=eo, count=co, bin_off=lay["bin_off"])


def river_batch(t, flux, n_off, period, flux_err=None, epoch_time=None, bin_points=1, minimum_phase=-0.5, maximum_phase=0.5,
                method="mean", bins=None, max_output_mb=4096, device=0):
    """River diagrams (cycle x phase images) of B ragged targets on host arrays (``lk_river_plan_batch`` + ``lk_river_batch``).
    Arguments and definition as ``DeviceLightCurveBatch.river``.  Returns dict(river, count: lists of per-target
    (n_cycles_b, n_bins_b) arrays; n_cycles, n_bins, status, cell_off, edges, edge_off, cycle_min, route)."""
    from . import river as rv
    h = Handle.get(device)
    t, flux = _f64(t), _f64(flux)
    n_off = _offsets(n_off, t.size)
    B = n_off.size - 1
    err = None if flux_err is None else _f64(np.broadcast_to(flux_err, t.shape))
    period, bins, code = rv.check_arguments(B, period, bin_points, minimum_phase, maximum_phase, method, bins, has_err=err is not None)
    epoch_given = epoch_time is not None
    epoch = _f64(np.broadcast_to(np.asarray(epoch_time if epoch_given else 0.0, dtype=np.float64), (B,)))
    plan = np.zeros((max(B, 1), rv.NPLAN), dtype=np.float64)
    _check(_lib.lk_river_plan_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(flux), _ptr(err), _ptr(period), _ptr(epoch),
                                    int(epoch_given), _ptr(plan)))
    plan = plan[:B]
    lay = rv.layout(np.diff(n_off), plan, period, bin_points, minimum_phase, maximum_phase, bins, max_output_mb)
    if not epoch_given:
        epoch = _f64(plan[:, 6])
    ncell = int(lay["cell_off"][-1])
    river, count = np.full(max(ncell, 1), np.nan, dtype=np.float64), np.zeros(max(ncell, 1), dtype=np.int32)
    route = np.zeros(max(B, 1), dtype=np.int32)
    _check(_lib.lk_river_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(flux), _ptr(err), _ptr(period), _ptr(epoch),
                               _ptr(np.ascontiguousarray(plan)), code, _ptr(lay["n_bins"], _c_i32p), _ptr(lay["n_cycles"], _c_i32p),
                               _ptr(lay["cell_off"], _c_ip), _ptr(lay["edges"]), _ptr(river), _ptr(count, _c_i32p),
                               _ptr(route, _c_i32p)))
    out = dict(lay)
    out.update(river=rv.split(river[:ncell], lay), count=rv.split(count[:ncell], lay), route=route[:B])
    return out


# --------------------------------------------------------------------------------------------- BLS
def bls_batch(t, y, ivar, n_off, period, duration, oversample=10, use_likelihood=True, device=0):
    """astropy ``bls_fast`` for B ragged targets (inputs already t-min(t), y-median(y), ivar).
    Returns a dict of float64[B, nP] arrays keyed by BLS_FIELDS (transit_time is the phase in (0, period))."""
    h = Handle.get(device)
    t, y, ivar = _f64(t), _f64(y), _f64(ivar)
    n_off = _offsets(n_off, t.size)
    if y.shape != t.shape or ivar.shape != t.shape:
        raise ValueError("t, y, ivar must have the same length")
    period, duration = _f64(period).ravel(), _f64(duration).ravel()
    B, nP = n_off.size - 1, period.size
    out = result_empty((7, B, nP))
    _check(_lib.lk_bls_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(y), _ptr(ivar), _ptr(period), nP,
                             _ptr(duration), duration.size, int(oversample), int(bool(use_likelihood)), _ptr(out)))
    return {k: out[i] for i, k in enumerate(BLS_FIELDS)}


def bls_max_period(duration, oversample=10):
    """The longest period the LDS kernels of ``bls_batch`` take for these durations; longer ones run the (slower, bit-identical)
    global-memory kernel.  Host-only."""
    load_library()
    duration = _f64(np.atleast_1d(duration)).ravel()
    out = ctypes.c_double(0.0)
    _check(_lib.lk_bls_max_period(_ptr(duration), duration.size, int(oversample), ctypes.byref(out)))
    return float(out.value)


def bls_batch_dev(handle, B, n_off_host, t_ptr, y_ptr, ivar_ptr, period_host, period_ptr, duration_host, oversample,
                  use_likelihood, out7_ptr, stream=0):
    n_off_host = np.ascontiguousarray(n_off_host, dtype=np.int64)
    period_host, duration_host = _f64(period_host).ravel(), _f64(duration_host).ravel()
    _check(_lib.lk_bls_batch_dev(handle._h, int(B), _ptr(n_off_host, _c_ip), _vp(t_ptr), _vp(y_ptr), _vp(ivar_ptr),
                                 _ptr(period_host), _vp(period_ptr), period_host.size, _ptr(duration_host),
                                 duration_host.size, int(oversample), int(bool(use_likelihood)), _vp(out7_ptr),
                                 _vp(stream or None)))


# --------------------------------------------------------------------------------------------- regression
def regress_batch(X, y, n_off, err=None, cadence_mask=None, prior_mu=None, prior_sigma=None, sigma=5.0, niters=5,
                  device=0, return_cov=False):
    """RegressionCorrector.correct numerics for B ragged targets sharing K columns.
    X: (sum N, K); returns dict(coefficients[B,K], model[sum N] (median-subtracted), outlier_mask[sum N] bool);
    ``return_cov``: also coefficients_cov[B,K,K] = inverse normal matrix of the last fit (propagate_errors=True)."""
    h = Handle.get(device)
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be 2-D (cadences x regressors)")
    ntot, K = X.shape
    y = _f64(y)
    n_off = _offsets(n_off, ntot)
    if y.shape != (ntot,):
        raise ValueError("y must have one value per row of X")
    B = n_off.size - 1
    err = None if err is None else _f64(np.broadcast_to(err, (ntot,)))
    cm = None if cadence_mask is None else np.ascontiguousarray(cadence_mask, dtype=np.uint8)
    if cm is not None and cm.shape != (ntot,):
        raise ValueError("cadence_mask must have one entry per row of X (got shape %s, need (%d,))" % (cm.shape, ntot))
    if (prior_mu is None) != (prior_sigma is None):
        raise ValueError("Please specify both `prior_mu` and `prior_sigma`")
    if prior_mu is not None:
        prior_mu = _f64(np.broadcast_to(np.asarray(prior_mu, dtype=np.float64), (B, K)))
        prior_sigma = _f64(np.broadcast_to(np.asarray(prior_sigma, dtype=np.float64), (B, K)))
    w = np.empty((B, K), dtype=np.float64)
    model = np.empty(ntot, dtype=np.float64)
    outl = np.empty(ntot, dtype=np.uint8)
    cov = np.empty((B, K, K), dtype=np.float64) if return_cov else None
    _check(_lib.lk_regress_cov_batch(h._h, B, _ptr(n_off, _c_ip), K, _ptr(X), _ptr(y), _ptr(err), _ptr(cm, _c_u8p),
                                     _ptr(prior_mu), _ptr(prior_sigma), float(sigma), int(niters), _ptr(w), _ptr(model),
                                     _ptr(outl, _c_u8p), _ptr(cov)))
    res = dict(coefficients=w, model=model, outlier_mask=outl.astype(bool))
    if return_cov:
        res["coefficients_cov"] = cov
    return res


def regress_shared_batch(X, y, err=None, cadence_mask=None, prior_mu=None, prior_sigma=None, sigma=5.0, niters=5, device=0,
                         want_cov=False):
    """``regress_batch`` for B targets of N cadences that share ONE design matrix ``X`` (N, K), K <= 64: ``y`` (B, N),
    ``err`` / ``cadence_mask`` (B, N) or None, priors (B, K) (or broadcastable to it) or None.  X crosses PCIe once and no
    (B N) x K matrix is ever built.  Returns dict(coefficients[B,K], model[B,N] (median-subtracted), outlier_mask[B,N] bool);
    ``want_cov``: also coefficients_cov[B,K,K]."""
    h = Handle.get(device)
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be 2-D (cadences x regressors)")
    N, K = X.shape
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 2 or y.shape[1] != N:
        raise ValueError("y must be (B, N) with N = len(X) = %d (got shape %s)" % (N, y.shape))
    B = y.shape[0]
    err = None if err is None else np.ascontiguousarray(np.broadcast_to(np.asarray(err, dtype=np.float64), (B, N)))
    cm = None if cadence_mask is None else np.ascontiguousarray(cadence_mask, dtype=np.uint8)
    if cm is not None and cm.shape != (B, N):
        raise ValueError("cadence_mask must be (B, N) = %s (got shape %s)" % ((B, N), cm.shape))
    if (prior_mu is None) != (prior_sigma is None):
        raise ValueError("Please specify both `prior_mu` and `prior_sigma`")
    if prior_mu is not None:
        prior_mu = _f64(np.broadcast_to(np.asarray(prior_mu, dtype=np.float64), (B, K)))
        prior_sigma = _f64(np.broadcast_to(np.asarray(prior_sigma, dtype=np.float64), (B, K)))
    w = np.empty((B, K), dtype=np.float64)
    model = np.empty((B, N), dtype=np.float64)
    outl = np.empty((B, N), dtype=np.uint8)
    cov = np.empty((B, K, K), dtype=np.float64) if want_cov else None
    _check(_lib.lk_regress_shared_batch(h._h, B, N, K, _ptr(X), _ptr(y), _ptr(err), _ptr(cm, _c_u8p), _ptr(prior_mu),
                                        _ptr(prior_sigma), float(sigma), int(niters), _ptr(w), _ptr(model), _ptr(outl, _c_u8p),
                                        _ptr(cov)))
    res = dict(coefficients=w, model=model, outlier_mask=outl.astype(bool))
    if want_cov:
        res["coefficients_cov"] = cov
    return res


def _i32(a, n, name):
    a = np.asarray(a)
    if a.shape != (n,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s must be an integer array of shape (%d,) (got %s of shape %s)" % (name, n, a.dtype, a.shape))
    return np.ascontiguousarray(a, dtype=np.int32)


def align_rows_batch(cadenceno, n_off, grid_cadenceno, want_pos=False, device=0):
    """``CotrendingBasisVectors.align`` as indices: per target sorted ``cadenceno`` (packed, (sum n,)) against the grid's
    strictly increasing ``grid_cadenceno`` (Nx,) -> rows int32 (sum n,); ``want_pos``: also pos int32 (B, Nx), the
    target-relative cadence index at each grid row or -1.  ``ValueError`` naming the target when a cadence is not on the grid."""
    h = Handle.get(device)
    cad = np.asarray(cadenceno)
    n_off = _offsets(n_off, cad.size)
    cad = _i32(cad, cad.size, "cadenceno")
    grid = np.asarray(grid_cadenceno)
    grid = _i32(grid, grid.size, "grid_cadenceno")
    B, Nx = n_off.size - 1, grid.size
    rows = np.empty(cad.size, dtype=np.int32)
    pos = np.empty((B, Nx), dtype=np.int32) if want_pos else None
    _check(_lib.lk_align_rows_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(cad, _c_i32p), Nx, _ptr(grid, _c_i32p), _ptr(rows, _c_i32p),
                                    _ptr(pos, _c_i32p)))
    return (rows, pos) if want_pos else rows


def regress_shared_rows_batch(X, y, n_off, rows, err=None, cadence_mask=None, prior_mu=None, prior_sigma=None, sigma=5.0, niters=5,
                              device=0, want_cov=False):
    """``regress_shared_batch`` for B RAGGED targets on ONE design matrix ``X`` (Nx, K), K <= 64: ``y`` / ``err`` /
    ``cadence_mask`` packed (sum n,) by ``n_off``, ``rows`` int (sum n,) = the row of ``X`` each cadence uses, per target
    strictly increasing.  Per target the numerics are ``RegressionCorrector.correct`` on ``X[rows_b]``.  Returns
    dict(coefficients[B,K], model[sum n] (median-subtracted per target), outlier_mask[sum n] bool); ``want_cov``: also
    coefficients_cov[B,K,K]."""
    h = Handle.get(device)
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be 2-D (grid rows x regressors)")
    Nx, K = X.shape
    y = _f64(y)
    if y.ndim != 1:
        raise ValueError("y must be packed 1-D (sum n,) (got shape %s)" % (y.shape,))
    ntot = y.size
    n_off = _offsets(n_off, ntot)
    B = n_off.size - 1
    rows = _i32(rows, ntot, "rows")
    err = None if err is None else _f64(np.broadcast_to(err, (ntot,)))
    cm = None if cadence_mask is None else np.ascontiguousarray(cadence_mask, dtype=np.uint8)
    if cm is not None and cm.shape != (ntot,):
        raise ValueError("cadence_mask must have one entry per cadence (got shape %s, need (%d,))" % (cm.shape, ntot))
    if (prior_mu is None) != (prior_sigma is None):
        raise ValueError("Please specify both `prior_mu` and `prior_sigma`")
    if prior_mu is not None:
        prior_mu = _f64(np.broadcast_to(np.asarray(prior_mu, dtype=np.float64), (B, K)))
        prior_sigma = _f64(np.broadcast_to(np.asarray(prior_sigma, dtype=np.float64), (B, K)))
    w = np.empty((B, K), dtype=np.float64)
    model = np.empty(ntot, dtype=np.float64)
    outl = np.empty(ntot, dtype=np.uint8)
    cov = np.empty((B, K, K), dtype=np.float64) if want_cov else None
    _check(_lib.lk_regress_shared_rows_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(rows, _c_i32p), Nx, K, _ptr(X), _ptr(y), _ptr(err),
                                             _ptr(cm, _c_u8p), _ptr(prior_mu), _ptr(prior_sigma), float(sigma), int(niters),
                                             _ptr(w), _ptr(model), _ptr(outl, _c_u8p), _ptr(cov)))
    res = dict(coefficients=w, model=model, outlier_mask=outl.astype(bool))
    if want_cov:
        res["coefficients_cov"] = cov
    return res


def ridge_prior_rows_batch(flux_err, n_off, K, alpha, device=0):
    """(prior_mu, prior_sigma), each (B, K), of ``CBVCorrector.correct_gaussian_prior`` for ragged targets: mu = 0 and
    sigma_b = median(flux_err_b) / sqrt(|alpha_b|); ``alpha``: a non-zero scalar or B non-zero penalties."""
    h = Handle.get(device)
    e = _f64(flux_err)
    n_off = _offsets(n_off, e.size)
    B = n_off.size - 1
    mu, sg = np.empty((B, int(K)), dtype=np.float64), np.empty((B, int(K)), dtype=np.float64)
    if np.ndim(alpha) == 0:
        _check(_lib.lk_ridge_prior_rows_batch(h._h, B, _ptr(n_off, _c_ip), int(K), _ptr(e), float(alpha), _ptr(mu), _ptr(sg)))
    else:
        a = _f64(alpha)
        if a.shape != (B,) or not np.all(np.isfinite(a)) or np.any(a == 0.0):
            raise ValueError("alpha must be a scalar or B finite, non-zero penalties")
        _check(_lib.lk_ridge_prior_rows_alphas_batch(h._h, B, _ptr(n_off, _c_ip), int(K), _ptr(e), _ptr(a), _ptr(mu), _ptr(sg)))
    return mu, sg


def pchip_interp_batch(time, n_off, knot_time, Y, knot_keep=None, extrapolate=False, append_constant=False, device=0):
    """``CotrendingBasisVectors.interpolate`` for a ragged batch: the K columns ``Y`` (Nx, K) at ``knot_time`` (Nx,) ->
    (X (sum n, K + append_constant), inside bool (sum n,)) at the packed ``time``; ``knot_keep`` (bool (Nx,), None = all):
    the reference's ``~gap_indicators``.  Outside the kept knots' span: NaN, or scipy's extrapolation with ``extrapolate``.
    The device form of ``correctors.cbvcorrector.interpolate_cbvs``."""
    h = Handle.get(device)
    t = _f64(time)
    if t.ndim != 1:
        raise ValueError("time must be packed 1-D (sum n,) (got shape %s)" % (t.shape,))
    n_off = _offsets(n_off, t.size)
    x = _f64(knot_time)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if x.ndim != 1 or Y.ndim != 2 or Y.shape[0] != x.size:
        raise ValueError("knot_time must be 1-D and Y 2-D with one row per knot (got %s and %s)" % (x.shape, Y.shape))
    keep = None if knot_keep is None else np.ascontiguousarray(knot_keep, dtype=np.uint8)
    if keep is not None and keep.shape != x.shape:
        raise ValueError("knot_keep must have one entry per knot (got shape %s, need %s)" % (keep.shape, x.shape))
    Nx, K = Y.shape
    X = np.empty((t.size, K + int(bool(append_constant))), dtype=np.float64)
    inside = np.empty(t.size, dtype=np.uint8)
    _check(_lib.lk_pchip_interp_batch(h._h, n_off.size - 1, _ptr(n_off, _c_ip), _ptr(t), Nx, K, _ptr(x), _ptr(Y), _ptr(keep, _c_u8p),
                                      int(bool(extrapolate)), int(bool(append_constant)), _ptr(X), _ptr(inside, _c_u8p)))
    return X, inside.astype(bool)


# --------------------------------------------------------------------------------------------- under-fitting metric
def underfit_arguments(B, N, neighbors, cadence_mask=None, Bn=None):
    """The checks of the under-fitting metric that need no device, shared by its front ends: ``neighbors`` -> int32
    (B, M) C-contiguous (-1 = padding, else an index in [0, B) other than the row's own), ``cadence_mask`` (bool (N,), True
    = used) -> ascending int32 indices of the kept cadences, or None for all of them.  ``Bn``: the neighbours are the rows of
    another array of Bn rows: indices in [0, Bn), the row's own number included.  Returns (neighbors, keep_idx, n)."""
    nb = np.asarray(neighbors)
    if nb.size == 0 and nb.ndim == 2:
        nb = nb.astype(np.int32)
    if nb.ndim != 2 or nb.shape[0] != B or not np.issubdtype(nb.dtype, np.integer):
        raise ValueError("neighbors must be an integer array of shape (B, M) = (%d, M) (got %s of shape %s)" % (B, nb.dtype, nb.shape))
    if nb.size:
        rows = B if Bn is None else int(Bn)
        if nb.min() < -1 or nb.max() >= rows:
            raise ValueError("a neighbour is -1 (padding) or an index in [0, %d): got values between %d and %d" % (rows, nb.min(), nb.max()))
        own = np.nonzero(nb == np.arange(B)[:, None]) if Bn is None else ((),)
        if len(own[0]):
            raise ValueError("a target cannot be its own neighbour: row %d lists %d" % (own[0][0], own[0][0]))
    nb = np.ascontiguousarray(nb, dtype=np.int32)
    keep_idx, n = None, int(N)
    if cadence_mask is not None:
        cm = np.asarray(cadence_mask)
        if cm.shape != (N,):
            raise ValueError("cadence_mask must be one bool per cadence, shape (%d,), shared by every target (got shape %s)" % (N, cm.shape))
        keep_idx = np.ascontiguousarray(np.nonzero(cm.astype(bool))[0], dtype=np.int32)
        n = int(keep_idx.size)
    if n < 2:
        raise ValueError("the under-fitting metric needs at least two kept cadences (got %d)" % n)
    return nb, keep_idx, n


def underfit_neighbors_batch(flux, neighbors, cadence_mask=None, device=0):
    """The under-fitting goodness metric (reference metrics.py:141-257, 451-475) of every row of ``flux`` (B, N; NaN-free)
    against its neighbours, which are other rows of ``flux``: ``neighbors`` int (B, M), -1 = padding; ``cadence_mask`` bool
    (N,), True = used.  Returns dict(metric[B], correlations[B, M] (NaN at padding))."""
    flux = np.ascontiguousarray(flux, dtype=np.float64)
    if flux.ndim != 2 or flux.shape[0] < 1:
        raise ValueError("flux must be (B, N) with B >= 1 (got shape %s)" % (flux.shape,))
    B, N = flux.shape
    nb, keep_idx, n = underfit_arguments(B, N, neighbors, cadence_mask)
    if np.isnan(flux).any():
        raise ValueError("the under-fitting metric needs NaN-free flux: drop the NaN cadences of every target first (remove_nans())")
    M = nb.shape[1]
    h = Handle.get(device)
    metric = np.empty(B, dtype=np.float64)
    corr = np.empty((B, M), dtype=np.float64)
    _check(_lib.lk_underfit_neighbors_batch(h._h, B, N, _ptr(flux), n, _ptr(keep_idx, _c_i32p), M, _ptr(nb if M else None, _c_i32p),
                                            _ptr(corr if M else None), _ptr(metric)))
    return dict(metric=metric, correlations=corr)


UNDERFIT_GRID_MAX_NX = 245760   # the largest cadence grid of lk_underfit_grid_* (include/lkhip.h)


def underfit_grid_neighbors_batch(flux, n_off, rows, Nx, neighbors, cadence_mask=None, device=0):
    """The under-fitting metric of B RAGGED light curves on a grid of ``Nx`` cadences (``lk_underfit_grid_neighbors_batch``):
    ``flux`` packed (sum n,) by ``n_off``, NaN-free; ``rows`` int (sum n,) = the grid row of each cadence, per target strictly
    increasing (``align_rows_batch``); ``neighbors`` int (B, M), -1 = padding; ``cadence_mask`` (sum n,) bool, True = used.
    Per target the dots run over the grid rows the target and all of its neighbours have.  Returns dict(metric[B],
    correlations[B, M] (NaN at padding), n_common[B]); fewer than two common cadences: NaN."""
    flux = _f64(flux)
    if flux.ndim != 1:
        raise ValueError("flux must be packed 1-D (sum n,) (got shape %s)" % (flux.shape,))
    ntot = flux.size
    n_off = _offsets(n_off, ntot)
    B, Nx = n_off.size - 1, int(Nx)
    if B < 1 or Nx < 1:
        raise ValueError("need at least one light curve and one grid row (got B=%d, Nx=%d)" % (B, Nx))
    rows = _i32(rows, ntot, "rows")
    nb = underfit_arguments(B, max(Nx, 2), neighbors)[0]
    cm = None if cadence_mask is None else np.ascontiguousarray(cadence_mask, dtype=np.uint8)
    if cm is not None and cm.shape != (ntot,):
        raise ValueError("cadence_mask must have one entry per cadence (got shape %s, need (%d,))" % (cm.shape, ntot))
    if np.isnan(flux).any():
        raise ValueError("the under-fitting metric needs NaN-free flux: drop the NaN cadences of every target first (remove_nans())")
    M = nb.shape[1]
    h = Handle.get(device)
    metric = np.empty(B, dtype=np.float64)
    corr = np.empty((B, M), dtype=np.float64)
    n_common = np.empty(B, dtype=np.int32)
    _check(_lib.lk_underfit_grid_neighbors_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(rows, _c_i32p), Nx, _ptr(flux), _ptr(cm, _c_u8p), M,
                                                 _ptr(nb if M else None, _c_i32p), _ptr(corr if M else None),
                                                 _ptr(n_common, _c_i32p), _ptr(metric)))
    return dict(metric=metric, correlations=corr, n_common=n_common)


# --------------------------------------------------------------------------------------------- over-fitting metric
OVERFIT_SCRATCH_DEFAULT = 4 << 30   # LK_OVERFIT_SCRATCH_DEFAULT in include/lkhip.h


def overfit_grid(frequency):
    """``frequency`` [1/d] -> (f0, df, M) as the LS 'fast' path takes a grid (f0 = frequency[0], df = frequency[1] -
    frequency[0]); ValueError unless it is a regular grid (astropy's ``_is_regular``) of at least two ascending frequencies."""
    from .periodogram import is_regular
    f = np.asarray(frequency, dtype=np.float64)
    if f.ndim != 1 or f.size < 2:
        raise ValueError("the over-fitting metric needs a regular grid of at least two frequencies (got shape %s)" % (f.shape,))
    if not np.all(np.isfinite(f)) or not is_regular(f) or not f[1] > f[0] or f[0] < 0:
        raise ValueError("the over-fitting metric needs a regular, ascending grid of non-negative frequencies in 1/d (the default "
                         "Lomb-Scargle method takes no other)")
    return float(f[0]), float(f[1] - f[0]), int(f.size)


def overfit_default_grid(time):
    """The grid ``LombScarglePeriodogram.from_lightcurve`` builds for a light curve with these (kept) times: amplitude
    normalisation, oversample factor 5, up to the Nyquist frequency (reference periodogram.py:793-798, 850-911) [1/d]."""
    time = np.asarray(time, dtype=np.float64)
    nyquist = 0.5 * (1.0 / np.median(np.diff(time)))
    fs = (1.0 / (time[-1] - time[0])) / 5.0
    return np.arange(fs, nyquist, fs)


def overfit_arguments(N, n_samples=10, cadence_mask=None, frequency=None, seed=0, first_target=0, stream_id=0, B=1):
    """The checks of the over-fitting metric that need no device, shared by its front ends.  Returns (keep_idx or None, n,
    grid or None): ``cadence_mask`` (bool (N,), True = used) -> ascending int32 indices; ``frequency`` -> ``overfit_grid``."""
    if int(n_samples) < 1:
        raise ValueError("n_samples must be >= 1 (got %r)" % (n_samples,))
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed must be in [0, 2^64) (got %r)" % (seed,))
    if int(first_target) < 0 or int(first_target) + int(B) > 1 << 32:
        raise ValueError("first_target + B must stay within 32 bits (got %r + %d)" % (first_target, B))
    if not 0 <= int(stream_id) < 1 << 32:
        raise ValueError("stream_id must be in [0, 2^32) (got %r)" % (stream_id,))
    keep_idx, n = None, int(N)
    if cadence_mask is not None:
        cm = np.asarray(cadence_mask)
        if cm.shape != (N,):
            raise ValueError("cadence_mask must be one bool per cadence, shape (%d,), shared by every target (got shape %s)" % (N, cm.shape))
        keep_idx = np.ascontiguousarray(np.nonzero(cm.astype(bool))[0], dtype=np.int32)
        n = int(keep_idx.size)
    if n < 3:
        raise ValueError("the over-fitting metric needs at least three kept cadences (got %d)" % n)
    return keep_idx, n, (None if frequency is None else overfit_grid(frequency))


def overfit_scratch_bytes(B, n, M, n_samples, max_scratch_bytes=None):
    """(bytes, samples per round) of the caller-owned scratch block of ``lk_overfit_metric_batch_dev``."""
    load_library()
    nbytes, rounds = ctypes.c_int64(0), ctypes.c_int(0)
    _check(_lib.lk_overfit_scratch_bytes(int(B), int(n), int(M), int(n_samples), int(max_scratch_bytes or 0), ctypes.byref(nbytes),
                                         ctypes.byref(rounds)))
    return nbytes.value, rounds.value


def overfit_metric_batch(time, flux, flux_corrected, flux_err_corrected, frequency=None, n_samples=10, cadence_mask=None, seed=0,
                         first_target=0, stream_id=0, device=0, max_scratch_bytes=None):
    """The over-fitting goodness metric (reference metrics.py:24-138) of every row of host arrays ``flux`` / ``flux_corrected``
    / ``flux_err_corrected`` (B, N; NaN-free flux) at ``time`` ((N,) shared, or (B, N)) -> metric[B]; the arguments of
    ``DeviceLightCurveBatch.over_fitting_metric``."""
    y0 = np.ascontiguousarray(flux, dtype=np.float64)
    if y0.ndim != 2 or y0.shape[0] < 1:
        raise ValueError("flux must be (B, N) with B >= 1 (got shape %s)" % (y0.shape,))
    B, N = y0.shape
    y1 = np.ascontiguousarray(flux_corrected, dtype=np.float64)
    if flux_err_corrected is None:
        raise ValueError("the over-fitting metric needs the flux errors of the corrected light curves")
    e1 = np.ascontiguousarray(np.broadcast_to(np.asarray(flux_err_corrected, dtype=np.float64), y0.shape))
    if y1.shape != y0.shape:
        raise ValueError("flux and flux_corrected must have one shape (got %s and %s)" % (y0.shape, y1.shape))
    t = np.asarray(time, dtype=np.float64)
    if t.shape not in ((N,), (B, N)):
        raise ValueError("time must be (N,) or (B, N) = (%d,) or (%d, %d) (got shape %s)" % (N, B, N, t.shape))
    keep_idx, n, grid = overfit_arguments(N, n_samples, cadence_mask, frequency, seed, first_target, stream_id, B)
    if np.isnan(y0).any() or np.isnan(y1).any():
        raise ValueError("the over-fitting metric needs NaN-free flux: drop the NaN cadences of every target first (remove_nans())")
    t = np.ascontiguousarray(np.broadcast_to(t, (B, N)))
    if grid is None:
        grid = overfit_grid(overfit_default_grid(t[0] if keep_idx is None else t[0, keep_idx]))
    h = Handle.get(device)
    metric = np.empty(B, dtype=np.float64)
    _check(_lib.lk_overfit_metric_batch(h._h, B, N, _ptr(t), _ptr(y0), _ptr(y1), _ptr(e1), n, _ptr(keep_idx, _c_i32p), grid[0],
                                        grid[1], grid[2], int(n_samples), int(seed), int(first_target), int(stream_id),
                                        int(max_scratch_bytes or 0), _ptr(metric)))
    return metric


def overfit_rows_arguments(n_off, n_samples=10, cadence_mask=None, frequency=None, seed=0, first_target=0, stream_id=0):
    """``overfit_arguments`` for a ragged batch with offsets ``n_off``: ``cadence_mask`` (bool (sum n,), True = used) ->
    (keep_idx: target-relative ascending int32 indices packed by k_off, or None for all cadences; k_off int64 (B + 1,); grid or
    None).  ``ValueError`` naming the first target with fewer than three kept cadences."""
    n_off = np.ascontiguousarray(n_off, dtype=np.int64)
    B, ntot = n_off.size - 1, int(n_off[-1])
    overfit_arguments(3, n_samples, None, None, seed, first_target, stream_id, B)
    keep_idx, k_off = None, n_off
    if cadence_mask is not None:
        cm = np.asarray(cadence_mask)
        if cm.shape != (ntot,):
            raise ValueError("cadence_mask of a ragged batch must be one bool per cadence of the batch, shape (%d,) (got shape %s)"
                             % (ntot, cm.shape))
        idx = np.nonzero(cm.astype(bool))[0]
        tgt = np.searchsorted(n_off, idx, side="right") - 1
        keep_idx = np.ascontiguousarray(idx - n_off[tgt], dtype=np.int32)
        k_off = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=B)[:B])]).astype(np.int64)
    few = np.nonzero(np.diff(k_off) < 3)[0]
    if len(few):
        raise ValueError("target %d: the over-fitting metric needs at least three kept cadences (got %d)"
                         % (few[0], np.diff(k_off)[few[0]]))
    return keep_idx, k_off, (None if frequency is None else overfit_grid(frequency))


def overfit_scratch_rows_bytes(k_off, M, n_samples, max_scratch_bytes=None):
    """(bytes, samples per round) of the caller-owned block of ``lk_overfit_metric_rows_batch_dev`` / of a rows session."""
    load_library()
    k_off = np.ascontiguousarray(k_off, dtype=np.int64)
    nbytes, rounds = ctypes.c_int64(0), ctypes.c_int(0)
    _check(_lib.lk_overfit_scratch_rows_bytes(k_off.size - 1, _ptr(k_off, _c_ip), int(M), int(n_samples), int(max_scratch_bytes or 0),
                                              ctypes.byref(nbytes), ctypes.byref(rounds)))
    return nbytes.value, rounds.value


def overfit_metric_rows_batch(time, flux, flux_corrected, flux_err_corrected, n_off, frequency=None, n_samples=10, cadence_mask=None,
                              seed=0, first_target=0, stream_id=0, device=0, max_scratch_bytes=None):
    """The over-fitting goodness metric of B RAGGED light curves packed by ``n_off`` (``lk_overfit_metric_rows_batch``): ``time``,
    ``flux``, ``flux_corrected``, ``flux_err_corrected`` (sum n,), NaN-free flux; ``cadence_mask`` bool (sum n,), True = used;
    ``frequency`` None = the default grid of target 0's kept times -> metric[B]."""
    t = _f64(time)
    if t.ndim != 1:
        raise ValueError("time must be packed 1-D (sum n,) (got shape %s)" % (t.shape,))
    n_off = _offsets(n_off, t.size)
    if n_off.size < 2:
        raise ValueError("need at least one light curve")
    y0, y1 = _f64(flux), _f64(flux_corrected)
    if flux_err_corrected is None:
        raise ValueError("the over-fitting metric needs the flux errors of the corrected light curves")
    e1 = _f64(np.broadcast_to(np.asarray(flux_err_corrected, dtype=np.float64), t.shape))
    if y0.shape != t.shape or y1.shape != t.shape:
        raise ValueError("time, flux and flux_corrected must have one shape (got %s, %s and %s)" % (t.shape, y0.shape, y1.shape))
    keep_idx, k_off, grid = overfit_rows_arguments(n_off, n_samples, cadence_mask, frequency, seed, first_target, stream_id)
    if np.isnan(y0).any() or np.isnan(y1).any():
        raise ValueError("the over-fitting metric needs NaN-free flux: drop the NaN cadences of every target first (remove_nans())")
    if grid is None:
        t0 = t[:n_off[1]]
        grid = overfit_grid(overfit_default_grid(t0 if keep_idx is None else t0[keep_idx[:k_off[1]]]))
    h = Handle.get(device)
    B = n_off.size - 1
    metric = np.empty(B, dtype=np.float64)
    _check(_lib.lk_overfit_metric_rows_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(y0), _ptr(y1), _ptr(e1), _ptr(keep_idx, _c_i32p),
                                             _ptr(k_off if keep_idx is not None else None, _c_ip), grid[0], grid[1], grid[2],
                                             int(n_samples), int(seed), int(first_target), int(stream_id),
                                             int(max_scratch_bytes or 0), _ptr(metric)))
    return metric


# --------------------------------------------------------------------------------------------- flatten
def savgol_design(window, polyorder):
    """(taps[window], edge[2, window//2, window]) exactly as the kernel uses them (host-only, no GPU needed)."""
    load_library()
    half = window // 2
    c = np.empty(window, dtype=np.float64)
    e = np.empty((2, half, window), dtype=np.float64)
    _check(_lib.lk_savgol_design(int(window), int(polyorder), _ptr(c), _ptr(e)))
    return c, e


def savgol_trend_batch(t, flux, n_off, mask=None, window_length=101, polyorder=2, break_tolerance=5, niters=3,
                       sigma=3, return_fit_mask=False, device=0):
    """The trend LightCurve.flatten divides by, for B ragged targets.  ``mask``: True = exclude from the fit."""
    h = Handle.get(device)
    t, flux = _f64(t), _f64(flux)
    n_off = _offsets(n_off, t.size)
    if flux.shape != t.shape:
        raise ValueError("t and flux must have the same length")
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    if m is not None and m.shape != t.shape:
        raise ValueError("mask must have one entry per cadence (got shape %s, need %s)" % (m.shape, t.shape))
    bt = float("nan") if break_tolerance is None else float(break_tolerance)
    trend = result_empty(t.size)
    fm = np.empty(t.size, dtype=np.uint8) if return_fit_mask else None
    _check(_lib.lk_savgol_trend_batch(h._h, n_off.size - 1, _ptr(n_off, _c_ip), _ptr(t), _ptr(flux), _ptr(m, _c_u8p),
                                      int(window_length), int(polyorder), bt, int(niters), float(sigma), _ptr(trend),
                                      _ptr(fm, _c_u8p)))
    return (trend, fm.astype(bool)) if return_fit_mask else trend


# --------------------------------------------------------------------------------------------- PLD design matrix
def pld_design_width(P, Pb, pld_order, pca_components, n_knots):
    load_library()
    return int(_lib.lk_pld_design_width(int(P), int(Pb), int(pld_order), int(pca_components), int(n_knots)))


def pld_design_batch(pld_pix, bkg_pix, lc_flux, time, knots, pld_order, pca_components, spline_degree,
                     normalize_bkg=True, device=0):
    """PLD design matrices for B same-shaped cutouts.  pld_pix (B, N, P) or None, bkg_pix (B, N, Pb), lc_flux (B, N)
    float32; time (B, N); knots (B, n_inner + 2) = [min t, interior knots, max t].
    Returns (X[B, N, K], prior_sigma[B, K])."""
    h = Handle.get(device)
    bkg_pix = np.ascontiguousarray(bkg_pix, dtype=np.float32)
    B, N, Pb = bkg_pix.shape
    P = 0
    if pld_pix is not None and np.size(pld_pix):
        pld_pix = np.ascontiguousarray(pld_pix, dtype=np.float32)
        if pld_pix.ndim != 3 or pld_pix.shape[:2] != (B, N):
            raise ValueError("pld_pix must be (B, N, P) with the B, N of bkg_pix (got %s)" % (pld_pix.shape,))
        P = pld_pix.shape[2]
    else:
        pld_pix = None
    lc_flux = np.ascontiguousarray(lc_flux, dtype=np.float32)
    time, knots = _f64(time), _f64(knots)
    if lc_flux.shape != (B, N) or time.shape != (B, N) or knots.shape[0] != B:
        raise ValueError("inconsistent PLD batch shapes")
    n_inner = knots.shape[1] - 2
    n_knots = n_inner + int(spline_degree) + 1
    K = pld_design_width(P, Pb, pld_order, pca_components, n_knots)
    X = np.empty((B, N, K), dtype=np.float64)
    ps = np.empty((B, K), dtype=np.float64)
    _check(_lib.lk_pld_design_batch(h._h, B, N, P, Pb, _ptr(pld_pix, _c_fp), _ptr(bkg_pix, _c_fp), _ptr(lc_flux, _c_fp),
                                    _ptr(time), _ptr(knots), n_inner, int(pld_order), int(pca_components), n_knots,
                                    int(spline_degree), int(bool(normalize_bkg)), K, _ptr(X), _ptr(ps)))
    return X, ps


def pld_correct_batch(pld_pix, bkg_pix, lc_flux, time, knots, y, err, pld_order, pca_components, spline_degree,
                      normalize_bkg=True, cadence_mask=None, sigma=5.0, niters=5, want_spline=True, device=0,
                      p_count=None, pb_count=None):
    """``PLDCorrector.correct`` numerics for B same-shaped cutouts in ONE call (design matrices, regression + clip loop, the
    spline block's share of the model); the design matrices stay in device memory.  Inputs as ``pld_design_batch`` plus
    y / err (B, N) float64 = the SAP light curve; pass the SAME array as ``pld_pix`` and ``bkg_pix`` when both apertures
    are equal (uploaded once).  Returns dict(coefficients[B, K], model[B, N] (median removed), outlier_mask[B, N] bool,
    spline[B, N] or None).  ``p_count`` / ``pb_count`` (int32[B], either may be None): ragged pixel blocks — cutout b's first
    p_count[b] / pb_count[b] columns are pixels, the rest of the row is +0.0 (``lk_pld_correct_ragged_batch``)."""
    h = Handle.get(device)
    same = pld_pix is bkg_pix
    bkg_pix = np.ascontiguousarray(bkg_pix, dtype=np.float32)
    B, N, Pb = bkg_pix.shape
    P = 0
    if pld_pix is not None and np.size(pld_pix):
        pld_pix = bkg_pix if same else np.ascontiguousarray(pld_pix, dtype=np.float32)
        if pld_pix.ndim != 3 or pld_pix.shape[:2] != (B, N):
            raise ValueError("pld_pix must be (B, N, P) with the B, N of bkg_pix (got %s)" % (pld_pix.shape,))
        P = pld_pix.shape[2]
    else:
        pld_pix = None
    lc_flux = np.ascontiguousarray(lc_flux, dtype=np.float32)
    time, knots, y = _f64(time), _f64(knots), _f64(y)
    err = None if err is None else _f64(err)
    if lc_flux.shape != (B, N) or time.shape != (B, N) or knots.shape[0] != B or y.shape != (B, N) or (
            err is not None and err.shape != (B, N)):
        raise ValueError("inconsistent PLD batch shapes")
    cm = None if cadence_mask is None else np.ascontiguousarray(cadence_mask, dtype=np.uint8)
    if cm is not None and cm.shape != (B, N):
        raise ValueError("cadence_mask must be (B, N)")
    n_inner = knots.shape[1] - 2
    n_knots = n_inner + int(spline_degree) + 1
    K = pld_design_width(P, Pb, pld_order, pca_components, n_knots)
    w = np.empty((B, K), dtype=np.float64)
    model = np.empty((B, N), dtype=np.float64)
    outl = np.empty((B, N), dtype=np.uint8)
    sp = np.empty((B, N), dtype=np.float64) if want_spline else None
    if p_count is not None or pb_count is not None:
        pc = None if p_count is None else np.ascontiguousarray(p_count, dtype=np.int32)
        bc = None if pb_count is None else np.ascontiguousarray(pb_count, dtype=np.int32)
        if any(c is not None and c.shape != (B,) for c in (pc, bc)):
            raise ValueError("p_count / pb_count must hold one count per cutout")
        _check(_lib.lk_pld_correct_ragged_batch(
            h._h, B, N, P, Pb, _ptr(pld_pix, _c_fp), _ptr(bkg_pix, _c_fp), _ptr(lc_flux, _c_fp), _ptr(time), _ptr(knots), n_inner,
            int(pld_order), int(pca_components), n_knots, int(spline_degree), int(bool(normalize_bkg)), K, _ptr(y), _ptr(err),
            _ptr(cm, _c_u8p), float(sigma), int(niters), _ptr(w), _ptr(model), _ptr(outl, _c_u8p), _ptr(sp),
            _ptr(pc, _c_i32p), _ptr(bc, _c_i32p)))
        return dict(coefficients=w, model=model, outlier_mask=outl.astype(bool), spline=sp)
    _check(_lib.lk_pld_correct_batch(h._h, B, N, P, Pb, _ptr(pld_pix, _c_fp), _ptr(bkg_pix, _c_fp), _ptr(lc_flux, _c_fp),
                                     _ptr(time), _ptr(knots), n_inner, int(pld_order), int(pca_components), n_knots,
                                     int(spline_degree), int(bool(normalize_bkg)), K, _ptr(y), _ptr(err), _ptr(cm, _c_u8p),
                                     float(sigma), int(niters), _ptr(w), _ptr(model), _ptr(outl, _c_u8p), _ptr(sp)))
    return dict(coefficients=w, model=model, outlier_mask=outl.astype(bool), spline=sp)


# --------------------------------------------------------------------------------------------- design-matrix operations
def pca_batch(A, nterms, device=0):
    """``DesignMatrix.pca`` (reference correctors/designmatrix.py:252-282) for B same-shaped matrices: A (B, N, P) or (N, P)
    -> the first ``nterms`` left singular vectors of each column-centred matrix, (B, N, nterms) / (N, nterms)."""
    h = Handle.get(device)
    A = np.ascontiguousarray(A, dtype=np.float64)
    single = A.ndim == 2
    if single:
        A = A[None]
    if A.ndim != 3:
        raise ValueError("A must be (B, N, P) or (N, P)")
    B, N, P = A.shape
    k = int(nterms)
    U = np.empty((B, N, k), dtype=np.float64)
    _check(_lib.lk_pca_batch(h._h, B, N, P, k, _ptr(A), _ptr(U)))
    return U[0] if single else U


def spline_basis_batch(x, knots, degree=3, device=0):
    """Clamped B-spline basis (patsy ``bs(x, knots=..., degree, include_intercept=True)``) of x (B, N) or (N,) on
    knots (B, n_inner + 2) / (n_inner + 2,) = [lower bound, interior knots, upper bound] -> (B, N, n_inner + degree + 1)."""
    h = Handle.get(device)
    x, knots = _f64(x), _f64(knots)
    single = x.ndim == 1
    if single:
        x, knots = x[None], knots[None]
    B, N = x.shape
    if knots.ndim != 2 or knots.shape[0] != B or knots.shape[1] < 2:
        raise ValueError("knots must be (B, n_inner + 2)")
    n_inner = knots.shape[1] - 2
    out = np.empty((B, N, n_inner + int(degree) + 1), dtype=np.float64)
    _check(_lib.lk_spline_basis_batch(h._h, B, N, _ptr(x), _ptr(knots), n_inner, int(degree), _ptr(out)))
    return out[0] if single else out


def standardize_batch(A, device=0):
    """``DesignMatrix.standardize`` (reference correctors/designmatrix.py:215-250): A (B, N, P) or (N, P) -> same shape."""
    h = Handle.get(device)
    A = np.ascontiguousarray(A, dtype=np.float64)
    single = A.ndim == 2
    if single:
        A = A[None]
    B, N, P = A.shape
    out = np.empty_like(A)
    _check(_lib.lk_standardize_batch(h._h, B, N, P, _ptr(A), _ptr(out)))
    return out[0] if single else out


# --------------------------------------------------------------------------------------------- batch ingest (N4)
def sigma_clip_batch(y, n_off, sigma=5.0, maxiters=5, device=0):
    """astropy.stats.sigma_clip(y_b, sigma, maxiters).mask for B ragged arrays -> bool[sum N] (True = clipped / non-finite)."""
    h = Handle.get(device)
    y = _f64(y)
    n_off = _offsets(n_off, y.size)
    out = np.zeros(y.size, dtype=np.uint8)
    _check(_lib.lk_sigma_clip_batch(h._h, n_off.size - 1, _ptr(n_off, _c_ip), _ptr(y), float(sigma), int(maxiters),
                                    _ptr(out, _c_u8p)))
    return out.astype(bool)


def clip_bounds(sigma=5.0, sigma_lower=None, sigma_upper=None, maxiters=5):
    """(sigma_lower, sigma_upper, maxiters) as the C ABI takes them: ``None`` bounds fall back to ``sigma`` (astropy's
    rule), ``maxiters=None`` ("until nothing changes") becomes -1."""
    lo = float(sigma if sigma_lower is None else sigma_lower)
    hi = float(sigma if sigma_upper is None else sigma_upper)
    if np.isnan(lo) or np.isnan(hi):
        raise ValueError("sigma, sigma_lower and sigma_upper must not be NaN")
    if maxiters is None:
        return lo, hi, -1
    if int(maxiters) < 0:
        raise ValueError("maxiters must be >= 0 or None (got %r)" % (maxiters,))
    return lo, hi, int(maxiters)


def outlier_mask_batch(y, n_off, sigma=5.0, sigma_lower=None, sigma_upper=None, maxiters=5, device=0):
    """astropy.stats.sigma_clip(y_b, sigma, sigma_lower, sigma_upper, maxiters).mask for B ragged arrays -> bool[sum N]
    (True = clipped / non-finite); ``maxiters=None``: until a round removes nothing."""
    lo, hi, mi = clip_bounds(sigma, sigma_lower, sigma_upper, maxiters)
    h = Handle.get(device)
    y = _f64(y)
    n_off = _offsets(n_off, y.size)
    out = np.zeros(y.size, dtype=np.uint8)
    _check(_lib.lk_outlier_mask_batch(h._h, n_off.size - 1, _ptr(n_off, _c_ip), _ptr(y), lo, hi, mi, _ptr(out, _c_u8p)))
    return out.astype(bool)


def cdpp_batch(flat_flux, n_off, outlier=None, transit_duration=13, device=0):
    """The tail of ``LightCurve.estimate_cdpp`` (reference lightcurve.py:1764-1833) for B ragged, already flattened rows:
    ppm of the cadences ``outlier`` (bool / uint8 over all cadences, None: none) leaves, running mean over
    ``transit_duration`` cadences, np.std -> float64[B] (NaN for a row with nothing left)."""
    if not isinstance(transit_duration, (int, np.integer)) or isinstance(transit_duration, bool):
        raise ValueError("transit_duration must be an integer in units number of cadences, got {}.".format(transit_duration))
    if transit_duration < 1:
        raise ValueError("transit_duration must be >= 1 cadence (got %d)" % transit_duration)
    y = _f64(flat_flux)
    n_off = _offsets(n_off, y.size)
    B = n_off.size - 1
    m = None
    if outlier is not None:
        m = np.ascontiguousarray(outlier, dtype=np.uint8)
        if m.shape != y.shape:
            raise ValueError("outlier must have one entry per cadence (got shape %s, need %s)" % (m.shape, y.shape))
    h = Handle.get(device)
    out = np.empty(B, dtype=np.float64)
    _check(_lib.lk_cdpp_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(y), None if m is None else _ptr(m, _c_u8p),
                              int(transit_duration), _ptr(out)))
    return out


def _i32_column(a, n, name):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.shape != (n,):
        raise ValueError("%s must have one entry per cadence (got shape %s, need (%d,))" % (name, a.shape, n))
    return a


def fill_gaps_plan_batch(time, flux, n_off, cadenceno=None, device=0):
    """The plan of ``LightCurve.fill_gaps`` for B ragged light curves without NaN flux (``lk_fill_gaps_plan_batch``):
    -> (stats float64[B, 4] = m, mu, sd, n_inserted; pos int32[sum n] = where every original lands in its filled light curve;
    new_off int64[B + 1]).  ``cadenceno`` (int32 per cadence) selects the reference's cadence path, None its time path."""
    h = Handle.get(device)
    time, flux = _f64(time), _f64(flux)
    n_off = _offsets(n_off, time.size)
    if flux.shape != time.shape:
        raise ValueError("time and flux must have the same length")
    cad = _i32_column(cadenceno, time.size, "cadenceno")
    B = n_off.size - 1
    stats, pos, new_off = np.zeros((B, 4)), np.zeros(time.size, dtype=np.int32), np.zeros(B + 1, dtype=np.int64)
    _check(_lib.lk_fill_gaps_plan_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(time), _ptr(flux),
                                        None if cad is None else _ptr(cad, _c_i32p), _ptr(stats), _ptr(pos, _c_i32p),
                                        _ptr(new_off, _c_ip)))
    return stats, pos, new_off


def fill_gaps_batch(time, flux, n_off, stats, pos, new_off, noise_mean, noise_std, flux_err=None, quality=None, cadenceno=None,
                    seed=0, first_target=0, stream_id=0, device=0):
    """The filled columns of ``LightCurve.fill_gaps`` from ``fill_gaps_plan_batch``'s results (``lk_fill_gaps_batch``): inserted
    cadence j of light curve b gets flux ``noise_mean[b] + noise_std[b] * normal_j`` (Philox stream (seed, first_target + b,
    stream_id)), flux_err linear in time, quality 65536.  -> dict(time, flux, flux_err, quality, cadenceno (None where the input
    has none), inserted bool, n_off)."""
    h = Handle.get(device)
    time, flux = _f64(time), _f64(flux)
    n_off = _offsets(n_off, time.size)
    B, n = n_off.size - 1, time.size
    new_off = np.ascontiguousarray(new_off, dtype=np.int64)
    stats, pos = _f64(stats), np.ascontiguousarray(pos, dtype=np.int32)
    nm, ns = _f64(noise_mean), _f64(noise_std)
    if flux.shape != time.shape or pos.shape != time.shape or new_off.shape != (B + 1,) or stats.size != 4 * B:
        raise ValueError("time, flux, pos must have one length and stats / new_off one row per light curve")
    if nm.shape != (B,) or ns.shape != (B,):
        raise ValueError("noise_mean and noise_std must hold one value per light curve")
    err = None if flux_err is None else _f64(flux_err)
    if err is not None and err.shape != time.shape:
        raise ValueError("flux_err must have the length of time")
    q, cad = _i32_column(quality, n, "quality"), _i32_column(cadenceno, n, "cadenceno")
    nn = int(new_off[-1]) if B else 0
    out = {"time": np.empty(nn), "flux": np.empty(nn), "flux_err": None if err is None else np.empty(nn),
           "quality": None if q is None else np.empty(nn, dtype=np.int32),
           "cadenceno": None if cad is None else np.empty(nn, dtype=np.int32), "inserted": np.zeros(nn, dtype=np.uint8)}
    opt = lambda a, typ=_c_dp: None if a is None else _ptr(a, typ)     # noqa: E731
    _check(_lib.lk_fill_gaps_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(new_off, _c_ip), _ptr(time), _ptr(flux), opt(err),
                                   opt(q, _c_i32p), opt(cad, _c_i32p), _ptr(stats), _ptr(pos, _c_i32p), _ptr(nm), _ptr(ns),
                                   int(seed), int(first_target), int(stream_id), _ptr(out["time"]), _ptr(out["flux"]),
                                   opt(out["flux_err"]), opt(out["quality"], _c_i32p), opt(out["cadenceno"], _c_i32p),
                                   _ptr(out["inserted"], _c_u8p)))
    out["inserted"] = out["inserted"].astype(bool)
    out["n_off"] = new_off
    return out


def ingest_batch(t, flux, n_off, flux_err=None, normalize=True, device=0):
    """remove_nans (+ normalize) for B ragged light curves.  Returns (t, flux, flux_err or None, new_off, median[B])."""
    h = Handle.get(device)
    t, flux = _f64(t), _f64(flux)
    n_off = _offsets(n_off, t.size)
    if flux.shape != t.shape:
        raise ValueError("t and flux must have the same length")
    err = None if flux_err is None else _f64(np.broadcast_to(flux_err, t.shape))
    B = n_off.size - 1
    to, fo = np.empty_like(t), np.empty_like(t)
    eo = np.empty_like(t) if err is not None else None
    new_off = np.zeros(B + 1, dtype=np.int64)
    med = np.empty(B, dtype=np.float64)
    _check(_lib.lk_ingest_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(flux), _ptr(err), int(bool(normalize)), _ptr(to),
                                _ptr(fo), _ptr(eo), _ptr(new_off, _c_ip), _ptr(med)))
    k = int(new_off[-1])
    return to[:k], fo[:k], (eo[:k] if eo is not None else None), new_off, med


def fits_unpack_batch(raws, descs, bitmasks, device=0):
    """FITS binary tables -> packed (time, flux, flux_err, quality, n_off) for B files (see lightkurve_amd/fitsio.py).
    ``raws``: list of uint8 arrays (rows x record bytes, as in the file); ``descs``: B x 10 int32 (fitsio.lightcurve_columns);
    ``bitmasks``: B ints.  Rows with NaN time or (quality & bitmask) != 0 are dropped on the device."""
    h = Handle.get(device)
    B = len(raws)
    desc = np.ascontiguousarray(descs, dtype=np.int32).reshape(B, 10)
    mask = np.ascontiguousarray(bitmasks, dtype=np.int64).reshape(B)
    raw_off = np.zeros(B + 1, dtype=np.int64)
    for b, r in enumerate(raws):
        nbytes = int(desc[b, 0]) * int(desc[b, 1])
        if np.asarray(r).size != nbytes:
            raise ValueError("file %d: %d bytes of table data, descriptor says %d rows x %d bytes" % (b, np.asarray(r).size, desc[b, 1], desc[b, 0]))
        raw_off[b + 1] = raw_off[b] + ((nbytes + 3 + 15) // 16) * 16   # 3 spare bytes, then 16-byte alignment
    raw = np.zeros(int(raw_off[-1]), dtype=np.uint8)
    for b, r in enumerate(raws):
        raw[raw_off[b]:raw_off[b] + np.asarray(r).size] = np.asarray(r, dtype=np.uint8).reshape(-1)
    rows = int(desc[:, 1].sum())
    t, f, e = (np.empty(rows, dtype=np.float64) for _ in range(3))
    q = np.empty(rows, dtype=np.int32)
    new_off = np.zeros(B + 1, dtype=np.int64)
    _check(_lib.lk_fits_unpack_batch(h._h, B, _ptr(raw, _c_u8p), _ptr(raw_off, _c_ip), _ptr(desc, _c_i32p), _ptr(mask, _c_ip),
                                     _ptr(t), _ptr(f), _ptr(e), _ptr(q, _c_i32p), _ptr(new_off, _c_ip)))
    k = int(new_off[-1])
    return t[:k], f[:k], e[:k], q[:k], new_off


def fits_cadenceno_batch(raws, descs, cols, bitmasks, new_off, device=0):
    """One integer column (CADENCENO) of the tables ``fits_unpack_batch`` decoded, for the rows it kept -> int32[new_off[-1]].
    ``raws`` / ``descs`` / ``bitmasks`` as there; ``cols``: B x (byte offset, TFORM code 2..5) (fitsio.int_column); ``new_off``:
    the offsets ``fits_unpack_batch`` returned.  The tables are packed back to back: this call needs no padding."""
    h = Handle.get(device)
    B = len(raws)
    desc = np.ascontiguousarray(descs, dtype=np.int32).reshape(B, 10)
    col = np.ascontiguousarray(cols, dtype=np.int32).reshape(B, 2)
    mask = np.ascontiguousarray(bitmasks, dtype=np.int64).reshape(B)
    new_off = np.ascontiguousarray(new_off, dtype=np.int64)
    if new_off.shape != (B + 1,):
        raise ValueError("new_off must be the B + 1 offsets fits_unpack_batch returned")
    flat = [np.asarray(r, dtype=np.uint8).reshape(-1) for r in raws]
    for b, r in enumerate(flat):
        if r.size != int(desc[b, 0]) * int(desc[b, 1]):
            raise ValueError("file %d: %d bytes of table data, descriptor says %d rows x %d bytes" % (b, r.size, desc[b, 1], desc[b, 0]))
    raw_off = np.zeros(B + 1, dtype=np.int64)
    raw_off[1:] = np.cumsum([r.size for r in flat])
    raw = np.concatenate(flat) if B else np.zeros(0, dtype=np.uint8)
    if raw.size == 0:
        raw = np.zeros(1, dtype=np.uint8)       # (a non-NULL pointer for a batch of empty tables)
    c = np.empty(max(int(new_off[-1]), 1) if B else 1, dtype=np.int32)
    _check(_lib.lk_fits_cadenceno_batch(h._h, B, _ptr(raw, _c_u8p), _ptr(raw_off, _c_ip), _ptr(desc, _c_i32p), _ptr(col, _c_i32p),
                                        _ptr(mask, _c_ip), _ptr(new_off, _c_ip), _ptr(c, _c_i32p)))
    return c[:int(new_off[-1])] if B else c[:0]


def fits_unpack_cube(raw, off_time, code_time, off_quality, code_quality, bitmask, keep_nan_time, col_offsets, npix, device=0):
    """One target-pixel file's table -> (time[k], quality[k], cubes[ncols, k, npix] float32) for the kept cadences."""
    h = Handle.get(device)
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    n_rows, row_bytes = raw.shape
    cols = np.ascontiguousarray(col_offsets, dtype=np.int32)
    ncols = cols.size
    t = np.empty(n_rows, dtype=np.float64)
    q = np.empty(n_rows, dtype=np.int32)
    cubes = np.empty((ncols, n_rows, npix), dtype=np.float32)
    kept = np.zeros(1, dtype=np.int64)
    _check(_lib.lk_fits_unpack_cube(h._h, _ptr(raw.reshape(-1), _c_u8p), int(row_bytes), int(n_rows), int(off_time), int(code_time),
                                    int(off_quality), int(code_quality), ctypes.c_int64(int(bitmask)), int(bool(keep_nan_time)),
                                    int(ncols), _ptr(cols, _c_i32p), int(npix), _ptr(t), _ptr(q, _c_i32p),
                                    cubes.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _ptr(kept, _c_ip)))
    k = int(kept[0])
    return t[:k], q[:k], cubes[:, :k, :]


BLS_NSTATS = 16                # LK_BLS_NSTATS (include/lkhip.h): columns of lk_bls_stats_batch's stats
_BLS_STAT_PAIRS = (("depth", 0), ("depth_phased", 2), ("depth_half", 4), ("depth_odd", 6), ("depth_even", 8))


def bls_stats_arguments(B, period, duration, transit_time):
    """The per-target box of ``lk_bls_stats_batch``: each of ``period`` / ``duration`` / ``transit_time`` a scalar or one value
    per target -> three float64[B]; positive finite periods and durations with duration < period, or ``ValueError``."""
    out = []
    for name, a in (("period", period), ("duration", duration), ("transit_time", transit_time)):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.size != B):
            raise ValueError("%s must be a scalar or one value per light curve (%d), got shape %r" % (name, B, a.shape))
        out.append(np.ascontiguousarray(np.broadcast_to(a, (B,))))
    period, duration, transit_time = out
    if not (np.all(np.isfinite(period)) and np.all(np.isfinite(duration)) and np.all(np.isfinite(transit_time))):
        raise ValueError("period, duration and transit_time must be finite")
    if not (np.all(period > 0) and np.all(duration > 0)):
        raise ValueError("period and duration must be positive")
    return period, duration, transit_time


def bls_stats_slots(t_first, t_last, period):
    """tr_off[B + 1]: target b's per-transit slot holds floor((t_last - t_first) / period) + 3 entries, which covers every
    transit id a box of that period can give to cadences between its first and last time."""
    span = np.maximum(np.asarray(t_last, dtype=np.float64) - np.asarray(t_first, dtype=np.float64), 0.0)
    cap = np.floor(span / period) + 3
    if len(cap) and not cap.max() < 2 ** 31:
        raise ValueError("a period of %g d gives more than 2^31 transits over the light curve" % float(period[np.argmax(cap)]))
    tr_off = np.zeros(len(cap) + 1, dtype=np.int64)
    tr_off[1:] = np.cumsum(cap.astype(np.int64))
    return tr_off


def bls_stats_dict(stats, tr_first, tr_n, tr_off, tr_count, tr_ll, period, transit_time, t_first):
    """The raw outputs of ``lk_bls_stats_batch`` -> the dict of ``DeviceBLSResult.compute_stats``: the slots compacted into
    packed per-transit arrays (``transit_off[B + 1]``), transit times absolute, formed like the reference's
    (period * id + (transit_time - t[0])) + t[0]).  ``tr_n = -1`` (ids that do not fit their slot): ``RuntimeError``."""
    B = len(tr_n)
    if np.any(tr_n < 0):
        raise RuntimeError("light curve %d: the transit ids do not fit the per-transit slot" % int(np.argmax(tr_n < 0)))
    out = {k: np.ascontiguousarray(stats[:, c:c + 2]) for k, c in _BLS_STAT_PAIRS}
    out["harmonic_amplitude"] = stats[:, 10].copy()
    out["harmonic_delta_log_likelihood"] = stats[:, 11].copy()
    n_tr = tr_n.astype(np.int64)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(n_tr)
    src = np.repeat(tr_off[:-1] - off[:-1], n_tr) + np.arange(off[-1])        # slot entry of every packed entry
    ids = np.repeat(tr_first.astype(np.int64) - off[:-1], n_tr) + np.arange(off[-1])
    rep = lambda v: np.repeat(v, n_tr)
    out["n_transits"] = n_tr
    out["transit_off"] = off
    out["transit_times"] = (rep(period) * ids + rep(transit_time - t_first)) + rep(t_first)
    out["per_transit_count"] = tr_count[src].astype(np.int64)
    out["per_transit_log_likelihood"] = tr_ll[src]
    return out


def bls_stats_batch(t, flux, ivar, n_off, period, duration, transit_time, want_model=False, tr_off=None, raw=False, device=0):
    """``BoxLeastSquaresPeriodogram.compute_stats`` of one box per light curve for B ragged, time-sorted, NaN-free light
    curves on the host (``lk_bls_stats_batch``).  ``t`` / ``transit_time`` absolute; ``ivar`` None = ones; ``period`` /
    ``duration`` / ``transit_time``: scalars or one value per target.  Returns the dict of ``DeviceBLSResult.compute_stats``
    (``want_model``: plus ``model``, the box model per cadence).  ``tr_off``: per-transit slots other than
    ``bls_stats_slots``'s; ``raw``: the C outputs as they are (stats, tr_first, tr_n, tr_off, tr_count, tr_ll, model)."""
    h = Handle.get(device)
    t, flux = _f64(t), _f64(flux)
    n_off = _offsets(n_off, t.size)
    if flux.shape != t.shape or (ivar is not None and np.shape(ivar) != t.shape):
        raise ValueError("t, flux, ivar must be 1-D arrays of one length")
    ivar = None if ivar is None else _f64(ivar)
    B = n_off.size - 1
    period, duration, transit_time = bls_stats_arguments(B, period, duration, transit_time)
    counts = np.diff(n_off)
    if B and counts.min() < 1:
        raise ValueError("a light curve of the batch has no cadence")
    t_first, t_last = t[n_off[:-1]], t[n_off[1:] - 1]
    tr_off = bls_stats_slots(t_first, t_last, period) if tr_off is None else np.ascontiguousarray(tr_off, dtype=np.int64)
    if tr_off.shape != (B + 1,) or tr_off[0] != 0 or np.any(np.diff(tr_off) < 0):
        raise ValueError("tr_off must be B + 1 non-decreasing prefix offsets starting at 0")
    ntr = int(tr_off[-1])
    stats = np.zeros((B, BLS_NSTATS), dtype=np.float64)
    tr_first, tr_n = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    tr_count, tr_ll = np.zeros(max(ntr, 1), dtype=np.int32), np.zeros(max(ntr, 1), dtype=np.float64)
    model = np.empty(t.size, dtype=np.float64) if want_model else None
    _check(_lib.lk_bls_stats_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(flux), _ptr(ivar), _ptr(period), _ptr(duration),
                                   _ptr(transit_time), _ptr(tr_off, _c_ip), _ptr(stats), _ptr(tr_first, _c_i32p),
                                   _ptr(tr_n, _c_i32p), _ptr(tr_count, _c_i32p), _ptr(tr_ll), _ptr(model)))
    if raw:
        return stats, tr_first, tr_n, tr_off, tr_count[:ntr], tr_ll[:ntr], model
    out = bls_stats_dict(stats, tr_first, tr_n, tr_off, tr_count, tr_ll, period, transit_time, t_first)
    if want_model:
        out["model"] = model
    return out


LS_MODEL_NSTATS = 4            # LK_LS_MODEL_NSTATS (include/lkhip.h): y_mean, chi2_ref, chi2_model, status


def ls_model_arguments(B, frequency, nterms):
    """The per-target frequency of ``lk_ls_model_batch``: a scalar or one value per target -> float64[B] (NaN and values
    <= 0 are kept: they mark a target to skip, status 0); ``nterms`` an integer 1 .. ``MAX_NTERMS``, or ``ValueError``."""
    a = np.asarray(frequency, dtype=np.float64)
    if a.ndim > 1 or (a.ndim == 1 and a.size != B):
        raise ValueError("frequency must be a scalar or one value per light curve (%d), got shape %r" % (B, a.shape))
    if int(nterms) != nterms or not 1 <= int(nterms) <= MAX_NTERMS:
        raise ValueError("nterms must be an integer 1 .. %d (got %r)" % (MAX_NTERMS, nterms))
    return np.ascontiguousarray(np.broadcast_to(a, (B,))), int(nterms)


def ls_model_dict(frequency, theta, stats):
    """The raw outputs of ``lk_ls_model_batch`` -> the dict of ``DeviceLightCurveBatch.ls_model``: ``frequency`` [B],
    ``theta`` [B, 2 nterms + 1], ``amplitude`` / ``phase`` [B, nterms] (hypot and atan2(cos, sin) of each harmonic's pair:
    the harmonic is amplitude * sin(2 pi m f t + phase)), ``offset`` = y_mean + bias, ``y_mean``, ``chi2_ref``,
    ``chi2_model``, ``status`` (int: 1 fitted, 0 skipped, -1 not fitted)."""
    th_s, th_c = theta[:, 1::2], theta[:, 2::2]
    return dict(frequency=np.array(frequency, dtype=np.float64), theta=theta, amplitude=np.hypot(th_s, th_c),
                phase=np.arctan2(th_c, th_s), offset=stats[:, 0] + theta[:, 0], y_mean=stats[:, 0].copy(),
                chi2_ref=stats[:, 1].copy(), chi2_model=stats[:, 2].copy(), status=stats[:, 3].astype(np.int64))


def ls_model_batch(t, flux, dy, n_off, frequency, nterms=1, fit_mean=True, center_data=True, keep_mean=True, want_model=True,
                   want_residual=False, t_fit=None, m_off=None, device=0):
    """``LombScargle.model`` at one frequency [1/d] per light curve for B ragged, NaN-free light curves on the host
    (``lk_ls_model_batch``).  ``t`` absolute; ``dy`` None = unit weights (a light curve whose ``dy`` are not all finite gets
    unit weights too); ``frequency``: a scalar or one value per target.  Returns the dict of ``ls_model_dict`` plus ``model``
    (``want_model``) and ``residual`` (``want_residual``; ``keep_mean``: the level stays in it) per cadence, and with
    ``t_fit`` / ``m_off`` (target b owns ``t_fit[m_off[b]:m_off[b + 1]]``, absolute) ``model_fit``, the series at those times
    (``lk_ls_model_eval_batch``)."""
    h = Handle.get(device)
    t, flux = _f64(t), _f64(flux)
    n_off = _offsets(n_off, t.size)
    if flux.shape != t.shape or (dy is not None and np.shape(dy) != t.shape):
        raise ValueError("t, flux, dy must be 1-D arrays of one length")
    dy = None if dy is None else _f64(dy)
    B = n_off.size - 1
    frequency, nterms = ls_model_arguments(B, frequency, nterms)
    theta = np.zeros((B, 2 * nterms + 1), dtype=np.float64)
    stats = np.zeros((B, LS_MODEL_NSTATS), dtype=np.float64)
    model = np.empty(t.size, dtype=np.float64) if want_model else None
    residual = np.empty(t.size, dtype=np.float64) if want_residual else None
    _check(_lib.lk_ls_model_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(flux), _ptr(dy), _ptr(frequency), nterms,
                                  int(bool(fit_mean)), int(bool(center_data)), int(bool(keep_mean)), _ptr(theta), _ptr(stats),
                                  _ptr(model), _ptr(residual)))
    out = ls_model_dict(frequency, theta, stats)
    if want_model:
        out["model"] = model
    if want_residual:
        out["residual"] = residual
    if t_fit is not None:
        t_fit = _f64(t_fit)
        m_off = _offsets(m_off, t_fit.size)
        if m_off.size != B + 1:
            raise ValueError("m_off must hold B + 1 prefix offsets over t_fit")
        t_ref = t[np.minimum(n_off[:-1], t.size - 1)] if t.size else np.zeros(B)     # (an empty light curve is not fitted)
        fit = np.empty(t_fit.size, dtype=np.float64)
        _check(_lib.lk_ls_model_eval_batch(h._h, B, _ptr(m_off, _c_ip), _ptr(t_fit), _ptr(_f64(t_ref)), _ptr(frequency), nterms,
                                           _ptr(theta), _ptr(stats), _ptr(fit)))
        out["model_fit"] = fit
    return out


def transit_mask_batch(t, n_off, period, duration, transit_time, planet_off=None, device=0):
    """create_transit_mask for B ragged light curves.  ``period`` / ``duration`` / ``transit_time``: flat arrays over all
    planets, ``planet_off[B + 1]`` says which belong to which target (default: every target gets all of them)."""
    h = Handle.get(device)
    t = _f64(t)
    n_off = _offsets(n_off, t.size)
    B = n_off.size - 1
    period, duration, transit_time = (_f64(np.atleast_1d(a)) for a in (period, duration, transit_time))
    if not (period.shape == duration.shape == transit_time.shape):
        raise ValueError("period, duration, and transit_time must have the same number of values.")
    if planet_off is None:
        k = period.size
        period, duration, transit_time = (np.tile(a, B) for a in (period, duration, transit_time))
        planet_off = np.arange(B + 1, dtype=np.int32) * k
    planet_off = np.ascontiguousarray(planet_off, dtype=np.int32)
    if planet_off.shape != (B + 1,) or planet_off[0] != 0 or planet_off[-1] != period.size:
        raise ValueError("planet_off must be B + 1 prefix offsets over the planet arrays")
    mask = np.zeros(t.size, dtype=np.uint8)
    _check(_lib.lk_transit_mask_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(planet_off, _c_i32p), _ptr(period),
                                      _ptr(duration), _ptr(transit_time), _ptr(mask, _c_u8p)))
    return mask.astype(bool)


def bin_batch(t, flux, n_off, flux_err=None, time_bin_size=0.5, time_bin_start=None, device=0):
    """LightCurve.bin(time_bin_size=...) for B ragged, time-sorted light curves.
    Returns (t_binned, flux_binned, flux_err_binned, bin_off[B + 1])."""
    h = Handle.get(device)
    t, flux = _f64(t), _f64(flux)
    n_off = _offsets(n_off, t.size)
    B = n_off.size - 1
    err = None if flux_err is None else _f64(np.broadcast_to(flux_err, t.shape))
    size_sec = float(time_bin_size) * 86400.0
    if not size_sec > 0:
        raise ValueError("time_bin_size must be positive")
    start = np.empty(B, dtype=np.float64)
    nb = np.zeros(B, dtype=np.int64)
    has_err = np.zeros(B, dtype=np.uint8)
    for b in range(B):
        lo, hi = int(n_off[b]), int(n_off[b + 1])
        if hi == lo:
            start[b] = 0.0
            continue
        tb = t[lo:hi]
        if np.any(np.diff(tb) < 0):
            raise ValueError("bin needs the light curve sorted by time")
        s0 = tb[0] if time_bin_start is None else np.broadcast_to(np.asarray(time_bin_start, float), (B,))[b]
        start[b] = s0
        nb[b] = max(0, int(np.ceil((tb[-1] - s0) * 86400.0 / size_sec)))     # downsample.py:75-76
        has_err[b] = 1 if (err is not None and np.any(np.isfinite(err[lo:hi]))) else 0
    bin_off = np.zeros(B + 1, dtype=np.int64)
    bin_off[1:] = np.cumsum(nb)
    edges = np.cumsum(np.hstack([0.0, np.repeat(size_sec, int(nb.max()) if B else 0)]))   # downsample.py:82
    nbt = int(bin_off[-1])
    to, fo, eo = (np.empty(nbt, dtype=np.float64) for _ in range(3))
    _check(_lib.lk_bin_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(t), _ptr(flux), _ptr(err), _ptr(bin_off, _c_ip), _ptr(start),
                             _ptr(edges), int(edges.size), size_sec, _ptr(has_err, _c_u8p), _ptr(to), _ptr(fo), _ptr(eo)))
    return to, fo, eo, bin_off


# --------------------------------------------------------------------------------------------- SFF
SFF_SCRATCH_DEFAULT = 4 << 30       # LK_SFF_SCRATCH_DEFAULT in include/lkhip.h
SFF_STATUS = {0: "ok", 1: "too short", 2: "non-finite input", 3: "too wide"}      # lk_sff_correct_batch's per-target status


def sff_n_knots(t_first, t_last, timescale):
    """Columns of the long-term spline per target, the reference's ``int((time[-1] - time[0]) / timescale)`` (0 where that is
    not a number a spline can have: the library reports such a target by its status)."""
    span = (np.asarray(t_last, dtype=np.float64) - np.asarray(t_first, dtype=np.float64)) / float(timescale)
    ok = np.isfinite(span) & (span >= 0) & (span < 1e6)
    return np.where(ok, np.trunc(np.where(ok, span, 0.0)), 0).astype(np.int32)


def sff_window_arrays(window_points, n_off):
    """One list of cut indices per target -> (win_off int32[B + 1], window_points int32) as lk_sff_correct_batch takes them;
    ascending indices inside (0, N) are required."""
    n_off = np.asarray(n_off, dtype=np.int64)
    B = n_off.size - 1
    if len(window_points) != B:
        raise ValueError("window_points needs one list of cut indices per target (got %d for %d targets)" % (len(window_points), B))
    wps = [np.asarray(w, dtype=np.int64).reshape(-1) for w in window_points]
    for b, w in enumerate(wps):
        N = int(n_off[b + 1] - n_off[b])
        if w.size and (w[0] <= 0 or w[-1] >= N or np.any(np.diff(w) <= 0)):
            raise ValueError("target %d: window_points must be ascending cut indices inside (0, %d)" % (b, N))
    win_off = np.zeros(B + 1, dtype=np.int32)
    win_off[1:] = np.cumsum([w.size for w in wps])
    wp = np.ascontiguousarray(np.concatenate(wps) if wps else np.zeros(0), dtype=np.int32)
    return win_off, wp


def sff_scratch_bytes(n_off, n_knots, win_off, bins=5, degree=3, max_scratch_bytes=None):
    """(bytes, chunks) of the device block ``lk_sff_correct_batch_dev`` needs: the design matrices of the largest chunk of
    targets that fits ``max_scratch_bytes`` (None: 4 GiB) plus the batch's arclength.  Host arithmetic only."""
    load_library()
    n_off = np.ascontiguousarray(n_off, dtype=np.int64)
    n_knots = np.ascontiguousarray(n_knots, dtype=np.int32)
    win_off = np.ascontiguousarray(win_off, dtype=np.int32)
    B = n_off.size - 1
    if n_knots.shape != (B,) or win_off.shape != (B + 1,):
        raise ValueError("n_knots needs B entries and win_off B + 1")
    nbytes, chunks = ctypes.c_int64(0), ctypes.c_int(0)
    _check(_lib.lk_sff_scratch_bytes(B, _ptr(n_off, _c_ip), _ptr(n_knots, _c_i32p), _ptr(win_off, _c_i32p), int(bins), int(degree),
                                     int(max_scratch_bytes or 0), ctypes.byref(nbytes), ctypes.byref(chunks)))
    return int(nbytes.value), int(chunks.value)


def sff_arclength_batch(centroid_col, centroid_row, n_off, device=0):
    """``SFFCorrector._estimate_arclength`` for B ragged targets -> (arclength[sum N], flipped bool[B])."""
    h = Handle.get(device)
    col, row = _f64(centroid_col), _f64(centroid_row)
    n_off = _offsets(n_off, col.size)
    if col.ndim != 1 or row.shape != col.shape:
        raise ValueError("centroid_col and centroid_row must be 1-D arrays of one length")
    B = n_off.size - 1
    arc = np.empty(col.size, dtype=np.float64)
    flipped = np.zeros(max(B, 1), dtype=np.int32)
    _check(_lib.lk_sff_arclength_batch(h._h, B, _ptr(n_off, _c_ip), _ptr(col), _ptr(row), _ptr(arc), _ptr(flipped, _c_i32p)))
    return arc, flipped[:B].astype(bool)


def sff_correct_batch(time, flux, flux_err, centroid_col, centroid_row, n_off, window_points, bins=5, degree=3, timescale=1.5,
                      restore_trend=False, cadence_mask=None, sigma=5.0, niters=5, max_scratch_bytes=None, device=0):
    """``SFFCorrector.correct`` numerics for B ragged targets (include/lkhip.h: lk_sff_correct_batch).  ``window_points``: one
    list of cut indices per target.  Returns dict(flux, flux_err, outlier_mask, status int32[B], arclength, spline, sff — all
    packed like the inputs — and coefficients: a list of B arrays, K_b each)."""
    h = Handle.get(device)
    time = _f64(time)
    n_off = _offsets(n_off, time.size)
    cols = [_f64(a) for a in (flux, flux_err, centroid_col, centroid_row)]
    if time.ndim != 1 or any(a.shape != time.shape for a in cols):
        raise ValueError("time, flux, flux_err and the centroids must be 1-D arrays of one length")
    B, ntot = n_off.size - 1, time.size
    win_off, wp = sff_window_arrays(window_points, n_off)
    cm = None if cadence_mask is None else np.ascontiguousarray(cadence_mask, dtype=np.uint8)
    if cm is not None and cm.shape != (ntot,):
        raise ValueError("cadence_mask must have one entry per cadence")
    nk = sff_n_knots(time[n_off[:-1]], time[n_off[1:] - 1], timescale)
    widths = nk + (np.diff(win_off) + 1) * (int(bins) + int(degree))
    pitch = int(max(widths.max(), 1))
    out_f, out_e, arc, spl, sff = (np.empty(ntot, dtype=np.float64) for _ in range(5))
    outl = np.empty(ntot, dtype=np.uint8)
    status = np.zeros(B, dtype=np.int32)
    w = np.empty((B, pitch), dtype=np.float64)
    _check(_lib.lk_sff_correct_batch(
        h._h, B, _ptr(n_off, _c_ip), _ptr(time), _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(cols[3]), _ptr(cm, _c_u8p),
        _ptr(win_off, _c_i32p), _ptr(wp, _c_i32p), int(bins), int(degree), float(timescale), int(bool(restore_trend)), float(sigma),
        int(niters), int(max_scratch_bytes or 0), _ptr(out_f), _ptr(out_e), _ptr(outl, _c_u8p), _ptr(status, _c_i32p), _ptr(arc),
        _ptr(spl), _ptr(sff), _ptr(w), pitch))
    return dict(flux=out_f, flux_err=out_e, outlier_mask=outl.astype(bool), status=status, arclength=arc, spline=spl, sff=sff,
                coefficients=[w[b, :widths[b]].copy() if status[b] == 0 else np.full(0, np.nan) for b in range(B)])
