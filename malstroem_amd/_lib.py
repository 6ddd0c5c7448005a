"""ctypes binding of libmalstroem_hip.so (C-ABI declared in include/malstroem_hip.h).

This is the only place that touches the shared library.  Loading never falls back to anything
else: if the library (or a HIP device) is missing the stage functions raise ``RuntimeError``.
"""
import ctypes
import os
import subprocess
import threading
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("MALSTROEM_HIP_LIB", _PKG / "lib" / "libmalstroem_hip.so"))  # override: dev builds
CSRC = _PKG / "csrc"

STAT_DTYPE = np.dtype([("min", "<f8"), ("max", "<f8"), ("sum", "<f8"), ("count", "<i8")])   # _label.pyx:22-24
INDEX_DTYPE = np.dtype([("value", "<f8"), ("row", "<i8"), ("col", "<i8")])                    # _label.pyx:26-28
FINAL_DTYPE = np.dtype([("drawdown", "<f8"), ("dmax_final", "<f8"), ("qmodel", "<f8"), ("wet_cells", "<i8")])   # mhip_final_record

# DEM adaptations (adaptations.py): mhip_burn_segment, mhip_burn_line, mhip_burn_result
BURN_SEGMENT_DTYPE = np.dtype([("r0", "<i4"), ("c0", "<i4"), ("r1", "<i4"), ("c1", "<i4"), ("line", "<i4"), ("koff", "<i4")])
BURN_LINE_DTYPE = np.dtype([("z0", "<f8"), ("z1", "<f8"), ("ntotal", "<i4"), ("flags", "<i4")])
BURN_RESULT_DTYPE = np.dtype([("z0", "<f8"), ("z1", "<f8"), ("cells", "<i8"), ("status", "<i4"), ("pad", "<i4")])

# object exposure (objects.py): mhip_zone_record; sources of mhip_ctx_zone_stats that are no member of mhip_raster
ZONE_DTYPE = np.dtype([("vmax", "<f8"), ("vmin_pos", "<f8"), ("cells", "<i8"), ("pos", "<i8")])
ZSRC_WETAT, ZSRC_FLOWDIST, ZSRC_HAND, ZSRC_DRAINDIST, ZSRC_INUNDATION, ZSRC_TRAVELTIME = 100, 101, 102, 103, 104, 105
PSRC_REACHCATCH = 110      # a source of mhip_ctx_polygonize that is no member of mhip_raster

# flooding from sources at a water level (coastal.py): mhip_sea_record, the most levels of one call, the sources of
# mhip_ctx_zone_stats and mhip_ctx_polygonize that the sea flood adds
SEA_DTYPE = np.dtype([("dem_sum", "<f8"), ("wet_cells", "<i8"), ("dem_cells", "<i8"), ("dem_min", "<f4"), ("pad", "<i4")])
SEA_MAX_LEVELS = 256
ZSRC_SEALEVEL, ZSRC_SEADEPTH, PSRC_SEACLASSES = 106, 107, 111

# flow paths (flowpaths.py): mhip_reach_record; the end kinds of a reach
REACH_DTYPE = np.dtype([("first_cell", "<i8"), ("last_cell", "<i8"), ("end_cell", "<i8"), ("up_cells", "<f8"), ("down_cells", "<f8"),
                        ("n_orth", "<i4"), ("n_diag", "<i4"), ("end_kind", "<i4"), ("to_reach", "<i4"), ("to_label", "<i4"),
                        ("from_label", "<i4"), ("order", "<i4"), ("reserved", "<i4")])
REACH_END = ("confluence", "edge", "sink", "bluespot", "below_threshold")

# travel time (algorithms/flow.py): mhip_traveltime_params; the largest cost of a step in ticks, the most bins of a time-area table
TRAVELTIME_DTYPE = np.dtype([("k_overland", "<f8"), ("k_channel", "<f8"), ("channel_threshold", "<f8"), ("smin", "<f8"), ("vmax", "<f8"),
                             ("tick", "<f8")])
TRAVELTIME_COST_MAX, TRAVELTIME_MAX_BINS = 2 ** 20 - 1, 256

WETAT_MAX_EVENTS = 16    # MHIP_WETAT_MAX_EVENTS: most rain events of one wet_at call

OK, EINVAL, EHIP, ENODEV, ELIMIT, ENOTCONV, ECOMM = 0, -1, -2, -3, -4, -5, -6

STAGE_FILL, STAGE_NOFLAT, STAGE_FLOWDIR, STAGE_ACCUM = 1, 2, 4, 8
STAGE_LABEL, STAGE_WATERSHED, STAGE_POURPOINTS, STAGE_ALL = 16, 32, 64, 0x7F
STAGE_HYPS, STAGE_FINALDEPTHS = 128, 256     # timing slots of mhip_ctx_hyps / mhip_ctx_final_depths, not stages of mhip_ctx_run
R_DEM, R_FILLED, R_DEPTHS, R_NOFLAT, R_FLOWDIR, R_ACCUM, R_LABELS, R_WATERSHEDS, R_NGDIST, R_FINALDEPTHS = range(10)
RASTER_DTYPE = {R_DEM: np.float32, R_FILLED: np.float32, R_DEPTHS: np.float32, R_NOFLAT: np.float64,
                R_FLOWDIR: np.uint8, R_ACCUM: np.float64, R_LABELS: np.int32, R_WATERSHEDS: np.int32, R_NGDIST: np.uint32,
                R_FINALDEPTHS: np.float32}

# every symbol include/malstroem_hip.h declares (checked by tests/test_cabi.py)
SYMBOLS = [
    "mhip_last_error", "mhip_version", "mhip_device_count", "mhip_set_device", "mhip_copy_bandwidth", "mhip_read_bandwidth",
    "mhip_fill_f32", "mhip_fill_noflat_f64", "mhip_short_diag", "mhip_depths_f32", "mhip_d8_f64", "mhip_accum",
    "mhip_ccl8_f32", "mhip_ccl8_u8", "mhip_relabel_keep", "mhip_keep_mask", "mhip_label_stats_f32", "mhip_label_stats_f64",
    "mhip_label_argmin_f64", "mhip_label_argmax_f64", "mhip_label_count", "mhip_label_max", "mhip_watersheds_i32",
    "mhip_trace_downstream_i32", "mhip_ctx_trace_downstream", "mhip_rain_events", "mhip_band_forest_solve", "mhip_band_ws_resolve",
    "mhip_ctx_create", "mhip_comm_unique_id", "mhip_comm_available", "mhip_ctx_create_band", "mhip_ctx_destroy", "mhip_ctx_upload_dem",
    "mhip_ctx_upload", "mhip_ctx_download", "mhip_ctx_upload_rows", "mhip_ctx_download_rows", "mhip_ctx_run", "mhip_ctx_sync", "mhip_ctx_stage_ms",
    "mhip_ctx_kernel_ms", "mhip_ctx_get_i64", "mhip_ctx_get_f64", "mhip_ctx_raw_stats", "mhip_ctx_apply_keep",
    "mhip_ctx_stats", "mhip_ctx_watershed_counts", "mhip_ctx_pourpoints",
    "mhip_ctx_band_info", "mhip_ctx_get_edge_row", "mhip_ctx_set_halo_row", "mhip_ctx_get_edge_row_dev",
    "mhip_ctx_set_halo_row_dev", "mhip_ctx_get_edge_rows", "mhip_ctx_set_halo_rows", "mhip_ctx_dem_minmax",
    "mhip_ctx_fill_begin", "mhip_ctx_fill_batch", "mhip_ctx_fill_halo_changed", "mhip_ctx_fill_certify", "mhip_ctx_fill_end",
    "mhip_ctx_geo_begin", "mhip_ctx_geo_batch", "mhip_ctx_geo_halo_changed", "mhip_ctx_geo_end", "mhip_ctx_fill_attach", "mhip_ctx_noflat_verify",
    "mhip_ctx_zero_raster", "mhip_ctx_band_accum_boundary", "mhip_ctx_band_ccl_local", "mhip_ctx_band_ccl_begin", "mhip_ctx_band_ccl_finish", "mhip_ctx_band_relabel", "mhip_ctx_band_relabel_sparse", "mhip_ctx_band_relabel_range", "mhip_ctx_band_trace", "mhip_ctx_band_watershed_local",
    "mhip_ctx_band_watershed_rooted",
    "mhip_ctx_band_apply_neg_lut", "mhip_ctx_band_records", "mhip_ctx_band_fetch", "mhip_ctx_band_gather",
    "mhip_ctx_band_foreign_counts", "mhip_ctx_side_begin", "mhip_ctx_side_end",
    "mhip_ctx_has_comm", "mhip_ctx_exchange_halo", "mhip_ctx_exchange_edge_rows", "mhip_ctx_comm_add_side", "mhip_band_union_find", "mhip_band_accum_pairs", "mhip_band_accum_solve", "mhip_band_label_pairs",
    "mhip_band_label_merge", "mhip_band_ws_publish", "mhip_band_ws_lut", "mhip_band_merge_records", "mhip_tg_create", "mhip_tg_destroy", "mhip_tg_barrier", "mhip_tg_allreduce_max", "mhip_tg_offer", "mhip_tg_take", "mhip_shm_barrier", "mhip_ctx_allreduce_max",
    "mhip_label_hyps_layout", "mhip_label_hyps_f32", "mhip_hyps_levels", "mhip_final_depths_f32", "mhip_ctx_hyps", "mhip_ctx_hyps_fetch",
    "mhip_ctx_final_depths", "mhip_label_wet_at_f32", "mhip_ctx_wet_at", "mhip_ctx_wet_at_rows",
    "mhip_flow_distance", "mhip_ctx_flow_distance", "mhip_ctx_flow_distance_rows", "mhip_ctx_flow_distance_records",
    "mhip_step_cost", "mhip_flow_cost_distance", "mhip_ctx_travel_time", "mhip_ctx_travel_time_rows", "mhip_ctx_travel_time_records",
    "mhip_ctx_travel_time_hist",
    "mhip_hand_f32", "mhip_ctx_hand", "mhip_ctx_hand_rows",
    "mhip_reach_catchments_i32", "mhip_inundate_f32", "mhip_ctx_reach_catchments", "mhip_ctx_reach_catchments_rows", "mhip_ctx_inundate",
    "mhip_ctx_inundation_rows",
    "mhip_sea_flood_f32", "mhip_ctx_sea_flood", "mhip_ctx_sea_flood_rows", "mhip_ctx_sea_levels", "mhip_ctx_sea_depths", "mhip_ctx_sea_classes",
    "mhip_ctx_sea_classes_rows",
    "mhip_burn_lines_f32", "mhip_ctx_burn_lines",
    "mhip_rasterize_zones_i32", "mhip_zone_stats_f32", "mhip_ctx_rasterize_zones", "mhip_ctx_zones_rows", "mhip_ctx_zone_stats",
    "mhip_polygonize_i32", "mhip_ctx_polygonize", "mhip_polygons_sizes", "mhip_polygons_fetch", "mhip_polygons_free",
    "mhip_flowpaths_f64", "mhip_ctx_flowpaths", "mhip_flowpaths_sizes", "mhip_flowpaths_fetch", "mhip_flowpaths_free",
    "mhip_weighted_accum_u32", "mhip_ctx_weighted_accum", "mhip_wacc_info", "mhip_wacc_rows_u64", "mhip_wacc_rows_f64", "mhip_wacc_zone_sums",
    "mhip_wacc_free", "mhip_mfd_fractions_f64", "mhip_mfd_accum_u32", "mhip_ctx_mfd_accum", "mhip_wacc_work",
]

_lib = None
# ctypes releases the GIL.  The library is thread safe (thread-local error text, locked buffer pool); a context is driven by
# one thread at a time, except for the side-stream bracket mhip_ctx_side_begin / _end.


def build(force=False):
    """Compile libmalstroem_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = list(CSRC.glob("*.hip")) + list(CSRC.glob("*.hpp")) + [_PKG.parent / "include" / "malstroem_hip.h"]
    if not force and LIB_PATH.exists() and all(LIB_PATH.stat().st_mtime >= s.stat().st_mtime for s in srcs):
        return LIB_PATH
    subprocess.check_call(["make", "-C", str(CSRC), "-j8"] + (["-B"] if force else []))
    return LIB_PATH


def load():
    """Load the shared library (no device needed for loading)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError("libmalstroem_hip.so is not built (%s); run malstroem_amd._lib.build() -- "
                               "there is no CPU fallback" % LIB_PATH)
        lib = ctypes.CDLL(str(LIB_PATH))
        lib.mhip_last_error.restype = ctypes.c_char_p
        lib.mhip_version.restype = ctypes.c_char_p
        _lib = lib
    return _lib


def device_count():
    try:
        return int(load().mhip_device_count())
    except (OSError, RuntimeError):
        return 0


def check(rc, what):
    if rc == OK:
        return
    msg = load().mhip_last_error().decode("utf-8", "replace")
    text = "%s: %s" % (what, msg)
    if rc == EINVAL:
        raise ValueError(text)
    if rc == ELIMIT:
        raise OverflowError(text)
    raise RuntimeError(text)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def i64(v):
    return ctypes.c_int64(int(v))


def call(name, *args):
    rc = getattr(load(), name)(*args)
    check(rc, name)
