"""The one ctypes handle of an ``mhip_ctx`` (include/malstroem_hip.h).

``HydroPipeline`` (pipeline.py, an undivided raster) and ``HipBand`` (distributed.py, one row band) derive from ``CtxHandle``:
the context's life cycle, the whole and windowed transfers of the rasters of ``RASTERS`` and the scalar getters live here and
nowhere else.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import (R_ACCUM, R_DEM, R_DEPTHS, R_FILLED, R_FINALDEPTHS, R_FLOWDIR, R_LABELS, R_NGDIST, R_NOFLAT, R_WATERSHEDS,
                   RASTER_DTYPE)

RASTERS = {"dem": R_DEM, "filled": R_FILLED, "depths": R_DEPTHS, "noflat": R_NOFLAT, "flowdir": R_FLOWDIR,
           "accum": R_ACCUM, "labels": R_LABELS, "watersheds": R_WATERSHEDS, "ngdist": R_NGDIST,
           "finaldepths": R_FINALDEPTHS}


class CtxHandle(object):
    """Owner of one ``mhip_ctx``; ``shape`` is (owned rows, W).  A subclass creates the context into ``self._ctx``."""

    def __init__(self, shape):
        self.shape = (int(shape[0]), int(shape[1]))
        self._ctx = ctypes.c_void_p()

    def close(self):
        if self._ctx:
            _lib.call("mhip_ctx_destroy", self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- data movement ---------------------------------------------------------------------------
    def _shape_error(self, got):
        return "raster shape %s does not match the context's shape %s" % (got, self.shape)

    def upload(self, name, array):
        which = RASTERS[name]
        a = np.ascontiguousarray(array, dtype=RASTER_DTYPE[which])
        if a.shape != self.shape:
            raise ValueError(self._shape_error(a.shape))
        _lib.call("mhip_ctx_upload", self._ctx, which, _lib.ptr(a))

    def download(self, name):
        which = RASTERS[name]
        out = np.empty(self.shape, dtype=RASTER_DTYPE[which])
        _lib.call("mhip_ctx_download", self._ctx, which, _lib.ptr(out))
        return out

    # ---- windowed data movement (malstroem_amd.io readers / writers): one window on the host, whatever the raster's size
    def upload_rows(self, name, row0, array):
        which = RASTERS[name]
        a = np.ascontiguousarray(array, dtype=RASTER_DTYPE[which])
        if a.ndim != 2 or a.shape[1] != self.shape[1]:
            raise ValueError("window must be full-width rows of the pipeline's raster")
        _lib.call("mhip_ctx_upload_rows", self._ctx, which, _lib.i64(row0), _lib.i64(a.shape[0]), _lib.ptr(a))

    def download_rows(self, name, row0, nrows):
        """rows [row0, row0 + nrows) of the OWNED rows"""
        which = RASTERS[name]
        out = np.empty((int(nrows), self.shape[1]), dtype=RASTER_DTYPE[which])
        _lib.call("mhip_ctx_download_rows", self._ctx, which, _lib.i64(row0), _lib.i64(nrows), _lib.ptr(out))
        return out

    # ---- scalars -----------------------------------------------------------------------------------
    def sync(self):
        _lib.call("mhip_ctx_sync", self._ctx)

    def get_int(self, key):
        v = ctypes.c_int64(0)
        _lib.call("mhip_ctx_get_i64", self._ctx, key.encode(), ctypes.byref(v))
        return v.value

    def get_float(self, key):
        v = ctypes.c_double(0)
        _lib.call("mhip_ctx_get_f64", self._ctx, key.encode(), ctypes.byref(v))
        return v.value
