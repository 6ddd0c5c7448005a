"""Spatially varying runoff: integer weights per cell, their accumulation and their sums per watershed.

A cell's WEIGHT is the share of its rain that runs off, times the relative depth of the rain on it, as a ``uint32`` in units of
``1 / UNIT``: ``UNIT`` is a cell of impermeable ground under the nominal rain -- what the library assumes everywhere when no
weights are given.  Sums of weights are integers (``uint64``), so every summation order gives the same bits; ``effective_area``
turns them into square metres.  The definition is ``tests/_wacc.py``; the accumulation is ``csrc/wacc.hip``.
"""
import ctypes

import numpy as np

from . import _lib

UNIT = 1000000                                # MHIP_WACC_UNIT
UNRESOLVED = np.uint64(2 ** 64 - 1)           # MHIP_WACC_UNRESOLVED: a cell on a flow cycle has no accumulated weight


def weights(coefficient=None, pattern=None, nodata=None):
    """``uint32 = rint(float64(coefficient) * float64(pattern) * UNIT)`` per cell: the runoff coefficient of the ground times the
    relative depth of the rain.  Either input may be ``None``, which means 1 (both ``None``: the scalar ``UNIT``).  A NaN cell and
    a cell that holds ``nodata`` in either input give 0.  A negative product, and one that does not fit a ``uint32``, is a
    ``ValueError`` that names the first such cell."""
    shape = None
    for a in (coefficient, pattern):
        if a is not None and np.ndim(a):
            if shape is not None and np.shape(a) != shape:
                raise ValueError("shape mismatch: coefficient is %s, pattern is %s" % (shape, np.shape(a)))
            shape = np.shape(a)
    prod = np.ones(shape or (), dtype=np.float64)
    void = np.zeros(shape or (), dtype=bool)
    for a in (coefficient, pattern):
        if a is None:
            continue
        f = np.asarray(a, dtype=np.float64)
        bad = np.isnan(f)
        if nodata is not None:
            bad = bad | (f == np.float64(nodata))
        void = void | bad
        prod = prod * np.where(bad, 1.0, f)
    q = np.rint(prod * np.float64(UNIT))
    q = np.where(void, 0.0, q)
    wrong = (q < 0) | (q > 4294967295.0)
    if wrong.any():
        first = tuple(int(i) for i in np.argwhere(wrong)[0])
        raise ValueError("weight out of range at cell %s: coefficient * pattern * %d = %r does not fit a uint32" % (first, UNIT, float(q[first])))
    return q.astype(np.uint32)


def effective_area(sums, cell_area):
    """Sums of weights as effective areas in square metres: ``(float64(sum) / UNIT) * cell_area``, each operation rounded on its
    own -- the float view of the device with ``div=UNIT, mul=cell_area``.  With weights of ``UNIT`` this is ``count * cell_area``
    bit for bit (the quotient is exact below 2**53)."""
    s = np.asarray(sums)
    if s.dtype != np.uint64:
        raise ValueError("Buffer dtype mismatch, expected 'uint64' but got '%s'" % s.dtype)
    return (s.astype(np.float64) / np.float64(UNIT)) * np.float64(cell_area)


def check_weight(weight, shape):
    """A weight raster for a raster of ``shape``: ``uint32``, C-contiguous (``ValueError`` otherwise; nothing touches the library)."""
    w = np.asarray(weight)
    if w.shape != tuple(shape):
        raise ValueError("shape mismatch: weight is %s, the raster is %s" % (w.shape, tuple(shape)))
    if w.dtype != np.uint32:
        raise ValueError("Buffer dtype mismatch, expected 'uint32' but got '%s'" % w.dtype)
    return np.ascontiguousarray(w)


class WeightedAccum(object):
    """A weighted accumulation of a pipeline (``HydroPipeline.weighted_accumulation``): a snapshot on the device, in buffers of its
    own.  It reads the same whatever happens to the pipeline afterwards -- new uploads, new runs, ``close`` -- and is freed by its
    own ``close`` (or as a context manager)."""

    def __init__(self, handle):
        self._h = handle
        H, W, nzone, unresolved = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.call("mhip_wacc_info", self._h, ctypes.byref(H), ctypes.byref(W), ctypes.byref(nzone), ctypes.byref(unresolved))
        self.shape = (H.value, W.value)
        self.nzone = nzone.value              # -1: made without the watersheds
        self.unresolved = unresolved.value    # cells on a flow cycle: they hold UNRESOLVED

    def close(self):
        if self._h:
            lib = _lib.load()
            lib.mhip_wacc_free.restype = None
            lib.mhip_wacc_free(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _open(self):
        if not self._h:
            raise ValueError("the weighted accumulation is closed")

    def download_rows_u64(self, row0, nrows):
        self._open()
        out = np.empty((int(nrows), self.shape[1]), dtype=np.uint64)
        _lib.call("mhip_wacc_rows_u64", self._h, _lib.i64(row0), _lib.i64(nrows), _lib.ptr(out))
        return out

    def download_u64(self):
        """The sums as they are (uint64; ``UNRESOLVED`` on a flow cycle)."""
        return self.download_rows_u64(0, self.shape[0])

    def download_rows(self, row0, nrows, div=UNIT, mul=1.0, nodata=-1.0):
        """Rows ``[row0, row0 + nrows)`` of the float view (below)."""
        self._open()
        out = np.empty((int(nrows), self.shape[1]), dtype=np.float64)
        _lib.call("mhip_wacc_rows_f64", self._h, _lib.i64(row0), _lib.i64(nrows), ctypes.c_double(div), ctypes.c_double(mul), ctypes.c_double(nodata),
                  _lib.ptr(out))
        return out

    def download(self, div=UNIT, mul=1.0, nodata=-1.0):
        """The float view ``(float64(sum) / div) * mul``, computed on the device with each operation rounded on its own;
        ``nodata`` on a flow cycle.  The defaults give upstream cells' worth of runoff; ``mul=cell_area`` the effective upstream
        area in square metres."""
        return self.download_rows(0, self.shape[0], div, mul, nodata)

    def download_to(self, writer, div=UNIT, mul=1.0, nodata=-1.0, max_rows=4096):
        """Stream the float view into a writer in row windows, as ``HydroPipeline.download_to`` does for the resident rasters."""
        from .pipeline import write_windows
        write_windows(writer, self.shape, np.float64, lambda row0, n: self.download_rows(row0, n, div, mul, nodata), max_rows)

    def work(self):
        """``{"rounds", "visits", "tiles"}``: what the tile schedule did for a result of ``HydroPipeline.mfd_accumulation`` (DESIGN.md
        21) -- launches that had a list, tile visits over all of them, tiles; zeros for a weighted accumulation."""
        self._open()
        r, v, t = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.call("mhip_wacc_work", self._h, ctypes.byref(r), ctypes.byref(v), ctypes.byref(t))
        return {"rounds": r.value, "visits": v.value, "tiles": t.value}

    def sums(self):
        """The sum of the weights per watershed (uint64, ``nlabels + 1`` entries); ``ValueError`` when the result was made without
        the watersheds."""
        self._open()
        if self.nzone < 0:
            raise ValueError("the weighted accumulation was made without the watersheds (by_watersheds=False)")
        out = np.zeros(self.nzone + 1, dtype=np.uint64)
        _lib.call("mhip_wacc_zone_sums", self._h, _lib.ptr(out))
        return out
