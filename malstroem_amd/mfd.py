"""Multiple-flow-direction accumulation: host helpers for the fixed-point fractions.

A cell's FRACTIONS are eight ``uint16`` in units of ``1 / ONE``, one per neighbour in the order of the direction codes (0 up, then
clockwise): the share of the flow through the cell that goes to that neighbour.  They sum to ``ONE``, or to 0 for a cell that sends
nothing.  ``algorithms.flow.mfd_fractions`` makes them from a surface, ``algorithms.flow.mfd_accumulation`` accumulates anybody's --
contour-length factors, non-integer exponents and D-infinity are fractions of the caller's.  The definition is ``tests/_mfd.py``;
the kernels are ``csrc/mfd.hip``.
"""
import numpy as np

ONE = 32768                                   # MHIP_MFD_ONE


def check_exponent(exponent):
    """The exponent of ``mfd_fractions``: an integer in 1..8 (``ValueError`` otherwise; nothing touches the library)."""
    if isinstance(exponent, bool) or not isinstance(exponent, (int, np.integer)) or not 1 <= int(exponent) <= 8:
        raise ValueError("exponent must be an integer in [1, 8], got %r" % (exponent,))
    return int(exponent)


def check_fractions(fractions, shape=None, sums=False):
    """A fractions array: ``uint16``, ``[H, W, 8]``, C-contiguous, for a raster of ``shape`` if given (``ValueError`` otherwise;
    nothing touches the library).  With ``sums`` also what the device checks: every cell's eight sum to 0 or to ``ONE``; the
    ``ValueError`` names the first cell that does not."""
    f = np.asarray(fractions)
    if f.ndim != 3 or f.shape[2] != 8:
        raise ValueError("fractions must be [H, W, 8], got %s" % (f.shape,))
    if f.dtype != np.uint16:
        raise ValueError("Buffer dtype mismatch, expected 'uint16' but got '%s'" % f.dtype)
    if shape is not None and f.shape[:2] != tuple(shape):
        raise ValueError("shape mismatch: fractions are %s, the raster is %s" % (f.shape[:2], tuple(shape)))
    if sums:
        total = f.sum(axis=2, dtype=np.uint32)
        wrong = (total != 0) & (total != ONE)
        if wrong.any():
            first = tuple(int(i) for i in np.argwhere(wrong)[0])
            raise ValueError("the fractions of cell %s sum to %d, neither 0 nor %d" % (first, int(total[first]), ONE))
    return np.ascontiguousarray(f)


def fractions_from_flowdir(flowdir):
    """The fractions of a D8 raster: ``ONE`` in the slot of the cell's direction code, none for a code above 7.  Accumulating them
    gives ``algorithms.flow.weighted_accumulation`` of the same directions, value for value and with the same unresolved cells."""
    fd = np.asarray(flowdir)
    if fd.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2, got %d)" % fd.ndim)
    if fd.dtype != np.uint8:
        raise ValueError("Buffer dtype mismatch, expected 'uint8' but got '%s'" % fd.dtype)
    out = np.zeros(fd.shape + (8,), dtype=np.uint16)
    r, c = np.nonzero(fd <= 7)
    out[r, c, fd[r, c]] = ONE
    return out
