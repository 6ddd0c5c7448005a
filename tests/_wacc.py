"""The definition of the runoff-weighted flow accumulation (csrc/wacc.hip, malstroem_amd/runoff.py), in plain
NumPy / Python integers.  The device must give these bits.

``flowdir``: uint8, codes 0..7 step to a neighbour (0 up, then clockwise), a code above 7 has no direction.  ``weight``: uint32,
``UNIT`` for a cell that sends all of its rain downstream.  ``wacc[c] = weight[c] + sum(wacc[n])`` over the neighbours ``n`` inside
the raster whose direction points at ``c``, in uint64.  A cell without a direction receives and does not forward; a cell whose step
leaves the raster keeps its sum.  The walk is Kahn's, by in-degree: the cells it never releases -- those on a flow cycle, and
whatever lies downstream of one -- are UNRESOLVED and hold ``UNRESOLVED`` (a weight of 0 is legal, so 0 is no sentinel)."""
import numpy as np

UNIT = 1000000
UNRESOLVED = 2 ** 64 - 1
_DR = np.array([-1, -1, 0, 1, 1, 1, 0, -1])
_DC = np.array([0, 1, 1, 1, 0, -1, -1, -1])


def downstream(flowdir):
    """Per cell the flat index of the cell it flows into, -1 without a direction or when the step leaves the raster."""
    fd = np.asarray(flowdir)
    H, W = fd.shape
    r, c = np.divmod(np.arange(H * W), W)
    code = fd.ravel().astype(np.int64)
    has = code <= 7
    k = np.where(has, code, 0)
    nr, nc = r + _DR[k], c + _DC[k]
    ok = has & (nr >= 0) & (nr < H) & (nc >= 0) & (nc < W)
    return np.where(ok, nr * W + nc, -1)


def accumulate(flowdir, weight, zones=None, nzone=None):
    """``(wacc uint64, unresolved)``, and with ``zones`` (int32, values 0..nzone) ``(wacc, unresolved, sums uint64[nzone + 1])``."""
    fd, w = np.asarray(flowdir), np.asarray(weight)
    assert fd.dtype == np.uint8 and w.dtype == np.uint32 and fd.shape == w.shape and fd.ndim == 2
    n = fd.size
    assert n < 2 ** 31
    down = downstream(fd)
    indeg = np.bincount(down[down >= 0], minlength=n).tolist()
    down = down.tolist()
    acc = [int(v) for v in w.ravel()]
    released = bytearray(n)
    stack = [i for i in range(n) if indeg[i] == 0]
    while stack:
        i = stack.pop()
        released[i] = 1
        d = down[i]
        if d >= 0:
            acc[d] += acc[i]
            indeg[d] -= 1
            if indeg[d] == 0:
                stack.append(d)
    out = np.array([acc[i] if released[i] else UNRESOLVED for i in range(n)], dtype=np.uint64).reshape(fd.shape)
    unresolved = n - sum(released)
    if zones is None:
        return out, unresolved
    return out, unresolved, zone_sums(w, zones, nzone)


def zone_sums(weight, zones, nzone):
    """``sums[l]``: the sum of ``weight`` over the cells with ``zones == l``; no directions, no resolution in it."""
    z = np.asarray(zones)
    assert z.dtype == np.int32 and z.shape == np.shape(weight) and (z.size == 0 or (z.min() >= 0 and z.max() <= nzone))
    sums = np.zeros(int(nzone) + 1, dtype=np.uint64)
    np.add.at(sums, z.ravel(), np.asarray(weight).ravel().astype(np.uint64))
    return sums


def view(sums, div=UNIT, mul=1.0, nodata=-1.0):
    """The float view: ``(float64(sum) / div) * mul``, each of the three operations rounded on its own; ``nodata`` where the cell is
    unresolved."""
    s = np.asarray(sums, dtype=np.uint64)
    q = s.astype(np.float64) / np.float64(div)
    v = q * np.float64(mul)
    return np.where(s == np.uint64(UNRESOLVED), np.float64(nodata), v)


def effective_area(sums, cell_area):
    """Sums of weights as square metres: the float view with ``div = UNIT``, ``mul = cell_area`` (no cell of a sum is unresolved)."""
    return (np.asarray(sums, dtype=np.uint64).astype(np.float64) / np.float64(UNIT)) * np.float64(cell_area)


def weights(coefficient=None, pattern=None, nodata=None):
    """``uint32 = rint(float64(coefficient) * float64(pattern) * UNIT)``; ``None`` means 1; a NaN or ``nodata`` cell gives 0; a
    negative or overflowing product is a ``ValueError`` that names the first such cell (raster order)."""
    arrs = [np.asarray(a, dtype=np.float64) for a in (coefficient, pattern) if a is not None]
    shape = ()
    for a in arrs:
        if a.ndim:
            assert shape in ((), a.shape)
            shape = a.shape
    out = np.zeros(shape, dtype=np.uint32)
    for idx in np.ndindex(*shape):
        p, void = 1.0, False
        for a in arrs:
            v = float(a[idx] if a.ndim else a)
            if v != v or (nodata is not None and v == float(nodata)):
                void = True
            else:
                p = p * v
        if void:
            continue
        q = float(np.rint(np.float64(p) * np.float64(UNIT)))
        if q < 0 or q > 2 ** 32 - 1:
            raise ValueError("weight out of range at cell %s" % (tuple(int(i) for i in idx),))
        out[idx] = int(q)
    return out
