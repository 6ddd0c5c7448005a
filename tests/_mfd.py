"""The definition of the multiple-flow-direction accumulation (csrc/mfd.hip, malstroem_amd/mfd.py), in plain NumPy /
Python integers.  The device must give these bits.

Neighbour order: that of the direction codes (0 up, then clockwise).  ``ONE = 32768``.

``fractions(z, exponent)``: for an interior cell with a finite ``z``: ``dz_k = z - z_k``, the diagonal ones times ``INV_SQRT2``;
``s_k = dz_k`` if ``0 < dz_k < inf``, else 0 (a NaN or infinite neighbour, a neighbour that is not lower, a difference of finite
values that overflows).  All ``s_k`` 0: eight zeros, the cell is a sink.  Otherwise ``m`` is the first ``k`` with the largest ``s_k``
(the D8 choice), ``r_k = s_k / s_m``, ``t_k = r_k`` multiplied by itself ``exponent - 1`` times from the left,
``T = ((t_0 + t_1) + t_2) + ... + t_7``, ``q_k = floor((t_k / T) * ONE)``, ``q_m += ONE - sum(q)``; every operation rounded on its
own (float64).  Cells on the border and cells whose ``z`` is not finite: eight zeros.

``accumulate(fractions, weight)``: a cell's eight sum to 0 or ``ONE`` (``ValueError`` otherwise).  ``acc[c] = weight[c]`` + what its
neighbours send.  A cell sends exactly once, when every in-edge (a neighbour with a positive fraction towards it) has delivered:
``(acc * p_k) >> 15`` to neighbour ``k != m`` with ``p_k > 0``, ``m`` the first largest ``p_k``, and ``acc`` minus these to ``m``.
A share whose neighbour lies outside the raster leaves the raster.  A cell keeps its own ``acc``.  The order is Kahn's; the cells
it never releases hold ``UNRESOLVED`` and are counted."""
import numpy as np

ONE = 32768
UNIT = 1000000
UNRESOLVED = 2 ** 64 - 1
INV_SQRT2 = 0.7071067811865475
_DR = np.array([-1, -1, 0, 1, 1, 1, 0, -1])
_DC = np.array([0, 1, 1, 1, 0, -1, -1, -1])


def slopes(z):
    """``s[H - 2, W - 2, 8]`` of the interior cells (0 where the cell's own z is not finite)."""
    z = np.asarray(z)
    assert z.dtype == np.float64 and z.ndim == 2
    H, W = z.shape
    zc = z[1:-1, 1:-1]
    s = np.zeros((H - 2, W - 2, 8), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(8):
            dz = zc - z[1 + _DR[k]:H - 1 + _DR[k], 1 + _DC[k]:W - 1 + _DC[k]]
            if k & 1:
                dz = dz * np.float64(INV_SQRT2)
            s[..., k] = np.where((dz > 0.0) & (dz < np.inf), dz, 0.0)
    s[~np.isfinite(zc)] = 0.0
    return s


def fractions(z, exponent=1, remainders=None):
    """``uint16[H, W, 8]``.  Asserts ``0 <= ONE - sum(q)`` before the remainder goes to ``m``; with a list ``remainders`` appends
    the smallest and the largest remainder it saw (nothing for a surface without a sending cell)."""
    z = np.asarray(z)
    assert z.dtype == np.float64 and z.ndim == 2 and isinstance(exponent, int) and 1 <= exponent <= 8
    H, W = z.shape
    out = np.zeros((H, W, 8), dtype=np.uint16)
    if H < 3 or W < 3:
        return out
    s = slopes(z)
    m = np.argmax(s, axis=2)                      # (the first of equal maxima)
    sm = np.take_along_axis(s, m[..., None], axis=2)[..., 0]
    send = sm > 0.0
    with np.errstate(all="ignore"):
        r = s / np.where(send, sm, 1.0)[..., None]
        t = r.copy()
        for _ in range(exponent - 1):
            t = t * r
        T = t[..., 0] + t[..., 1]
        for k in range(2, 8):
            T = T + t[..., k]
        q = np.floor((t / np.where(send, T, 1.0)[..., None]) * np.float64(ONE)).astype(np.int64)
    q[~send] = 0
    rem = np.where(send, ONE - q.sum(axis=2), 0)
    assert (rem >= 0).all()
    if remainders is not None and send.any():
        remainders += [int(rem[send].min()), int(rem[send].max())]
    np.put_along_axis(q, m[..., None], np.take_along_axis(q, m[..., None], axis=2) + rem[..., None], axis=2)
    out[1:-1, 1:-1] = q.astype(np.uint16)
    return out


def fractions_from_flowdir(flowdir):
    """``ONE`` in the slot of the code, none for a code above 7."""
    fd = np.asarray(flowdir)
    assert fd.dtype == np.uint8 and fd.ndim == 2
    out = np.zeros(fd.shape + (8,), dtype=np.uint16)
    for (r, c), code in np.ndenumerate(fd):
        if code <= 7:
            out[r, c, code] = ONE
    return out


def check_fractions(fractions):
    f = np.asarray(fractions)
    if f.dtype != np.uint16 or f.ndim != 3 or f.shape[2] != 8:
        raise ValueError("fractions must be uint16 [H, W, 8]")
    total = f.sum(axis=2, dtype=np.int64)
    if ((total != 0) & (total != ONE)).any():
        raise ValueError("fractions that sum to neither 0 nor ONE")
    return f


def first_max(p):
    m = 0
    for k in range(1, 8):
        if p[k] > p[m]:
            m = k
    return m


def shares(acc, p):
    """What a cell with sum ``acc`` and fractions ``p`` sends to its eight neighbours (Python integers)."""
    m = first_max(p)
    out = [(acc * int(p[k])) >> 15 if k != m else 0 for k in range(8)]
    out[m] = acc - sum(out) if p[m] else 0
    return out


def accumulate(fractions, weight, left=None):
    """``(acc uint64[H, W], unresolved)``: Kahn's walk in Python integers.  With a list ``left``: appends what left the raster."""
    f, w = check_fractions(fractions), np.asarray(weight)
    assert w.dtype == np.uint32 and w.shape == f.shape[:2]
    H, W = w.shape
    assert H * W < 2 ** 31
    p = f.tolist()
    acc = [[int(v) for v in row] for row in w.tolist()]
    indeg = [[0] * W for _ in range(H)]
    for r in range(H):
        for c in range(W):
            for k in range(8):
                rr, cc = r + int(_DR[k]), c + int(_DC[k])
                if p[r][c][k] and 0 <= rr < H and 0 <= cc < W:
                    indeg[rr][cc] += 1
    fired = [[False] * W for _ in range(H)]
    stack = [(r, c) for r in range(H) for c in range(W) if indeg[r][c] == 0]
    gone = 0
    while stack:
        r, c = stack.pop()
        fired[r][c] = True
        out = shares(acc[r][c], p[r][c])
        for k in range(8):
            if not p[r][c][k]:
                continue
            rr, cc = r + int(_DR[k]), c + int(_DC[k])
            if 0 <= rr < H and 0 <= cc < W:
                acc[rr][cc] += out[k]
                indeg[rr][cc] -= 1
                if indeg[rr][cc] == 0:
                    stack.append((rr, cc))
            else:
                gone += out[k]
    res = np.array([[acc[r][c] if fired[r][c] else UNRESOLVED for c in range(W)] for r in range(H)], dtype=np.uint64).reshape(H, W)
    if left is not None:
        left.append(gone)
    return res, H * W - sum(sum(row) for row in fired)


def accumulate_levels(fractions, weight):
    """The same bits by levels in NumPy, for rasters too large for the walk above: every cell whose inflows are complete sends in
    one step.  The product is split as ``(a_hi * p << 17) + (a_lo * p >> 15)``: no intermediate leaves 64 bits."""
    f, w = check_fractions(fractions), np.asarray(weight)
    assert w.dtype == np.uint32 and w.shape == f.shape[:2]
    H, W = w.shape
    n = H * W
    assert n < 2 ** 31
    p = f.reshape(n, 8).astype(np.uint64)
    r, c = np.divmod(np.arange(n), W)
    tgt = np.empty((n, 8), dtype=np.int64)
    for k in range(8):
        rr, cc = r + _DR[k], c + _DC[k]
        tgt[:, k] = np.where((rr >= 0) & (rr < H) & (cc >= 0) & (cc < W), rr * W + cc, -1)
    edge = (p > 0) & (tgt >= 0)
    indeg = np.bincount(tgt[edge], minlength=n).astype(np.int64)
    m = np.argmax(p, axis=1)
    acc = w.reshape(n).astype(np.uint64)
    fired = np.zeros(n, dtype=bool)
    front = np.flatnonzero(indeg == 0)
    while front.size:
        fired[front] = True
        a, pf, mf = acc[front], p[front], m[front]
        out = ((a >> np.uint64(32))[:, None] * pf << np.uint64(17)) + ((a & np.uint64(0xffffffff))[:, None] * pf >> np.uint64(15))
        out[np.arange(front.size), mf] = 0
        rest = a - out.sum(axis=1, dtype=np.uint64)
        out[np.arange(front.size), mf] = np.where(pf[np.arange(front.size), mf] > 0, rest, np.uint64(0))
        e = edge[front]
        t = tgt[front][e]
        np.add.at(acc, t, out[e])
        np.subtract.at(indeg, t, 1)
        t = np.unique(t)
        front = t[indeg[t] == 0]
    res = np.where(fired, acc, np.uint64(UNRESOLVED)).reshape(H, W)
    return res, int(n - fired.sum())


def view(sums, div=UNIT, mul=1.0, nodata=-1.0):
    """The float view of DESIGN.md 20: ``(float64(sum) / div) * mul``, ``nodata`` where the cell is unresolved."""
    s = np.asarray(sums, dtype=np.uint64)
    v = (s.astype(np.float64) / np.float64(div)) * np.float64(mul)
    return np.where(s == np.uint64(UNRESOLVED), np.float64(nodata), v)
