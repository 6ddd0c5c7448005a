"""NumPy / Python model of the height above the nearest drainage (csrc/hand.hip).  It loads no library.

A cell is a DRAINAGE cell when accum >= threshold (compared in float64; a NaN is none) or, with labels, its label is != 0.  D(c) is the
first drainage cell on the downstream walk from c, c included, after no(c) orthogonal (codes 0, 2, 4, 6) and nd(c) diagonal steps --
the first one, whatever the accumulation does further down.  A cell is UNDRAINED when its walk ends before it meets one: at a code
> 7, at a step out of the raster, on a flow cycle or on a path into one.

  hand       float32: elev[c] - elev[D(c)] as ONE float32 subtraction; a result that is a NaN (a NaN elevation at either end, or two
             equal infinities) is the quiet NaN 0x7fc00000; a drainage cell holds +0.0; an undrained cell holds `nodata` verbatim
  dist       float32((float64(no) + float64(nd) * SQRT2) * scale); -1 where undrained
  undrained  the number of undrained cells

`hand` walks every chain once (a stack, as tests/_flowdist.py does); `brute` walks from every cell on its own and shares no code with it.
"""
import numpy as np

SQRT2 = 1.4142135623730951
DR = (-1, -1, 0, 1, 1, 1, 0, -1)      # AGNPS codes 0..7: up, up-right, right, down-right, down, down-left, left, up-left
DC = (0, 1, 1, 1, 0, -1, -1, -1)
QNAN = np.uint32(0x7fc00000).view(np.float32)


def drainage(accum, threshold, labels=None):
    d = np.asarray(accum, np.float64) >= np.float64(threshold)      # (False for a NaN)
    if labels is not None:
        d = d | (np.asarray(labels) != 0)
    return d


def _next(flowdir):
    """flat index of the cell every cell steps to; -1: no direction, or the step leaves the raster"""
    fd = np.asarray(flowdir)
    h, w = fd.shape
    nxt = np.full(fd.size, -1, np.int64)
    for code in range(8):
        r, c = np.nonzero(fd == code)
        nr, nc = r + DR[code], c + DC[code]
        ok = (nr >= 0) & (nr < h) & (nc >= 0) & (nc < w)
        nxt[r[ok] * w + c[ok]] = nr[ok] * w + nc[ok]
    return nxt


def resolve(flowdir, drain):
    """(no, nd, end) flat int64 arrays; end = D(c), -1 for an undrained cell (no = nd = 0 there)"""
    fd = np.asarray(flowdir)
    nxt = _next(fd).tolist()
    diag = ((fd.ravel() & 1) == 1).tolist()
    dr = np.asarray(drain).ravel().tolist()
    n = len(nxt)
    no, nd, end = [0] * n, [0] * n, [-1] * n
    state = [0] * n      # 0 unknown, 1 on the stack, 2 drained, 3 undrained
    for c0 in range(n):
        if state[c0]:
            continue
        path, c = [], c0
        while state[c] == 0:
            if dr[c]:
                state[c], end[c] = 2, c
            elif nxt[c] < 0:
                state[c] = 3
            else:
                state[c] = 1
                path.append(c)
                c = nxt[c]
        good = state[c] == 2      # (state 1: the walk ran into its own stack -- a cycle)
        for p in reversed(path):
            if good:
                q = nxt[p]
                state[p], end[p] = 2, end[q]
                no[p], nd[p] = no[q] + (0 if diag[p] else 1), nd[q] + (1 if diag[p] else 0)
            else:
                state[p] = 3
    return np.array(no, np.int64), np.array(nd, np.int64), np.array(end, np.int64)


def rasters(no, nd, end, elev, scale=1.0, nodata=-9999.0):
    """(hand, dist, undrained) from a resolved walk"""
    z = np.asarray(elev)
    assert z.dtype == np.float32
    ok = end >= 0
    zf = z.ravel()
    with np.errstate(invalid="ignore"):
        h = zf - zf[np.where(ok, end, 0)]
    h = np.where(np.isnan(h), QNAN, h)
    hand = np.where(ok, h, np.float32(nodata)).astype(np.float32)
    u = (no.astype(np.float64) + nd.astype(np.float64) * SQRT2) * np.float64(scale)
    dist = np.where(ok, u.astype(np.float32), np.float32(-1.0)).astype(np.float32)
    return hand.reshape(z.shape), dist.reshape(z.shape), int((~ok).sum())


def hand(flowdir, accum, elev, threshold, labels=None, scale=1.0, nodata=-9999.0):
    """dict(hand, dist, undrained, no, nd, end); no / nd / end have the raster's shape (0, 0, -1 where undrained)"""
    fd = np.asarray(flowdir)
    no, nd, end = resolve(fd, drainage(accum, threshold, labels))
    h, d, u = rasters(no, nd, end, elev, scale, nodata)
    return dict(hand=h, dist=d, undrained=u, no=no.reshape(fd.shape), nd=nd.reshape(fd.shape), end=end.reshape(fd.shape))


def brute(flowdir, accum, elev, threshold, labels=None, scale=1.0, nodata=-9999.0):
    """(hand, dist, undrained) by a walk from every cell on its own, cell by cell in Python scalars; more than n steps: a cycle"""
    fd, acc, z = np.asarray(flowdir), np.asarray(accum), np.asarray(elev)
    h, w = fd.shape
    out_h, out_d = np.full((h, w), np.float32(nodata), np.float32), np.full((h, w), np.float32(-1), np.float32)
    undrained = 0
    for r0 in range(h):
        for c0 in range(w):
            r, c, a, b, steps = r0, c0, 0, 0, 0
            found = False
            while steps <= h * w:
                if np.float64(acc[r, c]) >= np.float64(threshold) or (labels is not None and labels[r, c] != 0):
                    found = True
                    break
                code = int(fd[r, c])
                if code > 7:
                    break
                r2, c2 = r + DR[code], c + DC[code]
                if not (0 <= r2 < h and 0 <= c2 < w):
                    break
                a, b = a + (0 if code & 1 else 1), b + (code & 1)
                r, c, steps = r2, c2, steps + 1
            if not found:
                undrained += 1
                continue
            with np.errstate(invalid="ignore"):
                v = np.float32(z[r0, c0]) - np.float32(z[r, c])
            out_h[r0, c0] = QNAN if np.isnan(v) else v
            out_d[r0, c0] = np.float32((np.float64(a) + np.float64(b) * SQRT2) * np.float64(scale))
    return out_h, out_d, undrained


def same_bits(got, want):
    """the two float32 arrays hold the same bit patterns (a NaN included: the contract names its bits)"""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------
def serpentine(h, w):
    """(flowdir, last cell): one path through every cell -- right along the even rows, left along the odd ones, one step down at the
    ends -- whose last cell has no direction: h * w - 1 orthogonal steps from cell (0, 0)"""
    fd = np.empty((h, w), np.uint8)
    fd[0::2], fd[1::2] = 2, 6
    fd[0::2, w - 1], fd[1::2, 0] = 4, 4
    last = (h - 1, w - 1 if (h - 1) % 2 == 0 else 0)
    fd[last] = 8
    return fd, last


def random_case(shape, seed):
    """(flowdir, accum, elev, labels): codes 0..9 (sinks, cycles, codes beyond 8), accumulations around a threshold of 50 with a few
    NaNs, elevations with a few NaNs and infinities, sparse labels"""
    rng = np.random.default_rng(seed)
    fd = rng.integers(0, 10, size=shape).astype(np.uint8)
    acc = np.floor(rng.random(shape) * 55.0) + 1.0
    acc[rng.random(shape) < 0.01] = np.nan
    z = (rng.random(shape) * 100).astype(np.float32)
    z[rng.random(shape) < 0.01] = np.nan
    z[rng.random(shape) < 0.005] = np.inf
    lab = np.where(rng.random(shape) < 0.02, rng.integers(1, 40, size=shape), 0).astype(np.int32)
    return fd, acc, z, lab
