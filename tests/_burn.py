"""NumPy / Python model of the DEM adaptations: THE DEFINITION of ``mhip_burn_lines_f32`` -- the library is compared
with it bit for bit.  Plain loops over the steps; nothing here is fast.

A line is a chain of segments between cell coordinates.  Segment ``(r0, c0) -> (r1, c1)``: ``n = max(|dr|, |dc|)`` steps along the
major axis (the column when ``|dc| >= |dr|``); step ``k = 0 .. n`` sits at ``major = start + sign * k``, ``minor = start + sign *
m(k)`` with ``m(k) = (2 * k * dmin + n) // (2 * n)`` (``0`` when ``n == 0``).  A 4-connected line also owns, at a step ``k >= 1`` with
``m(k) != m(k - 1)``, the corner cell (major of ``k``, minor of ``k - 1``).  The enumeration depends on the segment's direction.
"""
import math

import numpy as np

SEGMENT_DTYPE = np.dtype([("r0", "<i4"), ("c0", "<i4"), ("r1", "<i4"), ("c1", "<i4"), ("line", "<i4"), ("koff", "<i4")])
LINE_DTYPE = np.dtype([("z0", "<f8"), ("z1", "<f8"), ("ntotal", "<i4"), ("flags", "<i4")])
RESULT_DTYPE = np.dtype([("z0", "<f8"), ("z1", "<f8"), ("cells", "<i8"), ("status", "<i4"), ("pad", "<i4")])
RAISE, CONN4 = 1, 2


def _sign(v):
    return (v > 0) - (v < 0)


def steps_of(r0, c0, r1, c1):
    """``n`` of a segment"""
    return max(abs(int(r1) - int(r0)), abs(int(c1) - int(c0)))


def segment_cells(r0, c0, r1, c1, conn4=False, shape=None):
    """``[(k, row, col)]`` in order; a corner cell comes in front of the cell of its step.  ``shape``: only the steps whose major
    coordinate lies inside a raster of that shape (one interval of ``k``; no other step has a cell inside) -- what lets a segment
    with ends 10**9 cells apart be enumerated at all"""
    r0, c0, r1, c1 = int(r0), int(c0), int(r1), int(c1)
    dr, dc = r1 - r0, c1 - c0
    colmajor = abs(dc) >= abs(dr)
    n, dmin = max(abs(dr), abs(dc)), min(abs(dr), abs(dc))
    m_of = lambda k: (2 * k * dmin + n) // (2 * n) if n else 0
    klo, khi = 0, n
    if shape is not None:
        a, s, size = (c0, _sign(dc), shape[1]) if colmajor else (r0, _sign(dr), shape[0])
        if s > 0:
            klo, khi = max(0, -a), min(n, size - 1 - a)
        elif s < 0:
            klo, khi = max(0, a - (size - 1)), min(n, a)
        elif not 0 <= a < size:
            khi = -1
    out = []
    for k in range(klo, khi + 1):
        m = m_of(k)
        cell = (lambda mm: (r0 + _sign(dr) * mm, c0 + _sign(dc) * k) if colmajor else (r0 + _sign(dr) * k, c0 + _sign(dc) * mm))
        if conn4 and k >= 1 and m != m_of(k - 1):
            out.append((k,) + cell(m_of(k - 1)))
        out.append((k,) + cell(m))
    return out


def level(z0, z1, koff, k, ntotal, raise_):
    """float32 level of step ``k``: one division, one subtraction, two products, one sum in float64, one rounding"""
    z0, z1 = float(z0), float(z1)
    if ntotal == 0:
        return np.float32(max(z0, z1) if raise_ else min(z0, z1))
    t = float(koff + k) / float(ntotal)
    return np.float32(z0 * (1.0 - t) + z1 * t)


def burn(dem, lines, segments, nodata=float("nan")):
    """-> ``(adapted, results)``; ``dem`` float32 ``H x W``, ``lines`` / ``segments`` of LINE_DTYPE / SEGMENT_DTYPE"""
    dem = np.asarray(dem)
    assert dem.dtype == np.float32 and dem.ndim == 2
    H, W = dem.shape
    out = dem.copy()
    res = np.zeros(len(lines), dtype=RESULT_DTYPE)
    of_line = [[] for _ in range(len(lines))]
    for s in segments:
        of_line[int(s["line"])].append(s)

    def inside(r, c):
        return 0 <= r < H and 0 <= c < W

    ends = []
    for i, l in enumerate(lines):
        segs = of_line[i]
        # the first vertex: of the segment with the smallest koff (the earliest among equals); the last vertex: of the segment with
        # the largest koff + n (the latest among equals) -- equals are segments of no length, which share their vertex in a connected line
        first = last = None
        for s in segs:
            if first is None or s["koff"] < first["koff"]:
                first = s
            if last is None or s["koff"] + steps_of(s["r0"], s["c0"], s["r1"], s["c1"]) >= last["koff"] + steps_of(last["r0"], last["c0"], last["r1"], last["c1"]):
                last = s
        z = [float(l["z0"]), float(l["z1"])]
        vert = [(int(first["r0"]), int(first["c0"])) if segs else None, (int(last["r1"]), int(last["c1"])) if segs else None]
        sample = [math.isnan(v) for v in z]
        status = 0
        if any(sm and (vt is None or not inside(*vt)) for sm, vt in zip(sample, vert)):
            status = 1
        else:
            for e in range(2):
                if sample[e]:
                    z[e] = float(dem[vert[e]])      # the ORIGINAL DEM
                    if not math.isfinite(z[e]) or z[e] == nodata:
                        status = 2
        res[i] = (z[0], z[1], 0, status, 0) if status == 0 else (math.nan, math.nan, 0, status, 0)
        ends.append((z[0], z[1], status))
    for want_raise in (False, True):
        for i, l in enumerate(lines):
            raise_, conn4 = bool(l["flags"] & RAISE), bool(l["flags"] & CONN4)
            z0, z1, status = ends[i]
            if raise_ != want_raise or status:
                continue
            for s in of_line[i]:
                for k, r, c in segment_cells(s["r0"], s["c0"], s["r1"], s["c1"], conn4, (H, W)):
                    if not inside(r, c):
                        continue
                    res["cells"][i] += 1
                    if math.isnan(out[r, c]):
                        continue
                    z = level(z0, z1, int(s["koff"]), k, int(l["ntotal"]), raise_)
                    if (z > out[r, c]) if raise_ else (z < out[r, c]):
                        out[r, c] = z
    return out, res


def polylines(vertex_lists, z0=None, z1=None, flags=None):
    """LINE / SEGMENT arrays of polylines given as lists of ``(row, col)`` vertices (one vertex alone: a segment of no length)"""
    nl = len(vertex_lists)
    lines = np.zeros(nl, dtype=LINE_DTYPE)
    lines["z0"] = np.nan if z0 is None else z0
    lines["z1"] = np.nan if z1 is None else z1
    lines["flags"] = 0 if flags is None else flags
    segs = []
    for i, vs in enumerate(vertex_lists):
        vs = list(vs) if len(vs) > 1 else [vs[0], vs[0]]
        koff = 0
        for (a, b), (c, d) in zip(vs[:-1], vs[1:]):
            segs.append((a, b, c, d, i, koff))
            koff += steps_of(a, b, c, d)
        lines["ntotal"][i] = koff
    return lines, np.array(segs, dtype=SEGMENT_DTYPE).reshape(-1)


def reorder_lines(lines, segs, perm):
    """the same lines in the order `perm` (new position i holds old line perm[i]), the segments re-pointed"""
    inv = np.empty(len(perm), dtype=np.int64)
    inv[perm] = np.arange(len(perm))
    s2 = segs.copy()
    s2["line"] = inv[segs["line"]]
    return lines[perm], s2
