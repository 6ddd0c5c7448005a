"""Object exposure: which buildings, parcels or road sections get wet, at which rain, and how deep (no reference
counterpart).

Polygons become a *zone raster* on the device -- ``zones[r, c]`` is the largest zone id whose polygon holds the centre of the
cell, 0 for none -- and any float32 raster is reduced over it to one record per zone: the largest value, the smallest value > 0,
the cells and the cells > 0.  Both are exact; the definition is ``tests/_zones.py``.

``rings_from_features`` turns GeoJSON features into the three arrays the library takes, ``rasterize`` and ``zone_stats`` are the
stateless forms on host arrays; on resident rasters they are ``HydroPipeline.rasterize_zones`` / ``zone_stats``.  The kernels are
``csrc/zones.hip``.
"""
import numpy as np

from . import _lib
from ._lib import ZONE_DTYPE

COORD_MAX = float(1 << 29)


def _feature_name(k, f):
    fid = f.get("id") if isinstance(f, dict) else None
    return "feature %d%s" % (k, "" if fid is None else " (id %r)" % (fid,))


def rings_from_features(features, transform):
    """GeoJSON ``Polygon`` / ``MultiPolygon`` features -> ``(xy, ring_offsets, ring_zone, nzone)`` for ``rasterize``: feature ``k`` is
    zone ``k + 1``, every ring of it -- exterior, hole, part -- a ring of that zone (even-odd: a hole is a hole whatever its
    direction).  ``transform``: the north-up geotransform of the raster; a vertex ``(x, y)`` lies at ``((x - t[0]) / t[1],
    (y - t[3]) / t[5])`` in cell coordinates, where the centre of cell ``(r, c)`` is ``(c + 0.5, r + 0.5)``.  The closing vertex a
    GeoJSON ring repeats stays: it is an edge of no length."""
    t = [float(v) for v in transform]
    if len(t) != 6 or t[2] != 0.0 or t[4] != 0.0 or t[1] == 0.0 or t[5] == 0.0:
        raise ValueError("the transform must be north-up (transform[2] == transform[4] == 0), got %r" % (tuple(transform),))
    parts, zone = [], []
    nzone = 0
    for k, f in enumerate(features):
        nzone = k + 1
        geom = (f.get("geometry") or {}) if isinstance(f, dict) else {}
        gtype = geom.get("type")
        if gtype == "Polygon":
            polys = [geom.get("coordinates") or []]
        elif gtype == "MultiPolygon":
            polys = list(geom.get("coordinates") or [])
        else:
            raise ValueError("%s: geometry type %r is not Polygon or MultiPolygon" % (_feature_name(k, f), gtype))
        for poly in polys:
            for ring in poly:
                a = np.asarray(ring, dtype=np.float64)
                if a.ndim != 2 or a.shape[0] < 3 or a.shape[1] < 2:
                    raise ValueError("%s: a ring needs at least 3 vertices of (x, y)" % _feature_name(k, f))
                parts.append(a[:, :2])
                zone.append(k + 1)
    ring_zone = np.asarray(zone, dtype=np.int32)
    ring_offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    if not parts:
        return np.zeros((0, 2), dtype=np.float64), ring_offsets, ring_zone, nzone
    ring_offsets[1:] = np.cumsum([len(p) for p in parts])
    world = np.concatenate(parts)      # every vertex of every ring at once
    xy = np.empty_like(world)
    with np.errstate(invalid="ignore", over="ignore"):
        xy[:, 0] = (world[:, 0] - t[0]) / t[1]
        xy[:, 1] = (world[:, 1] - t[3]) / t[5]
    ok = np.all(np.abs(xy) <= COORD_MAX, axis=1)      # (false for NaN)
    if not np.all(ok):
        bad = int(np.flatnonzero(~ok)[0])
        k = int(ring_zone[np.searchsorted(ring_offsets, bad, side="right") - 1]) - 1
        raise ValueError("%s: a vertex is not finite or lies more than 2**29 cells from the raster's origin" % _feature_name(k, features[k]))
    return np.ascontiguousarray(xy), ring_offsets, ring_zone, nzone


def check_shape(shape):
    if len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1 or int(shape[0]) >= 1 << 31 or int(shape[1]) >= 1 << 31:
        raise ValueError("shape must be (rows, cols), each in [1, 2**31 - 1], got %r" % (shape,))
    return int(shape[0]), int(shape[1])


def check_rings(xy, ring_offsets, ring_zone, nzone, grow=0):
    """The argument rules of ``mhip_rasterize_zones_i32`` on the arrays (``ValueError``; nothing touches the library): -> ``(xy,
    ring_offsets, ring_zone, nzone, grow)``, the arrays C-contiguous float64 [nvert, 2], int64 [nring + 1], int32 [nring]."""
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    if xy.size == 0:
        xy = xy.reshape(0, 2)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError("xy must have the shape (nvert, 2), got %r" % (xy.shape,))
    off = np.asarray(ring_offsets)
    zone = np.asarray(ring_zone)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("ring_offsets must be a 1-D integer array of nring + 1 entries")
    if zone.ndim != 1 or zone.size != off.size - 1 or not (np.issubdtype(zone.dtype, np.integer) or zone.size == 0):
        raise ValueError("ring_zone must be a 1-D integer array of nring entries")
    off = np.ascontiguousarray(off, dtype=np.int64)
    if isinstance(nzone, bool) or int(nzone) != nzone or not 0 <= int(nzone) < 1 << 31:
        raise ValueError("nzone must be an integer in [0, 2**31 - 1], got %r" % (nzone,))
    if isinstance(grow, bool) or grow not in (0, 1):
        raise ValueError("grow must be 0 or 1, got %r" % (grow,))
    if off[0] != 0 or off[-1] != xy.shape[0]:
        raise ValueError("ring_offsets must start at 0 and end at nvert")
    n = np.diff(off)
    if np.any(n < 0):
        raise ValueError("ring_offsets decrease")
    if np.any(n < 3):
        raise ValueError("a ring of fewer than 3 vertices")
    if zone.size and (int(zone.min()) < 1 or int(zone.max()) > int(nzone)):
        raise ValueError("a zone id outside [1, nzone]")
    if not np.all(np.abs(xy) <= COORD_MAX):      # (false for NaN)
        raise ValueError("a coordinate that is not finite or beyond 2**29")
    return xy, off, np.ascontiguousarray(zone, dtype=np.int32), int(nzone), int(grow)


def check_zones(data, zones, nzone):
    """The argument rules of ``zone_stats`` on host arrays: -> ``(data, zones, nzone)``, C-contiguous float32 / int32 of one shape"""
    a, z = np.asarray(data), np.asarray(zones)
    if a.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32' but got '%s'" % a.dtype)
    if z.dtype != np.int32:
        raise ValueError("Buffer dtype mismatch, expected 'int32' but got '%s'" % z.dtype)
    if a.shape != z.shape or a.size < 1:
        raise ValueError("data and zones must have one shape and at least one cell, got %r and %r" % (a.shape, z.shape))
    if isinstance(nzone, bool) or int(nzone) != nzone or not 0 <= int(nzone) < 1 << 31:
        raise ValueError("nzone must be an integer in [0, 2**31 - 1], got %r" % (nzone,))
    return np.ascontiguousarray(a), np.ascontiguousarray(z), int(nzone)


def rasterize(shape, xy, ring_offsets, ring_zone, nzone, grow=0):
    """The zone raster (int32, ``shape``) of the polygons on the device.  ``grow=1``: one step more, a cell of zone 0 takes the
    largest zone among its 8 neighbours -- where buildings stand as blocks in the DEM the water is beside the footprint, not under it.
    The result depends on no order of rings or vertices.  No rings: the zero raster, without a device."""
    H, W = check_shape(shape)
    xy, off, zone, nzone, grow = check_rings(xy, ring_offsets, ring_zone, nzone, grow)
    out = np.zeros((H, W), dtype=np.int32)
    _lib.call("mhip_rasterize_zones_i32", _lib.i64(H), _lib.i64(W), _lib.i64(xy.shape[0]), _lib.ptr(xy), _lib.i64(zone.size), _lib.ptr(off),
              _lib.ptr(zone), _lib.i64(nzone), int(grow), _lib.ptr(out))
    return out


def zone_stats(data, zones, nzone):
    """``nzone + 1`` records (``_lib.ZONE_DTYPE``) of the float32 raster ``data`` over the int32 raster ``zones``: ``vmax`` the largest
    value that is no NaN (``-inf`` without one), ``vmin_pos`` the smallest value > 0 (``inf`` without one), ``cells``, ``pos`` the cells
    > 0; record 0 is the background.  A zone outside ``[0, nzone]`` raises ``ValueError``."""
    a, z, nzone = check_zones(data, zones, nzone)
    rec = np.zeros(nzone + 1, dtype=ZONE_DTYPE)
    W = a.shape[-1] if a.ndim == 2 else 0
    _lib.call("mhip_zone_stats_f32", _lib.ptr(a), _lib.ptr(z), _lib.i64(a.size), _lib.i64(W), _lib.i64(nzone), _lib.ptr(rec))
    return rec
