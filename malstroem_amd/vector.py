"""Outlines of bluespots and watersheds -- mirror of ``malstroem.vector`` (reference vector.py:21-87) without GDAL.

The reference polygonizes a label raster file with ``gdal.Polygonize(..., ['8CONNECTED=8'])``.  Here the rings are computed on the
device (``csrc/polygonize.hip``; the definition is ``tests/_polygonize.py``): ``polygonize`` turns an int32 label raster into the
three arrays ``objects.rasterize`` takes -- ``xy`` (int32, lattice vertices in cell coordinates: cell ``(r, c)`` has the corners
``(c, r) .. (c + 1, r + 1)``), ``ring_offsets``, ``ring_label`` -- and rasterizing them gives the raster back.  On resident rasters it
is ``HydroPipeline.polygonize``: no raster leaves the device.  ``features_from_rings`` makes GeoJSON features of the arrays, one per
label: exterior rings counter-clockwise in world coordinates (RFC 7946), holes clockwise, every ring closed.
"""
import ctypes

import numpy as np

from . import _lib


def transform_cell_to_world(cell, transform):
    """Centre of cell (row, col) in world coordinates for a GDAL geotransform (reference vector.py:21-39)."""
    row, col = cell[0] + 0.5, cell[1] + 0.5
    x = transform[0] + col * transform[1] + row * transform[2]
    y = transform[3] + col * transform[4] + row * transform[5]
    return x, y


# ---- argument rules (ValueError; nothing touches the library) --------------------------------------------------------------------------
def check_labels(labels):
    """-> the raster as a C-contiguous int32 array [H, W], H and W in [1, 2**31 - 1], no label negative"""
    a = np.asarray(labels)
    if a.dtype != np.int32:
        raise ValueError("Buffer dtype mismatch, expected 'int32' but got '%s'" % a.dtype)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1 or a.shape[0] >= 1 << 31 or a.shape[1] >= 1 << 31:
        raise ValueError("labels must have the shape (rows, cols), each in [1, 2**31 - 1], got %r" % (a.shape,))
    if int(a.min()) < 0:
        raise ValueError("a negative label")
    return np.ascontiguousarray(a)


def check_polygons(xy, ring_offsets, ring_label):
    """-> ``(xy, ring_offsets, ring_label)`` as int64 [nvert, 2], int64 [nring + 1], int64 [nring]"""
    xy = np.asarray(xy)
    if xy.size == 0:
        xy = np.zeros((0, 2), dtype=np.int64)
    if xy.ndim != 2 or xy.shape[1] != 2 or not np.issubdtype(xy.dtype, np.integer):
        raise ValueError("xy must be an integer array of the shape (nvert, 2), got %s %r" % (xy.dtype, xy.shape))
    off, lab = np.asarray(ring_offsets), np.asarray(ring_label)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("ring_offsets must be a 1-D integer array of nring + 1 entries")
    if lab.ndim != 1 or lab.size != off.size - 1 or not (np.issubdtype(lab.dtype, np.integer) or lab.size == 0):
        raise ValueError("ring_label must be a 1-D integer array of nring entries")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != xy.shape[0]:
        raise ValueError("ring_offsets must start at 0 and end at nvert")
    if np.any(np.diff(off) < 3):
        raise ValueError("a ring of fewer than 3 vertices")
    if lab.size and int(lab.min()) < 1:
        raise ValueError("a ring label below 1")
    return xy.astype(np.int64), off, lab.astype(np.int64)


def check_transform(transform):
    t = [float(v) for v in transform]
    if len(t) != 6 or not np.all(np.isfinite(t)) or t[1] * t[5] - t[2] * t[4] == 0.0:
        raise ValueError("the transform must be six finite numbers of an invertible geotransform, got %r" % (tuple(transform),))
    return t


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def take_polygons(handle):
    """The three arrays out of an ``mhip_polygons`` handle, which is freed."""
    lib = _lib.load()
    try:
        nring, nvert = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.call("mhip_polygons_sizes", handle, ctypes.byref(nring), ctypes.byref(nvert))
        xy = np.empty((nvert.value, 2), dtype=np.int32)      # (the fetch writes every element)
        off = np.empty(nring.value + 1, dtype=np.int64)
        lab = np.empty(nring.value, dtype=np.int32)
        _lib.call("mhip_polygons_fetch", handle, _lib.ptr(xy), _lib.ptr(off), _lib.ptr(lab))
    finally:
        lib.mhip_polygons_free.restype = None
        lib.mhip_polygons_free(handle)
    return xy, off, lab


def polygonize(labels):
    """``(xy, ring_offsets, ring_label)`` of an int32 label raster (0: background) on the device: every region's outline as rings of
    lattice vertices, cells that touch by a corner joined (``8CONNECTED=8``), holes as rings of their own with negative area, in the
    order of ``tests/_polygonize.py``.  A raster without a label gives no ring and asks for no device."""
    a = check_labels(labels)
    handle = ctypes.c_void_p()
    _lib.call("mhip_polygonize_i32", _lib.ptr(a), _lib.i64(a.shape[0]), _lib.i64(a.shape[1]), ctypes.byref(handle))
    return take_polygons(handle)


# ---- features ---------------------------------------------------------------------------------------------------------------------------
def ring_areas(xy, ring_offsets):
    """the shoelace area of every ring in cell coordinates (int64): positive for an exterior ring, negative for a hole"""
    off = np.asarray(ring_offsets, dtype=np.int64)
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    if off.size < 2:
        return np.zeros(0, dtype=np.int64)
    ring = np.repeat(np.arange(off.size - 1), np.diff(off))
    a = np.arange(xy.shape[0])
    b = np.where(a + 1 == off[1:][ring], off[:-1][ring], a + 1)      # the last vertex of a ring goes back to its first
    return np.add.reduceat(xy[a, 0] * xy[b, 1] - xy[b, 0] * xy[a, 1], off[:-1]) // 2


def _holds(ring, px, py):
    """even-odd: is the point inside the ring (int64 [n, 2]; the point is a cell centre, never on an edge)"""
    x0, y0 = ring[:, 0], ring[:, 1]
    x1, y1 = np.roll(x0, -1), np.roll(y0, -1)
    crossing = ((y0 < py) != (y1 < py)) & (x0 == x1) & (x0 > px)      # (the edges are axis-parallel: only vertical ones cross the ray)
    return bool(np.count_nonzero(crossing) & 1)


def features_from_rings(xy, ring_offsets, ring_label, transform, id_attribute='bspot_id'):
    """One GeoJSON feature per label, ascending, of the arrays ``polygonize`` gives: a ``Polygon`` for a label of one exterior ring,
    a ``MultiPolygon`` for several (a hole then goes to the exterior ring of smallest area, of its label, that holds the centre of
    the cell above the hole's first vertex); every ring starts at its first vertex and is closed by it, exterior rings run
    counter-clockwise in world coordinates (a north-up transform mirrors the cell coordinates: the vertices then come in reverse
    order); world coordinates by the six-term ``transform`` in float64.  The label is the property ``id_attribute`` and the feature's id."""
    xy, off, lab = check_polygons(xy, ring_offsets, ring_label)
    t = check_transform(transform)
    if not isinstance(id_attribute, str) or not id_attribute:
        raise ValueError("id_attribute must be a non-empty string, got %r" % (id_attribute,))
    nring = lab.size
    if nring == 0:
        return []
    area = ring_areas(xy, off)
    # every ring closed, all vertices to world coordinates at once
    n = np.diff(off)
    coff = off + np.arange(nring + 1)
    j = np.arange(coff[-1]) - np.repeat(coff[:-1], n + 1)              # position in the closed ring, 0 .. n
    nn = np.repeat(n, n + 1)
    # a ring of positive area in cell coordinates (y down) runs clockwise on the map when the transform is north-up: RFC 7946 wants
    # the exterior counter-clockwise, so the ring is walked backwards from its first vertex there
    flip = t[1] * t[5] - t[2] * t[4] < 0.0
    src = np.repeat(off[:-1], n + 1) + ((nn - j) % nn if flip else j % nn)
    cx, cy = xy[src, 0].astype(np.float64), xy[src, 1].astype(np.float64)
    world = np.stack([t[0] + cx * t[1] + cy * t[2], t[3] + cx * t[4] + cy * t[5]], axis=1)
    order = np.argsort(lab, kind="stable")                              # the rings of a label, in ring order
    bounds = np.flatnonzero(np.diff(lab[order])) + 1
    features = []
    for rings in np.split(order, bounds):
        label = int(lab[rings[0]])
        ext = [int(k) for k in rings if area[k] > 0]
        holes = [int(k) for k in rings if area[k] < 0]
        coords = lambda k: world[coff[k]:coff[k + 1]].tolist()
        if len(ext) == 1:
            geometry = dict(type="Polygon", coordinates=[coords(ext[0])] + [coords(k) for k in holes])
        else:
            parts = {k: [coords(k)] for k in ext}
            by_area = sorted(ext, key=lambda k: (int(area[k]), k))
            for h in holes:
                px, py = float(xy[off[h], 0]) + 0.5, float(xy[off[h], 1]) - 0.5
                home = next((k for k in by_area if _holds(xy[off[k]:off[k + 1]], px, py)), None)
                if home is None:
                    raise ValueError("a hole of label %d lies in none of its exterior rings" % label)
                parts[home].append(coords(h))
            geometry = dict(type="MultiPolygon", coordinates=[parts[k] for k in ext])
        features.append(dict(type="Feature", id=label, properties={id_attribute: label}, geometry=geometry))
    return features


def vectorize_labels(labels, transform, id_attribute='bspot_id'):
    """The features of an int32 label raster: ``polygonize`` then ``features_from_rings``."""
    check_transform(transform)
    return features_from_rings(*polygonize(labels), transform, id_attribute)


def vectorize_labels_file(labeled_file, id_attribute='bspot_id'):
    """Vectorize a bluespot id raster file (reference vector.py:42-87): yields GeoJSON features, read through ``io.RasterReader``.
    The file must hold integers (a float raster is ``ValueError``: nothing is rounded) and carry a geotransform."""
    from .io import RasterReader
    with RasterReader(labeled_file) as reader:
        labels, transform = reader.read(), reader.transform
    if transform is None:
        raise ValueError("%s carries no geotransform" % (labeled_file,))
    check_transform(transform)
    labels = np.asarray(labels)
    if not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("%s holds %s values: a label raster holds integers" % (labeled_file, labels.dtype))
    if labels.size and (int(labels.max()) > np.iinfo(np.int32).max or int(labels.min()) < 0):
        raise ValueError("%s holds a label that is negative or beyond int32" % (labeled_file,))
    for feature in vectorize_labels(np.ascontiguousarray(labels, dtype=np.int32), transform, id_attribute):
        yield feature
