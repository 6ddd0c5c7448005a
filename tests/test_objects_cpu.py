"""CPU: the host layer of the object exposure (malstroem_amd/objects.py): what the model makes of reordered input,
GeoJSON features to rings, and every argument rule -- raised before the library is touched."""
import numpy as np
import pytest

import _zones
from malstroem_amd import objects


def star(rng, cx, cy, n, r0, r1):
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(r0, r1, n)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)


def test_ring_order_rotation_and_direction_change_nothing():
    rng = np.random.default_rng(3)
    shape = (40, 52)
    rings, zones = [], []
    for z in range(1, 13):
        cx, cy = rng.uniform(5, 47), rng.uniform(5, 35)
        rings.append(star(rng, cx, cy, int(rng.integers(3, 10)), 4, 12))
        zones.append(z)
        if z % 3 == 0:      # a hole
            rings.append(star(rng, cx, cy, 5, 1, 3))
            zones.append(z)
    want = _zones.rasterize(shape, *_zones.pack(rings, zones), 12)
    assert len(np.unique(want)) > 8
    perm = rng.permutation(len(rings))
    again = _zones.rasterize(shape, *_zones.pack([rings[i] for i in perm], [zones[i] for i in perm]), 12)
    assert again.tobytes() == want.tobytes()
    turned = [np.roll(r, int(rng.integers(0, len(r))), axis=0)[::(-1 if k % 2 else 1)] for k, r in enumerate(rings)]
    assert _zones.rasterize(shape, *_zones.pack(turned, zones), 12).tobytes() == want.tobytes()
    # a repeated first vertex is an edge of no length
    closed = [np.concatenate([r, r[:1]]) for r in rings]
    assert _zones.rasterize(shape, *_zones.pack(closed, zones), 12).tobytes() == want.tobytes()


GT = (1000.0, 2.0, 0.0, 5000.0, 0.0, -2.0)


def world(pts):
    """cell coordinates (x, y) as world coordinates of GT"""
    return [[GT[0] + x * GT[1], GT[3] + y * GT[5]] for x, y in pts]


def closed(pts):
    return world(list(pts) + [pts[0]])


def test_rings_from_features():
    outer, hole, part = _zones.rect(1, 1, 11, 9), _zones.rect(4, 3, 8, 6), _zones.rect(12, 2, 15, 4)
    feats = [dict(type="Feature", properties={}, geometry=dict(type="Polygon", coordinates=[closed(outer), closed(hole)])),
             dict(type="Feature", id="parts", properties={}, geometry=dict(type="MultiPolygon", coordinates=[[closed(part)], [closed(hole)]])),
             dict(type="Feature", properties={}, geometry=dict(type="Polygon", coordinates=[]))]
    xy, off, zone, nzone = objects.rings_from_features(feats, GT)
    assert nzone == 3 and zone.tolist() == [1, 1, 2, 2] and off.tolist() == [0, 5, 10, 15, 20]
    assert xy.dtype == np.float64 and xy.shape == (20, 2) and xy[:5].tolist() == [list(map(float, p)) for p in outer + [outer[0]]]
    objects.check_rings(xy, off, zone, nzone)
    z = _zones.rasterize((12, 16), xy, off, zone, nzone)
    want = np.zeros((12, 16), dtype=np.int32)
    want[1:9, 1:11] = 1
    want[3:6, 4:8] = 2
    want[2:4, 12:15] = 2
    assert np.array_equal(z, want)
    # no features at all
    xy0, off0, zone0, n0 = objects.rings_from_features([], GT)
    assert xy0.shape == (0, 2) and off0.tolist() == [0] and zone0.size == 0 and n0 == 0
    assert objects.rasterize((3, 4), xy0, off0, zone0, 0).tolist() == [[0] * 4] * 3      # (asks for no device)
    with pytest.raises(ValueError, match="north-up"):
        objects.rings_from_features(feats, (0, 1, 0.5, 0, 0, -1))
    with pytest.raises(ValueError, match="feature 0.*not Polygon"):
        objects.rings_from_features([dict(type="Feature", geometry=dict(type="LineString", coordinates=world(outer)))], GT)
    with pytest.raises(ValueError, match=r"feature 1 \(id 'x'\).*at least 3"):
        objects.rings_from_features([feats[0], dict(type="Feature", id="x", geometry=dict(type="Polygon", coordinates=[world(outer[:2])]))], GT)
    with pytest.raises(ValueError, match="feature 1.*2\\*\\*29"):
        objects.rings_from_features([feats[0], dict(type="Feature", geometry=dict(type="Polygon", coordinates=[world([(0, 0), (3e9, 0), (0, 5)])]))], GT)
    with pytest.raises(ValueError, match="not finite"):
        objects.rings_from_features([dict(type="Feature", geometry=dict(type="Polygon", coordinates=[[[0, 0], [float("nan"), 1], [2, 2]]]))], GT)


def test_every_argument_rule_raises_before_the_library_is_touched(monkeypatch):
    from malstroem_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", no_library)
    xy, off, zone = _zones.pack([_zones.rect(1, 1, 5, 4), [(0, 0), (3, 0), (0, 3)]], [1, 2])
    ok = lambda **kw: objects.rasterize(kw.pop("shape", (6, 7)), kw.pop("xy", xy), kw.pop("off", off), kw.pop("zone", zone), kw.pop("nzone", 2), **kw)
    with pytest.raises(AssertionError, match="the library was touched"):
        ok()
    bad_xy = xy.copy()
    for v in (np.nan, np.inf, -np.inf, 2.0 ** 29 + 1, -2.0 ** 29 - 1):
        bad_xy[3, 1] = v
        with pytest.raises(ValueError, match="not finite or beyond"):
            ok(xy=bad_xy)
    for o, what in (([1, 4, 7], "start at 0"), ([0, 4, 6], "end at nvert"), ([0, 4, 8], "end at nvert"), ([0, 5, 4, 7], "ring_zone"), ([0, 2, 7], "fewer than 3"),
                    ([0, 7, 7], "fewer than 3")):
        with pytest.raises(ValueError, match=what):
            ok(off=np.array(o))
    with pytest.raises(ValueError, match="decrease"):
        objects.check_rings(xy, [0, 5, 4, 7], [1, 1, 2], 2)
    for zz in ([0, 2], [1, 3], [-1, 1]):
        with pytest.raises(ValueError, match="zone id outside"):
            ok(zone=np.array(zz))
    for g in (2, -1, True, 0.5):
        with pytest.raises(ValueError, match="grow"):
            ok(grow=g)
    for n in (-1, 1 << 31, 1.5):
        with pytest.raises(ValueError, match="nzone"):
            ok(nzone=n)
    for s in ((0, 5), (5, 0), (5,), (3, 1 << 31)):
        with pytest.raises(ValueError, match="shape"):
            ok(shape=s)
    with pytest.raises(ValueError, match="nvert, 2"):
        ok(xy=np.zeros((7, 3)))
    with pytest.raises(ValueError, match="ring_zone"):
        ok(zone=np.array([1.0, 2.0]))
    # zone_stats
    v, z = np.zeros((4, 5), dtype=np.float32), np.zeros((4, 5), dtype=np.int32)
    with pytest.raises(AssertionError, match="the library was touched"):
        objects.zone_stats(v, z, 0)
    with pytest.raises(ValueError, match="float32"):
        objects.zone_stats(v.astype(np.float64), z, 0)
    with pytest.raises(ValueError, match="int32"):
        objects.zone_stats(v, z.astype(np.int64), 0)
    with pytest.raises(ValueError, match="one shape"):
        objects.zone_stats(v, z[:3], 0)
    with pytest.raises(ValueError, match="nzone"):
        objects.zone_stats(v, z, -1)


def test_the_model_of_the_statistics():
    v = np.array([[np.nan, -0.0, 1e-40, 2.0], [-1, 0.0, np.inf, -np.inf]], dtype=np.float32)
    rec = _zones.zone_stats(v, np.array([[0, 1, 1, 2], [2, 1, 0, 3]], dtype=np.int32), 4)
    assert rec["cells"].tolist() == [2, 3, 2, 1, 0] and rec["pos"].tolist() == [1, 1, 1, 0, 0]
    assert rec["vmax"].tolist() == [np.inf, float(np.float32(1e-40)), 2.0, -np.inf, -np.inf]
    assert rec["vmin_pos"].tolist() == [np.inf, float(np.float32(1e-40)), 2.0, np.inf, np.inf]
    only_zero = _zones.zone_stats(np.array([-0.0, np.nan], dtype=np.float32), np.array([1, 1], dtype=np.int32), 1)
    assert only_zero["vmax"][1] == 0.0 and not np.signbit(only_zero["vmax"][1]) and only_zero["cells"][1] == 2
    with pytest.raises(ValueError):
        _zones.zone_stats(v, np.full((2, 4), 5, dtype=np.int32), 4)
    assert _zones.ZONE_DTYPE == __import__("malstroem_amd._lib", fromlist=["x"]).ZONE_DTYPE and _zones.ZONE_DTYPE.itemsize == 32


def test_the_library_refuses_bad_arguments_before_it_asks_for_a_device():
    """MHIP_EINVAL comes from the host arrays alone: the same answers with and without a GPU"""
    from malstroem_amd import _lib
    _lib.build()
    xy, off, zone = _zones.pack([_zones.rect(1, 1, 5, 4), [(0, 0), (3, 0), (0, 3)]], [1, 2])
    out = np.full((6, 7), -1, dtype=np.int32)

    def call(H=6, W=7, nvert=7, xy=xy, nring=2, off=off, zone=zone, nzone=2, grow=0):
        _lib.call("mhip_rasterize_zones_i32", _lib.i64(H), _lib.i64(W), _lib.i64(nvert), _lib.ptr(np.ascontiguousarray(xy, dtype=np.float64)), _lib.i64(nring),
                  _lib.ptr(np.ascontiguousarray(off, dtype=np.int64)), _lib.ptr(np.ascontiguousarray(zone, dtype=np.int32)), _lib.i64(nzone), int(grow),
                  _lib.ptr(out))
    bad_xy = xy.copy()
    bad_xy[5, 0] = np.inf
    for kw, what in ((dict(xy=bad_xy), "not finite"), (dict(xy=np.where(xy == 5, 2.0 ** 29 + 64, xy)), "beyond 2\\*\\*29"), (dict(off=[1, 4, 7]), "start at 0"),
                     (dict(off=[0, 4, 6]), "end at nvert"), (dict(off=[0, 9, 7]), "decrease"), (dict(off=[0, 5, 7]), "fewer than 3"), (dict(zone=[1, 3]), "zone id"),
                     (dict(zone=[0, 1]), "zone id"), (dict(grow=2), "grow"), (dict(grow=-1), "grow"), (dict(nvert=-1), "negative count"),
                     (dict(nring=-1), "negative count"), (dict(nzone=-1), "negative count"), (dict(H=0), "H, W"), (dict(W=0), "H, W")):
        with pytest.raises(ValueError, match=what):
            call(**kw)
    assert (out == -1).all()
    # no rings: the zero raster from the host, whatever the machine
    call(nvert=0, xy=np.zeros((0, 2)), nring=0, off=[0], zone=np.zeros(0, dtype=np.int32), nzone=5, grow=1)
    assert not out.any()
    rec = np.zeros(1, dtype=_lib.ZONE_DTYPE)
    with pytest.raises(ValueError, match="zone_stats_f32"):
        _lib.call("mhip_zone_stats_f32", _lib.ptr(np.zeros(4, dtype=np.float32)), _lib.ptr(np.zeros(4, dtype=np.int32)), _lib.i64(4), _lib.i64(0), _lib.i64(-1),
                  _lib.ptr(rec))
