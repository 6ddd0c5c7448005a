"""GPU: object exposure (csrc/zones.hip, malstroem_amd/objects.py) against its definition, the NumPy model
tests/_zones.py, bit for bit: the zone raster of polygons, the statistics of a float32 raster per zone, the context that keeps the
zones next to the resident rasters, and ``complete`` with an objects file.  Everything is exact: nothing here has a tolerance."""
import ctypes
import json

import numpy as np
import pytest

import _zones
from _cases import fixtures

pytestmark = pytest.mark.gpu


def check(shape, xy, off, zone, nzone, grow=0):
    from malstroem_amd.objects import rasterize
    want = _zones.rasterize(shape, xy, off, zone, nzone, grow)
    got = rasterize(shape, xy, off, zone, nzone, grow)
    assert got.dtype == np.int32 and got.shape == tuple(shape)
    assert got.tobytes() == want.tobytes(), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])
    return want


def check_stats(data, zones, nzone):
    from malstroem_amd.objects import zone_stats
    want = _zones.zone_stats(data, zones, nzone)
    got = zone_stats(data, zones, nzone)
    assert got.tobytes() == want.tobytes(), (np.flatnonzero(got != want)[:5], got[got != want][:3], want[got != want][:3])
    return want


# ---- random objects -----------------------------------------------------------------------------------------------------------------
def crowd(shape, seed, n=300):
    """n objects on `shape`: 3- to 12-gons (self-intersecting as they come), stars, stars with a hole, zones of several rings; a third
    snapped to halves.  -> (rings, zones, nzone)"""
    rng = np.random.default_rng(seed)
    H, W = shape
    rings, zones = [], []
    span = max(2.0, min(25.0, 0.1 * float(np.sqrt(H * W))))

    def star(cx, cy, nv, r0, r1):
        ang = np.sort(rng.uniform(0, 2 * np.pi, nv))
        rad = rng.uniform(r0, r1, nv)
        return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)
    for z in range(1, n + 1):
        cx, cy = rng.uniform(-4, W + 4), rng.uniform(-4, H + 4)
        kind = z % 4
        mine = []
        if kind == 0:
            nv = int(rng.integers(3, 13))
            mine.append(np.stack([cx + rng.uniform(-span, span, nv), cy + rng.uniform(-span, span, nv)], axis=1))
        elif kind == 1:
            mine.append(star(cx, cy, int(rng.integers(5, 13)), 0.3 * span, span))
        elif kind == 2:
            mine.append(star(cx, cy, int(rng.integers(5, 13)), 0.5 * span, span))
            mine.append(star(cx, cy, int(rng.integers(3, 7)), 0.1 * span, 0.4 * span)[::-1])
        else:
            for _ in range(int(rng.integers(2, 5))):
                mine.append(star(cx + rng.uniform(-span, span), cy + rng.uniform(-span, span), int(rng.integers(3, 8)), 0.1 * span, 0.5 * span))
        if z % 3 == 0:
            mine = [np.round(r * 2) / 2 for r in mine]
        rings += mine
        zones += [z] * len(mine)
    return rings, zones, n


SHAPES = [(130, 257), (130, 256), (1, 300), (200, 1), (64, 64)]


@pytest.fixture(scope="module")
def crowds():
    return {shape: crowd(shape, 100 + k) for k, shape in enumerate(SHAPES)}


@pytest.mark.parametrize("grow", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_objects(crowds, shape, grow):
    from malstroem_amd.objects import rasterize
    rings, zones, nzone = crowds[shape]
    xy, off, zone = _zones.pack(rings, zones)
    want = check(shape, xy, off, zone, nzone, grow)
    assert len(np.unique(want)) > 12 and (want == 0).any()
    # the rings in another order, every ring rotated and every other one turned round: identical bytes
    rng = np.random.default_rng(7)
    perm = rng.permutation(len(rings))
    turned = [np.roll(rings[i], int(rng.integers(0, len(rings[i]))), axis=0)[::(-1 if k % 2 else 1)] for k, i in enumerate(perm)]
    again = rasterize(shape, *_zones.pack(turned, [zones[i] for i in perm]), nzone, grow)
    assert again.tobytes() == want.tobytes()


def test_far_vertices_and_objects_outside():
    far = 5e8
    shape = (11, 64)
    rings = [[(-far, 2.2), (far, 3.9), (far, 7.1), (-far, 5.3)],                 # a band across the raster
             [(-far, -far), (far, -far), (far, far), (-far, far)],               # all of it
             [(10.3, -far), (30.7, -far), (far, 6.4), (20.1, far)],              # steep edges, crossings beyond W
             [(-far, 4.0), (-3.0, 1.5), (-far + 9, 9.0)],                        # crossings left of column 0
             [(70.5, 2.0), (far, 3.0), (80.0, 9.5)],                             # wholly right
             [(5, -far), (9, -far), (9, -2.0), (5, -2.0)],                       # wholly above
             [(5, 12.0), (9, 12.5), (9, far), (5, far)],                         # wholly below
             [(-far, 0.1), (far, 10.7), (far, 10.9), (-far, 0.3)],               # a sliver over the centres of row 5
             [(-2.5, -3.5), (40.5, -3.5), (40.5, 5.5), (-2.5, 5.5)]]             # over two edges of the raster
    zones = [3, 1, 5, 6, 7, 8, 9, 4, 2]
    xy, off, zone = _zones.pack(rings, zones)
    want = check(shape, xy, off, zone, 9)
    assert (want >= 1).all() and not np.isin(want, (7, 8, 9)).any() and (want[:5, :40] >= 2).all() and (want == 6).sum() == 0
    check(shape, xy, off, zone, 9, grow=1)
    # each alone; the ones outside write nothing
    for ring, z in zip(rings, zones):
        one = check(shape, *_zones.pack([ring], [z]), 9)
        assert one.any() == (z not in (6, 7, 8, 9))
    with pytest.raises(ValueError, match="2\\*\\*29"):
        from malstroem_amd import _lib
        bad = np.array([[0.0, 0.0], [6e8, 0.0], [0.0, 5.0]])
        out = np.zeros(shape, dtype=np.int32)
        _lib.call("mhip_rasterize_zones_i32", _lib.i64(11), _lib.i64(64), _lib.i64(3), _lib.ptr(bad), _lib.i64(1), _lib.ptr(np.array([0, 3], dtype=np.int64)),
                  _lib.ptr(np.array([1], dtype=np.int32)), _lib.i64(1), 0, _lib.ptr(out))


def test_a_comb_of_600_teeth():
    """1200 crossings on each of two scanlines"""
    pts = []
    for i in range(600):
        pts += [(4 * i + 0.25 * (i % 3), 0.1), (4 * i + 2, 0.1), (4 * i + 2.5, 2.2), (4 * i + 4, 2.2)]
    pts += [(2400, 2.9), (0, 2.9)]
    xy, off, zone = _zones.pack([pts, _zones.rect(100, 0, 300, 3)], [1, 2])
    z, r, cf = _zones.crossings((3, 2500), xy, off, zone)
    assert np.bincount(r[z == 1]).tolist() == [1200, 1200, 2]
    want = check((3, 2500), xy, off, zone, 2)
    assert (want[0] == 1).sum() > 1000 and (want[2, :2400] >= 1).all() and not want[:, 2400:].any()
    check((3, 2500), xy, off, zone, 2, grow=1)


def test_overlap_and_growing_at_edges_and_seams():
    shape = (70, 520)
    rings = [_zones.rect(10, 5, 500, 60), _zones.rect(40, 10, 300, 50), _zones.rect(100, 20, 200, 40), _zones.rect(150, 0, 160, 70)]
    want = check(shape, *_zones.pack(rings, [1, 2, 3, 4]), 4)
    assert want[30, 155] == 4 and want[30, 120] == 3 and want[15, 50] == 2 and want[7, 20] == 1 and want[2, 2] == 0
    assert check(shape, *_zones.pack(rings[::-1], [1, 2, 3, 4]), 4)[28:32, 118:122].tolist() == [[4] * 4] * 4       # (the ids the other way round: still the largest)
    # growing: blocks that touch the raster's edges and the seams of the 32 x 256 tiles, one free cell between neighbours
    rng = np.random.default_rng(5)
    blocks, ids = [], []
    for k, (x, y) in enumerate([(0, 0), (254, 30), (257, 30), (255, 33), (517, 66), (0, 66), (517, 0), (250, 62), (256, 0), (100, 31), (102, 31),
                                (100, 33), (511, 31), (513, 33)]):
        blocks.append(_zones.rect(x, y, x + int(rng.integers(1, 4)), y + int(rng.integers(1, 4))))
        ids.append(int(rng.integers(1, 10)))
    plain = check(shape, *_zones.pack(blocks, ids), 9)
    grown = check(shape, *_zones.pack(blocks, ids), 9, grow=1)
    assert np.array_equal(grown[plain > 0], plain[plain > 0]) and (grown > 0).sum() > (plain > 0).sum() + 40
    between = _zones.pack([_zones.rect(3, 3, 5, 6), _zones.rect(6, 3, 8, 6)], [2, 7])
    assert check((9, 11), *between, 7, grow=1)[2:7, 5].tolist() == [7] * 5
    assert check((1, 1), *_zones.pack([_zones.rect(0, 0, 1, 1)], [1]), 1, grow=1).tolist() == [[1]]
    assert check((2, 2), *_zones.pack([_zones.rect(1, 1, 2, 2)], [3]), 5, grow=1).tolist() == [[3, 3], [3, 3]]
    # rings that hold no cell centre, and no crossing at all
    assert not check((5, 5), *_zones.pack([_zones.rect(1.6, 1.6, 2.4, 2.4), [(0, 1), (4, 1), (2, 1)]], [1, 2]), 2, grow=1).any()


def test_limits():
    """more than 2**31 - 1 crossings: a million tall slivers, two edges each over 1100 rows, would be 2.2e9"""
    from malstroem_amd.objects import rasterize
    n = 1000001
    x = np.arange(n, dtype=np.float64) * 0.001
    rings = np.stack([np.stack([x, np.full(n, -1.0)], 1), np.stack([x + 0.0005, np.full(n, 3000.0)], 1), np.stack([x + 0.001, np.full(n, -1.0)], 1)], 1)
    xy = rings.reshape(-1, 2)
    off = np.arange(n + 1, dtype=np.int64) * 3
    with pytest.raises(OverflowError, match="crossings"):
        rasterize((1100, 8), xy, off, np.ones(n, dtype=np.int32), 1)


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
def awkward(shape, seed):
    """float32 values with NaN, both zeros, negatives, subnormals and infinities among them"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 3, shape).astype(np.float32)
    pick = rng.integers(0, 12, shape)
    for k, x in enumerate((np.nan, 0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, 1.4e-45)):
        v[pick == k] = np.float32(x)
    return v


@pytest.mark.parametrize("shape", [(130, 257), (130, 256), (1, 300), (200, 1), (64, 64)])
def test_zone_stats_over_random_objects(crowds, shape):
    rings, zones, nzone = crowds[shape]
    zr = _zones.rasterize(shape, *_zones.pack(rings, zones), nzone)
    data = awkward(shape, 9)
    want = check_stats(data, zr, nzone + 7)      # (zones without a cell among them)
    empty = want[want["cells"] == 0]
    assert len(empty) >= 7 and np.all(empty["vmax"] == -np.inf) and np.all(empty["vmin_pos"] == np.inf) and not empty["pos"].any()
    check_stats(data.ravel(), zr.ravel(), nzone + 7)      # (a flat array)
    check_stats(data, np.zeros(shape, dtype=np.int32), 1)
    check_stats(data, np.ones(shape, dtype=np.int32), 1)
    check_stats(np.full(shape, np.nan, dtype=np.float32), zr, nzone)
    check_stats(np.full(shape, -0.0, dtype=np.float32), zr, nzone)


def test_zone_stats_with_more_zones_in_a_tile_than_its_table_holds():
    shape = (100, 100)
    r, c = np.mgrid[0:100, 0:100]
    board = ((r + c) % 2 == 0)
    zr = np.zeros(shape, dtype=np.int32)
    zr[board] = np.random.default_rng(3).permutation(5000) + 1
    want = check_stats(awkward(shape, 10), zr, 5000)
    assert want["cells"].tolist() == [5000] + [1] * 5000
    # ... and long runs of few zones next to them
    zr[40:60] = 77
    check_stats(awkward(shape, 11), zr, 5000)


def test_a_zone_outside_the_range_is_refused():
    from malstroem_amd.objects import zone_stats
    v = awkward((40, 300), 12)
    for bad in (6, -1, 2 ** 31 - 1, -2 ** 31):
        zr = np.random.default_rng(13).integers(0, 6, (40, 300)).astype(np.int32)
        zone_stats(v, zr, 5)
        zr[33, 257] = bad
        with pytest.raises(ValueError, match="outside"):
            zone_stats(v, zr, 5)


# ---- context -------------------------------------------------------------------------------------------------------------------------
def test_the_dam_valley():
    """the 40 x 48 valley behind a dam of tests/test_gpu_burn.py: one bluespot of 61 cells, 2.75 deep"""
    from malstroem_amd.pipeline import HydroPipeline
    r, c = np.mgrid[0:40, 0:48]
    dem = (20 - 0.25 * c + 0.5 * np.abs(r - 20)).astype(np.float32)
    dem[:, 20:23] += 3
    with HydroPipeline(dem.shape) as p:
        p.upload("dem", dem)
        p.run("fill", "label")
        p.apply_keep(None)
        p.rasterize_zones(*_zones.pack([_zones.rect(0, 0, 48, 40)], [1]), 1)
        rec = p.zone_stats("depths")
        assert (rec["cells"][1], rec["pos"][1], rec["vmax"][1]) == (1920, 61, 2.75) and rec["cells"][0] == 0
        assert rec["vmin_pos"][1] == p.download("depths")[p.download("depths") > 0].min()
        assert p.download_zones().tolist() == [[1] * 48] * 40


def test_every_source_of_a_context_and_what_the_zones_survive():
    from malstroem_amd.pipeline import HydroPipeline
    dtm = fixtures()["dtm"]
    H, W = dtm.shape
    rings, zones, nzone = crowd((H, W), 21, n=60)
    xy, off, zone = _zones.pack(rings, zones)
    want_z = _zones.rasterize((H, W), xy, off, zone, nzone, 1)

    def chain(p):
        p.run("fill", "noflat", "flowdir", "label")
        n = p.apply_keep(None)
        p.hypsometry(0.05)
        q = np.full((2, n + 1), 0.5)
        p.final_depths(q[0])
        p.wet_at(q * np.array([[1.0], [3.0]]), [10.0, 20.0])
        p.flow_distance(1.6)

    def compare(p, wz, nz):
        rasters = dict(dem=p.download("dem"), filled=p.download("filled"), depths=p.download("depths"), finaldepths=p.download("finaldepths"),
                       wet_at=p.download_wet_at(), flow_distance=p.download_flow_distance())
        for name, a in rasters.items():
            got, want = p.zone_stats(name), _zones.zone_stats(a, wz, nz)
            assert got.tobytes() == want.tobytes(), name
        return rasters
    with HydroPipeline((H, W)) as p:
        assert p.get_int("zones") == -1
        with pytest.raises(ValueError, match="rasterize_zones"):
            p.zone_stats("dem")
        with pytest.raises(ValueError, match="rasterize_zones"):
            p.download_zones()
        p.upload("dem", dtm)
        p.rasterize_zones(xy, off, zone, nzone, grow=1)
        assert p.get_int("zones") == nzone and p.download_zones().tobytes() == want_z.tobytes()
        assert p.download_zones_rows(3, 5).tobytes() == want_z[3:8].tobytes()
        assert p.zone_stats("dem").tobytes() == _zones.zone_stats(dtm, want_z, nzone).tobytes()
        # a source that has not been computed: the error of its own getter
        for name in ("filled", "depths", "finaldepths", "wet_at", "flow_distance"):
            with pytest.raises(ValueError, match="has not been computed|needs mhip_ctx_"):
                p.zone_stats(name)
        with pytest.raises(ValueError, match="source"):
            p.zone_stats("labels")
        chain(p)
        first = compare(p, want_z, nzone)
        assert (first["wet_at"] > 0).any() and (first["finaldepths"] > 0).any()
        # the zones survive an upload of the DEM and the run behind it
        dem2 = (dtm + np.float32(0.5) * (np.arange(W, dtype=np.float32) % 7)).astype(np.float32)
        p.upload("dem", dem2)
        assert p.get_int("zones") == nzone and p.download_zones().tobytes() == want_z.tobytes()
        with pytest.raises(ValueError):
            p.zone_stats("depths")
        chain(p)
        second = compare(p, want_z, nzone)
        assert second["depths"].tobytes() != first["depths"].tobytes()
        # a second rasterize replaces them
        xy2, off2, zone2 = _zones.pack([_zones.rect(3, 4, W - 5.5, H - 2.5), _zones.rect(0, 0, 10, 10)], [2, 5])
        p.rasterize_zones(xy2, off2, zone2, 6)
        wz2 = _zones.rasterize((H, W), xy2, off2, zone2, 6)
        assert p.get_int("zones") == 6 and p.download_zones().tobytes() == wz2.tobytes()
        compare(p, wz2, 6)
        # no rings: the zero raster; a call refused for its arguments changes nothing
        p.rasterize_zones(np.zeros((0, 2)), [0], np.zeros(0, dtype=np.int32), 3)
        assert p.get_int("zones") == 3 and not p.download_zones().any() and p.zone_stats("dem")["cells"].tolist() == [H * W, 0, 0, 0]
        with pytest.raises(ValueError):
            p.rasterize_zones(xy2, off2, zone2, 4)
        assert p.get_int("zones") == 3 and not p.download_zones().any()


def test_a_row_band_refuses():
    from malstroem_amd import _lib
    from malstroem_amd.distributed import HipBand
    xy, off, zone = _zones.pack([_zones.rect(1, 1, 5, 6)], [1])
    rec = np.zeros(2, dtype=_lib.ZONE_DTYPE)
    band = HipBand(64, 48, 0, 32, device=0, rank=0, size=2)
    try:
        band.upload("dem", np.zeros((32, 48), dtype=np.float32))
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_rasterize_zones", band._ctx, _lib.i64(4), _lib.ptr(xy), _lib.i64(1), _lib.ptr(off), _lib.ptr(zone), _lib.i64(1), 0)
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_zone_stats", band._ctx, ctypes.c_int32(_lib.R_DEM), _lib.ptr(rec))
    finally:
        band.close()


# ---- tools ---------------------------------------------------------------------------------------------------------------------------
def test_complete_with_objects(tmp_path):
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterReader, RasterWriter, VectorReader
    from malstroem_amd.objects import rings_from_features
    fx = fixtures()
    dtm = fx["dtm"]
    gt = tuple(float(v) for v in fx["geotransform"])
    H, W = dtm.shape
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(dtm)
    rng = np.random.default_rng(60)
    world = lambda pts: [[gt[0] + x * gt[1], gt[3] + y * gt[5]] for x, y in pts]
    feats = []
    for k in range(36):
        x, y = rng.uniform(2, W - 8), rng.uniform(2, H - 8)
        w, h = rng.uniform(1.5, 7), rng.uniform(1.5, 7)
        ring = _zones.rect(x, y, x + w, y + h)
        feats.append(dict(type="Feature", properties=dict(name="house %d" % k), geometry=dict(type="Polygon", coordinates=[world(ring + ring[:1])])))
    yard, hole = _zones.rect(10, 10, 30, 24), _zones.rect(14, 13, 22, 20)
    feats.append(dict(type="Feature", id="yard", properties={}, geometry=dict(type="Polygon", coordinates=[world(yard + yard[:1]), world(hole + hole[:1])])))
    feats.append(dict(type="Feature", properties=dict(name="two parts"),
                      geometry=dict(type="MultiPolygon", coordinates=[[world(_zones.rect(40, 5, 44, 9))], [world(_zones.rect(50, 30, 53, 36))]])))
    feats.append(dict(type="Feature", properties=dict(name="outside"), geometry=dict(type="Polygon", coordinates=[world(_zones.rect(-20, -20, -10, -10))])))
    path = str(tmp_path / "objects.geojson")
    with open(path, "w") as fh:
        json.dump(dict(type="FeatureCollection", features=feats), fh)
    outs = {}
    for name, kw in (("plain", {}), ("objects", dict(objects=path))):
        d = tmp_path / name
        d.mkdir()
        outs[name] = (d, process_all(src, str(d), [10, 100], finalstate=True, onset=True, **kw))
    (d0, r0), (d1, r1) = outs["plain"], outs["objects"]
    assert "objects" not in r0 and not (d0 / "vector" / "objects.geojson").exists()
    # every other output: byte for byte what it is without the argument
    names0 = sorted(str(f.relative_to(d0)) for f in d0.rglob("*") if f.is_file())
    names1 = sorted(str(f.relative_to(d1)) for f in d1.rglob("*") if f.is_file())
    assert [n for n in names1 if n not in names0] == [str((d1 / "vector" / "objects.geojson").relative_to(d1))] and len(names0) >= 12
    for n in names0:
        assert (d0 / n).read_bytes() == (d1 / n).read_bytes(), n
    # the layer against the model on the written rasters
    xy, off, zone, nzone = rings_from_features(feats, gt)
    assert nzone == len(feats) == 39
    zr = _zones.rasterize((H, W), xy, off, zone, nzone, grow=1)
    read = lambda f: RasterReader(str(d1 / f)).read()
    dep = _zones.zone_stats(read("bs_depths.tif"), zr, nzone)
    wet = _zones.zone_stats(read("wet_at.tif"), zr, nzone)
    fin = {tag: _zones.zone_stats(read("finaldepths_%s.tif" % tag), zr, nzone) for tag in ("10", "100")}
    layer = VectorReader(r1["objects"]).read_geojson_features()
    assert len(layer) == len(feats)
    for k, (f, g) in enumerate(zip(feats, layer)):
        p = g["properties"]
        assert g["geometry"] == f["geometry"] and all(p[key] == v for key, v in f["properties"].items())
        assert p["cells"] == dep["cells"][k + 1] and p["bs_wet_cells"] == dep["pos"][k + 1]
        assert p["bs_dmax"] == (float(dep["vmax"][k + 1]) if dep["cells"][k + 1] else None)
        assert p["wet_at_mm"] == (float(wet["vmin_pos"][k + 1]) if wet["pos"][k + 1] else None)
        for tag in ("10", "100"):
            assert p["depth_" + tag] == (float(fin[tag]["vmax"][k + 1]) if dep["cells"][k + 1] else None)
    props = [g["properties"] for g in layer]
    assert layer[36]["id"] == "yard" and props[38]["cells"] == 0 and props[38]["bs_dmax"] is None and props[38]["wet_at_mm"] is None
    assert sum(p["bs_wet_cells"] > 0 for p in props) >= 5 and {p["wet_at_mm"] for p in props} >= {None, 10.0}
    # without growing the footprints are smaller
    d2 = tmp_path / "nogrow"
    d2.mkdir()
    r2 = process_all(src, str(d2), [10, 100], objects=path, objects_grow=0)
    plain = VectorReader(r2["objects"]).read_geojson_features()
    z0 = _zones.zone_stats(read("bs_depths.tif"), _zones.rasterize((H, W), xy, off, zone, nzone), nzone)
    assert [g["properties"]["cells"] for g in plain] == z0["cells"][1:].tolist() and "wet_at_mm" not in plain[0]["properties"]
    assert sum(g["properties"]["cells"] for g in plain) < sum(p["cells"] for p in props)
