"""GPU: DEM adaptations (csrc/burn.hip, malstroem_amd/adaptations.py) against their definition, the NumPy model
tests/_burn.py, bit for bit -- the adapted raster and the per-line records -- and against known answers of the oracle's hydrology
on the adapted DEMs.  Min and max are exact and commutative, so nothing here needs a tolerance."""
import ctypes
import json
from collections import OrderedDict

import numpy as np
import pytest

import _burn
import oracle
from _cases import fbm, fixtures

pytestmark = pytest.mark.gpu

NAN = float("nan")


def check(dem, lines, segs, nodata=NAN):
    """one stateless call against the model: -> (adapted, results) of the model"""
    from malstroem_amd.adaptations import burn_lines
    want, wres = _burn.burn(dem, lines, segs, nodata)
    got, res = burn_lines(dem, lines, segs, nodata)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    assert res.tobytes() == wres.tobytes(), (res[res != wres][:5], wres[res != wres][:5])
    return want, wres


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_every_octant_and_slope(flags):
    """from (11, 14) to every cell of the square ring of radius 9 around it, and segments of no length, one line each"""
    rng = np.random.default_rng(20 + flags)
    dem = rng.normal(5, 2, (23, 29)).astype(np.float32)
    ring = [(11 + dr, 14 + dc) for dr in range(-9, 10) for dc in range(-9, 10) if max(abs(dr), abs(dc)) == 9]
    assert len(ring) == 72
    verts = [[(11, 14), p] for p in ring] + [[(3, 4)], [(22, 28)], [(0, 0)], [(-1, 5)], [(23, 0)]]
    n = len(verts)
    # half of the lines between explicit levels, half from the DEM's own values
    z0 = np.where(np.arange(n) % 2 == 0, rng.normal(5, 2, n), np.nan)
    z1 = np.where(np.arange(n) % 2 == 0, rng.normal(5, 2, n), np.nan)
    lines, segs = _burn.polylines(verts, z0, z1, flags)
    want, res = check(dem, lines, segs)
    assert res["status"][-2:].tolist() == [1, 0] and res["cells"][-2:].tolist() == [0, 0]      # a vertex outside: sampled / explicit levels
    assert np.sum(want != dem) > 100
    # one line alone, sampled ends: its end cells are never moved by the line itself
    for p in ring[::7]:
        l1, s1 = _burn.polylines([[(11, 14), p]], flags=flags)
        w1, _ = check(dem, l1, s1)
        assert w1[11, 14] == dem[11, 14] and w1[p] == dem[p]


def test_far_ends_skipped_lines_and_nan_cells():
    far = 5 * 10 ** 8
    rng = np.random.default_rng(31)
    dem = rng.normal(0, 1, (11, 64)).astype(np.float32)       # (levels of both signs)
    dem[5, 20] = np.nan
    dem[2, 9] = -999.0
    verts = [[(3, -far), (8, far)], [(9, far), (1, -far)], [(-far, 30), (far, 33)], [(-far, -far), (far, far)], [(-far + 7, far), (far + 9, -far)],      # crossing
             [(20, -far), (20, far)], [(-far, -3), (far, -3)], [(-9, -far), (-2, far)], [(40, 3), (12, 70)],                # wholly outside
             [(5, 10), (5, 30)], [(0, 20), (10, 20)]]                                                                       # over the NaN cell
    n = len(verts)
    lines, segs = _burn.polylines(verts, rng.normal(0, 1, n), rng.normal(0, 1, n), [0, 1, 2, 3, 0, 0, 1, 2, 3, 0, 3])
    sampled = [[(4, 3), (4, 70)], [(-1, 3), (4, 8)],            # a sampled end outside: status 1
               [(5, 20), (9, 25)], [(1, 1), (5, 20)],             # ... on a NaN cell: status 2
               [(2, 9), (7, 12)],                                 # ... on a nodata cell: status 2
               [(1, 1), (2, 9)]]
    l2, s2 = _burn.polylines(sampled, flags=[0, 1, 2, 3, 0, 1])
    s2["line"] += n
    l2["z0"][5] = 0.25                                           # (explicit at the first vertex, the nodata cell at the last)
    lines, segs = np.concatenate([lines, l2]), np.concatenate([segs, s2])
    want, res = check(dem, lines, segs, nodata=-999.0)
    assert res["status"].tolist() == [0] * n + [1, 1, 2, 2, 2, 2]
    assert res["cells"][:2].tolist() == [64, 64] and res["cells"][2:5].tolist() == [12, 22, 9] and not res["cells"][5:9].any() and not res["cells"][n:].any()
    assert np.isnan(want[5, 20]) and np.isnan(want).sum() == 1 and res["cells"][9] == 21 and res["cells"][10] == 11
    # the lines that lie wholly outside, alone: the DEM is untouched
    keep = np.arange(5, 9)
    lo, so = lines[keep], segs[np.isin(segs["line"], keep)].copy()
    so["line"] -= 5
    w2, r2 = check(dem, lo, so)
    assert w2.tobytes() == dem.tobytes() and not r2["cells"].any() and not r2["status"].any()
    # without a nodata value the cell that holds -999 is a level like any other
    _, r3 = check(dem, lines[n + 4:n + 5], _burn.polylines([sampled[4]])[1])
    assert r3["status"].tolist() == [0] and r3["z0"][0] == -999.0


def test_long_lines():
    rng = np.random.default_rng(32)
    dem = rng.normal(50, 1, (3, 70001)).astype(np.float32)
    lines, segs = _burn.polylines([[(0, 0), (2, 70000)], [(1, 70000), (1, 0)]], [49.5, NAN], [NAN, 48.0], [0, 2])
    want, res = check(dem, lines, segs)
    assert res["cells"].tolist() == [70001, 70001] and np.all(want[1] <= dem[1]) and np.sum(want != dem) > 50000


def test_polylines_and_their_joints():
    rng = np.random.default_rng(33)
    dem = rng.normal(5, 2, (31, 45)).astype(np.float32)
    verts = [[(int(rng.integers(0, 31)), int(rng.integers(0, 45))) for _ in range(nv)] for nv in (2, 3, 4, 5, 5, 3)]
    verts.append([(4, 4), (4, 4), (9, 12), (9, 12), (2, 20)])       # repeated vertices: segments of no length inside a line
    n = len(verts)
    lines, segs = _burn.polylines(verts, np.where(np.arange(n) % 2, NAN, 4.0), np.where(np.arange(n) % 3, NAN, 6.0), rng.integers(0, 4, n))
    check(dem, lines, segs)
    # a joint gets the same level from both of its segments
    for s, t in zip(segs[:-1], segs[1:]):
        if s["line"] == t["line"]:
            l = lines[s["line"]]
            ns = _burn.steps_of(s["r0"], s["c0"], s["r1"], s["c1"])
            assert t["koff"] == s["koff"] + ns and (s["r1"], s["c1"]) == (t["r0"], t["c0"])
            assert _burn.level(1.5, 7.25, s["koff"], ns, l["ntotal"], False) == _burn.level(1.5, 7.25, t["koff"], 0, l["ntotal"], False)
    # every line alone, between two levels above the terrain: a joint holds the level of its step (or of a later crossing)
    for i, vs in enumerate(verts[:4]):
        l1, s1 = _burn.polylines([vs], 100.0, 200.0, 3)
        w1, _ = check(dem, l1, s1)
        for s in s1[1:]:
            assert 200.0 >= w1[s["r0"], s["c0"]] >= _burn.level(100.0, 200.0, s["koff"], 0, l1["ntotal"][0], True) > 100.0


@pytest.fixture(scope="module")
def crowd():
    """2000 random lines of every kind on 130 x 257, overlapping heavily, and what the model makes of them"""
    rng = np.random.default_rng(34)
    H, W, n = 130, 257, 2000
    dem = rng.normal(0, 2, (H, W)).astype(np.float32)
    dem[rng.integers(0, H, 12), rng.integers(0, W, 12)] = np.nan
    verts = []
    for _ in range(n):
        r, c = int(rng.integers(-4, H + 4)), int(rng.integers(-4, W + 4))
        vs = [(r, c)]
        for _ in range(int(rng.integers(1, 4))):
            r, c = r + int(rng.integers(-25, 26)), c + int(rng.integers(-25, 26))
            vs.append((r, c))
        verts.append(vs)
    z0 = np.where(rng.random(n) < 0.5, NAN, rng.normal(0, 2, n))
    z1 = np.where(rng.random(n) < 0.5, NAN, rng.normal(0, 2, n))
    for i in range(6):      # a few lines sample a NaN cell for certain
        verts[i][0] = (10 + i, 20 + 3 * i)
        dem[verts[i][0]] = np.nan
        z0[i] = NAN
    lines, segs = _burn.polylines(verts, z0, z1, rng.integers(0, 4, n))
    want, wres = _burn.burn(dem, lines, segs)
    assert set(wres["status"].tolist()) == {0, 1, 2} and np.sum(want.view(np.uint32) != dem.view(np.uint32)) > 10000
    return dem, lines, segs, want, wres


def test_no_order_of_lines_or_segments_matters(crowd):
    from malstroem_amd.adaptations import burn_lines
    dem, lines, segs, want, wres = crowd
    got, res = burn_lines(dem, lines, segs)
    assert got.tobytes() == want.tobytes() and res.tobytes() == wres.tobytes()
    perm = np.arange(len(lines))[::-1].copy()
    l2, s2 = _burn.reorder_lines(lines, segs, perm)
    got2, res2 = burn_lines(dem, l2, s2)
    assert got2.tobytes() == want.tobytes() and res2.tobytes() == wres[perm].tobytes()
    got3, res3 = burn_lines(dem, lines, segs[np.random.default_rng(35).permutation(len(segs))])
    assert got3.tobytes() == want.tobytes() and res3.tobytes() == wres.tobytes()


@pytest.mark.parametrize("nline,nseg", [(1, 1), (1, 2), (1, 257), (257, 257), (257, 1), (2, 2)])
def test_few_and_many_segments(crowd, nline, nseg):
    """the bisection at its edges: one segment, two, and 257 of them, of one line or of one line each"""
    dem = crowd[0]
    rng = np.random.default_rng(36 + nline + nseg)
    per = nseg // nline if nseg >= nline else 0
    verts = []
    for i in range(nline):
        k = per if per else (1 if i < nseg else 0)
        r, c = int(rng.integers(0, 130)), int(rng.integers(0, 257))
        vs = [(r, c)]
        for _ in range(k):
            r, c = r + int(rng.integers(-3, 4)), c + int(rng.integers(-3, 4))
            vs.append((r, c))
        verts.append(vs)
    lines, segs = _burn.polylines([v for v in verts if len(v) > 1], -1.0, NAN, 2)
    # lines without any segment keep their place in the results
    lines = np.concatenate([lines, np.zeros(nline - len(lines), dtype=lines.dtype)])
    assert len(lines) == nline and len(segs) == nseg
    _, res = check(dem, lines, segs)
    assert not res["cells"][min(nseg, nline):].any()


# ---- hydrology ---------------------------------------------------------------------------------------------------------------------
def bluespots(dem):
    """(bluespots, largest depth, wet cells, sum of the depths) of a DEM on the device chain"""
    from malstroem_amd.pipeline import HydroPipeline
    with HydroPipeline(dem.shape) as p:
        p.upload("dem", dem)
        p.run("fill", "label")
        n = p.apply_keep(None)
        dep = p.download("depths")
    return n, float(dep.max()), int((dep > 0).sum()), float(dep.sum(dtype=np.float64))


def test_a_culvert_through_a_dam_drains_the_valley():
    from malstroem_amd.adaptations import burn_lines
    r, c = np.mgrid[0:40, 0:48]
    dem = (20 - 0.25 * c + 0.5 * np.abs(r - 20)).astype(np.float32)
    dem[:, 20:23] += 3
    assert bluespots(dem) == (1, 2.75, 61, 64.0)
    lines, segs = _burn.polylines([[(20, 19), (20, 23)]])
    got, res = burn_lines(dem, lines, segs)
    assert np.sum(got != dem) == 3 and got[20, 19:24].tolist() == [15.25, 15.0, 14.75, 14.5, 14.25]
    assert [tuple(x) for x in res] == [(15.25, 14.25, 5, 0, 0)]
    assert bluespots(got) == (0, 0.0, 0, 0.0)


@pytest.mark.parametrize("conn4,wet,dmax", [(True, 102, 3.0), (False, 0, 0.0)])
def test_a_dike_holds_water_only_when_it_is_4_connected(conn4, wet, dmax):
    from malstroem_amd.adaptations import burn_lines
    r, c = np.mgrid[0:33, 0:33]
    dem = (30 - 0.25 * (r + c)).astype(np.float32)
    lines, segs = _burn.polylines([[(22, 6), (6, 22)], [(22, 6), (10, 6)], [(6, 22), (6, 10)]], 40.0, 40.0, 3 if conn4 else 1)
    got, res = burn_lines(dem, lines, segs)
    assert got.tobytes() == _burn.burn(dem, lines, segs)[0].tobytes() and got.max() == 40.0
    n, deepest, cells, _ = bluespots(got)
    assert (cells, deepest) == (wet, dmax) and n == (1 if wet else 0)


# ---- context -------------------------------------------------------------------------------------------------------------------------
STAGES = ("fill", "noflat", "flowdir", "accum", "label", "watershed", "pourpoints")
DERIVED = ("filled", "depths", "noflat", "flowdir", "accum", "labels", "watersheds")


def observe(p):
    """what a context answers for everything derived from its DEM: bytes, a number, or 'refused'"""
    state = OrderedDict()

    def ask(key, call):
        try:
            v = call()
            state[key] = tuple(x.tobytes() for x in v) if isinstance(v, tuple) else v.tobytes() if hasattr(v, "tobytes") else v
        except ValueError:
            state[key] = "refused"
    for name in DERIVED:
        ask(name, lambda: p.download(name))
    for g in ("stats", "watershed_counts", "pourpoints", "hypsometry_tables", "flow_distance_records", "download_flow_distance", "download_wet_at"):
        ask(g, lambda: getattr(p, g)())
    for k in ("hyps_bins", "wet_at_events", "flow_distance_unresolved", "nlabels"):
        state[k] = p.get_int(k)
    return state


def full_chain(p):
    p.run(*STAGES[:5])
    n = p.apply_keep(None)
    p.run("watershed", "pourpoints")
    p.hypsometry(0.05)
    q = np.full((2, n + 1), 0.5)
    p.wet_at(q, [10.0, 20.0])
    p.flow_distance(1.6)
    return n


def test_burning_the_resident_dem_is_a_write_of_the_dem():
    from malstroem_amd.adaptations import burn_lines
    from malstroem_amd.pipeline import HydroPipeline
    shape = (160, 224)
    dem = (np.round(fbm(*shape, beta=2.0, seed=11).astype(np.float64) * 64) / 64).astype(np.float32)
    rng = np.random.default_rng(40)
    verts = [[(int(rng.integers(0, 160)), int(rng.integers(0, 224))) for _ in range(3)] for _ in range(40)]
    lines, segs = _burn.polylines(verts, flags=rng.integers(0, 4, 40))
    lines["z1"][::3] = 55.0
    adapted, wres = burn_lines(dem, lines, segs)
    assert adapted.tobytes() == _burn.burn(dem, lines, segs)[0].tobytes() and np.sum(adapted != dem) > 500
    with HydroPipeline(shape) as p, HydroPipeline(shape) as fresh, HydroPipeline(shape) as up:
        p.upload("dem", dem)
        assert full_chain(p) > 20
        before = observe(p)
        assert "refused" not in before.values() and -1 not in before.values()
        # no segments: nothing is written, everything stays valid
        r0 = p.burn_lines(lines, segs[:0])
        assert r0["status"].tolist() == [1] * 40 and observe(p) == before and p.download("dem").tobytes() == dem.tobytes()
        res = p.burn_lines(lines, segs)
        assert res.tobytes() == wres.tobytes()
        after = observe(p)
        # ... as after an upload of a DEM
        up.upload("dem", dem)
        full_chain(up)
        up.upload("dem", adapted)
        assert after == observe(up)
        assert all(after[k] == "refused" for k in after if k not in ("hyps_bins", "wet_at_events", "flow_distance_unresolved", "nlabels"))
        assert (after["hyps_bins"], after["wet_at_events"], after["flow_distance_unresolved"], after["nlabels"]) == (-1, -1, -1, -1)
        assert p.download("dem").tobytes() == adapted.tobytes()
        # the rerun is the chain of the adapted DEM
        fresh.upload("dem", adapted)
        assert full_chain(p) == full_chain(fresh)
        again, want = observe(p), observe(fresh)
        assert "refused" not in again.values() and "refused" not in want.values()
        # (the float64 sums of the statistics and of the tables, and what hangs on them, may end in other bits from run to run: the
        # adapted levels are no multiples of 1/64)
        for k in DERIVED + ("watershed_counts", "pourpoints", "flow_distance_records", "download_flow_distance", "hyps_bins", "nlabels"):
            assert again[k] == want[k], k
        sa, sw = p.stats(), fresh.stats()
        assert all(np.array_equal(sa[f], sw[f]) for f in ("min", "max", "count")) and np.allclose(sa["sum"], sw["sum"], rtol=1e-12, atol=0)
        # a second adaptation of the adapted DEM
        l2, s2 = _burn.polylines([[(80, 0), (80, 223)]], 70.0, 70.0, 3)
        p.burn_lines(l2, s2)
        assert p.download("dem").tobytes() == _burn.burn(adapted, l2, s2)[0].tobytes()
        with pytest.raises(ValueError):
            p.burn_lines(lines, segs[["r0", "c0"]])
        with pytest.raises(ValueError):
            p.download("filled")


def test_a_row_band_and_a_context_without_a_dem_refuse():
    from malstroem_amd import _lib
    from malstroem_amd.distributed import HipBand
    from malstroem_amd.pipeline import HydroPipeline
    lines, segs = _burn.polylines([[(1, 1), (5, 6)]], 1.0, 2.0)
    res = np.zeros(1, dtype=_lib.BURN_RESULT_DTYPE)
    band = HipBand(64, 48, 0, 32, device=0, rank=0, size=2)
    try:
        band.upload("dem", np.zeros((32, 48), dtype=np.float32))
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_burn_lines", band._ctx, _lib.i64(1), _lib.ptr(segs), _lib.i64(1), _lib.ptr(lines), ctypes.c_double(NAN), _lib.ptr(res))
    finally:
        band.close()
    with HydroPipeline((32, 48)) as p:
        with pytest.raises(ValueError, match="needs the DEM"):
            p.burn_lines(lines, segs)


# ---- tools ---------------------------------------------------------------------------------------------------------------------------
def world(gt, cells):
    """the centres of cells (row, col) as GeoJSON coordinates"""
    return [[gt[0] + (c + 0.5) * gt[1], gt[3] + (r + 0.5) * gt[5]] for r, c in cells]


def oracle_counts(dem):
    """(bluespots, nodes of the stream network) of the oracle chain on a DEM, no filter: as tests/test_complete_chain.py does it"""
    from oracle import oracle as O
    from malstroem_amd.algorithms import net
    filled = oracle.fill_terrain(dem)
    dep = oracle.depths(filled, dem)
    short, diag = oracle.minimum_safe_short_and_diag(dem)
    noflat = oracle.fill_terrain_no_flats(dem, short, diag)
    fd = oracle.terrain_flowdirection(noflat)
    lab, n = oracle.connected_components(dep)
    pp = oracle.label_min_index(noflat, lab, n)
    upstream = OrderedDict()
    for pid in range(n + 1):
        cell = (int(pp["row"][pid]), int(pp["col"][pid]))
        down, geom = O.next_downstream_label(fd, lab, cell, 0)
        upstream.setdefault(down, []).append(dict(id=pid, downstream_id=down, nodetype='pourpoint', pix=cell, geometry=geom))
    nodes, nxt = [], n + 1
    for group in upstream.values():
        nxt = net._untangle(group, nxt, nodes)
    return n, len(nodes), lab, filled


def test_complete_with_adaptations(tmp_path):
    from malstroem_amd.adaptations import lines_from_features
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterReader, RasterWriter, VectorReader
    fx = fixtures()
    dtm = fx["dtm"]
    gt = tuple(float(v) for v in fx["geotransform"])
    H, W = dtm.shape
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(dtm)
    top = float(dtm.max()) + 2.0
    rng = np.random.default_rng(50)
    cell = lambda: (int(rng.integers(5, H - 5)), int(rng.integers(5, W - 5)))
    feats = [dict(type="Feature", geometry=dict(type="LineString", coordinates=world(gt, [cell() for _ in range(nv)])), properties=props)
             for nv, props in ((2, {}), (3, dict(mode="lower")), (4, dict(z_from=float(dtm.min()), z_to=None)), (2, dict(connectivity=4)),
                               (3, dict(mode="raise", z_from=top, z_to=top)), (2, dict(mode="raise", z_from=top, z_to=top + 1, connectivity=8)),
                               (5, dict(mode="raise", z_to=top)), (2, dict(mode="lower", z_from=1.0, z_to=2.0)))]
    feats.append(dict(type="Feature", id="two parts", properties=dict(mode="lower"),
                      geometry=dict(type="MultiLineString", coordinates=[world(gt, [cell(), cell()]), world(gt, [cell(), cell(), cell()])])))
    feats.append(dict(type="Feature", properties=dict(note="starts outside"), geometry=dict(type="LineString", coordinates=world(gt, [(-3, 10), (20, 30)]))))
    files = {}
    for name, fc in (("empty", []), ("lines", feats)):
        files[name] = str(tmp_path / (name + ".geojson"))
        with open(files[name], "w") as fh:
            json.dump(dict(type="FeatureCollection", features=fc), fh)
    outs = {}
    for name, kw in (("plain", {}), ("empty", dict(adaptations=files["empty"])), ("lines", dict(adaptations=files["lines"]))):
        d = tmp_path / name
        d.mkdir()
        outs[name] = (d, process_all(src, str(d), [10, 100], **kw))
    # an empty collection: everything byte for byte what it is without the argument
    (d0, r0), (d1, r1) = outs["plain"], outs["empty"]
    for f in ("filled.tif", "flowdir.tif", "bs_depths.tif", "bluespots.tif", "watersheds.tif"):
        assert (d0 / f).read_bytes() == (d1 / f).read_bytes(), f
    for layer in ("pourpoints", "nodes", "streams", "events"):
        assert (d0 / "vector" / (layer + ".geojson")).read_bytes() == (d1 / "vector" / (layer + ".geojson")).read_bytes(), layer
    assert "dem_adapted" not in r0 and r1["nlabels"] == r0["nlabels"]
    with RasterReader(r1["dem_adapted"]) as r:
        assert r.read().tobytes() == dtm.tobytes()
    assert VectorReader(r1["vector"], "adaptations").read_geojson_features() == []
    # ten lines: the adapted DEM is the model's, the chain behind it the oracle's on that DEM
    d2, r2 = outs["lines"]
    lines, segs, index = lines_from_features(feats, gt, dtm.shape, with_index=True)
    assert len(lines) == 11 and index.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 9]
    want, wres = _burn.burn(dtm, lines, segs, -999.0)
    assert wres["status"].tolist() == [0] * 10 + [1] and np.sum(want != dtm) > 50
    with RasterReader(r2["dem_adapted"]) as r:
        got = r.read()
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    n, nnodes, lab, filled = oracle_counts(want)
    assert r2["nlabels"] == n and n != r0["nlabels"]
    with RasterReader(str(d2 / "bluespots.tif")) as r:
        assert np.array_equal(r.read(), lab)
    with RasterReader(str(d2 / "filled.tif")) as r:
        assert np.array_equal(r.read(), filled)
    assert len(VectorReader(r2["vector"], "events").read_geojson_features()) == nnodes
    report = VectorReader(r2["adaptations"]).read_geojson_features()
    assert len(report) == len(feats)
    for k, (f, g) in enumerate(zip(feats, report)):
        mine = wres[index == k]
        p = g["properties"]
        assert g["geometry"] == f["geometry"] and all(p[key] == v for key, v in f["properties"].items())
        assert p["status"] == int(mine["status"].max()) and p["cells"] == int(mine["cells"].sum())
        assert p["z_from_used"] == (None if mine["status"][0] else float(mine["z0"][0]))
        assert p["z_to_used"] == (None if mine["status"][-1] else float(mine["z1"][-1]))
    assert report[8]["id"] == "two parts" and report[9]["properties"]["status"] == 1 and report[9]["properties"]["cells"] == 0
