"""GPU: the runoff-weighted flow accumulation (csrc/wacc.hip, malstroem_amd/runoff.py) against its definition, the
model tests/_wacc.py, or against closed forms in Python integers.  The arithmetic is integer: every comparison is ``==``.

In a D8 forest a cell has one downstream cell, so nothing but the cycle itself lies downstream of a flow cycle: the "tails" of the
hand-made cases run INTO their cycles, through two more tiles, and must stay resolved like every other tributary."""
import ctypes
import os

import numpy as np
import pytest

import _wacc as M
from _cases import assert_same_bits, fbm

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (7, 1), (63, 65), (64, 64), (65, 63), (130, 197), (200, 256)]      # 200 x 256: W % 16 == 0
SENT = np.uint64(M.UNRESOLVED)


@pytest.fixture(scope="module")
def alg():
    import malstroem_amd.algorithms as a
    assert a.hip.available
    return a


def chain_flowdir(alg, shape, seed):
    """flow directions of a small random terrain through the library's own chain"""
    dem = fbm(max(shape[0], 2), max(shape[1], 2), beta=2.0, seed=seed)[:shape[0], :shape[1]].copy()
    short, diag = alg.fill.minimum_safe_short_and_diag(dem)
    return alg.flow.terrain_flowdirection(alg.fill.fill_terrain_no_flats(dem, short, diag))


_fd_cache = {}


def flowdir_of(alg, shape):
    if shape not in _fd_cache:
        _fd_cache[shape] = chain_flowdir(alg, shape, 7 + sum(shape))
    return _fd_cache[shape]


def standalone(fd, w, zones=None, nzone=0):
    """the C entry point itself: (wacc, unresolved[, sums])"""
    from malstroem_amd import _lib
    out = np.empty(fd.shape, dtype=np.uint64)
    sums = np.zeros(nzone + 1, dtype=np.uint64) if zones is not None else None
    unresolved = ctypes.c_int64(-1)
    _lib.call("mhip_weighted_accum_u32", _lib.ptr(fd), _lib.ptr(w), _lib.ptr(zones) if zones is not None else None, _lib.i64(fd.shape[0]),
              _lib.i64(fd.shape[1]), _lib.i64(nzone), _lib.ptr(out), _lib.ptr(sums) if zones is not None else None, ctypes.byref(unresolved))
    return (out, unresolved.value, sums) if zones is not None else (out, unresolved.value)


def path_flowdir(shape, path, last_code=8):
    """directions that lead along ``path`` (a list of (r, c), each a neighbour of the one before); every other cell has none"""
    code = {(-1, 0): 0, (-1, 1): 1, (0, 1): 2, (1, 1): 3, (1, 0): 4, (1, -1): 5, (0, -1): 6, (-1, -1): 7}
    fd = np.full(shape, 8, np.uint8)
    for (r, c), (r2, c2) in zip(path[:-1], path[1:]):
        fd[r, c] = code[(r2 - r, c2 - c)]
    fd[path[-1]] = last_code
    return fd


def along(path, w):
    """the running sum of the weights along a path, per cell, in uint64 (exact: far below 2**64)"""
    idx = np.array(path)
    out = np.zeros(w.shape, dtype=np.uint64)
    out[idx[:, 0], idx[:, 1]] = np.cumsum(w[idx[:, 0], idx[:, 1]].astype(np.uint64))
    return out


# ---- 1. shapes: raster, zone sums and unresolved count against the model ---------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_against_the_model(alg, shape):
    rng = np.random.default_rng(31 + sum(shape))
    fd = flowdir_of(alg, shape)
    w = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    w.flat[0] = 2 ** 32 - 1
    # zones in runs (a thread folds them in registers) and, on the two largest shapes, thousands of labels (past the LDS table)
    nzone = 3000 if shape[0] * shape[1] > 20000 else 5
    zones = np.repeat(rng.integers(0, nzone + 1, size=fd.size, dtype=np.int32), rng.integers(1, 6, size=fd.size))[:fd.size].reshape(shape).copy()
    want, want_unres, want_sums = M.accumulate(fd, w, zones, nzone)
    got, unres, sums = standalone(fd, w, zones, nzone)
    assert_same_bits(got, want, "wacc %s" % (shape,))
    assert_same_bits(sums, want_sums, "zone sums %s" % (shape,))
    assert unres == want_unres == 0
    got2, sums2 = alg.flow.weighted_accumulation(fd, w, zones)
    assert_same_bits(got2, want, "algorithms.flow")
    assert_same_bits(sums2, want_sums[:int(zones.max()) + 1], "algorithms.flow sums")
    assert_same_bits(alg.flow.weighted_accumulation(fd, w), want, "without zones")


# ---- 2. weight == 1 is the accumulated flow ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(1000, 1000)])
def test_unit_weights_give_the_accumulated_flow(alg, shape):
    from malstroem_amd.pipeline import HydroPipeline
    fd = flowdir_of(alg, shape).copy()
    if fd.size > 100:      # the chain's directions have no cycle: plant two, one of them across a tile seam where the raster has one
        fd[3, 3], fd[3, 4] = 2, 6
        c = min(63, fd.shape[1] - 2)
        fd[5, c], fd[5, c + 1], fd[6, c + 1], fd[6, c] = 2, 4, 6, 0
    acc = alg.flow.accumulated_flow(fd)
    with HydroPipeline(shape) as p:
        p.upload("flowdir", fd)
        with p.weighted_accumulation(np.ones(shape, np.uint32), by_watersheds=False) as wa:
            got, unres = wa.download_u64(), wa.unresolved
    zero = acc == 0
    assert got.dtype == np.uint64 and np.array_equal(got[~zero], acc[~zero].astype(np.uint64))
    assert np.all(got[zero] == SENT)
    assert unres == int(zero.sum()) == (6 if fd.size > 100 else 0)


# ---- 3. hand-made directions on 192 x 192 (3 x 3 tiles) ---------------------------------------------------------------------------------
N = 192


def hand_weights(seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=(N, N), dtype=np.uint64).astype(np.uint32)


def test_a_serpentine_through_all_cells(alg):
    """row by row: the path enters every tile 64 times"""
    path = [(r, c) for r in range(N) for c in (range(N) if r % 2 == 0 else range(N - 1, -1, -1))]
    fd = path_flowdir((N, N), path, last_code=4)      # (the last cell steps out of the raster and keeps its sum)
    w = hand_weights(1)
    got, unres = standalone(fd, w)
    assert_same_bits(got, along(path, w), "serpentine")
    assert unres == 0 and int(got[path[-1]]) == int(w.astype(np.uint64).sum())


def test_a_spiral(alg):
    path, top, left, bottom, right = [], 0, 0, N - 1, N - 1
    while top <= bottom and left <= right:
        path += [(top, c) for c in range(left, right + 1)] + [(r, right) for r in range(top + 1, bottom + 1)]
        if top < bottom and left < right:
            path += [(bottom, c) for c in range(right - 1, left - 1, -1)] + [(r, left) for r in range(bottom - 1, top, -1)]
        top, left, bottom, right = top + 1, left + 1, bottom - 1, right - 1
    assert len(path) == N * N == len(set(path))
    fd = path_flowdir((N, N), path)
    w = hand_weights(2)
    got, unres = standalone(fd, w)
    assert_same_bits(got, along(path, w), "spiral inwards")
    assert unres == 0
    fd = path_flowdir((N, N), path[::-1], last_code=6)      # outwards, and out of the raster at (0, 0)
    got, unres = standalone(fd, w)
    assert_same_bits(got, along(path[::-1], w), "spiral outwards")
    assert unres == 0


def test_cycles_sinks_and_edges_by_hand(alg):
    fd = np.full((N, N), 8, np.uint8)
    w = hand_weights(3)
    u = w.astype(np.uint64)
    # a 2-cycle inside tile (0, 0) with two tributaries and a tail that comes from tile (0, 2) through tile (0, 1)
    fd[10, 10], fd[10, 11] = 2, 6
    fd[9, 10], fd[11, 11] = 4, 0
    fd[10, 12:181] = 6
    # a 4-cycle inside tile (1, 1) with a tributary and a tail from tile (2, 0) through tile (2, 1)
    fd[100, 100], fd[100, 101], fd[101, 101], fd[101, 100] = 2, 4, 6, 0
    fd[99, 100] = 4
    fd[150, 20:101] = 2
    fd[102:151, 101] = 0
    # a 2-cycle and a 4-cycle across the seam between the columns 63 and 64, the second with a tributary
    fd[30, 63], fd[30, 64] = 2, 6
    fd[40, 63], fd[40, 64], fd[41, 64], fd[41, 63] = 2, 4, 6, 0
    fd[39, 63] = 4
    fd[32:39, 63] = 4
    # a cell without a direction, fed by all of its eight neighbours
    for k, (dr, dc) in enumerate(zip(M._DR, M._DC)):
        fd[120 - dr, 30 - dc] = k
    # edge cells that step out of the raster, each fed from inside
    fd[0, 70:90], fd[1, 70:90] = 0, 0
    fd[N - 1, 70:90], fd[N - 2, 70:90] = 4, 3
    fd[140:180, 0], fd[140:180, 1] = 6, 7
    fd[140:180, N - 1], fd[140:180, N - 2] = 2, 2
    fd[0, 0], fd[0, N - 1], fd[N - 1, 0], fd[N - 1, N - 1] = 7, 1, 5, 3
    want, want_unres = M.accumulate(fd, w)
    got, unres = standalone(fd, w)
    assert_same_bits(got, want, "hand-made")
    cyc = [(10, 10), (10, 11), (100, 100), (100, 101), (101, 101), (101, 100), (30, 63), (30, 64), (40, 63), (40, 64), (41, 64), (41, 63)]
    assert unres == want_unres == len(cyc)
    assert sorted(map(tuple, np.argwhere(got == SENT))) == sorted(cyc)
    # the tributaries and the tails are resolved: closed forms
    assert int(got[10, 12]) == int(u[10, 12:181].sum()) and int(got[9, 10]) == int(w[9, 10]) and int(got[11, 11]) == int(w[11, 11])
    assert int(got[102, 101]) == int(u[150, 20:101].sum() + u[102:151, 101].sum()) and int(got[99, 100]) == int(w[99, 100])
    assert int(got[39, 63]) == int(u[32:40, 63].sum())
    assert int(got[120, 30]) == int(u[119:122, 29:32].sum())
    assert np.array_equal(got[0, 70:90], u[0, 70:90] + u[1, 70:90])
    assert int(got[N - 1, 80]) == int(u[N - 1, 80] + u[N - 2, 79])
    assert int(got[150, 0]) == int(u[150, 0] + u[151, 1]) and int(got[150, N - 1]) == int(u[150, N - 1] + u[150, N - 2])


# ---- 4. random direction codes: many cycles, many cells that are entry and exit at once -------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_random_direction_codes(alg, seed):
    rng = np.random.default_rng(400 + seed)
    fd = rng.integers(0, 9, size=(130, 197)).astype(np.uint8)
    w = rng.integers(0, 2 ** 32, size=fd.shape, dtype=np.uint64).astype(np.uint32)
    zones = rng.integers(0, 41, size=fd.shape, dtype=np.int32)
    want, want_unres, want_sums = M.accumulate(fd, w, zones, 40)
    got, unres, sums = standalone(fd, w, zones, 40)
    assert_same_bits(got, want, "random codes %d" % seed)
    assert_same_bits(sums, want_sums, "zone sums")
    assert unres == want_unres > 0


# ---- 5. beyond 2**53 --------------------------------------------------------------------------------------------------------------------
def test_sums_beyond_2_to_the_53(alg):
    from malstroem_amd.pipeline import HydroPipeline
    n, big = 1472, 2 ** 32 - 1
    fd = np.full((n, n), 4, np.uint8)
    fd[n - 1, :] = 2
    w = np.full((n, n), big, np.uint32)
    with HydroPipeline((n, n)) as p:
        p.upload("flowdir", fd)
        with p.weighted_accumulation(w, by_watersheds=False) as wa:
            got, view, unres = wa.download_u64(), wa.download(mul=0.16), wa.unresolved
            rows = wa.download_rows(n - 2, 2, div=3.0, mul=1.0, nodata=-7.0)
    assert unres == 0
    assert int(got[n - 1, n - 1]) == big * n * n > 2 ** 53
    assert [int(v) for v in got[n - 1]] == [big * n * (c + 1) for c in range(n)]
    assert np.array_equal(got[:n - 1], (np.arange(1, n, dtype=np.uint64) * np.uint64(big))[:, None].repeat(n, axis=1))
    assert_same_bits(view, M.view(got, M.UNIT, 0.16, -1.0), "float view")
    assert_same_bits(rows, M.view(got[n - 2:], 3.0, 1.0, -7.0), "float view of rows")


# ---- 6. on a context --------------------------------------------------------------------------------------------------------------------
def test_context_path_snapshot_and_refusals(alg):
    from malstroem_amd import _lib, runoff
    from malstroem_amd.distributed import HipBand
    from malstroem_amd.pipeline import HydroPipeline
    rng = np.random.default_rng(6)
    dem = fbm(300, 300, beta=2.0, seed=66)
    w = rng.integers(0, 2 ** 32, size=dem.shape, dtype=np.uint64).astype(np.uint32)
    p = HydroPipeline(dem.shape)
    try:
        p.upload("dem", dem)
        p.run("fill", "noflat", "flowdir", "accum", "label")
        nlab = p.apply_keep(None)
        p.run("watershed", "pourpoints")
        fd, ws = p.download("flowdir"), p.download("watersheds")
        wa = p.weighted_accumulation(w)
        want, want_unres = M.accumulate(fd, w)
        sums = wa.sums()
        assert sums.dtype == np.uint64 and sums.shape == (nlab + 1,)
        assert [int(v) for v in sums] == [int(v) for v in M.zone_sums(w, ws, nlab)]
        # (90000 weights below 2**32: every partial sum of the float64 bincount is an integer below 2**53, so it is exact)
        assert [int(v) for v in sums] == [int(v) for v in np.bincount(ws.ravel(), w.ravel(), minlength=nlab + 1)]
        first = wa.download_u64()
        assert_same_bits(first, want, "context")
        assert wa.unresolved == want_unres == 0 and wa.nzone == nlab and wa.shape == dem.shape
        assert_same_bits(wa.download(mul=2.5), M.view(want, M.UNIT, 2.5, -1.0), "view")
        assert_same_bits(wa.download_rows_u64(17, 5), want[17:22], "rows")
        assert_same_bits(runoff.effective_area(sums, 0.16), M.effective_area(sums, 0.16), "effective area")
        plain = p.weighted_accumulation(w, by_watersheds=False)
        with pytest.raises(ValueError, match="without the watersheds"):
            plain.sums()
        assert_same_bits(plain.download_u64(), want, "without the watersheds")
        plain.close()
        plain.close()
        with pytest.raises(ValueError, match="closed"):
            plain.download_u64()
        # a snapshot: a new DEM and a new run do not reach it, and neither does the end of the pipeline
        p.upload("dem", np.ascontiguousarray(dem[::-1]))
        assert_same_bits(wa.download_u64(), first, "after the DEM is uploaded again")
        p.run("fill", "noflat", "flowdir")
        assert_same_bits(wa.download_u64(), first, "after a new run")
        with pytest.raises(ValueError, match="WATERSHEDS"):      # (the new DEM dropped the watersheds)
            p.weighted_accumulation(w)
    finally:
        p.close()
    assert_same_bits(wa.download_u64(), first, "after the pipeline is closed")
    assert_same_bits(wa.sums(), sums, "sums after the pipeline is closed")
    wa.close()
    # refusals: no flow directions, a wrong weight, a row band
    handle = ctypes.c_void_p()
    with HydroPipeline((8, 9)) as q:
        with pytest.raises(ValueError, match="FLOWDIR"):
            q.weighted_accumulation(np.ones((8, 9), np.uint32), by_watersheds=False)
        q.upload("flowdir", np.full((8, 9), 2, np.uint8))
        with pytest.raises(ValueError, match="dtype"):
            q.weighted_accumulation(np.ones((8, 9), np.int32), by_watersheds=False)
        with pytest.raises(ValueError, match="shape"):
            q.weighted_accumulation(np.ones((9, 8), np.uint32), by_watersheds=False)
        with q.weighted_accumulation(np.full((8, 9), 3, np.uint32), by_watersheds=False) as small:
            assert np.array_equal(small.download_u64(), np.tile(3 * np.arange(1, 10, dtype=np.uint64), (8, 1)))
    band = HipBand(64, 48, 0, 32, device=0, rank=0, size=2)
    try:
        band.upload("flowdir", np.full((32, 48), 2, dtype=np.uint8))
        ones = np.ones((32, 48), np.uint32)
        assert _lib.load().mhip_ctx_weighted_accum(band._ctx, _lib.ptr(ones), ctypes.c_int32(0), ctypes.byref(handle)) == _lib.EINVAL and not handle
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_weighted_accum", band._ctx, _lib.ptr(ones), ctypes.c_int32(0), ctypes.byref(handle))
    finally:
        band.close()


def test_a_label_out_of_range_is_refused(alg):
    fd = np.full((4, 5), 2, np.uint8)
    w = np.ones((4, 5), np.uint32)
    zones = np.zeros((4, 5), np.int32)
    zones[2, 2] = 9
    with pytest.raises(ValueError, match="label outside"):
        standalone(fd, w, zones, 8)
    with pytest.raises(ValueError, match="negative"):
        alg.flow.weighted_accumulation(fd, w, -zones)


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------
def test_complete_with_runoff(tmp_path):
    """``process_all`` on the reference's fixture DEM: a coefficient of one changes nothing but the new property; half a coefficient on
    the left half gives the model's rain volumes and the model's float view as ``runoff_accum.tif``."""
    from _cases import fixtures
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterReader, RasterWriter, VectorReader
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    cell_area = abs(gt[1]) * abs(gt[5])
    shape = fx["dtm"].shape
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(fx["dtm"])
    rain, layers = [10, 100], ("pourpoints", "nodes", "streams", "events")

    def run(name, **kw):
        out = tmp_path / name
        out.mkdir()
        return out, process_all(src, str(out), rain, **kw)
    base_dir, base = run("base")
    ones_dir, ones = run("ones", runoff={"coefficient": np.ones(shape)})
    assert set(ones) == set(base)
    tifs = sorted(p.name for p in base_dir.iterdir() if p.suffix == ".tif")
    assert tifs == sorted(p.name for p in ones_dir.iterdir() if p.suffix == ".tif") and "watersheds.tif" in tifs
    for name in tifs:
        assert (base_dir / name).read_bytes() == (ones_dir / name).read_bytes(), name
    assert sorted(os.listdir(base["vector"])) == sorted(os.listdir(ones["vector"]))
    for layer in layers:
        want = VectorReader(base["vector"], layer).read_geojson_features()
        got = VectorReader(ones["vector"], layer).read_geojson_features()
        assert len(got) == len(want) > 0
        for g, w in zip(got, want):
            props = dict(g["properties"])
            if layer != "streams":
                assert props.pop("wshed_eff_area") == props["wshed_area"], (layer, props)
            assert props == w["properties"] and g["geometry"] == w["geometry"], (layer, w["properties"])
    # half a coefficient on the left half, written as a GeoTIFF on the DEM's grid, a pattern as an array
    coef = np.ones(shape, np.float32)
    coef[:, :shape[1] // 2] = 0.5
    coef[3, 5] = -1.0      # (its nodata: sheds nothing)
    RasterWriter(str(tmp_path / "coef.tif"), gt, None, nodata=-1.0).write(coef)
    pattern = np.full(shape, 1.25)
    half_dir, half = run("half", runoff={"coefficient": str(tmp_path / "coef.tif"), "pattern": pattern, "raster": True})
    for name in tifs:
        assert (base_dir / name).read_bytes() == (half_dir / name).read_bytes(), name
    with RasterReader(str(half_dir / "watersheds.tif")) as r:
        ws = r.read()
    with RasterReader(str(half_dir / "flowdir.tif")) as r:
        fd = r.read()
    w = M.weights(coef.astype(np.float64), pattern, -1.0)
    assert w[3, 5] == 0 and w[0, 0] == 625000 and w[0, shape[1] - 1] == 1250000
    eff = M.effective_area(M.zone_sums(w, ws, base["nlabels"]), cell_area)
    events = VectorReader(half["vector"], "events").read_geojson_features()
    assert len(events) == len(VectorReader(base["vector"], "events").read_geojson_features())
    npour = 0
    for f in events:
        p = f["properties"]
        area = float(eff[p["bspot_id"]]) if p["bspot_id"] is not None else 0.0
        npour += p["bspot_id"] is not None
        assert p["wshed_eff_area"] == area, p
        for mm in rain:
            assert p["rainv_%g" % mm] == area * mm * 0.001, (p["nodeid"], mm)
    assert npour == base["nlabels"] + 1
    want_acc, unresolved = M.accumulate(fd, w)
    assert half["runoff_accum"] == str(half_dir / "runoff_accum.tif") and unresolved == 0
    with RasterReader(half["runoff_accum"]) as r:
        got_acc = r.read()
    assert_same_bits(got_acc, M.view(want_acc, M.UNIT, cell_area, -1.0), "runoff_accum.tif")
    # refusals: a grid that is not the DEM's, an unknown key
    for bad in ({"coefficient": np.ones((3, 4))}, {"coefficent": 1.0}):
        out = tmp_path / ("bad%d" % len(bad.get("coefficient", ())))
        out.mkdir()
        with pytest.raises(ValueError, match="runoff"):
            process_all(src, str(out), rain, runoff=bad)
