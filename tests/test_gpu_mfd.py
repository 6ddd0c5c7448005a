"""GPU: the multiple-flow-direction accumulation (csrc/mfd.hip, malstroem_amd/mfd.py) against its definition, the
model tests/_mfd.py.  Fractions are float64 operations rounded one by one, sums are integers: every comparison is ``==``."""
import ctypes

import numpy as np
import pytest

import _mfd as M
from _cases import assert_same_bits, fbm, fixtures

pytestmark = pytest.mark.gpu

ONE = M.ONE
SENT = np.uint64(M.UNRESOLVED)
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 3), (64, 64), (65, 65), (63, 127), (130, 67)]


@pytest.fixture(scope="module")
def flow():
    import malstroem_amd.algorithms as a
    assert a.hip.available
    return a.flow


def check_surface(flow, z, exponent, weight=None, walk=None):
    """both stand-alone calls on a surface against the model, with ``==``; returns the model's (fractions, sums)"""
    z = np.ascontiguousarray(z, dtype=np.float64)
    want_f = M.fractions(z, exponent)
    assert_same_bits(flow.mfd_fractions(z, exponent), want_f, "fractions")
    w = np.full(z.shape, M.UNIT, np.uint32) if weight is None else weight
    walk = walk or (M.accumulate if z.size <= 10000 else M.accumulate_levels)
    want, want_unres = walk(want_f, w)
    got, unresolved = flow.mfd_accumulation(want_f, weight)
    assert got.dtype == np.uint64 and unresolved == want_unres == 0
    assert_same_bits(got, want, "sums")
    return want_f, want


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_against_the_model(flow, shape):
    rng = np.random.default_rng(3 + sum(shape))
    z = rng.random(shape)
    w = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    w.flat[0] = 2 ** 32 - 1
    for e in (1, 2, 8):
        check_surface(flow, z, e, w)
    # ... and a smooth one, where every interior cell has several lower neighbours
    rr, cc = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    check_surface(flow, 0.37 * rr + 0.11 * cc + 0.001 * rr * cc, 1, w)


# ---- 2. surfaces ----------------------------------------------------------------------------------------------------------------------
def cone(n, inverted):
    r, c = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    d = np.hypot(r - (n // 2 - 0.0), c - (n // 2 - 0.0))
    return d if inverted else -d


def test_a_cone_and_an_inverted_cone(flow):
    f, acc = check_surface(flow, cone(128, inverted=False), 1)      # full dispersion from the summit at a tile corner
    assert (np.count_nonzero(f[1:-1, 1:-1], axis=2) >= 2).mean() > 0.95
    f, acc = check_surface(flow, cone(128, inverted=True), 1)       # a sink with eight in-edges, at the corner of four tiles
    assert not f[64, 64].any() and all(f[64 + M._DR[k], 64 + M._DC[k], (k + 4) & 7] > 0 for k in range(8))
    # everything but the border drains to the sink: the border cells send nothing and keep their own
    assert int(acc[64, 64]) == (126 * 126) * M.UNIT


@pytest.mark.parametrize("tilt", ["rows", "columns", "diagonal"])
def test_tilted_planes(flow, tilt):
    """all three in-edges of a cell across a seam (rows, columns) and across a corner (diagonal)"""
    r, c = np.meshgrid(np.arange(130, dtype=np.float64), np.arange(131, dtype=np.float64), indexing="ij")
    z = {"rows": -r, "columns": -c, "diagonal": -(r + c)}[tilt]
    rng = np.random.default_rng(9)
    w = rng.integers(0, 2 ** 32, size=z.shape, dtype=np.uint64).astype(np.uint32)
    for e in (1, 3):
        f, _ = check_surface(flow, z, e, w)
    assert np.count_nonzero(f[64, 64]) == 3


def test_a_flat_and_cells_that_are_not_finite(flow):
    f, acc = check_surface(flow, np.full((70, 90), 3.25), 1)
    assert not f.any() and (acc == M.UNIT).all()
    rng = np.random.default_rng(10)
    z = fbm(140, 150, beta=2.0, seed=5).astype(np.float64)
    bad = rng.random(z.shape)
    z[bad < 0.03] = np.nan
    z[(bad >= 0.03) & (bad < 0.05)] = np.inf
    z[(bad >= 0.05) & (bad < 0.07)] = -np.inf
    z[63:66, 63:66] = np.nan
    z[64, 64] = 50.0
    for e in (1, 4):
        f, _ = check_surface(flow, z, e)
    assert not f[~np.isfinite(z)].any() and not f[64, 64].any()
    # values whose difference overflows, and subnormal slopes
    z = rng.random((66, 66)) * 1e308 * np.where(rng.random((66, 66)) < 0.5, -1.0, 1.0)
    check_surface(flow, z, 2)
    check_surface(flow, rng.random((66, 66)) * 1e-310, 8)


def test_a_serpentine_channel_that_crosses_one_seam_64_times(flow):
    """a walled channel, one cell wide, that runs to and fro across the seam between columns 63 and 64: a round per crossing"""
    z = np.full((131, 128), 1e6)
    path = []
    for i in range(64):
        cols = list(range(60, 68)) if i % 2 == 0 else list(range(67, 59, -1))
        path += [(1 + 2 * i, c) for c in cols]
        if i < 63:
            path.append((2 + 2 * i, cols[-1]))
    for n, (r, c) in enumerate(path):
        z[r, c] = float(len(path) - n)
    rng = np.random.default_rng(12)
    w = rng.integers(0, 2 ** 32, size=z.shape, dtype=np.uint64).astype(np.uint32)
    f, acc = check_surface(flow, z, 1, w, walk=M.accumulate_levels)
    seam = sum(1 for (r, c), (r2, c2) in zip(path[:-1], path[1:]) if {c, c2} == {63, 64})
    assert seam == 64
    # the channel's end has collected the channel and the walls that drain into it
    assert int(acc[path[-1]]) >= sum(int(w[p]) for p in path)


_fbm512 = {}


def fbm512():
    if not _fbm512:
        z = fbm(512, 512, beta=2.0, seed=21).astype(np.float64)
        z.setflags(write=False)
        _fbm512["z"] = z
    return _fbm512["z"]


@pytest.mark.parametrize("exponent", [1, 4, 8])
def test_fbm_512(flow, exponent):
    f, acc = check_surface(flow, fbm512(), exponent)
    sinks = ~f.any(axis=2)
    assert sum(int(v) for v in acc[sinks]) == 512 * 512 * M.UNIT      # conservation: nothing is lost to the floors


# ---- 3. weights ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", [0, M.UNIT, 2 ** 32 - 1])
def test_weights_on_a_512_inverted_cone(flow, weight):
    z = cone(512, inverted=True)
    if "f" not in _fbm512:
        _fbm512["f"] = M.fractions(z, 1)
    f = _fbm512["f"]
    w = np.full(z.shape, weight, np.uint32)
    want, want_unres = M.accumulate_levels(f, w)
    got, unresolved = flow.mfd_accumulation(f, w)
    assert unresolved == want_unres == 0
    assert_same_bits(got, want, "sums")
    assert int(got[256, 256]) == 510 * 510 * weight      # 2**32 - 1: near 2**50, far past float64's integers


# ---- 4. the caller's own fractions ------------------------------------------------------------------------------------------------------------
def test_cycles_inside_a_tile_and_across_a_seam(flow):
    f = np.zeros((140, 150, 8), np.uint16)

    def send(r, c, **shares):
        for k, v in shares.items():
            f[r, c, int(k[1:])] = v
    # a cycle inside a tile: (10,10) -> (10,11) -> (11,11) -> (11,10) -> (10,10); (11,11) also leaks half of it down a channel that
    # crosses into the tile below and the one right of it
    send(10, 10, k2=ONE), send(10, 11, k4=ONE), send(11, 11, k6=ONE // 2, k4=ONE // 2), send(11, 10, k0=ONE)
    for r in range(12, 70):
        send(r, 11, k4=ONE)
    for c in range(11, 80):
        send(70, c, k2=ONE)
    send(9, 10, k4=ONE)                    # a feeder of the cycle: resolved
    # a cycle across the seam between columns 63 and 64, with a leak to the right
    send(20, 63, k2=ONE), send(20, 64, k4=ONE), send(21, 64, k6=ONE - 5, k2=5), send(21, 63, k0=ONE)
    for c in range(65, 140):
        send(21, c, k2=ONE)
    # ... and a resolved split that joins the second channel downstream of the cycle: still unresolved below the join
    send(19, 100, k4=ONE // 4, k3=ONE - ONE // 4)
    rng = np.random.default_rng(13)
    w = rng.integers(0, 2 ** 32, size=f.shape[:2], dtype=np.uint64).astype(np.uint32)
    want, want_unres = M.accumulate(f, w)
    got, unresolved = flow.mfd_accumulation(f, w)
    assert_same_bits(got, want, "sums")
    cells_downstream = (70 - 12) + (80 - 11) + (140 - 65)
    assert unresolved == want_unres == 8 + cells_downstream + 2      # (+ (70, 80) and (21, 140), where the channels end)
    assert got[9, 10] == w[9, 10] and got[10, 10] == SENT and got[70, 80] == SENT and got[21, 139] == SENT and got[20, 100] != SENT
    assert got[21, 100] == SENT and got[19, 100] == w[19, 100]


def test_fractions_that_sum_to_neither_0_nor_one_are_refused(flow):
    from malstroem_amd import _lib
    f = M.fractions(fbm(130, 70, beta=2.0, seed=2).astype(np.float64), 1)
    w = np.ones(f.shape[:2], np.uint32)
    sending = tuple(int(v) for v in np.argwhere(f.any(axis=2))[0])      # (one below ONE needs a cell that has fractions)
    for cell, delta in (((64, 33), 1), ((129, 69), 7), (sending, -1)):
        bad = f.copy()
        k = int(np.argmax(bad[cell]))
        bad[cell][k] = int(bad[cell][k]) + delta
        assert int(bad[cell].sum(dtype=np.int64)) not in (0, ONE)
        with pytest.raises(ValueError, match="neither 0 nor 32768"):
            flow.mfd_accumulation(bad, w)
        out, unresolved = np.empty(w.shape, np.uint64), ctypes.c_int64(0)
        rc = _lib.load().mhip_mfd_accum_u32(_lib.ptr(bad), _lib.ptr(w), _lib.i64(130), _lib.i64(70), _lib.ptr(out), ctypes.byref(unresolved))
        assert rc == _lib.EINVAL
    got, unresolved = flow.mfd_accumulation(f, w)      # (and the library is fine afterwards)
    assert unresolved == 0 and np.array_equal(got, M.accumulate(f, w)[0])
    with pytest.raises(ValueError, match="exponent"):
        _lib.call("mhip_mfd_fractions_f64", _lib.ptr(np.zeros((3, 3))), _lib.i64(3), _lib.i64(3), ctypes.c_int32(9), _lib.ptr(np.zeros((3, 3, 8), np.uint16)))


def test_the_hinge_d8_fractions_against_the_weighted_accumulation(flow):
    from malstroem_amd import mfd
    import malstroem_amd.algorithms as alg
    dem = fbm(200, 170, beta=2.0, seed=31)
    short, diag = alg.fill.minimum_safe_short_and_diag(dem)
    fd = flow.terrain_flowdirection(alg.fill.fill_terrain_no_flats(dem, short, diag))      # acyclic: the chain's own
    rng = np.random.default_rng(14)
    w = rng.integers(0, 2 ** 32, size=fd.shape, dtype=np.uint64).astype(np.uint32)
    got, unresolved = flow.mfd_accumulation(mfd.fractions_from_flowdir(fd), w)
    assert unresolved == 0
    assert_same_bits(got, flow.weighted_accumulation(fd, w), "the D8 hinge")


# ---- 5. on a context ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lift", [0.0, 3.0])
def test_context_path_and_snapshot(flow, monkeypatch, lift):
    """On the reference's DEM fixture.  As it is, 340 of its cells lie at elevation 0, where the integer no-flats transform has no
    constant ulp and hands the surface to the relaxation, which stores it: such a context is never pending (cf. ``sea_at_zero`` of
    test_gpu_noflat_lazy.py), and the first call finds the surface written.  Raised by 3 m -- the same terrain, no cell at 0 -- the
    finishing pass defers the surface, ``noflat_pending == 1`` holds before the first call, and the call has to write it first."""
    from malstroem_amd.pipeline import HydroPipeline
    monkeypatch.setenv("MHIP_DEVELOPER", "1")
    monkeypatch.setenv("MHIP_NOFLAT_LAZY", "1")
    dem = np.ascontiguousarray(fixtures()["dtm"] + np.float32(lift), dtype=np.float32)
    rng = np.random.default_rng(15)
    w = rng.integers(0, 2 ** 32, size=dem.shape, dtype=np.uint64).astype(np.uint32)
    p = HydroPipeline(dem.shape)
    try:
        p.upload("dem", dem)
        p.run("fill", "noflat", "flowdir")
        p.sync()
        pending = p.get_int("noflat_pending")
        print("lift %g: noflat_pending %d, noflat_algorithm %d" % (lift, pending, p.get_int("noflat_algorithm")))
        if lift:
            assert pending == 1
        first = p.mfd_accumulation(4, w)                 # writes a pending surface first
        assert p.get_int("noflat_pending") == 0
        g = p.download("noflat")
        want_f = M.fractions(g, 4)
        assert_same_bits(flow.mfd_fractions(g, 4), want_f, "fractions of the no-flats surface")
        want, want_unres = M.accumulate_levels(want_f, w)
        assert want_unres == 0 and first.unresolved == 0 and first.nzone == -1 and first.shape == dem.shape
        bits = first.download_u64()
        assert_same_bits(bits, want, "the first call")
        assert_same_bits(flow.mfd_accumulation(want_f, w)[0], want, "the stand-alone pair")
        work = first.work()
        assert work["tiles"] == 3 * 4 and work["rounds"] >= 2 and work["visits"] >= work["tiles"]
        # after a reader has written the surface; the default weight is UNIT everywhere
        with p.mfd_accumulation() as unit:
            want1, _ = M.accumulate_levels(M.fractions(g, 1), np.full(dem.shape, M.UNIT, np.uint32))
            assert_same_bits(unit.download_u64(), want1, "written, exponent 1, unit weights")
            assert_same_bits(unit.download(), M.view(want1), "upstream cells")
            assert_same_bits(unit.download_rows_u64(70, 3), want1[70:73], "rows")
            with pytest.raises(ValueError, match="without the watersheds"):
                unit.sums()
        # a snapshot: a new DEM and a new run do not reach it
        p.upload("dem", np.ascontiguousarray(dem[::-1]))
        with pytest.raises(ValueError, match="NOFLAT"):
            p.mfd_accumulation()
        p.run("fill", "noflat", "flowdir")
        assert_same_bits(first.download_u64(), bits, "after a new run")
    finally:
        p.close()
    assert_same_bits(first.download_u64(), bits, "after the pipeline is closed")
    assert_same_bits(first.download(mul=0.16), M.view(want, M.UNIT, 0.16), "the view after the pipeline is closed")
    first.close()
    with pytest.raises(ValueError, match="closed"):
        first.download_u64()


def test_context_refusals(flow):
    from malstroem_amd import _lib
    from malstroem_amd.distributed import HipBand
    from malstroem_amd.pipeline import HydroPipeline
    # refusals: no surface, an exponent out of range at the C entry, a row band
    handle = ctypes.c_void_p()
    with HydroPipeline((8, 9)) as q:
        with pytest.raises(ValueError, match="NOFLAT"):
            q.mfd_accumulation()
        q.upload("noflat", np.zeros((8, 9)))
        for e in (0, 9):
            assert _lib.load().mhip_ctx_mfd_accum(q._ctx, ctypes.c_int32(e), None, ctypes.byref(handle)) == _lib.EINVAL and not handle
        with q.mfd_accumulation(2, np.full((8, 9), 3, np.uint32)) as small:
            assert (small.download_u64() == 3).all()
    band = HipBand(64, 48, 0, 32, device=0, rank=0, size=2)
    try:
        band.upload("noflat", np.zeros((32, 48)))
        assert _lib.load().mhip_ctx_mfd_accum(band._ctx, ctypes.c_int32(1), None, ctypes.byref(handle)) == _lib.EINVAL and not handle
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_mfd_accum", band._ctx, ctypes.c_int32(1), None, ctypes.byref(handle))
    finally:
        band.close()


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------------------
def test_complete_with_mfd(tmp_path):
    """``process_all`` on the reference's fixture DEM: ``accum_mfd.tif`` is the model's float view of the model's sums on the no-flats
    surface, and every other output is the file of the run without the argument."""
    import os
    import oracle
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterReader, RasterWriter
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(fx["dtm"])

    def run(name, **kw):
        out = tmp_path / name
        out.mkdir()
        return out, process_all(src, str(out), [10, 100], accum=True, **kw)
    base_dir, base = run("base")
    mfd_dir, res = run("mfd", mfd={"exponent": 4})
    assert set(res) == set(base) | {"accum_mfd"} and res["accum_mfd"] == str(mfd_dir / "accum_mfd.tif")
    tifs = sorted(p.name for p in base_dir.iterdir() if p.suffix == ".tif")
    assert sorted(p.name for p in mfd_dir.iterdir() if p.suffix == ".tif") == sorted(tifs + ["accum_mfd.tif"])
    for name in tifs:
        assert (base_dir / name).read_bytes() == (mfd_dir / name).read_bytes(), name
    assert sorted(os.listdir(base["vector"])) == sorted(os.listdir(res["vector"]))
    for name in os.listdir(base["vector"]):
        assert open(os.path.join(base["vector"], name), "rb").read() == open(os.path.join(res["vector"], name), "rb").read(), name
    dem = np.ascontiguousarray(fx["dtm"], dtype=np.float32)
    short, diag = oracle.minimum_safe_short_and_diag(dem)
    g = oracle.fill_terrain_no_flats(dem, short, diag)
    want, unresolved = M.accumulate_levels(M.fractions(g, 4), np.full(dem.shape, M.UNIT, np.uint32))
    assert unresolved == 0
    with RasterReader(res["accum_mfd"]) as r:
        got = r.read()
        assert r.nodata == -1
    assert got.dtype == np.float64
    assert_same_bits(got, M.view(want), "accum_mfd.tif")
    run2_dir, res2 = run("default", mfd=True)
    with RasterReader(res2["accum_mfd"]) as r:
        assert_same_bits(r.read(), M.view(M.accumulate_levels(M.fractions(g, 1), np.full(dem.shape, M.UNIT, np.uint32))[0]), "exponent 1")
