"""GPU: the onset raster of a rain series (csrc/wetat.hip) bit for bit against the NumPy model of tests/_onset.py --
the standalone call on small, ragged and flat rasters with draw-downs in no order, the context call against three final_depths
calls, and `complete.process_all(finalstate=True, onset=True)` on the reference's fixture DEM."""
import ctypes

import numpy as np
import pytest

import _finalstate as M
import _onset as O
from _cases import assert_same_bits, fbm, fixtures

pytestmark = pytest.mark.gpu

KS = [1, 2, 5, 16]      # rows of 4, 4, 8 and 16 thresholds a label


@pytest.fixture(scope="module")
def alg():
    import malstroem_amd.algorithms as a
    assert a.hip.available
    return a


def values_for(K):
    return (np.arange(K) * 7 + 3).astype(np.float32)


def depths_with_ties(rng, lab, T):
    """random depths; a tenth of the labelled cells exactly at float32(a draw-down of their label), a tenth one ulp above"""
    d = (rng.random(lab.shape) * 3).astype(np.float32)
    k = rng.integers(0, len(T), lab.shape)
    t = T[k, lab]
    with np.errstate(over="ignore", invalid="ignore"):
        t32 = t.astype(np.float32)
    s = rng.random(lab.shape)
    at, above = (lab > 0) & np.isfinite(t32) & (s < 0.1), (lab > 0) & np.isfinite(t32) & (s >= 0.1) & (s < 0.2)
    d[at] = t32[at]
    d[above] = np.nextafter(t32[above], np.float32(np.inf))
    return d, int(at.sum()), int(above.sum())


def drawdowns(rng, K, nlab):
    """no order in k, NaN and both infinities; half of the finite ones are float32 numbers, so that a float32 depth can tie"""
    T = O.random_drawdowns(rng, K, nlab, scale=3.0)
    half = rng.random(T.shape) < 0.5
    with np.errstate(invalid="ignore"):
        T[half] = T[half].astype(np.float32).astype(np.float64)
    return T


def check_standalone(alg, d, lab, T, values, what):
    want, wwet = O.wet_at(d, lab, T, values)
    out, wet = alg.label.wet_at(d, lab, T, values)
    assert out.dtype == np.float32 and out.shape == d.shape and wet.dtype == np.int64 and wet.shape == T.shape
    assert_same_bits(out, want, what + " raster")
    assert np.array_equal(wet, wwet), what
    for k in range(len(T)):      # identity (2)
        assert np.array_equal(wet[k], M.wet_cells(M.final(d, lab, T[k]), lab, T.shape[1] - 1)), (what, k)
    return out, wet


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (1, 300), (300, 1), (33, 257), (95, 515), (64, 1028), (1000,)])
def test_standalone_on_small_ragged_and_flat_rasters(alg, shape):
    """one row and one column past a 32 x 256 tile, a width that is no multiple of four (one cell a thread), one that is (four),
    and a flat array; labels are 8-connected components of a random mask"""
    rng = np.random.default_rng(sum(shape) + len(shape))
    mask = (rng.random(shape if len(shape) == 2 else (1,) + shape) < 0.35).astype(np.float32)
    lab, nlab = alg.label.connected_components(mask)
    lab = lab.reshape(shape)
    ties = 0
    for K in KS:
        T = drawdowns(rng, K, nlab)
        d, at, above = depths_with_ties(rng, lab, T)
        ties += at
        out, wet = check_standalone(alg, d, lab, T, values_for(K), "%s K=%d" % (shape, K))
        assert set(np.unique(out)) <= set(values_for(K).tolist()) | {0.0} and not out[lab == 0].any()
    if lab.size >= 300:
        assert ties >= 5 and nlab >= 1
    # a label beyond the draw-downs' rows is refused
    if nlab >= 1:
        with pytest.raises(ValueError, match="label outside"):
            alg.label.wet_at(d, lab, T[:, :nlab], values_for(KS[-1]))


@pytest.mark.parametrize("kind", ["tables", "rects", "dominant"])
def test_standalone_on_labels_that_are_no_components(alg, kind):
    """"tables" holds 700 to 4000 labels in a 32 x 256 tile, more than the tile's table has slots: those runs take the global
    atomics, and the result is the same"""
    from _inputs import label_rasters
    labs, claims = label_rasters(256, 256, 23)
    lab, nlab = labs[kind], claims["nlabels"][kind]
    rng = np.random.default_rng(len(kind))
    for K in KS:
        T = drawdowns(rng, K, nlab)
        d, at, above = depths_with_ties(rng, lab, T)
        assert at > 1000 and above > 1000
        out, wet = check_standalone(alg, d, lab, T, values_for(K), "%s K=%d" % (kind, K))
        assert wet.sum() > 0
    if kind == "tables":
        from _inputs import tile_label_counts
        assert tile_label_counts(lab)[0].max() > 512
    # the same cells as a flat array
    out1, wet1 = check_standalone(alg, d.ravel(), lab.ravel(), T, values_for(K), kind + " flat")
    assert_same_bits(out1, out.ravel(), "flat")
    with pytest.raises(ValueError, match="label outside"):
        bad = lab.copy()
        bad[200, 100] = nlab + 1
        alg.label.wet_at(d, bad, T, values_for(K))


def fixture_bluespots():
    """the reference fixture DEM (188 x 250) with the 486-bluespot filtered labelling"""
    from malstroem_amd.bluespots import filterbluespots
    from malstroem_amd.complete import parse_filter
    from malstroem_amd.pipeline import HydroPipeline
    fx = fixtures()
    gt = [float(v) for v in fx["geotransform"]]
    p = HydroPipeline(fx["dtm"].shape)
    p.upload("dem", fx["dtm"])
    p.run("fill", "label")
    keep = filterbluespots(parse_filter('area > 20.5 and maxdepth > 0.5 or volume > 2.5'), abs(gt[1] * gt[5]), p.raw_stats())
    assert p.apply_keep(keep) == 486
    return p


def fbm_bluespots():
    from malstroem_amd.pipeline import HydroPipeline
    dem = fbm(700, 700, seed=9)
    p = HydroPipeline(dem.shape)
    p.upload("dem", dem)
    p.run("fill", "label")
    assert p.apply_keep(None) > 100
    return p


class Windows(object):
    """a raster writer that takes row windows"""

    def open(self, shape, dtype):
        self.out, self.rows = np.full(shape, -1, dtype), []

    def write_window(self, row0, rows):
        self.out[row0:row0 + len(rows)] = rows
        self.rows.append((row0, len(rows)))

    def close(self):
        self.closed = True


@pytest.mark.parametrize("make", [fixture_bluespots, fbm_bluespots])
def test_context_series_equals_three_final_depths_calls(make):
    pipe = make()
    try:
        d, lab, n = pipe.download("depths"), pipe.download("labels"), pipe.get_int("nlabels")
        with pytest.raises(ValueError, match="hypsometry"):
            pipe.wet_at(np.zeros((1, n + 1)), [10])
        pipe.hypsometry(0.05)
        assert pipe.get_int("wet_at_events") == -1
        with pytest.raises(ValueError, match="wet_at"):
            pipe.download_wet_at()
        vol = pipe.stats()["sum"].copy()
        vol[0] = 0.0
        qs = np.stack([0.25 * vol, 0.5 * vol, 2.0 * vol])
        values = np.array([10, 30, 100], np.float32)
        # a wet_at call between two final_depths calls leaves the finaldepths raster alone
        rec0 = pipe.final_depths(qs[0])
        fin0 = pipe.download("finaldepths")
        recs = pipe.wet_at(qs, values)
        assert_same_bits(pipe.download("finaldepths"), fin0, "finaldepths after wet_at")
        assert pipe.get_int("wet_at_events") == 3 and pipe.kernel_ms("wet_at")[0] > 0
        singles, fins = [rec0], [fin0]
        for k in (1, 2):
            singles.append(pipe.final_depths(qs[k]))
            fins.append(pipe.download("finaldepths"))
        assert recs.shape == (3, n + 1) and recs.dtype == M.FINAL_DTYPE
        for k in range(3):
            assert_same_bits(recs[k], singles[k], "records of event %d" % k)      # all four fields, wet_cells included
            assert np.array_equal(recs[k]["wet_cells"], M.wet_cells(fins[k], lab, n))
        T = np.ascontiguousarray(recs["drawdown"])
        out = pipe.download_wet_at()
        want, wwet = O.wet_at(d, lab, T, values)
        assert_same_bits(out, want, "context raster")
        assert np.array_equal(recs["wet_cells"], wwet)
        assert (np.diff(T, axis=0) <= 0).all() and not T[2].any()      # more water, higher level; twice the volume: full
        for k in range(3):      # identity (1) against the rasters of the single events
            assert np.array_equal((out > 0) & (out <= values[k]), fins[k] > 0), k
        assert set(np.unique(out)) == {0.0, 10.0, 30.0, 100.0}
        # in row windows
        w = Windows()
        pipe.download_wet_at_to(w, max_rows=37)
        assert w.closed and len(w.rows) == -(-d.shape[0] // 37)
        assert_same_bits(w.out, out, "windows")
        # arguments
        with pytest.raises(ValueError, match="strictly increasing"):
            pipe.wet_at(qs, [10, 30, 30])
        with pytest.raises(ValueError, match="\\(K, nlabels \\+ 1\\)"):
            pipe.wet_at(qs[:2], values)
        assert pipe.get_int("wet_at_events") == 3
        # new labels: the raster is gone with the tables
        pipe.upload("labels", lab)
        assert pipe.get_int("wet_at_events") == -1
        with pytest.raises(ValueError, match="wet_at"):
            pipe.download_wet_at()
    finally:
        pipe.close()


def test_a_band_context_is_refused():
    from malstroem_amd import _lib
    ctx = ctypes.c_void_p()
    _lib.call("mhip_ctx_create_band", ctypes.byref(ctx), _lib.i64(64), _lib.i64(64), _lib.i64(0), _lib.i64(32), 0, 0, 2, None)
    try:
        q, v, rec = np.zeros((1, 1)), np.array([10], np.float32), np.zeros((1, 1), _lib.FINAL_DTYPE)
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_wet_at", ctx, ctypes.c_int32(1), _lib.ptr(q), _lib.ptr(v), _lib.ptr(rec))
    finally:
        _lib.call("mhip_ctx_destroy", ctx)


def test_complete_chain_with_onset(tmp_path):
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterReader, RasterWriter, VectorReader
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(fx["dtm"])
    flt = 'area > 20.5 and maxdepth > 0.5 or volume > 2.5'
    dirs = {}
    for name in ("onset", "lean", "plain"):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
    res = process_all(src, str(dirs["onset"]), [10, 30], filter=flt, finalstate=True, onset=True)
    lean = process_all(src, str(dirs["lean"]), [10, 30], filter=flt, finalstate=True, onset=True, final_rasters=False)
    plain = process_all(src, str(dirs["plain"]), [10, 30], filter=flt, finalstate=True)
    # without `onset` the keys are the ones of today, and no wet_at.tif
    assert sorted(plain) == sorted(["outdir", "vector", "nlabels", "events", "nodes", "streams", "pourpoints", "finalstate", "finaldepths"])
    assert not (dirs["plain"] / "wet_at.tif").exists() and sorted(res) == sorted(list(plain) + ["wet_at"])
    assert res["wet_at"] == str(dirs["onset"] / "wet_at.tif")
    with RasterReader(res["wet_at"]) as r:
        onset = r.read()
    with RasterReader(str(dirs["onset"] / "bluespots.tif")) as r:
        lab = r.read()
    assert onset.dtype == np.float32 and onset.shape == lab.shape
    assert set(np.unique(onset)) == {0.0, 10.0, 30.0} and not onset[lab == 0].any()
    for tag, mm in (("10", 10.0), ("30", 30.0)):
        with RasterReader(res["finaldepths"][tag]) as r:
            fin = r.read()
        assert np.array_equal(fin > 0, (onset > 0) & (onset <= mm)), tag
        assert (dirs["onset"] / ("finaldepths_%s.tif" % tag)).read_bytes() == (dirs["plain"] / ("finaldepths_%s.tif" % tag)).read_bytes()
    # without the depth rasters: none written, the same layer and the same map
    assert not list(dirs["lean"].glob("finaldepths*")) and lean["finaldepths"] == {}
    assert (dirs["lean"] / "wet_at.tif").read_bytes() == (dirs["onset"] / "wet_at.tif").read_bytes()
    layers = [VectorReader(r["vector"], "finalstate").read_geojson_features() for r in (res, lean, plain)]
    assert len(layers[0]) == len(layers[1]) == len(layers[2]) > 486
    for a, b, c in zip(*layers):
        assert a == b == c
    assert any("wetarea_30" in f["properties"] for f in layers[1])
