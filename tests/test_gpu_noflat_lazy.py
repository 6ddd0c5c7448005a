"""GPU: the deferred no-flats surface (csrc/noflat_geo.hip: ng_finish_kernel<true, false>, noflat_assemble_dev; csrc/ctx.hip:
ctx_noflat; csrc/ctx_run.hip, MHIP_NOFLAT_LAZY = 0 | 1) and the accumulation's set-up ahead of its stage (csrc/accum.hip: AccumPrep).

A request that holds NOFLAT and FLOWDIR on one undivided context, and whose integer transform finishes the job alone, does not store
the surface G: the finishing pass derives the directions from it in registers.  The context says so (`noflat_pending`), and whoever
reads NOFLAT afterwards gets it written first, from the filled surface and the distances, by the function the pass checked it with.

Nothing but the time of one store moves: every case compares the lazy run with the eager one (knob 0) byte for byte -- rasters and
records -- and both with the oracle.  The knob is read per request (monkeypatch.setenv)."""
import ctypes

import numpy as np
import pytest

from _cases import assert_same_bits, fbm
from test_gpu_label_start import ALL, assert_equals_oracle, assert_same_results, collect

import oracle

pytestmark = pytest.mark.gpu


def _fbm(h, w):
    return fbm(h, w, beta=2.0, seed=300 + h + w) + np.float32(3.0)


def _lake():
    """192 x 192, one lake over 3 x 3 no-flats tiles (62 cells each) and 3 x 3 accumulation tiles: the distances cross every seam"""
    dem = fbm(192, 192, beta=2.0, seed=33) * np.float32(0.01) + np.float32(10.0)
    dem[20:172, 20:172] -= np.float32(5.0)
    return np.ascontiguousarray(dem)


def _sea_at_zero():
    """a flat at elevation 0 has no constant ulp above it: the transform leaves it to the relaxation (noflat_algorithm 3)"""
    dem = fbm(131, 190, beta=2.0, seed=13)
    dem[40:80, :150] = 0.0
    return dem


DEMS = {"fbm188x250": lambda: _fbm(188, 250),      # H = 62 * 3 + 2: the ragged last window
        "fbm131x67": lambda: _fbm(131, 67),
        "fbm64x64": lambda: _fbm(64, 64),          # one window
        "fbm63x190": lambda: _fbm(63, 190),
        "lake192": _lake,
        "sea_at_zero": _sea_at_zero, "two_rows": lambda: _fbm(2, 70)}
LAZY_NAMES = ["fbm188x250", "fbm131x67", "fbm64x64", "fbm63x190", "lake192"]
_cache, _eager = {}, {}


def case(name):
    """the DEM and what the oracle makes of it, computed once per module and never written to"""
    if name not in _cache:
        dem = np.ascontiguousarray(DEMS[name](), dtype=np.float32)
        filled = oracle.fill_terrain(dem)
        short, diag = oracle.minimum_safe_short_and_diag(dem)
        if np.isnan(dem).any():      # fill.py:246-249 takes np.amax / np.amin: one NaN cell makes both epsilons NaN
            short = diag = float("nan")
        noflat = oracle.fill_terrain_no_flats(dem, short, diag)
        flowdir = oracle.terrain_flowdirection(noflat)
        accum = oracle.accumulated_flow(flowdir)
        depths = oracle.depths(filled, dem)
        labels, n = oracle.connected_components(depths)
        ws = labels.copy()
        oracle.watersheds_from_labels(flowdir, ws)
        want = {"dem": dem, "filled": filled, "depths": depths, "noflat": noflat, "flowdir": flowdir, "accum": accum, "labels": labels,
                "watersheds": ws, "nlabels": n, "stats": oracle.label_stats(depths, labels, n), "counts": oracle.label_count(ws),
                "pour": oracle.label_max_index(accum, labels, n), "pour_min": oracle.label_min_index(noflat, labels, n)}
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = want
    return _cache[name]


def knob(monkeypatch, lazy):
    monkeypatch.setenv("MHIP_DEVELOPER", "1")
    monkeypatch.setenv("MHIP_NOFLAT_LAZY", "1" if lazy else "0")


def pipeline(shape):
    from malstroem_amd.pipeline import HydroPipeline
    return HydroPipeline(shape)


def chain(pipe, dem, stages=ALL):
    pipe.upload("dem", dem)
    pipe.run(*stages)
    pipe.sync()
    return pipe.get_int("noflat_pending")


def eager(name, monkeypatch):
    """the whole chain with the surface stored by the finishing pass, once per raster: what every lazy case has to equal"""
    if name not in _eager:
        knob(monkeypatch, False)
        with pipeline(case(name)["dem"].shape) as p:
            assert chain(p, case(name)["dem"]) == 0
            _eager[name] = collect(p)
        assert_equals_oracle(_eager[name], case(name))
    knob(monkeypatch, True)
    return _eager[name]


def check_everything(pipe, name, monkeypatch):
    """rasters and records of a context that has run the whole chain: the eager run's, byte for byte, and the oracle's"""
    got = collect(pipe)
    assert pipe.get_int("noflat_pending") == 0      # (collect downloads the surface)
    assert_same_results(got, eager(name, monkeypatch))
    assert_equals_oracle(got, case(name))
    return got


# ---- the chain request --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAZY_NAMES)
def test_a_chain_request_leaves_the_surface_pending_until_somebody_reads_it(monkeypatch, name):
    want = case(name)
    dem = want["dem"]
    h = dem.shape[0]
    knob(monkeypatch, True)
    with pipeline(dem.shape) as p:
        assert chain(p, dem) == 1
        assert (p.get_int("fill_algorithm"), p.get_int("noflat_algorithm")) == (1, 2)
        # a window of a few rows while pending: those rows (across the seam of the first two windows where the raster has one)
        r0, n = min(60, h - 4), 4
        assert_same_bits(p.download_rows("noflat", r0, n), want["noflat"][r0:r0 + n], "rows while pending")
        assert p.get_int("noflat_pending") == 0
        # again, and the whole raster twice
        assert chain(p, dem) == 1
        first = p.download("noflat")
        assert p.get_int("noflat_pending") == 0
        assert_same_bits(p.download("noflat"), first, "second download")
        assert_same_bits(first, want["noflat"], "noflat")
        check_everything(p, name, monkeypatch)


# ---- every reader, started from a pending context ---------------------------------------------------------------------------------
READER_NAMES = ["fbm188x250", "lake192"]


@pytest.mark.parametrize("name", READER_NAMES)
def test_flowdir_alone_from_a_pending_surface(monkeypatch, name):
    want = case(name)
    knob(monkeypatch, True)
    with pipeline(want["dem"].shape) as p:
        assert chain(p, want["dem"]) == 1
        p.run("flowdir")
        assert p.get_int("noflat_pending") == 0
        assert p.get_int("flowdir_computed") == 1
        assert_same_bits(p.download("flowdir"), want["flowdir"], "flowdir of its own")
        check_everything(p, name, monkeypatch)


@pytest.mark.parametrize("name", READER_NAMES)
def test_pour_points_without_accumulation_from_a_pending_surface(monkeypatch, name):
    """bluespots.py:195-206 without accumulated flow: the first arg-min of the no-flats surface per label"""
    want = case(name)
    got = {}
    for lazy in (True, False):
        knob(monkeypatch, lazy)
        with pipeline(want["dem"].shape) as p:
            assert chain(p, want["dem"], ("fill", "noflat", "flowdir", "label")) == (1 if lazy else 0)
            p.run("pourpoints")
            assert p.get_int("noflat_pending") == 0
            assert p.get_int("pour_algorithm") == 0
            got[lazy] = (p.pourpoints(), p.download("noflat"), p.download("flowdir"))
    for a, b, what in zip(got[True], got[False], ("pour points", "noflat", "flowdir")):
        assert_same_bits(a, b, what)
    assert_same_bits(got[True][0], want["pour_min"], "arg-min of the surface")
    assert_same_bits(got[True][1], want["noflat"], "noflat")
    assert_same_bits(got[True][2], want["flowdir"], "flowdir")


@pytest.mark.parametrize("name", READER_NAMES)
def test_d8_steady_from_a_pending_surface(monkeypatch, name):
    want = case(name)
    knob(monkeypatch, True)
    with pipeline(want["dem"].shape) as p:
        assert chain(p, want["dem"]) == 1
        ms, launches = p.kernel_ms("d8_steady")
        assert launches == 16 and ms > 0
        assert p.get_int("noflat_pending") == 0
        assert_same_bits(p.download("flowdir"), want["flowdir"], "flowdir of the steady-state launches")
        check_everything(p, name, monkeypatch)


@pytest.mark.parametrize("name", READER_NAMES)
def test_noflat_verify_and_a_band_getter_from_a_pending_surface(monkeypatch, name):
    from malstroem_amd import _lib
    want = case(name)
    knob(monkeypatch, True)
    with pipeline(want["dem"].shape) as p:
        assert chain(p, want["dem"]) == 1
        ok = ctypes.c_int32(0)
        _lib.call("mhip_ctx_noflat_verify", p._ctx, ctypes.byref(ok))
        assert ok.value == 1
        assert p.get_int("noflat_pending") == 0
        assert chain(p, want["dem"]) == 1
        first, last = (np.empty(want["dem"].shape[1], dtype=np.float64) for _ in range(2))
        _lib.call("mhip_ctx_get_edge_rows", p._ctx, _lib.R_NOFLAT, _lib.ptr(first), _lib.ptr(last))
        assert p.get_int("noflat_pending") == 0
        assert_same_bits(first, want["noflat"][0], "first row")
        assert_same_bits(last, want["noflat"][-1], "last row")
        check_everything(p, name, monkeypatch)


# ---- invalidation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy", [True, False])
def test_a_dem_upload_while_pending_makes_the_surface_absent(monkeypatch, lazy):
    want = case("fbm131x67")
    knob(monkeypatch, lazy)
    with pipeline(want["dem"].shape) as p:
        assert chain(p, want["dem"]) == (1 if lazy else 0)
        p.upload("dem", want["dem"] + np.float32(1.0))
        assert p.get_int("noflat_pending") == 0
        with pytest.raises(ValueError, match="raster has not been computed or uploaded"):      # (the same under either knob)
            p.download("noflat")
        with pytest.raises(ValueError, match="FLOWDIR needs the no-flats surface"):
            p.run("flowdir")
        # ... and the context goes on with the new DEM's own surface
        assert chain(p, want["dem"]) == (1 if lazy else 0)
        assert_same_bits(p.download("noflat"), want["noflat"], "noflat")


@pytest.mark.parametrize("name", READER_NAMES)
def test_the_contexts_own_fill_while_pending_leaves_the_surface_valid(monkeypatch, name):
    """the same DEM gives the same filled surface bit for bit: what the pending surface is made of does not change"""
    want = case(name)
    knob(monkeypatch, True)
    with pipeline(want["dem"].shape) as p:
        assert chain(p, want["dem"]) == 1
        p.run("fill")
        assert p.get_int("noflat_pending") == 1
        assert_same_bits(p.download("noflat"), want["noflat"], "noflat after a fill of its own")
        assert_same_bits(p.download("filled"), want["filled"], "filled")
        p.run("label", "watershed", "pourpoints")      # (the fill replaced the depths: the label branch again)
        check_everything(p, name, monkeypatch)


@pytest.mark.parametrize("name", READER_NAMES)
def test_a_foreign_filled_surface_while_pending_leaves_the_original_surface(monkeypatch, name):
    """an upload of FILLED has never touched NOFLAT: the surface of the ORIGINAL filled surface stays, under either knob"""
    want = case(name)
    other = np.ascontiguousarray(want["filled"] + np.float32(2.5))
    got = {}
    for lazy in (True, False):
        knob(monkeypatch, lazy)
        with pipeline(want["dem"].shape) as p:
            assert chain(p, want["dem"]) == (1 if lazy else 0)
            p.upload("filled", other)
            assert p.get_int("noflat_pending") == 0
            got[lazy] = (p.download("noflat"), p.download("flowdir"), p.download("filled"))
    for a, b, what in zip(got[True], got[False], ("noflat", "flowdir", "filled")):
        assert_same_bits(a, b, what)
    assert_same_bits(got[True][0], want["noflat"], "noflat")
    assert_same_bits(got[True][1], want["flowdir"], "flowdir")
    assert_same_bits(got[True][2], other, "the uploaded surface")


# ---- paths that stay eager ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,algorithms,env", [("sea_at_zero", (3,), None),                  # an irregular level: the hybrid
                                                ("fbm131x67", (0,), "MHIP_NG_CORRUPT"),       # a rejected finishing pass, then the relaxation
                                                ("lake192", (0,), "MHIP_NG_CORRUPT"),
                                                ("two_rows", (0,), None)])                    # no interior: no transform
def test_requests_the_transform_does_not_finish_alone_store_the_surface(monkeypatch, name, algorithms, env):
    want = case(name)
    got = {}
    for lazy in (True, False):
        knob(monkeypatch, lazy)
        if env:
            monkeypatch.setenv(env, "1")
        with pipeline(want["dem"].shape) as p:
            assert chain(p, want["dem"]) == 0
            assert p.get_int("noflat_algorithm") in algorithms
            got[lazy] = collect(p)
        if env:
            monkeypatch.delenv(env)
    assert_same_results(got[True], got[False])
    assert_equals_oracle(got[True], want)


@pytest.mark.parametrize("lazy", [True, False])
def test_a_nan_cell_ends_the_request_as_ever(monkeypatch, lazy):
    """One NaN cell makes both epsilons NaN (fill.py:246-249): the transform does not apply, and the float64 relaxation does not
    settle on them and says so -- the request ends the same way under either knob, nothing is left pending, and the context goes on."""
    want = case("fbm131x67")
    dem = want["dem"].copy()
    dem[65, 22] = np.nan
    knob(monkeypatch, lazy)
    with pipeline(dem.shape) as p:
        p.upload("dem", dem)
        with pytest.raises(RuntimeError, match="did not converge"):
            p.run(*ALL)
        assert p.get_int("noflat_pending") == 0
        assert chain(p, want["dem"]) == (1 if lazy else 0)
        assert_equals_oracle(collect(p), want)


@pytest.mark.parametrize("name", READER_NAMES)
def test_noflat_without_flowdir_stores_the_surface(monkeypatch, name):
    want = case(name)
    knob(monkeypatch, True)
    with pipeline(want["dem"].shape) as p:
        assert chain(p, want["dem"], ("fill", "noflat")) == 0
        assert p.get_int("noflat_algorithm") == 2
        assert_same_bits(p.download("noflat"), want["noflat"], "noflat")
        p.run("flowdir")
        assert_same_bits(p.download("flowdir"), want["flowdir"], "flowdir")


# ---- lifetime ---------------------------------------------------------------------------------------------------------------------
def test_three_chain_requests_in_a_row_then_close(monkeypatch):
    """(the pool offers no count of the blocks it has handed out: a fourth context on the same shape stands in for it)"""
    name = "fbm188x250"
    want = case(name)
    knob(monkeypatch, True)
    p = pipeline(want["dem"].shape)
    try:
        first = None
        for k in range(3):
            assert chain(p, want["dem"]) == 1
            got = check_everything(p, name, monkeypatch)
            first = first or got
            assert_same_results(got, first)
        assert chain(p, want["dem"]) == 1      # closed while pending
    finally:
        p.close()
    with pipeline(want["dem"].shape) as q:
        assert chain(q, want["dem"]) == 1
        check_everything(q, name, monkeypatch)


# ---- the accumulation's set-up ahead of its stage -----------------------------------------------------------------------------------
def test_a_rejected_finishing_pass_still_gets_its_accumulation(monkeypatch):
    name = "lake192"
    want = case(name)
    knob(monkeypatch, True)
    with pipeline(want["dem"].shape) as p:
        monkeypatch.setenv("MHIP_NG_CORRUPT", "1")
        assert chain(p, want["dem"]) == 0
        assert p.get_int("noflat_algorithm") != 2
        assert_equals_oracle(collect(p), want)
        monkeypatch.delenv("MHIP_NG_CORRUPT")
        assert chain(p, want["dem"]) == 1      # the context runs again
        check_everything(p, name, monkeypatch)


def test_a_chain_without_accumulation_prepares_nothing(monkeypatch):
    name = "fbm188x250"
    want = case(name)
    knob(monkeypatch, True)
    with pipeline(want["dem"].shape) as p:
        assert chain(p, want["dem"], ("fill", "noflat", "flowdir", "label", "watershed")) == 1
        with pytest.raises(ValueError, match="raster has not been computed or uploaded"):
            p.download("accum")
        assert_same_bits(p.download("watersheds"), want["watersheds"], "watersheds")
        assert_same_bits(p.download("flowdir"), want["flowdir"], "flowdir")
        assert chain(p, want["dem"]) == 1      # the context runs again, with the accumulation
        check_everything(p, name, monkeypatch)
