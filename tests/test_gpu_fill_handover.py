"""GPU: the flood's last pass and its proof inside the no-flats fill's first visit (csrc/noflat_geo.hip: ng_handover_kernel;
csrc/ctx_run.hip, MHIP_FILL_HANDOVER = 0 | 1).

A request that holds FILL and NOFLAT on one undivided raster may stop the flood behind pf_final_kernel: the transform's first
visit computes the filled surface of every 64 x 64 window from dem + basin slots + final levels, writes FILLED and DEPTHS and
evaluates the flood's proof next to its own classification.  `fill_handover` (ctx_get_int) says whether the last request did.

The path moves work between two kernels and nothing else: every case runs the whole request twice, knob 1 and knob 0, and
compares all seven rasters, the label count, the label statistics, the watershed counts and the pour points with the oracle --
label sums by the rule of test_gpu_parity.py, everything else bit for bit -- and the engine numbers of the two runs with each
other.  The fused visit runs where the transform runs: a DEM with a NaN cell has NaN epsilons (fill.py:246-249), a raster of two
rows has no interior -- there the flood finishes its own last pass and `fill_handover` is 0 under either knob.

The knob is read per request, so one process switches it between requests (monkeypatch.setenv)."""
import numpy as np
import pytest

from _cases import assert_same_bits, fbm
from test_gpu_label_start import ALL, _lake, _sea_at_zero, assert_equals_oracle, assert_same_results, collect

import oracle

pytestmark = pytest.mark.gpu

# H x W: the smallest shapes at which the tile arithmetic (62 x 62 tiles + ring, origin ti * 62) can go wrong
SHAPES = [(3, 3),          # one interior cell
          (3, 200), (200, 3),
          (64, 64),        # exactly one tile
          (65, 65),        # 2 x 2 tiles, the second one cell wide
          (126, 126),      # 2 x 2 full tiles
          (127, 190), (131, 67),
          (188, 250),      # H = 62 k + 2: the raster's last row is the window's last row
          (200, 264),
          (130, 512),      # a width the flood's own fused last pass takes (a multiple of 256)
          (2, 70)]         # no interior: no flood, no transform
CONTENT_SHAPES = [(65, 65), (127, 190), (130, 512)]


def _fbm(h, w):
    return fbm(h, w, beta=2.0, seed=100 + h + w) + np.float32(3.0)


def _nan_inside(h, w):
    dem = _fbm(h, w)
    dem[h // 2, w // 3] = np.nan
    return dem


def _nan_on_border(h, w):
    dem = _fbm(h, w)
    dem[0, w // 2] = np.nan          # the depth there is NaN
    dem[h // 3, w - 1] = np.nan
    return dem


def _minus_zero_run(h, w):
    dem = _fbm(h, w) - np.float32(40.0)       # straddles 0
    dem[h // 2, 5:w - 5] = np.float32(-0.0)
    return dem


def _constant(h, w):
    return np.full((h, w), np.float32(7.25), dtype=np.float32)


DEMS = {"fbm%dx%d" % s: (lambda s=s: _fbm(*s)) for s in SHAPES}
for _name, _fn in (("nan_inside", _nan_inside), ("nan_on_border", _nan_on_border), ("minus_zero", _minus_zero_run), ("constant", _constant)):
    for _s in CONTENT_SHAPES:
        DEMS["%s%dx%d" % ((_name,) + _s)] = (lambda fn=_fn, s=_s: fn(*s))
DEMS["lake192"] = _lake                 # one flat over 3 x 3 tiles
DEMS["sea_at_zero"] = _sea_at_zero      # an irregular level: hybrid, noflat_algorithm 3
DEMS["fbm420x380"] = lambda: _fbm(420, 380)
DEMS["fbm200x264b"] = lambda: fbm(200, 264, beta=2.2, seed=77) + np.float32(3.0)
_cache = {}


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
                "pour": oracle.label_max_index(accum, labels, n), "transform": bool(min(dem.shape) >= 3 and short > 0 and diag > 0)}
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = want
    return _cache[name]


def run_all(dem, monkeypatch, knob, pipe=None):
    from malstroem_amd.pipeline import HydroPipeline
    monkeypatch.setenv("MHIP_DEVELOPER", "1")
    monkeypatch.setenv("MHIP_FILL_HANDOVER", str(knob))
    if pipe is None:
        with HydroPipeline(dem.shape) as p:
            return run_all(dem, monkeypatch, knob, p)
    pipe.upload("dem", dem)
    pipe.run(*ALL)
    got = collect(pipe)
    got["handover"] = pipe.get_int("fill_handover")
    return got


def both_ways(name, monkeypatch, sign_of_zero=True):
    """sign_of_zero=False: the filled surface and what is derived from it equal the oracle's as VALUES (the contract of
    test_gpu_edgecases.py for a DEM with -0.0 cells: the flood orders elevations by keys that take -0.0 for +0.0, so an interior
    cell at -0.0 and a lake that spills over one come out as +0.0 under either knob); the two runs still have the same bits"""
    want = case(name)
    on = run_all(want["dem"], monkeypatch, 1)
    off = run_all(want["dem"], monkeypatch, 0)
    assert on.pop("handover") == (1 if want["transform"] else 0), name
    assert off.pop("handover") == 0
    if sign_of_zero:
        assert_equals_oracle(on, want)
        assert_equals_oracle(off, want)
    else:
        assert_same_results(on, off)
        for k in ("filled", "depths", "noflat"):
            assert np.array_equal(on[k], want[k]), k
        on_bits = dict(on, filled=want["filled"], depths=want["depths"], noflat=want["noflat"])
        assert_equals_oracle(on_bits, want)       # everything else bit for bit
    assert on["engines"] == off["engines"]
    return on


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_tile_remainder_gives_the_oracles_results(monkeypatch, shape):
    on = both_ways("fbm%dx%d" % shape, monkeypatch)
    if min(shape) >= 3:
        assert on["engines"] == {"fill_algorithm": 1, "noflat_algorithm": 2}


@pytest.mark.parametrize("shape", CONTENT_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("content", ["minus_zero", "constant"])
def test_special_values_give_the_oracles_results(monkeypatch, content, shape):
    """a run of -0.0 (the flood's keys take it for +0.0; a level without integer weights) and a raster that is one flat"""
    both_ways("%s%dx%d" % ((content,) + shape), monkeypatch, sign_of_zero=content != "minus_zero")


@pytest.mark.parametrize("shape", CONTENT_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("content", ["nan_inside", "nan_on_border"])
def test_a_nan_cell_keeps_the_request_on_the_floods_own_last_pass(monkeypatch, content, shape):
    """One NaN cell makes both epsilons NaN (fill.py:246-249 takes np.amax / np.amin), and with NaN epsilons the transform never
    runs: the hand-over is offered, nobody takes it, and the flood completes its own last pass -- `fill_handover` 0.  What the
    no-flats stage then makes of NaN epsilons is not this path's business: the request ends the same way under either knob (the
    float64 relaxation does not settle on them and says so), and FILLED / DEPTHS -- the NaN depth of a NaN border cell among
    them -- equal the oracle's under either knob."""
    from malstroem_amd.pipeline import HydroPipeline
    want = case("%s%dx%d" % ((content,) + shape))
    assert not want["transform"]
    ends = []
    for knob in (1, 0):
        monkeypatch.setenv("MHIP_DEVELOPER", "1")
        monkeypatch.setenv("MHIP_FILL_HANDOVER", str(knob))
        with HydroPipeline(want["dem"].shape) as pipe:
            pipe.upload("dem", want["dem"])
            try:
                pipe.run(*ALL)
                pipe.sync()
                ends.append("ran")
            except RuntimeError as e:
                ends.append(str(e))
            assert pipe.get_int("fill_handover") == 0
            assert pipe.get_int("fill_algorithm") == 1
            assert_same_bits(pipe.download("filled"), want["filled"], "filled")
            assert_same_bits(pipe.download("depths"), want["depths"], "depths")
            if ends[-1] == "ran":
                got = collect(pipe)
                assert_equals_oracle(got, want)
    assert ends[0] == ends[1], ends
    if content == "nan_on_border":
        assert np.isnan(want["depths"][0, shape[1] // 2])


def test_a_lake_over_three_by_three_tiles(monkeypatch):
    assert both_ways("lake192", monkeypatch)["engines"] == {"fill_algorithm": 1, "noflat_algorithm": 2}


def test_an_irregular_level_takes_the_hybrid_path_behind_the_fused_visit(monkeypatch):
    assert both_ways("sea_at_zero", monkeypatch)["engines"] == {"fill_algorithm": 1, "noflat_algorithm": 3}


def test_the_proof_in_the_fused_visit_is_alive(monkeypatch):
    """MHIP_PF_CORRUPT with a hand-over: the final level of one basin is raised behind pf_final_kernel.  The fused visit writes the
    raised surface -- an upper bound --, its proof fails, the iterative schedule repairs the surface (fill_algorithm 4), the depths
    are recomputed and the classification runs again on the repaired raster.  Without the hook the same context is back at 1."""
    from malstroem_amd.pipeline import HydroPipeline
    want = case("fbm420x380")
    with HydroPipeline(want["dem"].shape) as pipe:
        monkeypatch.setenv("MHIP_PF_CORRUPT", "1")
        got = run_all(want["dem"], monkeypatch, 1, pipe)
        assert got.pop("handover") == 1
        assert got["engines"]["fill_algorithm"] == 4, got["engines"]
        assert_equals_oracle(got, want)
        monkeypatch.delenv("MHIP_PF_CORRUPT")
        again = run_all(want["dem"], monkeypatch, 1, pipe)
        assert again.pop("handover") == 1
        assert again["engines"]["fill_algorithm"] == 1, again["engines"]
        assert_equals_oracle(again, want)


def test_a_failed_proof_in_the_fused_visit_goes_through_the_floods_own_last_pass(monkeypatch):
    """MHIP_HO_RECHECK: the fused visit's proof is taken as failed although the surface is right.  The flood's workspace is still
    there: its own last pass writes and proves the raster -- it passes, `fill_algorithm` stays 1 --, the classification runs again
    from the raster, and the context counts the event (`fill_handover_rechecks`)."""
    from malstroem_amd.pipeline import HydroPipeline
    want = case("fbm200x264")
    with HydroPipeline(want["dem"].shape) as pipe:
        monkeypatch.setenv("MHIP_HO_RECHECK", "1")
        got = run_all(want["dem"], monkeypatch, 1, pipe)
        assert got.pop("handover") == 1
        assert pipe.get_int("fill_handover_rechecks") == 1
        assert got["engines"] == {"fill_algorithm": 1, "noflat_algorithm": 2}
        assert_equals_oracle(got, want)
        monkeypatch.delenv("MHIP_HO_RECHECK")
        again = run_all(want["dem"], monkeypatch, 1, pipe)
        assert again.pop("handover") == 1
        assert pipe.get_int("fill_handover_rechecks") == 1
        assert_equals_oracle(again, want)


@pytest.mark.parametrize("start", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["fbm200x264", "lake192"])
def test_every_label_start_behind_the_fused_visit(monkeypatch, name, start):
    """the label branch reads the depths the fused visit writes: at start 0 its hook fires behind that visit, not in front of the
    stage.  MHIP_NG_BATCH=1: these small rasters reach the tail rounds where start 1 fires."""
    monkeypatch.setenv("MHIP_NG_BATCH", "1")
    monkeypatch.setenv("MHIP_LABEL_START", str(start))
    got = run_all(case(name)["dem"], monkeypatch, 1)
    assert got.pop("handover") == 1
    assert_equals_oracle(got, case(name))
    assert got["engines"] == {"fill_algorithm": 1, "noflat_algorithm": 2}


def test_request_shapes_on_one_context(monkeypatch):
    """fill alone and noflat behind a resident FILLED stay on the two-kernel path; a whole request takes the fused visit, again and
    again on pooled (under MHIP_DEVELOPER: poisoned) workspaces"""
    from malstroem_amd.pipeline import HydroPipeline
    monkeypatch.setenv("MHIP_DEVELOPER", "1")
    monkeypatch.setenv("MHIP_FILL_HANDOVER", "1")
    first, second, last = case("fbm200x264"), case("fbm127x190"), case("fbm200x264b")
    third = np.ascontiguousarray(first["dem"][::-1, ::-1])
    with HydroPipeline(first["dem"].shape) as pipe:
        pipe.upload("dem", first["dem"])
        pipe.run("fill")
        pipe.sync()
        assert pipe.get_int("fill_handover") == 0
        assert_same_bits(pipe.download("filled"), first["filled"], "filled")
        assert_same_bits(pipe.download("depths"), first["depths"], "depths")
        pipe.run("noflat", "flowdir")
        pipe.sync()
        assert pipe.get_int("fill_handover") == 0
        assert_same_bits(pipe.download("noflat"), first["noflat"], "noflat")
        assert_same_bits(pipe.download("flowdir"), first["flowdir"], "flowdir")
        got = run_all(third, monkeypatch, 1, pipe)          # a new DEM
        assert got.pop("handover") == 1
        again = run_all(last["dem"], monkeypatch, 1, pipe)    # and a third one
        assert again.pop("handover") == 1
        assert_equals_oracle(again, last)
    fresh = run_all(third, monkeypatch, 0)
    assert fresh.pop("handover") == 0
    assert_same_results(got, fresh)
    # NOFLAT alone on a fresh context: the stage runs the plain fill itself, on the two-kernel path
    with HydroPipeline(second["dem"].shape) as pipe:
        pipe.upload("dem", second["dem"])
        pipe.run("noflat")
        pipe.sync()
        assert pipe.get_int("fill_handover") == 0
        assert_same_bits(pipe.download("noflat"), second["noflat"], "noflat")
    # FILL + NOFLAT without the label branch (one stream): the fused visit as well
    monkeypatch.setenv("MHIP_FILL_HANDOVER", "1")
    with HydroPipeline(second["dem"].shape) as pipe:
        pipe.upload("dem", second["dem"])
        pipe.run("fill", "noflat")
        pipe.sync()
        assert pipe.get_int("fill_handover") == 1
        for k in ("filled", "depths", "noflat"):
            assert_same_bits(pipe.download(k), second[k], k)
