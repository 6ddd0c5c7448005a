"""GPU: one wet bit per cell instead of two rasters of floats (csrc/ctx_run.hip, MHIP_WETBITS = 0 | 1).

A request whose flood hands over to the no-flats fill computes "filled > dem" for every cell in its first visit
(ng_handover_kernel: the proof word `raised`).  The visit now stores those words -- one per tile row and raster column -- and, once
its proof has passed over a finite DEM, the finishing pass of the same request takes the DEM from them (ng_finish_kernel<.., WET>)
and the labelling's tile pass the foreground of the depths (ccl_tile_kernel<float, true>).  `wetbits_used` (ctx_get_int) tells
which variant ran in the last request: bit 0 the pass, bit 1 the labelling.

Nothing else may change: every case runs the whole chain twice on one context, knob 1 and knob 0, and compares every raster, every
record and every counter bit for bit; two shapes are compared with the oracle as well.  The shapes are the smallest at which the
62-row tiles of the transform and the 64-row tiles of the labelling / 32-row blocks of the pass can disagree, the surfaces put
lakes across those seams, next to the raster border, into single cells, and nowhere.  Where the bits do not stand for the floats --
a NaN or an infinity in the DEM, a proof taken as failed, depths that came from outside -- the kernels of before run."""
import numpy as np
import pytest

from _cases import assert_same_bits
from test_gpu_label_start import ALL, assert_equals_oracle, assert_same_results, collect

import oracle

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64),         # one tile of either kind
          (63, 125),        # ragged; the raster's last row is the labelling's last tile row
          (126, 190),       # H = 62 k + 2: the raster's last row is the window's last row
          (188, 250),       # ragged on both axes, three tile rows of the transform against three of the labelling
          (130, 200)]       # a third labelling tile row of two rows
COUNTERS = ("fill_algorithm", "noflat_algorithm", "pour_algorithm", "fill_handover", "noflat_reject", "noflat_reject_irregular",
            "noflat_reject_unreached", "noflat_reject_mismatch", "nlabels", "nlabels_raw")


def _ramp(h, w):
    """a tilted plane in steps of a quarter with a little relief: no cell without a lower neighbour -- no lake"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (np.float32(50.0) - np.float32(0.25) * (yy + xx).astype(np.float32)).astype(np.float32)


def _terraced(h, w):
    """terraces with lakes across rows and columns 62 | 63 | 64 and 124 | 125 | 128 (where the raster has them), a lake that touches
    the cell next to the raster border in both corners, and one-cell pits"""
    yy, xx = np.mgrid[0:h, 0:w]
    dem = (np.float32(30.0) + np.floor((yy * 0.011 + xx * 0.007)).astype(np.float32) * np.float32(0.5)      # (wide terraces: dry flats)
           + np.float32(0.125) * ((yy * 5 + xx * 3) % 7 == 0)).astype(np.float32)

    def lake(r0, r1, c0, c1, depth):
        r0, r1, c0, c1 = max(r0, 1), min(r1, h - 1), max(c0, 1), min(c1, w - 1)
        if r0 < r1 and c0 < c1:
            dem[r0:r1, c0:c1] -= np.float32(depth)

    for s in (63, 126):
        lake(s - 6, s + 5, 3, w - 3, 2.0)        # across the row seams, nearly the raster's width
        lake(3, h - 3, s - 6, s + 5, 2.5)        # across the column seams
    lake(1, 4, 1, 9, 3.0)                         # from the cell next to the border, top left ...
    lake(h - 5, h - 1, w - 8, w - 1, 3.0)         # ... and bottom right
    rng = np.random.default_rng(h * 1000 + w)
    for _ in range(12):                           # one-cell pits
        dem[rng.integers(1, h - 1), rng.integers(1, w - 1)] -= np.float32(1.0)
    return np.ascontiguousarray(dem)


SURFACES = {"terraced": _terraced, "ramp": _ramp}
_cache = {}


def dem_of(surface, shape):
    key = (surface,) + tuple(shape)
    if key not in _cache:
        d = SURFACES[surface](*shape)
        d.setflags(write=False)
        _cache[key] = d
    return _cache[key]


def run_chain(pipe, dem, monkeypatch, knob):
    monkeypatch.setenv("MHIP_DEVELOPER", "1")
    monkeypatch.setenv("MHIP_WETBITS", str(knob))
    pipe.upload("dem", dem)
    pipe.run(*ALL)
    got = collect(pipe)
    got["raw_stats"] = pipe.raw_stats()
    got["engines"] = {k: pipe.get_int(k) for k in COUNTERS}       # (compared with == by assert_same_results)
    return got, pipe.get_int("wetbits_used")


def both_knobs(dem, monkeypatch, expect_used=3):
    from malstroem_amd.pipeline import HydroPipeline
    with HydroPipeline(dem.shape) as pipe:
        on, used_on = run_chain(pipe, dem, monkeypatch, 1)
        off, used_off = run_chain(pipe, dem, monkeypatch, 0)
        again, used_again = run_chain(pipe, dem, monkeypatch, 1)     # (the buffer of the first request has gone back to the pool)
    assert (used_on, used_off, used_again) == (expect_used, 0, expect_used)
    assert_same_results(on, off)
    assert_same_results(again, off)
    return on


def oracle_of(dem):
    filled = oracle.fill_terrain(dem)
    short, diag = oracle.minimum_safe_short_and_diag(dem)
    noflat = oracle.fill_terrain_no_flats(dem, short, diag)
    flowdir = oracle.terrain_flowdirection(noflat)
    accum = oracle.accumulated_flow(flowdir)
    depths = oracle.depths(filled, dem)
    labels, n = oracle.connected_components(depths)
    ws = labels.copy()
    oracle.watersheds_from_labels(flowdir, ws)
    return {"dem": dem, "filled": filled, "depths": depths, "noflat": noflat, "flowdir": flowdir, "accum": accum, "labels": labels,
            "watersheds": ws, "nlabels": n, "stats": oracle.label_stats(depths, labels, n), "counts": oracle.label_count(ws),
            "pour": oracle.label_max_index(accum, labels, n)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("surface", sorted(SURFACES))
def test_the_bits_change_nothing(monkeypatch, surface, shape):
    dem = dem_of(surface, shape)
    on = both_knobs(dem, monkeypatch)
    assert on["engines"]["fill_algorithm"] == 1 and on["engines"]["noflat_algorithm"] == 2 and on["engines"]["fill_handover"] == 1
    assert on["engines"]["noflat_reject"] == 0 and on["engines"]["noflat_reject_mismatch"] == 0
    wet = on["depths"] != 0
    assert wet.any() == (surface == "terraced")
    if surface == "terraced":       # the lakes are where the cases want them
        h, w = shape
        assert wet[1, 1] and wet[h - 2, w - 2]
        assert all(wet[r, w // 2] for r in (62, 63, 64) if r < h - 1) and all(wet[h // 2, c] for c in (62, 63, 64, 124, 125, 128) if c < w - 1)
        assert not wet[0].any() and not wet[-1].any() and not wet[:, 0].any() and not wet[:, -1].any()
        assert on["nlabels"] >= 3
    if shape in ((188, 250), (63, 125)):
        assert_equals_oracle(on, oracle_of(dem))


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_dem_that_is_not_finite_keeps_the_floats(monkeypatch, value):
    """no bits over a NaN or an infinity: `filled > dem` is not `filled - dem != 0` there.  Whatever the request makes of such a DEM,
    it makes the same of it under either knob, with the kernels of before."""
    from malstroem_amd.pipeline import HydroPipeline
    dem = np.array(dem_of("terraced", (130, 200)))
    dem[70, 90] = value
    ends, got = [], []
    with HydroPipeline(dem.shape) as pipe:
        for knob in (1, 0):
            monkeypatch.setenv("MHIP_DEVELOPER", "1")
            monkeypatch.setenv("MHIP_WETBITS", str(knob))
            pipe.upload("dem", dem)
            try:
                pipe.run(*ALL)
                pipe.sync()
                ends.append("ran")
            except RuntimeError as e:
                ends.append(str(e))
            assert pipe.get_int("wetbits_used") == 0
            got.append(collect(pipe) if ends[-1] == "ran" else {k: pipe.download(k) for k in ("filled", "depths")})
    assert ends[0] == ends[1], ends
    assert_same_results(got[0], got[1])


def test_a_proof_taken_as_failed_keeps_the_floats(monkeypatch):
    """MHIP_HO_RECHECK: the visit's proof counts as failed, the flood's own last pass writes the raster -- the visit's words are
    not taken; without the hook the same context takes them again"""
    from malstroem_amd.pipeline import HydroPipeline
    dem = dem_of("terraced", (188, 250))
    with HydroPipeline(dem.shape) as pipe:
        off, used = run_chain(pipe, dem, monkeypatch, 0)
        assert used == 0
        monkeypatch.setenv("MHIP_HO_RECHECK", "1")
        got, used = run_chain(pipe, dem, monkeypatch, 1)
        assert used == 0 and pipe.get_int("fill_handover_rechecks") == 1
        assert_same_results(got, off)
        monkeypatch.delenv("MHIP_HO_RECHECK")
        got, used = run_chain(pipe, dem, monkeypatch, 1)
        assert used == 3
        assert_same_results(got, off)


def test_depths_from_outside_are_labelled_from_the_floats(monkeypatch):
    """fill, then uploaded depths, then label: three requests -- the bits of a request end with it"""
    from malstroem_amd.pipeline import HydroPipeline
    dem = dem_of("terraced", (126, 190))
    other = np.zeros(dem.shape, dtype=np.float32)
    other[10:20, 10:30] = 1.5
    other[60:70, 100:180] = np.float32(1e-45)      # a denormal depth is foreground
    other[0, 5] = 2.0                               # and so is a border cell, here
    want_labels, want_n = oracle.connected_components(other)
    monkeypatch.setenv("MHIP_DEVELOPER", "1")
    monkeypatch.setenv("MHIP_WETBITS", "1")
    with HydroPipeline(dem.shape) as pipe:
        pipe.upload("dem", dem)
        pipe.run(*ALL)
        pipe.sync()
        assert pipe.get_int("wetbits_used") == 3
        pipe.run("fill")
        pipe.sync()
        assert pipe.get_int("wetbits_used") == 0
        pipe.upload("depths", other)
        pipe.run("label")
        pipe.sync()
        assert pipe.get_int("wetbits_used") == 0
        assert pipe.get_int("nlabels") == want_n == 3
        assert_same_bits(pipe.download("labels"), want_labels, "labels")
        pipe.upload("dem", dem)
        pipe.run("fill", "noflat", "label")        # without flowdir: the plain finishing pass takes the bits too
        pipe.sync()
        assert pipe.get_int("wetbits_used") == 3
        want = oracle.depths(oracle.fill_terrain(dem), dem)
        lab, n = oracle.connected_components(want)
        assert pipe.get_int("nlabels") == n
        assert_same_bits(pipe.download("labels"), lab, "labels")
        short, diag = oracle.minimum_safe_short_and_diag(dem)
        assert_same_bits(pipe.download("noflat"), oracle.fill_terrain_no_flats(dem, short, diag), "noflat")
