"""GPU: where the label branch of a whole request starts (csrc/ctx_run.hip, MHIP_LABEL_START = 0 | 1 | 2 | 3).

0: with the no-flats fill, 1: at its latency-bound tail rounds, 2: behind it, 3: at its finishing pass (GeoRun::end fires the
hook in front of ng_finish_kernel / ng_assemble_kernel).  The start point moves work in time and nothing else: every case
runs the whole request and compares all seven rasters, the label count, the label statistics, the watershed counts and the pour
points with the oracle -- label sums by the rule of test_gpu_parity.py, everything else bit for bit.

The knob is read per request, so one process switches it between requests (monkeypatch.setenv)."""
import numpy as np
import pytest

import oracle
from _cases import assert_label_sums, assert_same_bits, fbm

pytestmark = pytest.mark.gpu

ALL = ("fill", "noflat", "flowdir", "accum", "label", "watershed", "pourpoints")
RASTERS = ("filled", "depths", "noflat", "flowdir", "accum", "labels", "watersheds")


def _fbm_264():
    return fbm(200, 264, beta=2.0, seed=31) + np.float32(3.0)     # 4 x 5 CCL tiles of 64, 4 x 5 no-flats tiles of 62, ragged edges


def _fbm_67():
    return fbm(131, 67, beta=2.5, seed=32) + np.float32(3.0)


def _lake():
    """192 x 192, one lake over 3 x 3 no-flats tiles: a basin 152 cells wide, 5 m below a rough plain, that spills over the
    lowest point of its rim -- the distances travel across the whole flat, tile by tile: many rounds, a long tail."""
    dem = fbm(192, 192, beta=2.0, seed=33) * np.float32(0.01) + np.float32(10.0)
    dem[20:172, 20:172] -= np.float32(5.0)
    return np.ascontiguousarray(dem)


def _sea_at_zero():
    """the raster of test_gpu_noflat_geodesic.py with a flat at elevation 0: no constant ulp above 0, the integer transform
    does not cover that flat and the float64 relaxation settles it"""
    dem = fbm(400, 300, beta=2.0, seed=13)
    dem[100:200, :250] = 0.0
    return dem


def _two_rows():
    return fbm(2, 70, beta=2.0, seed=34) + np.float32(3.0)        # H < 3: the transform is not applicable, no round is launched


DEMS = {"fbm200x264": _fbm_264, "fbm131x67": _fbm_67, "lake192": _lake, "sea_at_zero": _sea_at_zero, "two_rows": _two_rows}
_cache = {}


def case(name):
    """the DEM and what the oracle makes of it, computed once per module and never written to"""
    if name not in _cache:
        dem = np.ascontiguousarray(DEMS[name](), dtype=np.float32)
        filled = oracle.fill_terrain(dem)
        short, diag = oracle.minimum_safe_short_and_diag(dem)
        noflat = oracle.fill_terrain_no_flats(dem, short, diag)
        flowdir = oracle.terrain_flowdirection(noflat)
        accum = oracle.accumulated_flow(flowdir)
        depths = oracle.depths(filled, dem)
        labels, n = oracle.connected_components(depths)
        ws = labels.copy()
        oracle.watersheds_from_labels(flowdir, ws)
        want = {"dem": dem, "filled": filled, "depths": depths, "noflat": noflat, "flowdir": flowdir, "accum": accum, "labels": labels,
                "watersheds": ws, "nlabels": n, "stats": oracle.label_stats(depths, labels, n), "counts": oracle.label_count(ws),
                "pour": oracle.label_max_index(accum, labels, n)}
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = want
    return _cache[name]


def collect(pipe, rasters=RASTERS, pour=True, final_labels=True):
    pipe.sync()
    got = {k: pipe.download(k) for k in rasters}
    got["nlabels"] = pipe.get_int("nlabels")
    got["stats"] = pipe.stats() if final_labels else pipe.raw_stats()      # (labels are settled as final by WATERSHED / POURPOINTS)
    if "watersheds" in rasters:
        got["counts"] = pipe.watershed_counts()
    if pour:
        got["pour"] = pipe.pourpoints()
    got["engines"] = {k: pipe.get_int(k) for k in ("fill_algorithm", "noflat_algorithm")}
    return got


def run_all(dem, pipe=None):
    from malstroem_amd.pipeline import HydroPipeline
    if pipe is not None:
        pipe.upload("dem", dem)
        pipe.run(*ALL)
        return collect(pipe)
    with HydroPipeline(dem.shape) as p:
        return run_all(dem, p)


def assert_equals_oracle(got, want):
    for k in RASTERS:
        assert_same_bits(got[k], want[k], k)
    assert got["nlabels"] == want["nlabels"]
    for f in ("min", "max", "count"):
        assert_same_bits(got["stats"][f], want["stats"][f], "stats." + f)
    assert_label_sums(got["stats"]["sum"], want["stats"]["sum"], want["depths"], want["labels"])
    assert_same_bits(got["counts"], want["counts"], "watershed counts")
    assert_same_bits(got["pour"], want["pour"], "pour points")


def assert_same_results(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == "engines" or k == "nlabels":
            assert a[k] == b[k], k
        else:
            assert_same_bits(a[k], b[k], k)      # (the same kernels in the same order of summation: the sums too)


@pytest.fixture(scope="module")
def engines_at_2():
    """the engines each raster takes at start 2 (behind the no-flats fill), one run per raster"""
    seen = {}

    def get(name, monkeypatch):
        if name not in seen:
            monkeypatch.setenv("MHIP_LABEL_START", "2")
            seen[name] = run_all(case(name)["dem"])["engines"]
        return seen[name]
    return get


@pytest.mark.parametrize("start", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["fbm200x264", "fbm131x67", "lake192"])
def test_every_start_point_gives_the_oracles_results(monkeypatch, engines_at_2, name, start):
    """MHIP_NG_BATCH=1: one round per host read-back, so that these small rasters reach the self-listing tail rounds, where start 1
    fires (and runs the one-wavefront round kernel beside the labelling)."""
    monkeypatch.setenv("MHIP_NG_BATCH", "1")
    want_engines = engines_at_2(name, monkeypatch)
    monkeypatch.setenv("MHIP_LABEL_START", str(start))
    got = run_all(case(name)["dem"])
    assert_equals_oracle(got, case(name))
    assert got["engines"] == want_engines
    assert got["engines"]["noflat_algorithm"] == 2      # the geodesic transform: the hooks of 1 and 3 sit in its rounds / its end


def test_a_rejected_finishing_pass_reruns_beside_the_label_branch(monkeypatch):
    """MHIP_NG_CORRUPT: wrong distances in one row.  The hook has fired in front of the finishing pass, the pass rejects its
    surface, and the float64 relaxation re-runs the no-flats fill while the label branch is in flight: it reads the depths and
    writes labels and work buffers of its own, the relaxation reads the DEM and writes the no-flats surface."""
    monkeypatch.setenv("MHIP_LABEL_START", "3")
    monkeypatch.setenv("MHIP_NG_CORRUPT", "1")
    for name in ("fbm200x264", "lake192"):
        got = run_all(case(name)["dem"])
        assert got["engines"]["noflat_algorithm"] != 2, got["engines"]
        assert_equals_oracle(got, case(name))


@pytest.mark.parametrize("name,algorithms", [("sea_at_zero", (3,)), ("two_rows", (0,))])
def test_start_3_where_the_transform_does_not_finish_the_job(monkeypatch, name, algorithms):
    """sea_at_zero: the flat at 0 has no integer weights -- the transform covers the other levels (its hook fires in front of
    ng_assemble_kernel), the relaxation settles the rest beside the label branch.  two_rows: not applicable, rejected before
    any round -- no finishing pass to fire at, the label branch starts behind the stage like at 2.  It runs either way."""
    monkeypatch.setenv("MHIP_LABEL_START", "3")
    got = run_all(case(name)["dem"])
    assert got["engines"]["noflat_algorithm"] in algorithms, got["engines"]
    assert_equals_oracle(got, case(name))


def test_partial_requests_at_start_3_equal_the_serial_run(monkeypatch):
    """request masks that leave the main side short: (a) label, watershed, accum with the flow directions resident -- no
    no-flats fill in the request, the hook fires from mhip_ctx_run itself; (b) fill, noflat, label without flowdir -- the
    finishing pass is ng_finish_kernel<false>.  Both return and equal the same stages on one stream (MHIP_SERIAL=1)."""
    from malstroem_amd.pipeline import HydroPipeline
    want = case("fbm200x264")

    def request_a(pipe):
        pipe.upload("depths", want["depths"])
        pipe.upload("flowdir", want["flowdir"])
        pipe.run("label", "watershed", "accum")
        return collect(pipe, ("accum", "labels", "watersheds"), pour=False)

    def request_b(pipe):
        pipe.upload("dem", want["dem"])
        pipe.run("fill", "noflat", "label")
        return collect(pipe, ("filled", "depths", "noflat", "labels"), pour=False, final_labels=False)

    for request in (request_a, request_b):
        monkeypatch.setenv("MHIP_LABEL_START", "3")
        monkeypatch.delenv("MHIP_SERIAL", raising=False)
        with HydroPipeline(want["dem"].shape) as pipe:
            got = request(pipe)
        monkeypatch.setenv("MHIP_SERIAL", "1")
        with HydroPipeline(want["dem"].shape) as pipe:
            serial = request(pipe)
        assert_same_results(got, serial)
        for k in got:
            if k in RASTERS:
                assert_same_bits(got[k], want[k], k)
        assert got["nlabels"] == want["nlabels"]


def test_two_requests_in_a_row_on_one_context(monkeypatch):
    """the hook is once-only per request and the knob is read per request: one context runs a request at start 1, the same DEM
    again at start 3, then -- after a new DEM upload -- a third request at start 3, which equals a fresh context's"""
    from malstroem_amd.pipeline import HydroPipeline
    monkeypatch.setenv("MHIP_NG_BATCH", "1")
    first, second = case("lake192"), case("fbm200x264")
    flipped = np.ascontiguousarray(second["dem"][:192, :192][::-1])       # a third DEM of the context's shape
    with HydroPipeline(first["dem"].shape) as pipe:
        monkeypatch.setenv("MHIP_LABEL_START", "1")
        assert_equals_oracle(run_all(first["dem"], pipe), first)
        monkeypatch.setenv("MHIP_LABEL_START", "3")
        again = run_all(first["dem"], pipe)
        assert_equals_oracle(again, first)
        reused = run_all(flipped, pipe)
    fresh = run_all(flipped)
    assert_same_results(reused, fresh)
    assert fresh["engines"]["noflat_algorithm"] == 2
