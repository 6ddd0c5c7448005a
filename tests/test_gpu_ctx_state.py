"""GPU: what a context still vouches for after one of its resident rasters has been (re)written (csrc/ctx.hip: ctx_wrote;
the table is DESIGN.md 4.5a).  The per-label record sets -- statistics, watershed counts, pour points -- and the hypsometry
table describe the rasters they were computed from: a getter either returns the records of the RESIDENT rasters or refuses,
whichever way the raster came in (a stage, a whole upload, a windowed upload, a band call).

The DEMs are quantised to 1/64 m, so the depths are small multiples of 1/64 and every float64 sum of them is exact in any
order: the records are compared with the oracle's bit for bit, the sums included.
Every held result of a context, under mixed sequences of calls, against a host shadow of it: tests/test_gpu_ctx_sequences.py."""
import math

import numpy as np
import pytest

import oracle
from _cases import fbm

pytestmark = pytest.mark.gpu

SHAPE = (160, 224)
RES = 0.05
GETTERS = ("stats", "watershed_counts", "pourpoints")


def quantised(beta, seed):
    return (np.round(fbm(*SHAPE, beta=beta, seed=seed).astype(np.float64) * 64) / 64).astype(np.float32)


def chain(dem):
    """the oracle's rasters and records of one DEM (every bluespot kept)"""
    dep = oracle.depths(oracle.fill_terrain(dem), dem)
    lab, n = oracle.connected_components(dep)
    assert n > 0
    sh, dg = oracle.minimum_safe_short_and_diag(dem)
    fd = oracle.terrain_flowdirection(oracle.fill_terrain_no_flats(dem, sh, dg))
    return dict(dem=dem, depths=dep, labels=lab, n=n, flowdir=fd, **records(dep, lab, n, fd))


def records(dep, lab, n, fd):
    acc = oracle.accumulated_flow(fd)
    ws = lab.copy()
    oracle.watersheds_from_labels(fd, ws, 0)
    return dict(stats=oracle.label_stats(dep, lab, n), watershed_counts=np.bincount(ws.ravel(), minlength=n + 1).astype(np.int64),
                pourpoints=oracle.label_max_index(acc, lab, n))


@pytest.fixture(scope="module")
def A():
    return chain(quantised(2.0, 11))


@pytest.fixture(scope="module")
def B():
    return chain(quantised(1.2, 12))      # rougher: more bluespots


def same_records(got, want):
    assert got.shape == want.shape
    if want.dtype.names is None:
        return np.array_equal(got[1:], want[1:])
    return all(np.array_equal(got[f][1:], want[f][1:]) for f in want.dtype.names)


def refused(call):
    with pytest.raises(ValueError):
        call()
    return True


def test_new_dem_and_partial_rerun(A, B):
    from malstroem_amd.pipeline import HydroPipeline
    assert 20 < A["n"] < B["n"]
    with HydroPipeline(SHAPE) as p:
        p.upload("dem", A["dem"])
        p.run("fill", "noflat", "flowdir", "accum", "label", "watershed", "pourpoints")
        for g in GETTERS:
            assert same_records(getattr(p, g)(), A[g]), g
        p.upload("dem", B["dem"])
        p.run("fill", "label")
        assert p.apply_keep(None) == B["n"]
        assert same_records(p.stats(), B["stats"])
        # the counts and pour points on the device are DEM A's (and shorter than B's): refused, not copied out
        assert refused(p.watershed_counts) and refused(p.pourpoints)
        p.run("noflat", "flowdir", "accum", "watershed", "pourpoints")
        for g in GETTERS:
            assert same_records(getattr(p, g)(), B[g]), g


def test_uploaded_depths_drop_the_statistics(A, B):
    from malstroem_amd.pipeline import HydroPipeline
    with HydroPipeline(SHAPE) as p:
        p.upload("dem", A["dem"])
        p.run("fill", "label")
        p.apply_keep(None)
        assert same_records(p.stats(), A["stats"])
        p.upload("depths", B["depths"])
        assert refused(p.stats) and p.get_int("hyps_bins") == -1
        p.hypsometry(RES)                    # (computes the statistics of uploaded rasters first)
        assert same_records(p.stats(), oracle.label_stats(B["depths"], A["labels"], A["n"]))


def observe(p):
    """the observable validity state of a context: the table's size and what every record getter answers"""
    state = {"hyps_bins": p.get_int("hyps_bins")}
    for g in GETTERS:
        try:
            state[g] = getattr(p, g)().tobytes()
        except ValueError:
            state[g] = "refused"
    return state


# raster -> (what the table of DESIGN.md 4.5a says is refused right after it was written, the stages to run again)
WRITES = {
    "dem": (GETTERS, ("fill", "noflat", "flowdir", "accum", "label", "watershed", "pourpoints")),
    "depths": (("stats",), ("label", "watershed", "pourpoints")),
    "flowdir": ((), ("accum", "watershed", "pourpoints")),
    "labels": (GETTERS, ("watershed", "pourpoints")),
}


@pytest.mark.parametrize("name", sorted(WRITES))
def test_whole_and_windowed_upload_agree(A, B, name):
    from malstroem_amd.pipeline import HydroPipeline
    gone, stages = WRITES[name]
    h = SHAPE[0]
    windows = [(h // 3, 2 * h // 3), (0, h // 3), (2 * h // 3, h)]       # any order, the last window last
    states = []
    for windowed in (False, True):
        with HydroPipeline(SHAPE) as p:
            p.upload("dem", A["dem"])
            p.run("fill", "noflat", "flowdir", "accum", "label", "watershed", "pourpoints")
            p.hypsometry(RES)
            before = observe(p)
            assert before["hyps_bins"] >= 0 and "refused" not in before.values()
            if windowed:
                for r0, r1 in windows:
                    p.upload_rows(name, r0, B[name][r0:r1])
            else:
                p.upload(name, B[name])
            after = observe(p)
            for g in GETTERS:
                assert (after[g] == "refused") == (g in gone), (name, g)
                assert g in gone or after[g] == before[g], (name, g)
            assert after["hyps_bins"] == (before["hyps_bins"] if name == "flowdir" else -1)
            assert np.array_equal(p.download(name), B[name])
            p.run(*stages)
            p.hypsometry(RES)
            final = observe(p)
            assert final["hyps_bins"] >= 0 and "refused" not in final.values()
            states.append((after, final, p.download("watersheds"), p.download("labels")))
    (a0, f0, ws0, lab0), (a1, f1, ws1, lab1) = states
    assert a0 == a1 and f0 == f1
    assert np.array_equal(ws0, ws1) and np.array_equal(lab0, lab1)
    if name == "dem":
        with HydroPipeline(SHAPE) as p:      # (and what the rerun gives is the new DEM's)
            p.upload_rows("dem", 0, B["dem"])
            p.run(*stages)
            for g in GETTERS:
                assert same_records(getattr(p, g)(), B[g]), g


def test_band_relabelling_drops_the_band_records(A):
    """two bands of one raster on one device; no bluespot crosses the seam, so the band-local components in band order are the
    undivided raster's"""
    from malstroem_amd.distributed import HipBand
    h, w = SHAPE
    half = h // 2
    dep = A["depths"].copy()
    dep[half - 1:half + 1] = 0
    lab, n = oracle.connected_components(dep)
    want = oracle.label_stats(dep, lab, n)
    bands = [HipBand(h, w, 0, half, device=0, rank=0, size=2), HipBand(h, w, half, h - half, device=0, rank=1, size=2)]
    try:
        bands[0].upload("depths", dep[:half])
        bands[1].upload("depths", dep[half:])
        bands[0].set_halo_row("depths", 1, dep[half])
        bands[1].set_halo_row("depths", 0, dep[half - 1])
        nloc = [b.ccl_local() for b in bands]
        assert sum(nloc) == n and min(nloc) > 2
        none = np.zeros(0, np.int32)
        for b, (lo, hi) in zip(bands, ((1, nloc[0]), (nloc[0] + 1, n))):
            assert refused(lambda: b.records_fetch(0, lo, hi - lo + 1))               # labelled, no records yet
            b.relabel_sparse(hi - lo + 1, lo - 1, none, none, n)
            assert refused(lambda: b.records_fetch(0, lo, hi - lo + 1))
            b.records_compute(0)
            assert same_records(b.records_fetch(0, lo - 1, hi - lo + 2), want[lo - 1:hi + 1])
            # the filter: every second bluespot of this band goes
            keep = np.arange(hi - lo + 1) % 2 == 0
            lut = np.where(keep, lo - 1 + np.cumsum(keep), 0).astype(np.int32)
            b.relabel_range(lo, hi, lut, none, none, n)
            assert refused(lambda: b.records_fetch(0, lo, int(keep.sum())))
            assert refused(lambda: b.records_gather(0, np.array([lo], np.int64)))
            b.records_compute(0)
            got = b.records_fetch(0, lo, int(keep.sum()))
            kept = want[lo:hi + 1][keep]
            assert all(np.array_equal(got[f], kept[f]) for f in kept.dtype.names)
    finally:
        for b in bands:
            b.close()


def test_stage_timers_start_out_unset(A):
    from malstroem_amd.pipeline import HydroPipeline
    with HydroPipeline(SHAPE) as p:
        p.upload("dem", A["dem"])
        p.run("fill", "label")
        with pytest.raises(ValueError, match="stage has not been run"):
            p.stage_ms("accum")
        with pytest.raises(ValueError, match="stage has not been run"):
            p.kernel_ms("hyps_table")
        p.run("noflat", "flowdir", "accum")
        ms = p.stage_ms("accum")
        assert math.isfinite(ms) and ms >= 0
        p.apply_keep(None)
        p.hypsometry(RES)
        ms, launches = p.kernel_ms("hyps_table")
        assert math.isfinite(ms) and ms >= 0 and launches == 1


# every raster a context holds outside RASTERS: the key that reports it, its row getter, its name as a source of zone_stats (None: no
# source), and what the getter and the source say while none is held -- the getters that ask the key first answer from Python
# (pipeline.py), the others and every source with the message of the library's table (csrc/ctx.hip: HELD)
HELD = (
    ("wet_at_events", "download_wet_at_rows", "wet_at", "ctx_wet_at_rows needs mhip_ctx_wet_at on the resident depths and labels", None),
    ("flow_distance_unresolved", "download_flow_distance_rows", "flow_distance",
     "ctx_flow_distance_rows needs mhip_ctx_flow_distance on the resident flow directions and labels", None),
    ("travel_time_unresolved", "download_travel_time_rows", "travel_time", "ctx_travel_time_rows needs mhip_ctx_travel_time on the resident rasters", None),
    ("hand_undrained", "download_hand_rows", "hand", "ctx_hand_rows needs mhip_ctx_hand on the resident rasters", r"hand\(\) has not been run on the resident rasters"),
    ("hand_undrained", "download_drain_distance_rows", "drain_distance", "ctx_hand_rows needs mhip_ctx_hand on the resident rasters",
     r"hand\(\) has not been run on the resident rasters"),
    ("reach_catchments", "download_reach_catchments_rows", None, "ctx_reach_catchments_rows needs mhip_ctx_reach_catchments on the resident rasters",
     r"reach_catchments\(\) has not been run on the resident rasters"),
    ("inundation", "download_inundation_rows", "inundation", "ctx_inundation_rows needs mhip_ctx_inundate on the held hand and reach catchments",
     r"inundate\(\) has not been run on the held hand and reach catchments"),
    ("zones", "download_zones_rows", None, "ctx_zones_rows needs mhip_ctx_rasterize_zones", None),
    ("sea_flood", "download_sea_level_rows", "sea_level", "ctx_sea_flood_rows needs mhip_ctx_sea_flood on the resident DEM",
     r"sea_flood\(\) has not been run on the resident DEM"),
    ("sea_depths", "download_sea_depths_rows", "sea_depths", "ctx_sea_flood_rows needs mhip_ctx_sea_depths on the held sea levels",
     r"sea_depths\(\) has not been run on the held sea levels"),
    ("sea_classes", "download_sea_classes_rows", None, "ctx_sea_classes_rows needs mhip_ctx_sea_classes on the held sea levels",
     r"sea_classes\(\) has not been run on the held sea levels"),
)


def test_a_fresh_context_holds_nothing_and_every_reader_of_a_held_raster_says_so():
    from malstroem_amd.pipeline import HydroPipeline
    with HydroPipeline((16, 16)) as p:
        p.upload("dem", fbm(16, 16, beta=2.0, seed=3))
        for key in [h[0] for h in HELD] + ["travel_time_saturated", "travel_time_bins"]:
            assert p.get_int(key) == -1, key
        for key, getter, source, library, python in HELD:
            with pytest.raises(ValueError, match=python or library):
                getattr(p, getter)(0, 16)
        assert {h[2] for h in HELD if h[2]} == set(p.ZONE_SOURCES) - {"dem", "filled", "depths", "finaldepths"}
        for source in p.ZONE_SOURCES:
            with pytest.raises(ValueError, match=r"rasterize_zones\(\) has not been run"):
                p.zone_stats(source)
        with pytest.raises(ValueError, match="ctx_reach_catchments_rows needs mhip_ctx_reach_catchments on the resident rasters"):
            p.polygonize("reach_catchments")
        with pytest.raises(ValueError, match="ctx_sea_classes_rows needs mhip_ctx_sea_classes on the held sea levels"):
            p.polygonize("sea_classes")
        # with (empty) zones every held source gets as far as the library's table, and none of the other products has appeared
        p.rasterize_zones(np.zeros((0, 2)), [0], np.zeros(0, dtype=np.int32), 3)
        assert p.get_int("zones") == 3 and not p.download_zones_rows(0, 16).any()
        for key, getter, source, library, python in HELD:
            if source:
                with pytest.raises(ValueError, match=library):
                    p.zone_stats(source)
            if key != "zones":
                assert p.get_int(key) == -1, key
        assert p.zone_stats("dem").shape == (4,)
