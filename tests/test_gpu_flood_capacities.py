"""GPU: every capacity fall-back of the tiled priority-flood (csrc/pflood.hip), AT the limit (the flood runs) and just OVER it (the
iterative schedule runs, and fill_overflow names the capacity and nothing else; the link fields, whose seeds depend on the order
of the kernel's relaxations, may come out on either side of LMAX and assert that much), on one context, on a reused context, through
the rest of the chain, through the stage function and on row bands where one band falls back while its neighbours stay on the
flood.  The fields and what they claim come from _flood_inputs.py; the claims are checked on the CPU by test_pflood_model.py.
The suite's environment (conftest.py: MHIP_DEVELOPER) poisons the device pool: a count or a table a tile left unwritten when it
gave up reads as garbage, not as the previous run's values."""
import functools

import numpy as np
import pytest

import _flood_inputs as FI
import oracle
from _cases import assert_same_bits
from test_gpu_bands import check_bands_against_oracle, run_bands

pytestmark = pytest.mark.gpu

MEMBERS = dict(FI.members())
PAIRS_OF_A_SHAPE = [(over, over.replace("-over", "-at") if over != "basins-over" else "basins-edge") for over in MEMBERS if "-over" in over]
ONE_OVER_PER_LIMIT = [n for n in MEMBERS if "-over" in n and "w256" not in n]


@functools.lru_cache(maxsize=None)
def case(name):
    """(dem, claims, oracle's filled, oracle's depths): computed once, shared, never written to"""
    dem, claims = MEMBERS[name]()
    want = oracle.fill_terrain(dem)
    dep = oracle.depths(want, dem)
    for a in (dem, want, dep):
        a.setflags(write=False)
    return dem, claims, want, dep


def fill_and_check(pipe, name):
    dem, claims, want, dep = case(name)
    pipe.upload("dem", dem)
    pipe.run("fill")
    pipe.sync()
    got = (pipe.get_int("fill_algorithm"), pipe.get_int("fill_overflow"))
    print(name, "fill_algorithm, fill_overflow =", got, "claimed", (claims["algorithm"], claims["mask"]))
    assert_same_bits(pipe.download("filled"), want, name + " filled")
    assert_same_bits(pipe.download("depths"), dep, name + " depths")
    if "either" in claims:      # a field whose seeds depend on the order of the kernel's relaxations: on either side of its limit, nothing else
        assert got in claims["either"], (name, got, claims)
    else:
        assert got == (claims["algorithm"], claims["mask"]), (name, got, claims)      # (4 = the proof had to repair the flood's surface: a failure)


@pytest.mark.parametrize("name", list(MEMBERS))
def test_at_the_limit_the_flood_runs_and_over_it_the_mask_names_the_limit(name):
    from malstroem_amd.pipeline import HydroPipeline
    with HydroPipeline(case(name)[0].shape) as pipe:
        fill_and_check(pipe, name)


@pytest.mark.parametrize("over,at", PAIRS_OF_A_SHAPE)
def test_one_context_over_at_over_at(over, at):
    """what a tile that gave up left behind (counts, tables, links, the flags word) must not reach the next run of the context"""
    from malstroem_amd.pipeline import HydroPipeline
    with HydroPipeline(case(over)[0].shape) as pipe:
        for name in (over, at, over, at):
            fill_and_check(pipe, name)


@pytest.mark.parametrize("name", ONE_OVER_PER_LIMIT)
def test_the_rest_of_the_chain_after_a_fall_back(name):
    from malstroem_amd.pipeline import HydroPipeline
    dem, claims, want, _ = case(name)
    with HydroPipeline(dem.shape) as pipe:
        fill_and_check(pipe, name)
        pipe.run("noflat", "flowdir")
        pipe.sync()
        short, diag = oracle.minimum_safe_short_and_diag(dem)
        fnf = oracle.fill_terrain_no_flats(dem, short, diag)
        assert_same_bits(pipe.download("noflat"), fnf, name + " noflat")
        assert_same_bits(pipe.download("flowdir"), oracle.terrain_flowdirection(fnf), name + " flowdir")


@pytest.mark.parametrize("name", list(MEMBERS))
def test_stage_function_on_the_same_members(name):
    import malstroem_amd.algorithms as alg
    dem, _, want, _ = case(name)
    assert_same_bits(alg.fill.fill_terrain(dem), want, name)


@pytest.mark.parametrize("which", ["middle", "first", "links"])
def test_one_band_falls_back_while_its_neighbours_stay_on_the_flood(which):
    """three bands with their seams on the tile grid; the capacity gives out in PfRun::begin of one band (mhip_ctx_fill_begin
    switches that band to the iterative schedule), the others trade edge rows with it from the flood"""
    dem, claims = FI.band_case(which)
    out = run_bands(dem, 3)
    engines = tuple(o["engines"][0] for o in out)
    print(which, "engines", engines, "masks", [o["fill_overflow"] for o in out])
    check_bands_against_oracle(dem, out)
    got = [(e, o["fill_overflow"]) for e, o in zip(engines, out)]
    want = list(zip(claims["engines"], claims["masks"]))
    if "middle_either" in claims:
        assert got[1] in claims["middle_either"], got
        got[1] = want[1]
    assert got == want
