"""CPU: the NumPy model of the tiled priority-flood's tables (_pflood_model.py) against the oracle, and every claim of the
capacity families (_flood_inputs.py) against the model.  The GPU tests (test_gpu_flood_capacities.py) trust these claims."""
import functools

import numpy as np
import pytest

import _flood_inputs as FI
import _pflood_model as M
import oracle


def _noise(h, w, seed):
    return np.random.default_rng(seed).random((h, w)).astype(np.float32)


def _waves(h, w, seed):
    """smooth hills (few basins, long drainage paths across tiles) + noise far above float32 resolution: no equal neighbours"""
    r, c = np.mgrid[0:h, 0:w]
    z = 3 * np.sin(r / 17.0) * np.cos(c / 23.0) + 0.01 * r + 0.05 * np.random.default_rng(seed).random((h, w))
    return z.astype(np.float32)


RASTERS = [("noise 188x188", _noise(188, 188, 1)), ("noise 131x77 ragged", _noise(131, 77, 2)), ("noise 200x260 ragged", _noise(200, 260, 3)),
           ("noise 64x64 one tile", _noise(64, 64, 4)), ("noise 40x50 one tile", _noise(40, 50, 5)), ("noise 3x3", _noise(3, 3, 6)),
           ("noise 65x64 a one-row tile", _noise(65, 64, 7)), ("noise 64x127", _noise(64, 127, 8)),
           ("waves 300x190", _waves(300, 190, 9)), ("waves 126x126 two tiles each way", _waves(126, 126, 10)),
           ("waves 64x250", _waves(64, 250, 11)), ("negative 90x100", _noise(90, 100, 13) - np.float32(0.5)),
           ("ring pits", FI.ring_pits(188, 188, None)), ("lattice", FI.lattice(188, 188, 300, 63, 63))]


@pytest.mark.parametrize("name,dem", RASTERS, ids=[n for n, _ in RASTERS])
def test_model_fill_equals_the_oracle(name, dem):
    assert not M.has_ties(dem)
    assert np.array_equal(M.model(dem).filled.view(np.uint32), oracle.fill_terrain(dem).view(np.uint32))


@pytest.mark.parametrize("rows", [(0, 64), (62, 126), (124, 188)], ids=["top band", "middle band", "bottom band"])
def test_model_fill_of_a_band_slice_equals_the_oracle(rows):
    """a band's local raster: its halo rows are ring rows whose cells carry the neighbour's filled edge row (here: the final one)"""
    dem = _noise(188, 150, 21)
    dem[60:130, 40:110] -= np.float32(0.3)            # a depression across both seams
    want = oracle.fill_terrain(dem)
    a, b = rows
    top, bot = a > 0, b < 188
    m = M.model(dem[a:b], top, bot, want[a] if top else None, want[b - 1] if bot else None)
    assert np.array_equal(m.filled, want[a:b])
    assert (np.array(m.nhalo) > 0).any()
    # before the first exchange nothing is known about the neighbours: an upper bound of the final surface
    assert (M.model(dem[a:b], top, bot).filled[1:-1] >= want[a:b][1:-1]).all()


def test_model_refuses_plateaus_and_nan():
    dem = _noise(70, 70, 1)
    for r, c, v in ((10, 10, dem[11, 11]), (5, 5, np.nan), (20, 20, dem[20, 21])):
        d = dem.copy()
        d[r, c] = v
        with pytest.raises(ValueError):
            M.model(d)


def test_hash_run_argument():
    """linear probing: the set of taken slots does not depend on the insertion order"""
    rng = np.random.default_rng(3)
    home = rng.integers(0, 97, 80)
    assert len({M.max_run(rng.permutation(home), 97) for _ in range(20)}) == 1
    assert M.max_run(np.array([5, 5, 5, 96, 96]), 97) == 3 and M.max_run(np.arange(97), 97) == 97


MEMBERS = dict(FI.members())


@functools.lru_cache(maxsize=None)
def modelled(name):
    dem, claims = MEMBERS[name]()
    return dem, claims, M.model(dem)


def _count(m, claims):
    i, j = claims["where"]
    c = m.counts(i, j)
    if claims["limit"] == "EMAX":
        return int(m.block_relaxations()[i, j])
    return {"NB": c["NB"], "PAIRS": c["pairs"], "SPILL": c["spill"], "LINKS": c["links"]}[claims["limit"]]


LIMIT = dict(NB=M.NBMAX, PAIRS=M.HEU, SPILL=M.SPMAX, LINKS=M.LMAX, EMAX=M.EMAX)

@pytest.mark.parametrize("name", list(MEMBERS))
def test_family_claims(name):
    dem, claims, m = modelled(name)
    assert dem.dtype == np.float32 and not M.has_ties(dem)
    assert not m.undecided()                                   # no hash anywhere that an insertion order could overflow or not
    # which seed a basin ends with must not depend on the order of the relaxations, or the counts behind the seeds are no prediction
    # for the device (the spread is not bounded by anything the model knows, so a margin around a limit does not replace this)
    # -- every member whose GPU case asserts an exact mask; the link fields are order dependent and claim `either`
    assert all(m.tiles[i][j].seeds_stable for i in range(m.ntr) for j in range(m.ntc)) == ("either" not in claims)
    assert name.startswith("links") == ("either" in claims)
    assert np.array_equal(m.filled, oracle.fill_terrain(dem))
    count, limit = _count(m, claims), LIMIT[claims["limit"]]
    print(name, claims["limit"], "count", count, "limit", limit)
    assert count == claims["count"]          # what the "at" member reaches (== the limit wherever the family can) / by how little "over" exceeds it
    firsts = {(i, j): m.tile_first_limit(i, j) for i in range(m.ntr) for j in range(m.ntc)}
    blocks_over = [tuple(b) for b in np.argwhere(m.block_relaxations() > M.EMAX).tolist()]
    if claims["member"] == "at":
        assert count <= limit and claims["mask"] == 0 and claims["algorithm"] == 1
        assert not any(firsts.values()) and not blocks_over and m.reasons() == 0
    else:
        assert claims["algorithm"] == 0 and m.reasons() == claims["mask"]
        if claims["limit"] == "EMAX":
            assert count > limit and not any(firsts.values()) and blocks_over == [claims["where"]]
        else:
            want = {"edge": "PAIRS", "over": claims["limit"]}[claims["member"]]          # (basins-edge: 1024 basins pass, the pair hash behind them gives out)
            assert count > limit or claims["member"] == "edge"
            assert firsts.pop(claims["where"]) == want and not any(firsts.values()) and not blocks_over
    # the tables a member is not aimed at: every hash at or below half load and without a run of 64 taken slots (the run length is
    # what decides whether an insertion can fail).  The basin-pair hash is the target of the pairs members, and in the basins members
    # it sits behind the 1024 basins they are about: the designated tile of those four is left out of its half-load bound
    for i in range(m.ntr):
        for j in range(m.ntc):
            t = m.tiles[i][j]
            aimed = (i, j) == claims["where"]
            if not (aimed and claims["limit"] in ("NB", "PAIRS")):
                assert t.npairs <= M.HEU // 2, (i, j, t.npairs)
            if aimed and claims["member"] != "at":
                continue
            assert t.nspill <= M.SE // 2 and m.nlinks[i][j] <= M.LH // 2
            assert t.pair_hash[0] == "safe" and t.spill_hash[0] == "safe" and m.link_hash[i][j][0] == "safe"


def test_the_mask_of_the_edge_case_suite_s_pit_field():
    """test_gpu_edgecases.py::test_priority_flood_and_its_fallback_give_the_same_fill asserts fill_overflow == 3 for its `pits`
    field: corner and edge tiles hold more than 1024 basins, the tiles inside exactly 1024 and more pairs than the hash has entries"""
    rng = np.random.default_rng(33)
    pits = (1.0 + rng.random((300, 260))).astype(np.float32)
    pits[::2, ::2] = (rng.random((150, 130)) * 0.5).astype(np.float32)
    m = M.model(pits)
    firsts = {m.tile_first_limit(i, j) for i in range(m.ntr) for j in range(m.ntc)}
    assert not m.undecided() and firsts == {"NB", "PAIRS", None} and m.reasons() == (FI.NB | FI.PAIRS) == 3


def _band_models(dem):
    from malstroem_amd.distributed import band_rows
    out = []
    for k in range(3):
        r0, n = band_rows(dem.shape[0], 3, k)
        top, bot = k > 0, k < 2
        out.append(M.model(dem[r0 - top:r0 + n + bot], top, bot))
    return out


@pytest.mark.parametrize("which", ["middle", "first", "links"])
def test_band_claims(which):
    dem, claims = FI.band_case(which)
    models = _band_models(dem)
    assert tuple(m.reasons() for m in models) == claims["masks"]          # (in the model's order of relaxations, for "links")
    assert tuple(int(m.reasons() == 0) for m in models) == claims["engines"]
    assert not any(m.halo_over for m in models)


def test_seed_capacity_is_out_of_reach():
    """NSMAX = 128 seeds per tile: the densest fields found (a pit on every other cell of the window ring) have 124; a hill-climb over
    the cells next to the ring lines (flood_search.py seeds; the run was not recorded) found no more.  See DESIGN.md 7.0b for the argument."""
    for dem in (FI.ring_pits(188, 188, None), FI.pyramid(188, 188, None)):
        assert M.model(dem).counts(1, 1)["NS"] == 124 <= M.NSMAX


def test_no_family_member_overflows_the_halo_links():
    """LMAX again, in pf_halo_links_kernel: tileNL0 + one link per seed with a ring cell on a halo row.  The bands of every 188-row
    member (three bands, seams on the tile grid), before and after the exchange: the largest sum found, far from 256."""
    worst = 0
    for name in ("spill-at", "spill-over", "pairs-at"):
        dem = MEMBERS[name]()[0]
        want = oracle.fill_terrain(dem)
        from malstroem_amd.distributed import band_rows
        for k in range(3):
            r0, n = band_rows(188, 3, k)
            top, bot = k > 0, k < 2
            loc = slice(r0 - top, r0 + n + bot)
            m = M.model(dem[loc], top, bot, want[loc][0] if top else None, want[loc][-1] if bot else None)
            assert not m.halo_over
            worst = max(worst, max(min(m.nlinks[i][j], M.LMAX) + m.nhalo[i][j] for i in range(m.ntr) for j in range(m.ntc) if m.nhalo[i][j]))
    print("largest tileNL0 + halo seeds", worst)
    assert worst <= M.LMAX
