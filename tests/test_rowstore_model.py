"""CPU: the two ways a visit of the geodesic transform can know which rows it moved (tools/lab/rowstore_model.py; the kernel's
version: csrc/noflat_geo.hip, block_rows).

Scheme A: one change accumulator per six-row block in the first half of a cycle (lane = column), the ballot of the second half's one
accumulator (lane = row).  Scheme B: a bit per row and lane in the first half, OR-reduced over the lanes.  On random terraced windows
-- one, two and three or more classes, with and without walls, seeded and unseeded, one flat over the whole window -- after one cycle
and after several:
  * every cell whose final value differs from the loaded one lies in a flagged row (or a skipped store loses it),
  * scheme B flags exactly the rows that changed,
  * scheme A flags only rows of a block that holds a changed row.
The model's round schedule on a small terraced DEM has to end at the chamfer distances a plain Dijkstra finds."""
import heapq
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools" / "lab"))
import rowstore_model as rm      # noqa: E402

KINDS = {"one_class": dict(classes=1), "two_classes": dict(classes=2), "four_classes": dict(classes=4),
         "no_walls": dict(classes=1, walls=False), "unseeded": dict(classes=2, seeds=False), "open": dict(classes=1, open_window=True)}


@pytest.mark.parametrize("maxcyc", (1, 4))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_flags_cover_what_moved(kind, maxcyc):
    rng = np.random.default_rng(sorted(KINDS).index(kind) * 10 + maxcyc)
    d, F, mov, S, G = rm.random_windows(60, rng, **KINDS[kind])
    loaded = d.copy()
    rows_a, rows_b, _ = rm.visit(d, F, mov, S, G, maxcyc)
    diff = d != loaded
    assert diff.any() and (d <= loaded).all()                      # something moved, and only downwards
    assert not diff[~mov].any()                                    # ring, walls and sources stay
    exact = rm.mask_of_rows(diff.any(axis=2))
    assert (exact & ~np.uint64(((1 << rm.TI) - 1) << 1) == 0).all()
    for flags in (rows_a, rows_b):
        assert ((flags & exact) == exact).all()
    assert (rows_b == exact).all()
    assert ((rows_a & ~rm.blocks_of(exact)) == 0).all()
    assert rm.popcount(rows_a) >= rm.popcount(rows_b)


def test_blocks_are_the_kernels():
    assert [rm.acc_of(r) for r in (1, 2, 7, 8, 55, 56, 61, 62)] == [0, 1, 1, 2, 9, 10, 10, 11]
    both = np.uint64(0)
    for b, m in enumerate(rm.BLOCK_ROWS):
        rows = [r for r in range(64) if (int(m) >> r) & 1]
        assert rows and all(rm.acc_of(r) == b for r in rows)
        assert int(both) & int(m) == 0
        both |= m
    assert int(both) == ((1 << rm.TI) - 1) << 1


def _dijkstra(F, flat, S, G):
    h, w = F.shape
    d = np.where(flat, rm.INF, 0).astype(np.int64)
    heap = [(0, r, c) for r, c in zip(*np.nonzero(~flat))]
    heapq.heapify(heap)
    while heap:
        v, r, c = heapq.heappop(heap)
        if v > d[r, c]:
            continue
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                rr, cc = r + dr, c + dc
                if (dr or dc) and 0 <= rr < h and 0 <= cc < w and flat[rr, cc] and F[rr, cc] == F[r, c]:
                    nv = v + int(S[rr, cc] if dr == 0 or dc == 0 else G[rr, cc])
                    if nv < d[rr, cc]:
                        d[rr, cc] = nv
                        heapq.heappush(heap, (nv, rr, cc))
    return d


def test_round_schedule_reaches_the_chamfer_distances():
    dem = rm.terraced(150, seed=5)
    lines = []
    total, d = rm.rounds(dem, maxcyc=1, report=lines.append)
    F = rm.plain_fill(dem)
    flat, S, G = rm.classify(F)
    assert flat.sum() > 2000 and total["rounds"] >= 3
    assert np.array_equal(d, _dijkstra(F, flat, S, G))
    assert total["exact"] == total["b"] <= total["a"] <= total["now"] and total["exact"] < total["now"]
