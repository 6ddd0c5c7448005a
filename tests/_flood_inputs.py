"""Seeded DEMs that sit AT and just OVER the capacities of the tiled priority-flood (csrc/pflood.hip), in the idiom of
_inputs.py: every generator returns (dem, claims); tests/test_pflood_model.py checks every claim with the CPU model of the
flood's tables (_pflood_model.py), the GPU tests trust the claims and never run the model.

All fields are float32 without equal 8-neighbours.  The background is a tilted plane (one basin per tile, nothing near a limit),
so that only the designated tile / block comes near a capacity.  Tiles are 62 x 62 owned cells; tile (i, j) owns rows
62 i + 1 .. 62 i + 62, its window adds one ring cell all round; blocks are 4 x 4 tiles.

claims: limit (which capacity the member aims at), member ("at": nothing is exceeded anywhere, the flood runs; "edge": the count
EQUALS the limit and passes, but the field cannot avoid the next capacity behind it; "over": the limit is exceeded in `where` and
nothing in front of it, nowhere else anything), where (tile or block), count (the model's count there), algorithm / mask (what
fill_algorithm / fill_overflow must report)."""
import numpy as np

NB, PAIRS, NS, SPILL, LINKS, EMAX, HALO = 1, 2, 4, 8, 16, 32, 64      # fill_overflow bits (include/malstroem_hip.h)


def plane(h, w):
    r, c = np.mgrid[0:h, 0:w]
    return (2.0 + 0.003 * r + 0.0017 * c).astype(np.float32)


def _pits(dem, cells, top=0.5):
    """distinct pit elevations below everything else, in the order of `cells`"""
    for k, (r, c) in enumerate(cells):
        dem[r, c] = np.float32(top * (k + 1) / (len(cells) + 1))


def lattice(h, w, n, r0, c0):
    """the first n cells (row by row) of the period-2 lattice of 31 x 31 pits in the tile whose first owned cell is (r0, c0):
    every pit is a basin of its own, and neighbouring pit basins touch: ~3 basin pairs per basin"""
    dem = plane(h, w)
    rr, cc = np.mgrid[r0:r0 + 62:2, c0:c0 + 62:2]
    _pits(dem, list(zip(rr.ravel()[:n].tolist(), cc.ravel()[:n].tolist())))
    return dem


def basins(member):
    """NBMAX = 1024 basins per tile, on a one-tile raster (64 x 64: its 252 border cells are basins by decree).  No field holds
    1024 basins in fewer basin pairs than the pair hash takes (neighbouring basins touch), so there is no member with 1024 basins
    that exceeds nothing: "edge" has exactly 1024 -- the basin count passes, the pair hash behind it gives out -- and "over" 1025.
    The densest field of this kind that exceeds nothing is pairs("at")."""
    n = {"edge": 772, "over": 773}[member]
    dem = lattice(64, 64, n, 1, 1)
    return dem, dict(limit="NB", member=member, where=(0, 0), count=252 + n, algorithm=0, mask=PAIRS if member == "edge" else NB)


PAIRS_AT, PAIRS_OVER = 500, 545


def pairs(member, w=188):
    """HEU = 2032 basin-pair hash entries (and 64 probes) in the centre tile of 3 x 3.  "at": the densest lattice for which the
    model proves that no insertion order fails (no 64 taken slots in a row); "over": the first with more pairs than entries."""
    n = {"at": PAIRS_AT, "over": PAIRS_OVER}[member]
    dem = lattice(188, w, n, 63, 63)
    return dem, dict(limit="PAIRS", member=member, where=(1, 1), count={"at": 1859, "over": 2036}[member], algorithm=int(member == "at"), mask=0 if member == "at" else PAIRS)


def ring_pits(h, w, keep, seed=0):
    """white noise inside the centre tile of 3 x 3 and a pit on every other cell of its window ring (the first `keep` of 126; None:
    all): every ring pit is a seed, and the noise basins between them join ~2 seed pairs per seed.  Which seed a noise basin ends
    with depends on the order of the kernel's relaxations (_pflood_model.py: seeds_stable), so this field only serves the CPU tests"""
    rng = np.random.default_rng(seed)
    dem = plane(h, w)
    dem[63:125, 63:125] = (3.0 + rng.random((62, 62))).astype(np.float32)
    cells = ([(62, c) for c in range(62, 126, 2)] + [(125, c) for c in range(62, 126, 2)]
             + [(r, 62) for r in range(64, 125, 2)] + [(r, 125) for r in range(64, 125, 2)])[:keep]
    for k, (r, c) in enumerate(cells):
        dem[r, c] = np.float32(0.5 * (k + 1) / 300)
    return dem


def pyramid(h, w, keep, seed=0):
    """the centre tile's window as a pyramid that falls towards its ring (slope 0.01 per cell + noise of 0.004: every inner cell has
    a lower neighbour further out, so the tile has no basin the label-correcting could move), the ring itself rising monotonely
    from its first corner, and a pit on every other ring cell (the first `keep` of 126): every basin is rooted in a ring pit, its
    seed is fixed, and neighbouring catchments make ~2 spill edges per seed -- counts that no order of relaxations changes"""
    rng = np.random.default_rng(seed)
    dem = plane(h, w)
    r, c = np.mgrid[0:64, 0:64]
    dist = np.minimum(np.minimum(r, 63 - r), np.minimum(c, 63 - c))
    z = np.where(dist == 0, 1.0 + 1e-4 * (r + 1.3 * c), 1.0 + 0.01 * dist + 0.004 * rng.random((64, 64)))
    dem[62:126, 62:126] = z.astype(np.float32)
    cells = ([(62, c) for c in range(62, 126, 2)] + [(125, c) for c in range(62, 126, 2)]
             + [(r, 62) for r in range(64, 125, 2)] + [(r, 125) for r in range(64, 125, 2)])[:keep]
    for k, (r, c) in enumerate(cells):
        dem[r, c] = np.float32(0.5 * (k + 1) / 300)
    return dem


SPILL_KEEP = (96, 97)


def spill(member, w=188):
    """SPMAX = 192 spill edges (distinct seed pairs) per tile; w = 256: the raster takes the fused apply-and-proof pass"""
    dem = pyramid(188, w, SPILL_KEEP[member == "over"])
    return dem, dict(limit="SPILL", member=member, where=(1, 1), count={"at": 192, "over": 194}[member], algorithm=int(member == "at"), mask=0 if member == "at" else SPILL)


EMAX_EXTRA = {"at": 51, "over": 50}
EMAX_AT_PIT = (434, 464)


def relaxations(member):
    """EMAX = 6144 directed relaxations (links + 2 x spill edges) in block (1, 1) of a 498 x 498 raster (8 x 8 tiles), every tile of
    the block inside its own capacities.  The block is a pyramid per tile (as in `pyramid`: no inner basin) between seams of two
    ring lines: line 62 m is the first ring line of tile m and carries a pit on every other cell; line 62 m + 1 is the last ring
    line of tile m - 1 and carries, next to every pit, a cell between the pit and the ring's level: to tile m - 1 the pit is an
    inner basin whose own outlet -- that cell -- lies below every pass to its neighbours, so its seed is its own whatever the order
    of the relaxations.  Five pits of every seven are kept (~185 spill edges per inner tile instead of ~250), then the first
    `EMAX_EXTRA` of them are left out: one pit less is 5 to 7 relaxations less, which reaches 6140 and 6147 ("over").  "at" adds
    one pit without an outlet cell to the 6140 field, at `EMAX_AT_PIT` (worth 4 there): 6144 exactly."""
    n, lo = 498, 248
    rng = np.random.default_rng(9)
    x = np.arange(n)
    d1 = np.min(np.stack([np.minimum(np.abs(x - 62 * m), np.abs(x - 62 * m - 1)) for m in range(9)]), 0)      # distance to the nearest seam
    dist = np.minimum(d1[:, None], d1[None, :])
    r, c = np.mgrid[0:n, 0:n]
    z = np.where(dist == 0, 1.0 + 1e-5 * (r + 1.3 * c), 1.0 + 0.01 * dist + 0.004 * rng.random((n, n)))
    dem = np.where((r > lo) & (c > lo) & (r < n - 1) & (c < n - 1), z, plane(n, n)).astype(np.float32)
    cells = []
    for m in range(4, 8):
        for y in range(lo + 2, n - 2, 2):
            cells += [(62 * m, y, 0), (y, 62 * m, 1)]
    cells = sorted(set(cells))
    kept, taken = [], set()
    for rr, cc, o in cells:     # (no two pits next to each other, where the seams cross)
        if any((rr + a, cc + b) in taken for a in (-1, 0, 1) for b in (-1, 0, 1)):
            continue
        taken.add((rr, cc))
        kept.append((rr, cc, o))
    live = [(k, p) for k, p in enumerate(kept) if ((p[0] + p[1]) // 2) % 7 >= 2][EMAX_EXTRA[member]:]
    for k, (rr, cc, o) in live:
        dem[rr, cc] = np.float32(0.5 * (k + 1) / len(cells))
        mr, mc = (rr + 1, cc) if o == 0 else (rr, cc + 1)
        if (mr, mc) not in taken:
            dem[mr, mc] = np.float32(0.9 + 0.05 * (k + 1) / len(cells))
    if member == "at":
        dem[EMAX_AT_PIT] = np.float32(0.7)
    return dem, dict(limit="EMAX", member=member, where=(1, 1), count={"at": 6144, "over": 6147}[member], algorithm=int(member == "at"), mask=0 if member == "at" else EMAX)


def links(member):
    """LMAX = 256 links per tile (distinct (own seed, direction, neighbour's seed) over the tile's ring cells and the neighbours' ring
    cells it owns).  No regular pattern came near (a pit on every other ring cell: 132): the two fields are the first with 256 and
    with 257 links (in the model's order of relaxations) that a seeded hill-climb found -- random new elevations for a few of the
    cells within two of the centre tile's ring lines per step, from pyramid(188, 188, 90), every other capacity of every tile
    respected.  They show that the limit can be reached, but they hold basins whose seed depends on the order of the relaxations
    (_pflood_model.py: seeds_stable; three probe orders did not show it, twelve do -- and fields from the same climb under sixteen
    probe orders failed under 150: the climb learns the probe), so the device's count may differ by a few and may fall on either
    side of the limit.  The searches that found them were not recorded; the fields are kept as data (tests/golden/flood_links.npz)
    and tests/flood_search.py repeats the kind of search, not its bits.  claims: `either` -- a GPU case asserts the oracle's bits
    and that (fill_algorithm, fill_overflow) is (1, 0) or (0, LINKS), nothing else; the CPU test checks the model's own count."""
    from pathlib import Path
    dem = np.load(Path(__file__).resolve().parent / "golden" / "flood_links.npz")[member]
    return dem, dict(limit="LINKS", member=member, where=(1, 1), count={"at": 256, "over": 257}[member], algorithm=int(member == "at"), mask=0 if member == "at" else LINKS,
                     either=((1, 0), (0, LINKS)))


def band_case(which):
    """188 rows = three bands of one tile row each (seams on the tile grid).  "middle": spill("over") -- the centre tile belongs to
    the middle band; "first": 1025+ basins in tile (0, 1), the first band's; "links": links("over"), whose seeds depend on the order
    of the relaxations.  claims: engines per band, mask per band (`middle_either`: what else the middle band may report)."""
    if which == "middle":
        dem, _ = spill("over")
        return dem, dict(engines=(1, 0, 1), masks=(0, SPILL, 0))
    if which == "links":      # the link field's centre tile in the middle band: its halo sides carry no links there, so no band comes near LMAX
        dem, _ = links("over")
        return dem, dict(engines=(1, 1, 1), masks=(0, 0, 0), middle_either=((1, 0), (0, SPILL), (0, LINKS)))      # (184 spill edges in the model's order)
    dem = lattice(188, 188, 961, 1, 63)
    return dem, dict(engines=(0, 1, 1), masks=(NB, 0, 0))


def members():
    """every (name, generator call) of the one-context GPU cases"""
    out = [("basins-edge", lambda: basins("edge")), ("basins-over", lambda: basins("over"))]
    for name, fn in (("pairs", pairs), ("spill", spill), ("links", links), ("relaxations", relaxations)):
        for member in ("at", "over"):
            out.append(("%s-%s" % (name, member), lambda fn=fn, member=member: fn(member)))
    for member in ("at", "over"):
        out.append(("spill-%s-w256" % member, lambda member=member: spill(member, 256)))
    return out
