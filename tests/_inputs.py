"""Seeded input generators for the standalone algorithms API: inputs the chain never produces (flow cycles, inward edges, codes
above 8, labels that are no connected components, signed zeros, infinities, NaN).  Everything is NumPy and vectorised; every
generator returns its arrays together with the properties it claims, and tests/test_inputs_cpu.py checks those claims against
the oracle, so the GPU tests know what they exercise.

Tile sizes the generators aim at: accumulation / watershed / labelling tiles of 64 x 64 cells (accum.hip, watershed.hip,
ccl.hip); label_stats / label_count / the packed arg-max keep an LDS table per tile of 32 rows x 256 columns (label_ops.hip:
512, 2048 and 1024 slots), and a flat raster (the standalone label_stats / label_count) is cut as if it were 256 columns wide.
"""
import numpy as np

AT = 64                                   # accumulation / watershed / CCL tile edge
TR, TW = 32, 256                          # rows x columns of a label_ops tile
TABLE_SLOTS = {"stats": 512, "argmax": 1024, "count": 2048}
NODIR = 8
DR = np.array([-1, -1, 0, 1, 1, 1, 0, -1])          # AGNPS codes 0..7: up, up-right, right, ... (reference flow.py:30-38)
DC = np.array([0, 1, 1, 1, 0, -1, -1, -1])


def code_of(dr, dc):
    """AGNPS code of the step (dr, dc)."""
    for k in range(8):
        if DR[k] == dr and DC[k] == dc:
            return k
    raise ValueError((dr, dc))


# ---- flow fields ------------------------------------------------------------------------------------------------------

def _tile_path(end):
    """Codes of one 64 x 64 tile covered by a single path; -> (codes, position of every cell along the path 1..4096).
    leave: serpentine along the rows from (0, 0) to (63, 0), whose last cell flows down out of the tile;
    sink: clockwise spiral from (0, 0) inwards, its 4096th cell an interior NODIR sink;
    cycle: rows 1..63 of the serpentine over columns 1..63, back up column 0: one 4096-cell cycle."""
    fd = np.empty((AT, AT), np.uint8)
    pos = np.zeros((AT, AT), np.int64)
    if end == "leave":
        order = [(r, c) for r in range(AT) for c in (range(AT) if r % 2 == 0 else range(AT - 1, -1, -1))]
        last = (1, 0)
    elif end == "sink":
        order, seen = [], np.zeros((AT, AT), bool)
        r, c, d = 0, 0, 0
        steps = ((0, 1), (1, 0), (0, -1), (-1, 0))
        for _ in range(AT * AT):
            order.append((r, c))
            seen[r, c] = True
            nr, nc = r + steps[d][0], c + steps[d][1]
            if not (0 <= nr < AT and 0 <= nc < AT) or seen[nr, nc]:
                d = (d + 1) % 4
                nr, nc = r + steps[d][0], c + steps[d][1]
            r, c = nr, nc
        last = None
    elif end == "cycle":
        order = [(0, 0)] + [(r, c) for r in range(AT) for c in (range(1, AT) if r % 2 == 0 else range(AT - 1, 0, -1))]
        order += [(r, 0) for r in range(AT - 1, 0, -1)]
        last = order[0]
        last = (last[0] - order[-1][0], last[1] - order[-1][1])
    else:
        raise ValueError(end)
    for k, (r, c) in enumerate(order):
        pos[r, c] = k + 1
        if k + 1 < len(order):
            fd[r, c] = code_of(order[k + 1][0] - r, order[k + 1][1] - c)
    r, c = order[-1]
    fd[r, c] = NODIR if last is None else code_of(*last)
    return fd, pos


def tile_hamiltonian(h, w, end):
    """Every full 64 x 64 tile covered by one path (see _tile_path); cells outside the full tiles flow straight down.
    With end="leave" the tiles of a tile column form one river: the path of tile (tr, tc) continues in the tile below.
    Claims: `pos` (1..4096 along the path, 0 outside the full tiles), `ntr` x `ntc` full tiles, `end`, and `acc`, the
    accumulated flow the claims imply (0 on cycles)."""
    fd = np.full((h, w), 4, np.uint8)
    ntr, ntc = h // AT, w // AT
    tile, pos = _tile_path(end)
    P = np.zeros((h, w), np.int64)
    fd[:ntr * AT, :ntc * AT] = np.tile(tile, (ntr, ntc))
    P[:ntr * AT, :ntc * AT] = np.tile(pos, (ntr, ntc))
    acc = np.zeros((h, w), np.float64)
    if end == "leave":
        acc[:ntr * AT, :ntc * AT] = P[:ntr * AT, :ntc * AT] + (np.arange(ntr * AT) // AT * AT * AT)[:, None]
    elif end == "sink":
        acc[:ntr * AT, :ntc * AT] = P[:ntr * AT, :ntc * AT]
    # cells outside the full tiles flow straight down; below a tile column the river of end="leave" arrives at its top
    acc[:, ntc * AT:] = (np.arange(h) + 1.0)[:, None]
    col_in = np.zeros(ntc * AT, np.float64)
    if end == "leave" and ntr:
        col_in[::AT] = ntr * AT * AT
    acc[ntr * AT:, :ntc * AT] = (np.arange(h - ntr * AT) + 1.0)[:, None] + col_in[None, :]
    return fd, dict(pos=P, ntr=ntr, ntc=ntc, end=end, acc=acc)


def _descend(pot, rng):
    """A random neighbour of strictly lower potential for every cell (vectorised), NODIR where there is none."""
    h, w = pot.shape
    pad = np.pad(pot, 1, constant_values=np.inf)
    best = np.full((h, w), -1.0)
    fd = np.full((h, w), NODIR, np.uint8)
    for k in range(8):
        nb = pad[1 + DR[k]:1 + DR[k] + h, 1 + DC[k]:1 + DC[k] + w]
        score = np.where(nb < pot, rng.random((h, w)), -1.0)
        take = score > best
        fd[take] = k
        best = np.maximum(best, score)
    return fd


def random_forest(h, w, seed, sink_frac=0.0):
    """Acyclic by construction: every cell steps to a random neighbour of strictly lower potential, so no path can close.  The
    potential winds through lanes of 24 rows (a lane falls to the right, the next one to the left, each lane lower than the one
    below it) plus unique noise below one step: paths meander up and down inside a lane, run along it over many tiles and
    climb into the lane above.  Cells without a lower neighbour and a `sink_frac` of random cells are NODIR sinks.
    Claims: `acyclic` (every cell's accumulation >= 1), `sinks` (NODIR mask)."""
    rng = np.random.default_rng(seed)
    lane = (np.arange(h) // 24)[:, None]
    c = np.arange(w)[None, :]
    pot = lane * (w + 10.0) + np.where(lane % 2 == 1, c, w - 1 - c)
    pot = pot + rng.permutation(h * w).reshape(h, w) * (0.9 / max(h * w, 1))
    fd = _descend(pot, rng)
    if sink_frac:
        fd[rng.random((h, w)) < sink_frac] = NODIR
    return fd, dict(acyclic=True, sinks=fd == NODIR)


def _ring(r0, c0, r1, c1):
    """Cells and codes of the clockwise ring on the outline of the rectangle [r0, r1] x [c0, c1]."""
    cells = ([(r0, c, 2) for c in range(c0, c1)] + [(r, c1, 4) for r in range(r0, r1)]
             + [(r1, c, 6) for c in range(c1, c0, -1)] + [(r, c0, 0) for r in range(r1, r0, -1)])
    return cells


def tile_crossing_cycles(h, w, seed):
    """Flow cycles laid over tile outlines (h, w >= 260): 2-cycles straddling a tile edge (across rows, columns and a corner),
    rings around tile corners, a ring along a tile edge and a ring spanning 3 x 3 tiles; the rest is a random forest whose
    trees drain into the cycles from several tiles (a funnel of strictly decreasing potential around every cycle).
    Claims: `cycle` (mask of the constructed cycle cells; nothing else lies on a cycle, no cycle touches the raster's edge)."""
    assert h >= 260 and w >= 260, (h, w)
    rng = np.random.default_rng(seed)
    cycles = []
    cycles.append([(AT - 1, 10, 4), (AT, 10, 0)])                         # across a row edge
    cycles.append([(30, AT - 1, 2), (30, AT, 6)])                         # across a column edge
    cycles.append([(2 * AT - 1, 3 * AT - 1, 3), (2 * AT, 3 * AT, 7)])     # across a corner, diagonally
    cycles.append(_ring(AT - 1, AT - 1, AT, AT))                           # the 2 x 2 ring around a corner
    cycles.append(_ring(2 * AT - 3, 2 * AT - 3, 2 * AT + 2, 2 * AT + 2))   # a 6 x 6 ring around a corner
    cycles.append(_ring(AT - 1, 2 * AT + 5, AT, w - 5))                    # two rows along a tile edge, over several tiles
    cycles.append(_ring(AT + 38, AT + 3, 3 * AT + 40, 3 * AT + 40))      # over 3 x 3 tiles
    fd = np.full((h, w), NODIR, np.uint8)
    cyc = np.zeros((h, w), bool)
    for cells in cycles:
        rows, cols, codes = (np.array(x) for x in zip(*cells))
        assert not cyc[rows, cols].any()
        cyc[rows, cols] = True
        fd[rows, cols] = codes
    # funnel: within 24 cells of a cycle the potential falls towards it, elsewhere a random forest's potential
    from scipy.ndimage import distance_transform_cdt
    dist = distance_transform_cdt(~cyc, metric="chessboard").astype(np.float64)
    pot = rng.random((h, w)) * 0.5 + np.where(dist <= 24, dist - 100.0, 0.0)
    pot = np.where(dist <= 24, pot, 1.0 + rng.random((h, w)) + np.add.outer(np.arange(h), np.arange(w)) * -0.01)
    pot[cyc] = -1000.0
    free = _descend(pot, rng)
    fd[~cyc] = free[~cyc]
    return fd, dict(cycle=cyc)


def edge_variants(fd, seed=0):
    """The same field four ways: border cells flowing off the raster ("outward"), NODIR ("nodir"), pointing inwards or along
    the border ("inward": a border cell that would then lie on a flow cycle is NODIR, the reference's watersheds never return
    from such a cycle), and "codes" with 3 % of the cells replaced by codes 9..255 (never flow, but are not NODIR either).
    Claims per variant: `border_codes` (what the border holds)."""
    from malstroem_amd.algorithms.flow import set_edges_flow_outward
    rng = np.random.default_rng(seed)
    h, w = fd.shape
    border = np.zeros((h, w), bool)
    border[0, :] = border[-1, :] = True
    border[:, 0] = border[:, -1] = True
    out = {}
    a = fd.copy()
    set_edges_flow_outward(a)
    out["outward"] = a
    b = fd.copy()
    b[border] = NODIR
    out["nodir"] = b
    c = fd.copy()
    rr, cc = np.nonzero(border)
    choice = np.full(rr.size, NODIR, np.uint8)
    best = np.full(rr.size, -1.0)
    for k in range(8):
        nr, nc = rr + DR[k], cc + DC[k]
        inside = (nr >= 0) & (nr < h) & (nc >= 0) & (nc < w)
        score = np.where(inside, rng.random(rr.size), -1.0)
        choice[score > best] = k
        best = np.maximum(best, score)
    c[rr, cc] = choice
    import oracle
    on_cycle = border & (oracle.accumulated_flow(c) == 0)
    c[on_cycle] = NODIR
    out["inward"] = c
    d = fd.copy()
    sprinkle = rng.random((h, w)) < 0.03
    d[sprinkle] = rng.integers(9, 256, int(sprinkle.sum()))
    out["codes"] = d
    return out, dict(border=border)


def spiral_mask(h, w):
    """A one-cell-wide rectangular spiral, one 8-connected component that crosses tile outlines hundreds of times."""
    m = np.zeros((h, w), bool)
    o = 0
    while h - 1 - 2 * o > o + 2 and w - 1 - 2 * o > o + 2:
        r0, c0, r1, c1 = o, o, h - 1 - o, w - 1 - o
        m[r0, c0:c1 + 1] = True
        m[r0:r1 + 1, c1] = True
        m[r1, c0:c1 + 1] = True
        m[r0 + 2:r1 + 1, c0] = True           # the gap at (r0 + 1, c0) opens the ring ...
        m[r0 + 2, c0 + 1] = True              # ... and this cell joins it to the next one inside
        o += 2
    return m


# ---- label rasters ----------------------------------------------------------------------------------------------------

def _tile_distinct(lab, rows, cols):
    """Distinct labels (background included) of every rows x cols tile of `lab` -> 2D array."""
    h, w = lab.shape
    out = np.zeros((-(-h // rows), -(-w // cols)), np.int64)
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            out[i, j] = np.unique(lab[i * rows:(i + 1) * rows, j * cols:(j + 1) * cols]).size
    return out


def tile_label_counts(lab):
    """Distinct labels per 32 x 256 tile of the 2D raster and per 8192-cell tile of the flat raster (the standalone
    label_stats / label_count view it as 256 columns wide) -> (2D counts, flat counts)."""
    flat = lab.ravel()
    pad = (-flat.size) % (TR * TW)
    flat = np.concatenate([flat, np.full(pad, flat[-1], flat.dtype)]).reshape(-1, TW)
    return _tile_distinct(lab, TR, TW), _tile_distinct(flat, TR, TW)


def label_rasters(h, w, seed):
    """int32 label rasters that are no connected components (h >= 256, w >= 256):
    "tables": 64-row bands drawing from 700, 1400 and 4000 sparse ids (more distinct labels per 32 x 256 tile than the stats,
    arg-max and count tables hold), the rest of the raster one label;
    "rects": random rectangles of sparse ids (up to 300 wide) over every tile edge on a background of 0;
    "dominant": one label over most of the raster, a scatter of others and of 0.
    Claims: `bands` (row slices of the three dense bands) and `nlabels`, max label of every raster."""
    assert h >= 256 and w >= 256, (h, w)
    rng = np.random.default_rng(seed)
    out = {}
    t = np.full((h, w), 3, np.int32)
    bands = {}
    for k, (name, pool) in enumerate((("stats", 700), ("argmax", 1400), ("count", 4000))):
        ids = rng.choice(np.arange(4, 60_000, dtype=np.int32), pool, replace=False)
        rows = slice(64 * k, 64 * k + 64)
        t[rows] = ids[rng.integers(0, pool, (64, w))]
        bands[name] = rows
    out["tables"] = t
    r = np.zeros((h, w), np.int32)
    for _ in range(300):
        hh, ww = int(rng.integers(1, 80)), int(rng.integers(1, 300))
        r0, c0 = int(rng.integers(-hh + 1, h)), int(rng.integers(-ww + 1, w))
        r[max(r0, 0):r0 + hh, max(c0, 0):c0 + ww] = 7 * int(rng.integers(1, 5000)) + 1
    out["rects"] = r
    d = np.full((h, w), 2, np.int32)
    s = rng.random((h, w))
    d[s < 0.05] = 0
    d[s > 0.97] = rng.integers(3, 60, int((s > 0.97).sum()))
    out["dominant"] = d
    return out, dict(bands=bands, nlabels={k: int(v.max()) for k, v in out.items()})


# ---- values -----------------------------------------------------------------------------------------------------------

SUBNORMAL32 = np.float32(1e-41)
SUBNORMAL64 = 5e-320


def label_values(lab, seed, dtype):
    """Per-cell values for the per-label reductions.  "zeros": only +0.0 and -0.0 (every label's min and max is a zero whose
    sign the label's first cell decides); "mixed": exact ties, both zeros, +-inf; "subnormal": subnormals and both zeros;
    "nan": like mixed but NaN in the cells of one label only.  Claims: `nan_label`."""
    rng = np.random.default_rng(seed)
    shape = lab.shape
    sub = SUBNORMAL32 if dtype == np.float32 else SUBNORMAL64
    zeros = np.where(rng.random(shape) < 0.5, -0.0, 0.0).astype(dtype)
    pool = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.5, 2.0, np.inf, -np.inf, 3.0, -3.0], dtype)
    mixed = pool[rng.integers(0, pool.size, shape)]
    # subnormals on their own: a sum that mixes them with 1.0 rounds in an order dependent way, which the label_stats sum
    # rule (_cases.assert_label_sums) does not cover; among themselves every partial sum is exact
    tiny = np.array([0.0, -0.0, sub, -sub, 2 * sub, -3 * sub], dtype)[rng.integers(0, 6, shape)]
    labels = np.unique(lab)
    nan_label = int(labels[len(labels) // 2])
    nan = mixed.copy()
    sel = (lab == nan_label) & (rng.random(shape) < 0.3)
    nan[sel] = np.nan
    return dict(zeros=zeros, mixed=mixed, subnormal=tiny, nan=nan), dict(nan_label=nan_label)


def packed_argmax_values(lab, seed):
    """float64 integer values for label_max_index: "fast" holds only 0 and 2**32 - 1, the two ends of what the packed one-pass
    arg-max takes (0 <= v < 2**32, integral); "signed-zeros" turns its zeros into +-0.0; every other variant adds ONE cell the
    packed key cannot hold (2**32, -1, 0.5, NaN), which sends the whole raster to the two-pass kernels."""
    rng = np.random.default_rng(seed)
    base = np.where(rng.random(lab.shape) < 0.3, float(2 ** 32 - 1), 0.0)
    out = {"fast": base}
    h, w = lab.shape
    for name, v in (("2^32", float(2 ** 32)), ("-1", -1.0), ("0.5", 0.5), ("nan", np.nan)):
        d = base.copy()
        d[h // 2, w // 3] = v
        out[name] = d
    d = base.copy()
    d[d == 0.0] = np.where(rng.random(int((d == 0.0).sum())) < 0.5, -0.0, 0.0)
    out["signed-zeros"] = d
    return out


# ---- D8 surfaces ------------------------------------------------------------------------------------------------------

def d8_surfaces(h, w, seed):
    """float64 surfaces for terrain_flowdirection: "ints" (small integers: many equal drops), "muldiv" (the 3 x 3 surface of
    _cases.d8_mul_vs_div_case scaled by powers of two and stamped over a random integer surface: the diagonal drop times
    1/sqrt(2) equals the straight one), "special" (+-inf, NaN, -0.0 and magnitudes near 1e308 whose drops overflow)."""
    from _cases import d8_mul_vs_div_case
    rng = np.random.default_rng(seed)
    out = {}
    out["ints"] = rng.integers(0, 4, (h, w)).astype(np.float64)
    m = rng.integers(-3, 3, (h, w)).astype(np.float64) * 1024.0
    case = d8_mul_vs_div_case()[0]
    for _ in range(max(1, h * w // 40)):
        r, c = int(rng.integers(0, max(h - 2, 1))), int(rng.integers(0, max(w - 2, 1)))
        blk = case[:min(3, h - r), :min(3, w - c)] * 2.0 ** int(rng.integers(-4, 5))
        m[r:r + blk.shape[0], c:c + blk.shape[1]] = blk
    out["muldiv"] = m
    s = rng.standard_normal((h, w)) * 10
    pick = rng.random((h, w))
    s[pick < 0.04] = np.inf
    s[(pick >= 0.04) & (pick < 0.08)] = -np.inf
    s[(pick >= 0.08) & (pick < 0.12)] = np.nan
    s[(pick >= 0.12) & (pick < 0.2)] = -0.0
    s[(pick >= 0.2) & (pick < 0.26)] = 0.0
    s[(pick >= 0.26) & (pick < 0.33)] = 1.7e308
    s[(pick >= 0.33) & (pick < 0.4)] = -1.7e308
    out["special"] = s
    return out
