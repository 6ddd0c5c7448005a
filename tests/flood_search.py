"""A seeded hill-climb over the cells next to the centre tile's ring lines of a 188 x 188 field, scored with the CPU model of the
flood's tables (_pflood_model.py).  This is the KIND of search behind tests/golden/flood_links.npz (objective "links"), behind
"no field with more than 124 seeds" (objective "seeds") and behind "no halo-link overflow" (objective "halo": the middle band's
tileNL0 + halo seeds); the runs that produced those fixtures and figures were not recorded, so this tool repeats the search, not
its bits.  Not a test.

    python tests/flood_search.py links|seeds|halo [steps] [seed]

A step gives one to four of those cells a random new elevation and is kept when the score does not drop; every exceeded
capacity other than the objective's, every undecided hash and every tile whose seeds depend on the order of the relaxations
(under the model's probe orders -- which a long climb learns to satisfy without being order independent) costs points."""
import sys

import numpy as np

import _flood_inputs as FI
import _pflood_model as M

LINES = (62, 63, 124, 125)
CELLS = [(r, c) for r in range(58, 130) for c in range(58, 130) if min(min(abs(r - x), abs(c - x)) for x in LINES) <= 2]


def score(dem, what):
    m = M.model(dem[62:126], True, True) if what == "halo" else M.model(dem)
    ci = 0 if what == "halo" else 1
    pen = 0
    for i in range(m.ntr):
        for j in range(m.ntc):
            t = m.tiles[i][j]
            pen += max(0, t.NB - M.NBMAX) + max(0, t.nspill - M.SPMAX) + 15 * (not t.seeds_stable)
            pen += 50 * sum(h[0] != "safe" for h in (t.pair_hash, t.spill_hash, m.link_hash[i][j]))
            if what != "seeds":
                pen += max(0, t.NS - M.NSMAX)
            if what != "links" or (i, j) != (ci, 1):
                pen += max(0, m.nlinks[i][j] - M.LMAX)
    c = m.counts(ci, 1)
    value = {"links": c["links"], "seeds": c["NS"], "halo": min(c["links"], M.LMAX) + c["halo"]}[what]
    return value - 3 * pen, value, pen == 0


def climb(what, steps, seed):
    rng = np.random.default_rng(seed)
    dem = FI.pyramid(188, 188, 90) if what != "seeds" else FI.ring_pits(188, 188, None)
    best, value, clean = score(dem, what)
    for step in range(steps):
        d = dem.copy()
        for _ in range(int(rng.integers(1, 5))):
            r, c = CELLS[int(rng.integers(len(CELLS)))]
            d[r, c] = np.float32(rng.random() * 2)
        if M.has_ties(d):
            continue
        s, v, ok = score(d, what)
        if s >= best:
            if s > best:
                print(step, what, v, "every other capacity respected" if ok else "penalised", flush=True)
            best, value, clean, dem = s, v, ok, d
    return dem, value, clean


if __name__ == "__main__":
    what = sys.argv[1]
    dem, value, clean = climb(what, int(sys.argv[2]) if len(sys.argv) > 2 else 3000, int(sys.argv[3]) if len(sys.argv) > 3 else 1)
    print("final", what, value, clean)
    np.save("flood_search_%s.npy" % what, dem)
