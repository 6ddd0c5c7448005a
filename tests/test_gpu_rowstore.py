"""GPU: the rounds of the integer geodesic transform store only the rows a visit changed (csrc/noflat_geo.hip,
MHIP_NG_ROWSTORE = 0 | 1 | 2).

A later visit of a tile used to store all 62 rows of distances once any cell had moved.  It now keeps a wave-uniform mask of the rows
that moved -- exact in the transposed half of a cycle (lane = row), by six-row blocks in the first half (lane = column) -- and stores
those rows only (knob 1; knob 2 keeps a bit per lane and row in the first half and stores exactly the rows that moved).  Memory after the visit has to be what it was before the change, byte for byte, so nothing downstream may differ:
every case runs `fill, noflat, flowdir` and the whole chain with the knob at 0 (every row), 1 and 2 and compares NOFLAT, FLOWDIR,
ACCUM and WATERSHEDS bit for bit.  `noflat_algorithm` has to be the transform in every run -- a fall-back to the float64 relaxation
would hide a wrong store -- and `noflat_rows_stored` tells that rows were in fact left out where the case is built for that.

The surfaces are the smallest that reach each path of a visit: one window whose later visits move the lower corridors only, the
ragged last window on both axes (`r < last_row`), level channels one cell wide that move one row (transposed half only) or one column
(first half only) across tile seams, a lake that is reached late, terraces over several powers of two (windows of two and of three or
more classes), a lake over 3 x 3 tiles (a tile that is one flat) and a level at elevation 0 (irregular: transform + relaxation)."""
import numpy as np
import pytest

from _cases import assert_same_bits, fbm
from test_gpu_label_start import ALL
from test_gpu_wetbits import _terraced

pytestmark = pytest.mark.gpu

KNOBS = (0, 1, 2)
REPORTED = {0: 0, 1: 1, 2: 2}      # noflat_rowstore: what the last request's rounds ran with


def _plateau():
    """64 x 64, one window: a plateau at 5 inside a rim at 10, barriers at 10 every tenth row that leave a gap of eight cells at
    alternating ends, one outlet in the rim next to the first corridor.  A cycle (down, up, right, left) carries the distances about
    two corridors further and settles the ones behind: with one cycle per visit (MHIP_NG_BATCH=1 makes every round its own batch,
    the tile re-queues itself) the second visit already leaves rows 1 .. 9 -- row 1 and the block of rows 2 .. 7 -- alone."""
    dem = np.full((64, 64), 10.0, np.float32)
    dem[1:-1, 1:-1] = 5.0
    for k, r in enumerate(range(10, 61, 10)):
        dem[r, 1:-1] = 10.0
        if k % 2 == 0:
            dem[r, 55:63] = 5.0
        else:
            dem[r, 1:9] = 5.0
    dem[5, 0] = 1.0
    return dem


def _ramp(h, w):
    """no two neighbours on one level: no flat, no lake"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (100.0 - 0.25 * xx - 0.001 * yy).astype(np.float32)


def _channels():
    """190 x 190 (3 x 4 tiles) on a ramp that falls to the right: trenches one cell wide that the fill turns into level channels.
    Row 30, columns 5 .. 185, spills at its right end: the distances run left along ONE row, across the seams at columns 62 | 63 | 64
    and 124 | 125 | 126, and only the left pass of the transposed half moves them -- the visit of a tile they enter stores one row.
    Column 100, rows 60 .. 185, spills at its bottom: the distances run up one column, across the seams at the same rows, in the first
    half only, and every row of the tile changes.  The lake (rows 130 .. 180, columns 20 .. 80) spills at its right rim: the tile left
    of the seam is visited before the distances reach it and again when they do."""
    dem = _ramp(190, 190)
    dem[30, 5:186] = 10.0
    dem[60:186, 100] = 10.0
    dem[130:181, 20:81] -= np.float32(40.0)
    return dem


def _powers():
    """200 x 200 terraces (natural flats: every terrace drains over its edge) whose levels grow geometrically and start over every few
    steps: by 4 % a step from 20 to 36 left of column 100 -- a window there holds one or two classes -- and by 30 % a step from 12 to
    75 right of it: four classes in every window.  (The range stays within the binades whose step weights fit 28 bits.)  Two lakes put
    flats across the zones."""
    yy, xx = np.mgrid[0:200, 0:200]
    k = (yy * 3 + xx * 2) // 25
    dem = np.where(xx < 100, 20.0 * 1.04 ** (k % 16), 12.0 * 1.3 ** (k % 8)).astype(np.float32)
    dem[40:90, 30:80] *= np.float32(0.5)
    dem[120:170, 90:150] *= np.float32(0.5)
    return np.ascontiguousarray(dem)


def _lake192():
    dem = fbm(192, 192, beta=2.0, seed=33) * np.float32(0.01) + np.float32(10.0)
    dem[20:172, 20:172] -= np.float32(5.0)
    return np.ascontiguousarray(dem)


def _level_zero():
    """a flat at elevation 0 has no constant ulp above it: its cells are left to the float64 relaxation (noflat_algorithm 3), the
    rounds run on all other levels as ever"""
    dem = fbm(131, 190, beta=2.0, seed=13)
    dem[40:80, :150] = 0.0
    return dem


# name -> (surface, MHIP_NG_BATCH or None, noflat_algorithm, rows stored with tracking strictly below those without)
CASES = {
    "plateau64": (_plateau, 1, 2, True),
    "terraced188x250": (lambda: _terraced(188, 250), None, 2, False),      # H = 62 * 3 + 2
    "channels190": (_channels, 1, 2, True),
    "powers200": (_powers, 1, 2, False),
    "lake192": (_lake192, 1, 2, False),
    "level_zero": (_level_zero, None, 3, False),
}


def _run(pipe, dem, stages, rasters):
    pipe.upload("dem", dem)
    pipe.run(*stages)
    pipe.sync()
    got = {k: pipe.download(k) for k in rasters}
    got["ints"] = {k: pipe.get_int(k) for k in ("fill_algorithm", "noflat_algorithm", "noflat_rowstore", "noflat_rows_stored", "noflat_visits",
                                                 "noflat_rounds")}
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_rows_left_out_change_nothing(monkeypatch, name):
    from malstroem_amd.pipeline import HydroPipeline
    surface, batch, algorithm, strictly = CASES[name]
    dem = np.ascontiguousarray(surface(), dtype=np.float32)
    monkeypatch.setenv("MHIP_DEVELOPER", "1")
    if batch:
        monkeypatch.setenv("MHIP_NG_BATCH", str(batch))
    short, chain = {}, {}
    with HydroPipeline(dem.shape) as pipe:
        for knob in KNOBS:
            monkeypatch.setenv("MHIP_NG_ROWSTORE", str(knob))
            short[knob] = _run(pipe, dem, ("fill", "noflat", "flowdir"), ("noflat", "flowdir"))
            chain[knob] = _run(pipe, dem, ALL, ("noflat", "flowdir", "accum", "watersheds"))
    for knob in KNOBS:
        for got in (short[knob], chain[knob]):
            print(name, knob, got["ints"])
            assert got["ints"]["noflat_algorithm"] == algorithm, (knob, got["ints"])
            assert got["ints"]["noflat_rowstore"] == REPORTED[knob], (knob, got["ints"])
    assert short[0]["ints"]["noflat_visits"] >= 2      # the rounds ran (the first visit of a tile is not counted)
    for knob in KNOBS[1:]:
        for got, want in ((short[knob], short[0]), (chain[knob], chain[0])):
            for k in want:
                if k != "ints":
                    assert_same_bits(got[k], want[k], "%s, knob %d" % (k, knob))
            # the schedule is untouched: as many visits in as many rounds
            assert got["ints"]["noflat_visits"] == want["ints"]["noflat_visits"] and got["ints"]["noflat_rounds"] == want["ints"]["noflat_rounds"]
            assert got["ints"]["noflat_rows_stored"] <= want["ints"]["noflat_rows_stored"]
            if knob == 2:      # exact rows: never more than the blocks that hold them
                assert got["ints"]["noflat_rows_stored"] <= (short if got is short[knob] else chain)[1]["ints"]["noflat_rows_stored"]
            if strictly:
                assert got["ints"]["noflat_rows_stored"] < want["ints"]["noflat_rows_stored"]
    assert_same_bits(chain[0]["noflat"], short[0]["noflat"], "noflat, chain against the short request")
    assert short[0]["ints"]["noflat_rows_stored"] > 0
