"""CPU: the generators of tests/_inputs.py make what they claim, checked with the oracle (and scipy for the labelling), so the
GPU tests of test_gpu_uploaded_inputs.py know which kernel paths their inputs reach."""
import numpy as np
import pytest
import scipy.ndimage

import oracle
import _inputs as gen
from _cases import assert_same_bits


@pytest.mark.parametrize("shape", [(128, 192), (130, 129), (63, 200)])
@pytest.mark.parametrize("end", ["leave", "sink", "cycle"])
def test_tile_hamiltonian_paths(shape, end):
    fd, c = gen.tile_hamiltonian(*shape, end)
    acc = oracle.accumulated_flow(fd)
    assert_same_bits(acc, c["acc"])
    ntr, ntc = c["ntr"], c["ntc"]
    for tr in range(ntr):
        for tc in range(ntc):
            tile = np.s_[tr * gen.AT:(tr + 1) * gen.AT, tc * gen.AT:(tc + 1) * gen.AT]
            assert np.array_equal(np.sort(c["pos"][tile].ravel()), np.arange(1, 4097))     # one path over every cell
            if end == "sink":
                assert np.array_equal(np.sort(acc[tile].ravel()), np.arange(1.0, 4097.0))
                r, cc = np.unravel_index(np.argmax(acc[tile]), (gen.AT, gen.AT))
                assert fd[tile][r, cc] == gen.NODIR and 0 < r < gen.AT - 1 and 0 < cc < gen.AT - 1   # an interior sink
            elif end == "cycle":
                assert not acc[tile].any()
            else:
                assert np.array_equal(np.sort(acc[tile].ravel()), tr * 4096 + np.arange(1.0, 4097.0))
    assert (acc > 0).sum() == (0 if end == "cycle" else ntr * ntc * 4096) + fd.size - ntr * ntc * 4096


def test_random_forest_is_acyclic_with_long_paths():
    fd, c = gen.random_forest(700, 900, seed=1, sink_frac=0.001)
    acc = oracle.accumulated_flow(fd)
    assert acc.min() >= 1                                     # no cell on a cycle
    assert np.array_equal(c["sinks"], fd == gen.NODIR) and 100 < c["sinks"].sum() < 5000
    assert acc.max() > 20000                                  # long paths drain areas of many tiles
    # a long path crosses tile outlines many times: walk the path into the cell of the largest accumulation
    r, col = np.unravel_index(np.argmax(acc), acc.shape)
    tiles = set()
    while True:
        tiles.add((r // gen.AT, col // gen.AT))
        up = [(r + gen.DR[k], col + gen.DC[k]) for k in range(8) if 0 <= r + gen.DR[k] < 700 and 0 <= col + gen.DC[k] < 900
              and fd[r + gen.DR[k], col + gen.DC[k]] == (k + 4) % 8]
        if not up:
            break
        r, col = max(up, key=lambda p: acc[p])
    assert len(tiles) > 10


@pytest.mark.parametrize("shape,seed", [((300, 280), 1), ((513, 640), 2)])
def test_tile_crossing_cycles_are_the_only_cycles(shape, seed):
    fd, c = gen.tile_crossing_cycles(*shape, seed)
    acc = oracle.accumulated_flow(fd)
    assert np.array_equal(acc == 0, c["cycle"])               # accumulation 0 on the constructed cycle cells and nowhere else
    cyc = c["cycle"]
    assert not (cyc[0].any() or cyc[-1].any() or cyc[:, 0].any() or cyc[:, -1].any())
    # trees drain into the cycles: cells flowing into a cycle cell from outside it, in several tiles
    feeders = np.zeros(fd.shape, bool)
    for k in range(8):
        r, col = np.nonzero(~cyc & (fd == k))
        tr, tc = r + gen.DR[k], col + gen.DC[k]
        ok = (tr >= 0) & (tr < fd.shape[0]) & (tc >= 0) & (tc < fd.shape[1])
        feeders[r[ok][cyc[tr[ok], tc[ok]]], col[ok][cyc[tr[ok], tc[ok]]]] = True
    tiles = {(r // gen.AT, col // gen.AT) for r, col in zip(*np.nonzero(feeders))}
    assert len(tiles) >= 9
    ws = np.zeros(fd.shape, np.int32)
    ws[feeders] = 1
    oracle.watersheds_from_labels(fd, ws, 0)                   # terminates: no cycle through an edge cell


def test_edge_variants():
    fd, _ = gen.random_forest(200, 300, seed=3)
    v, c = gen.edge_variants(fd, seed=4)
    b = c["border"]
    assert np.array_equal(v["outward"][1:-1, 1:-1], fd[1:-1, 1:-1]) and v["outward"][0, 5] == 0 and v["outward"][-1, -1] == 3
    assert (v["nodir"][b] == gen.NODIR).all()
    inward = v["inward"]
    h, w = fd.shape
    r, col = np.nonzero(b & (inward != gen.NODIR))
    codes = inward[r, col].astype(int)
    tr, tc = r + gen.DR[codes], col + gen.DC[codes]
    assert ((tr >= 0) & (tr < h) & (tc >= 0) & (tc < w)).all()              # inwards or along the border, never off the raster
    assert r.size > 0.6 * b.sum()
    assert (oracle.accumulated_flow(inward)[b] > 0).all()                    # no cycle through an edge cell
    codes = v["codes"]
    kept = codes <= gen.NODIR
    assert codes.max() > 200 and ((codes > 8).sum() > 0.02 * fd.size) and np.array_equal(codes[kept], fd[kept])
    for f in v.values():
        lab = np.zeros(f.shape, np.int32)
        lab[::17, ::13] = 5
        oracle.watersheds_from_labels(f, lab, 0)


@pytest.mark.parametrize("shape", [(67, 300), (300, 67), (257, 255)])
def test_masks_for_the_labelling(shape):
    m = gen.spiral_mask(*shape)
    lab, n = scipy.ndimage.label(m, structure=np.ones((3, 3)))
    assert n == 1 and m.sum() > 0.3 * m.size
    ol, on = oracle.connected_components(m.astype(np.uint8))
    assert on == 1 and np.array_equal(ol, lab)
    # every ring of the spiral crosses every tile line it spans twice
    rows = np.arange(gen.AT, shape[0], gen.AT)
    cols = np.arange(gen.AT, shape[1], gen.AT)
    crossings = (m[rows - 1] & m[rows]).sum() + (m[:, cols - 1] & m[:, cols]).sum()
    assert crossings > 80


def test_label_rasters_overflow_the_tables():
    rasters, c = gen.label_rasters(300, 1100, seed=5)
    t = rasters["tables"]
    for name, rows in c["bands"].items():
        band = np.zeros_like(t)
        band[rows] = t[rows]
        per_tile, per_flat = gen.tile_label_counts(band)
        slots = gen.TABLE_SLOTS[name]
        assert per_tile.max() > slots + 1 and per_flat.max() > slots + 1, (name, per_tile.max(), per_flat.max())
    assert (t == 3).mean() > 0.3                                              # the rest: one label
    assert (rasters["dominant"] == 2).mean() > 0.9
    r = rasters["rects"]
    assert 100 < np.unique(r).size and np.unique(r).max() > 10000             # sparse ids
    for name, lab in rasters.items():
        assert lab.dtype == np.int32 and c["nlabels"][name] == lab.max()


def test_value_generators():
    lab = np.arange(12, dtype=np.int32).reshape(3, 4) % 5
    for dt in (np.float32, np.float64):
        v, c = gen.label_values(np.tile(lab, (40, 40)), 1, dt)
        z = v["zeros"]
        assert z.dtype == dt and not z.any() and np.signbit(z).any() and not np.signbit(z).all()
        m = v["mixed"]
        assert np.isinf(m).any() and (m == np.round(m * 2) / 2).all()                    # ties; every partial sum exact
        t = v["subnormal"]
        assert ((t != 0) & (np.abs(t) < np.finfo(dt).tiny)).any() and (np.abs(t) < np.finfo(dt).tiny).all()
        nan = np.isnan(v["nan"])
        assert nan.any() and np.array_equal(np.unique(np.tile(lab, (40, 40))[nan]), [c["nan_label"]])
    p = gen.packed_argmax_values(np.zeros((50, 60), np.int32), 2)
    assert set(np.unique(p["fast"])) == {0.0, 2.0 ** 32 - 1}
    for name in ("2^32", "-1", "0.5", "nan"):
        d = p[name]
        bad = ~((d >= 0) & (d < 2.0 ** 32) & (d == np.floor(d)))
        assert bad.sum() == 1
    s = gen.d8_surfaces(40, 60, 3)
    assert np.isnan(s["special"]).any() and (np.signbit(s["special"]) & (s["special"] == 0)).any()
    assert (np.abs(s["special"]) > 1e308).any() and (s["ints"] == np.round(s["ints"])).all()
    # the stamped 3 x 3 surfaces make the two D8 variants of the reference disagree
    a, b = oracle.terrain_flowdirection(s["muldiv"]), oracle.terrain_flowdirection(s["muldiv"], variant="python")
    assert (a != b).any()


def test_assert_same_bits():
    assert_same_bits(np.array([0.0, np.nan, 1.0]), np.array([0.0, np.nan, 1.0]))
    with pytest.raises(AssertionError):
        assert_same_bits(np.array([0.0]), np.array([-0.0]))
    with pytest.raises(AssertionError):
        assert_same_bits(np.array([1.0], np.float32), np.array([1.0], np.float64))
    rec = np.zeros(2, oracle.INDEX_DTYPE)
    assert_same_bits(rec, rec.copy())
    other = rec.copy()
    other["value"][1] = -0.0
    with pytest.raises(AssertionError):
        assert_same_bits(rec, other)
