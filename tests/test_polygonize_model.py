"""CPU: the definition of the polygonizer (tests/_polygonize.py) -- its known answers on the reference's fixtures, its
three invariants, rings written out by hand -- and the host side of malstroem_amd/vector.py on the model's output: the GeoJSON
features, their round trip back to the raster, the argument rules, the C-ABI's five symbols.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import _polygonize as P
import _zones
from _cases import fixtures

ROOT = Path(__file__).resolve().parent.parent


def rings_of(labels):
    xy, off, rl = P.polygonize(np.asarray(labels, dtype=np.int32))
    assert xy.dtype == np.int32 and off.dtype == np.int64 and rl.dtype == np.int32
    return [(int(rl[k]), [tuple(v) for v in xy[off[k]:off[k + 1]].tolist()]) for k in range(len(rl))]


# ---- the model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,want", [("labelled", (104, 119, 15, 2528, 0)), ("wsheds", (104, 105, 1, 6144, 0))])
def test_known_answers_on_the_fixtures(name, want):
    """(labels, rings, holes, vertices, labels with more than one exterior ring) of a direct implementation of the rule"""
    lab = fixtures()[name]
    got, (xy, off, rl) = P.summary(lab)
    assert got == want
    P.check_invariants(lab, xy, off, rl)


@pytest.mark.parametrize("shape", [(65, 130), (1, 70), (70, 1), (64, 64)])
def test_invariants_on_random_components(shape):
    lab = P.random_components(shape, 3)
    (nlab, nring, holes, nvert, multi), (xy, off, rl) = P.summary(lab)
    assert nlab == lab.max() > 10 and multi == 0 and nring == nlab + holes
    P.check_invariants(lab, xy, off, rl)
    # rings in the order of their start vertices, each starting at its smallest vertex
    start = xy[off[:-1]]
    key = start[:, 1].astype(np.int64) * (shape[1] + 1) + start[:, 0]
    assert np.all(np.diff(key) >= 0)
    for k in range(nring):
        ring = xy[off[k]:off[k + 1]]
        assert min((int(y), int(x)) for x, y in ring) == (int(ring[0, 1]), int(ring[0, 0]))


def test_rings_by_hand():
    # one cell; the whole raster
    assert rings_of([[7]]) == [(7, [(0, 0), (1, 0), (1, 1), (0, 1)])]
    assert rings_of(np.full((3, 5), 2)) == [(2, [(0, 0), (5, 0), (5, 3), (0, 3)])]
    assert rings_of(np.zeros((4, 4))) == []
    # two cells that touch by a corner are joined by the left turn: one ring that visits (1, 1) twice
    assert rings_of([[1, 0], [0, 1]]) == [(1, [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)])]
    # ... the other diagonal: the ring starts at (1, 0)
    assert rings_of([[0, 1], [1, 0]]) == [(1, [(1, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2), (0, 1), (1, 1)])]
    # cells of two labels at a corner: each label joins its own
    assert rings_of([[1, 2], [2, 1]]) == [(1, [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)]),
                                           (2, [(1, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2), (0, 1), (1, 1)])]
    # a frame with a hole: the exterior clockwise on screen (positive area), the hole the other way round, starting downwards
    frame = np.ones((3, 3))
    frame[1, 1] = 0
    assert rings_of(frame) == [(1, [(0, 0), (3, 0), (3, 3), (0, 3)]), (1, [(1, 1), (1, 2), (2, 2), (2, 1)])]
    # label 1 wholly inside label 2, flush with its top-left cell: 2's hole and 1's exterior share the start vertex, the exterior first
    nest = np.full((3, 3), 2)
    nest[1, 1] = 1
    got = rings_of(nest)
    assert got == [(2, [(0, 0), (3, 0), (3, 3), (0, 3)]), (1, [(1, 1), (2, 1), (2, 2), (1, 2)]), (2, [(1, 1), (1, 2), (2, 2), (2, 1)])]
    # the hole of a diamond of corner-touching cells is ONE hole per 4-connected component of what it encloses
    diamond = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]])
    got = rings_of(diamond)
    assert [l for l, _ in got] == [1, 1] and got[1][1] == [(1, 1), (1, 2), (2, 2), (2, 1)]
    assert P.ring_areas(*P.polygonize(diamond.astype(np.int32))[:2]).tolist() == [5, -1]
    # an L and a step: only corners are kept
    assert rings_of([[1, 0], [1, 1]]) == [(1, [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (0, 2)])]
    with pytest.raises(ValueError, match="negative"):
        P.polygonize(np.array([[1, -1]], dtype=np.int32))


def test_special_shapes_keep_the_invariants():
    sp = P.spiral(130)
    (nlab, nring, holes, nvert, multi), r = P.summary(sp)
    assert (nlab, nring, holes) == (1, 1, 0) and nvert > 250 and sp.sum() > 8000
    P.check_invariants(sp, *r)
    fr = P.frames(9)
    (nlab, nring, holes, nvert, multi), r = P.summary(fr)
    assert (nlab, nring, holes, nvert) == (2, 9, 4, 36)
    P.check_invariants(fr, *r, components=False)
    rr, cc = np.mgrid[0:66, 0:67]
    board = ((rr + cc) % 2 == 0).astype(np.int32) * 5
    (nlab, nring, holes, nvert, multi), r = P.summary(board)
    assert nlab == 1 and multi == 0 and nring == 1 + holes
    P.check_invariants(board, *r)


# ---- features -------------------------------------------------------------------------------------------------------------------------
AWKWARD = (600000.3, 0.4, 0, 6200000.7, 0, -0.4)


def shoelace(ring):
    a = np.asarray(ring, dtype=np.float64)
    a = a - a[0]      # (far from the origin the products would cancel badly)
    return 0.5 * float(np.sum(a[:-1, 0] * a[1:, 1] - a[1:, 0] * a[:-1, 1]))


@pytest.mark.parametrize("name", ["labelled", "wsheds", "random"])
@pytest.mark.parametrize("transform", [AWKWARD, (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)])
def test_features_round_trip(name, transform):
    from malstroem_amd.objects import rings_from_features
    from malstroem_amd.vector import features_from_rings
    lab = P.random_components((65, 130), 4) if name == "random" else fixtures()[name]
    xy, off, rl = P.polygonize(lab)
    feats = features_from_rings(xy, off, rl, transform, id_attribute="bspot_id")
    present = np.unique(lab[lab != 0])
    assert [f["properties"]["bspot_id"] for f in feats] == present.tolist() and [f["id"] for f in feats] == present.tolist()
    nrings = 0
    for f in feats:
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon"
        for k, ring in enumerate(f["geometry"]["coordinates"]):
            nrings += 1
            assert ring[0] == ring[-1] and len(ring) >= 5
            # exterior rings counter-clockwise in a north-up world, holes clockwise
            assert (shoelace(ring) > 0) == (k == 0)
    assert nrings == len(rl)
    # back through objects.rings_from_features (feature k is zone k + 1) and the rasterizer's model: the label raster
    fxy, foff, fzone, nzone = rings_from_features(feats, transform)
    back = _zones.rasterize(lab.shape, fxy, foff, fzone, nzone)
    lut = np.concatenate([[0], present]).astype(np.int32)
    assert lut[back].tobytes() == np.ascontiguousarray(lab, dtype=np.int32).tobytes()


def test_hole_goes_to_the_part_that_holds_it():
    """label 1 in two components: a big frame, and a small frame standing inside the big one's hole; each has a hole of its own"""
    from malstroem_amd.vector import features_from_rings
    lab = np.zeros((11, 12), dtype=np.int32)
    lab[0:11, 0:11] = 1
    lab[1:10, 1:10] = 0
    lab[3:8, 3:8] = 1
    lab[4:7, 4:7] = 0
    lab[5, 5] = 2
    xy, off, rl = P.polygonize(lab)
    assert rl.tolist() == [1, 1, 1, 1, 2] and P.ring_areas(xy, off).tolist() == [121, -81, 25, -9, 1]
    f1, f2 = features_from_rings(xy, off, rl, (0, 1, 0, 0, 0, -1))
    assert f1["geometry"]["type"] == "MultiPolygon" and f2["geometry"]["type"] == "Polygon"
    parts = f1["geometry"]["coordinates"]
    assert [len(p) for p in parts] == [2, 2]
    assert [abs(shoelace(r)) for p in parts for r in p] == [121, 81, 25, 9]
    # every part's exterior first and counter-clockwise, closed
    assert all(shoelace(p[0]) > 0 > shoelace(p[1]) and p[0][0] == p[0][-1] for p in parts)


def test_full_geotransform_is_applied():
    from malstroem_amd.vector import features_from_rings, transform_cell_to_world
    from malstroem_amd import bluespots
    assert bluespots.transform_cell_to_world is transform_cell_to_world
    t = (10.0, 2.0, 0.5, 100.0, 0.25, -2.0)
    (f,) = features_from_rings(*P.polygonize(np.array([[0, 3]], dtype=np.int32)), t, id_attribute="n")
    assert f["properties"] == {"n": 3}
    want = [[t[0] + x * t[1] + y * t[2], t[3] + x * t[4] + y * t[5]] for x, y in ((1, 0), (1, 1), (2, 1), (2, 0), (1, 0))]
    assert f["geometry"]["coordinates"] == [want]       # (north-up: from the first vertex backwards, counter-clockwise on the map)
    (g,) = features_from_rings(*P.polygonize(np.array([[0, 3]], dtype=np.int32)), (0, 1, 0, 0, 0, 1))      # y up the rows: edge order
    assert g["geometry"]["coordinates"] == [[[1, 0], [2, 0], [2, 1], [1, 1], [1, 0]]]
    assert transform_cell_to_world((0, 1), t) == (t[0] + 1.5 * t[1] + 0.5 * t[2], t[3] + 1.5 * t[4] + 0.5 * t[5])
    assert features_from_rings(np.zeros((0, 2), dtype=np.int32), [0], np.zeros(0, dtype=np.int32), t) == []


def test_argument_rules():
    from malstroem_amd import vector
    from malstroem_amd.pipeline import HydroPipeline
    ok = np.zeros((3, 3), dtype=np.int32)
    with pytest.raises(ValueError, match="dtype mismatch"):
        vector.polygonize(ok.astype(np.int64))
    with pytest.raises(ValueError, match="dtype mismatch"):
        vector.polygonize(ok.astype(np.float32))
    with pytest.raises(ValueError, match="shape"):
        vector.polygonize(np.zeros(9, dtype=np.int32))
    with pytest.raises(ValueError, match="shape"):
        vector.polygonize(np.zeros((0, 4), dtype=np.int32))
    bad = ok.copy()
    bad[2, 1] = -4
    with pytest.raises(ValueError, match="negative"):
        vector.polygonize(bad)
    xy, off, rl = P.polygonize(np.array([[1, 0, 2]], dtype=np.int32))
    t = (0, 1, 0, 0, 0, -1)
    with pytest.raises(ValueError, match="transform"):
        vector.features_from_rings(xy, off, rl, (0, 1, 0, 0, 0))
    with pytest.raises(ValueError, match="transform"):
        vector.features_from_rings(xy, off, rl, (0, 1, 0, 0, 0, np.nan))
    with pytest.raises(ValueError, match="transform"):
        vector.features_from_rings(xy, off, rl, (0, 0, 0, 0, 0, -1))
    with pytest.raises(ValueError, match="transform"):
        vector.vectorize_labels(bad, (0, 1, 0, 0, 0))
    with pytest.raises(ValueError, match="xy"):
        vector.features_from_rings(xy.astype(np.float64), off, rl, t)
    with pytest.raises(ValueError, match="ring_offsets"):
        vector.features_from_rings(xy, off[:-1], rl[:-1], t)
    with pytest.raises(ValueError, match="ring_label"):
        vector.features_from_rings(xy, off, rl[:-1], t)
    with pytest.raises(ValueError, match="fewer than 3"):
        vector.features_from_rings(xy, np.array([0, 2, 8]), rl, t)
    with pytest.raises(ValueError, match="below 1"):
        vector.features_from_rings(xy, off, np.array([0, 1]), t)
    with pytest.raises(ValueError, match="id_attribute"):
        vector.features_from_rings(xy, off, rl, t, id_attribute="")
    # the pipeline's sources are checked before the context is asked
    with pytest.raises(ValueError, match="source"):
        HydroPipeline.__new__(HydroPipeline).polygonize("depths")      # (no context was created)


def test_vector_on_row_bands_is_refused(tmp_path):
    from malstroem_amd.complete import process_all

    class TwoRanks(object):
        size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="vector on row bands"):
        process_all("unused.tif", str(tmp_path), [10], comm=TwoRanks(), vector=True)


def test_the_five_symbols_are_declared():
    from malstroem_amd import _lib
    header = (ROOT / "include" / "malstroem_hip.h").read_text()
    declared = set(re.findall(r"\b(mhip_[a-z0-9_]+)\s*\(", header))
    five = {"mhip_polygonize_i32", "mhip_ctx_polygonize", "mhip_polygons_sizes", "mhip_polygons_fetch", "mhip_polygons_free"}
    assert five <= declared and five <= set(_lib.SYMBOLS)
    _lib.build()
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in five)


def test_an_all_zero_raster_asks_for_no_device():
    from malstroem_amd import vector
    xy, off, rl = vector.polygonize(np.zeros((5, 7), dtype=np.int32))
    assert xy.shape == (0, 2) and xy.dtype == np.int32 and off.tolist() == [0] and off.dtype == np.int64 and rl.shape == (0,)
    assert vector.vectorize_labels(np.zeros((5, 7), dtype=np.int32), (0, 1, 0, 0, 0, -1)) == []


def test_the_file_form_refuses_what_is_no_label_raster(tmp_path):
    """float values and a file without a geotransform: ValueError when the generator starts, before the library is touched"""
    from malstroem_amd import vector
    from malstroem_amd.io import RasterWriter
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    RasterWriter(str(tmp_path / "floats.tif"), gt, None).write(fx["depths"])
    with pytest.raises(ValueError, match="integers"):
        next(vector.vectorize_labels_file(str(tmp_path / "floats.tif")))
    RasterWriter(str(tmp_path / "bare.tif"), None, None).write(fx["labelled"])
    with pytest.raises(ValueError, match="geotransform"):
        next(vector.vectorize_labels_file(str(tmp_path / "bare.tif")))
