"""CPU: the model of the DEM adaptations (tests/_burn.py, the definition of csrc/burn.hip), the conversion of GeoJSON
features to lines and segments (malstroem_amd/adaptations.py) and the argument rules, none of which needs a device."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import _burn


def incremental_walk(r0, c0, r1, c1):
    """the cells of a segment by an error accumulator, one step at a time: minor moves when the doubled error passes n"""
    dr, dc = r1 - r0, c1 - c0
    n, dmin = max(abs(dr), abs(dc)), min(abs(dr), abs(dc))
    colmajor = abs(dc) >= abs(dr)
    sr, sc = (dr > 0) - (dr < 0), (dc > 0) - (dc < 0)
    r, c, err, out = r0, c0, n, [(r0, c0)]      # err = (2 * k * dmin + n) mod 2n, carried
    for _ in range(n):
        err += 2 * dmin
        move = err >= 2 * n
        if move:
            err -= 2 * n
        if colmajor:
            c += sc
            r += sr if move else 0
        else:
            r += sr
            c += sc if move else 0
        out.append((r, c))
    return out


def test_every_segment_of_a_9x9_box():
    pts = list(itertools.product(range(9), range(9)))
    assert len(pts) ** 2 == 6561
    for (r0, c0), (r1, c1) in itertools.product(pts, pts):
        dr, dc = abs(r1 - r0), abs(c1 - c0)
        n = max(dr, dc)
        c8 = [(r, c) for _, r, c in _burn.segment_cells(r0, c0, r1, c1, False)]
        c4 = [(r, c) for _, r, c in _burn.segment_cells(r0, c0, r1, c1, True)]
        assert c8[0] == c4[0] == (r0, c0) and c8[-1] == c4[-1] == (r1, c1)
        assert len(c8) == n + 1 and len(c4) == dr + dc + 1
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(c8, c8[1:]))
        assert all(abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 for a, b in zip(c4, c4[1:]))
        assert c8 == incremental_walk(r0, c0, r1, c1)
        assert set(c8) <= set(c4)
        # the steps clipped to a raster are the cells inside it, whatever the raster
        for shape in ((4, 6), (9, 3)):
            inside = lambda cells: [(k, r, c) for k, r, c in cells if 0 <= r < shape[0] and 0 <= c < shape[1]]
            for conn4 in (False, True):
                assert inside(_burn.segment_cells(r0, c0, r1, c1, conn4, shape)) == inside(_burn.segment_cells(r0, c0, r1, c1, conn4))


def test_levels_return_the_ends_exactly():
    rng = np.random.default_rng(3)
    for z0, z1 in rng.normal(0, 100, (200, 2)).astype(np.float32):
        for n in (1, 7, 1000):
            assert _burn.level(z0, z1, 0, 0, n, False) == z0 and _burn.level(z0, z1, 0, n, n, False) == z1
    assert _burn.level(2.0, 5.0, 0, 0, 0, False) == 2.0 and _burn.level(2.0, 5.0, 0, 0, 0, True) == 5.0


def random_case(seed=5, shape=(37, 53), nlines=60):
    rng = np.random.default_rng(seed)
    H, W = shape
    dem = rng.normal(10, 3, shape).astype(np.float32)
    dem[H // 2, W // 3] = np.nan
    verts = [[(int(rng.integers(-5, H + 5)), int(rng.integers(-5, W + 5))) for _ in range(int(rng.integers(2, 5)))] for _ in range(nlines)]
    z0 = np.where(rng.random(nlines) < 0.5, np.nan, rng.normal(10, 3, nlines))
    z1 = np.where(rng.random(nlines) < 0.5, np.nan, rng.normal(10, 3, nlines))
    lines, segs = _burn.polylines(verts, z0, z1, rng.integers(0, 4, nlines))
    return dem, lines, segs


def test_the_model_does_not_depend_on_the_order_of_the_lines():
    dem, lines, segs = random_case()
    out, res = _burn.burn(dem, lines, segs)
    perm = np.arange(len(lines))[::-1].copy()
    l2, s2 = _burn.reorder_lines(lines, segs, perm)
    out2, res2 = _burn.burn(dem, l2, s2[::-1])
    assert out.tobytes() == out2.tobytes()
    assert res[perm].tobytes() == res2.tobytes()
    changed = int(np.sum(out.view(np.uint32) != dem.view(np.uint32)))
    assert changed > 300 and set(res["status"].tolist()) >= {0, 1}, (changed, res["status"])
    assert np.isnan(out[37 // 2, 53 // 3]) and np.isnan(out).sum() == 1
    assert np.all(res["cells"][res["status"] != 0] == 0) and np.all(np.isnan(res["z0"][res["status"] != 0]))


GT = (1000.0, 2.0, 0.0, 5000.0, 0.0, -2.0)


def feature(coords, gtype="LineString", **props):
    return dict(type="Feature", geometry=dict(type=gtype, coordinates=coords), properties=props)


def test_lines_from_features():
    from malstroem_amd import _lib
    from malstroem_amd.adaptations import CONN4, RAISE, lines_from_features
    assert _lib.BURN_SEGMENT_DTYPE.itemsize == 24 and _lib.BURN_LINE_DTYPE.itemsize == 24 and _lib.BURN_RESULT_DTYPE.itemsize == 32
    assert (_lib.BURN_SEGMENT_DTYPE, _lib.BURN_LINE_DTYPE, _lib.BURN_RESULT_DTYPE) == (_burn.SEGMENT_DTYPE, _burn.LINE_DTYPE, _burn.RESULT_DTYPE)
    # world -> cell with a negative t[5]: x = 1000 + 2 * col, y = 5000 - 2 * row; a vertex on a cell's edge belongs to the next cell
    feats = [feature([[1001.0, 4999.0], [1009.9, 4999.0], [1010.0, 4990.0], [1003.0, 4970.5]]),
             feature([[[1000.0, 5000.0], [1004.0, 4996.0]], [[996.0, 5004.0], [998.1, 5001.9]]], "MultiLineString", mode="raise", z_from=3, z_to=4.5),
             feature([[1020.0, 4980.0]], mode="raise", connectivity=8), feature([[1020.0, 4980.0], [1030.0, 4980.0]], connectivity=4, z_to=None)]
    lines, segs, index = lines_from_features(feats, GT, (40, 40), with_index=True)
    assert lines_from_features(feats, GT, (40, 40))[1].tobytes() == segs.tobytes()
    assert index.tolist() == [0, 1, 1, 2, 3]
    assert [tuple(s) for s in segs[:3]] == [(0, 0, 0, 4, 0, 0), (0, 4, 5, 5, 0, 4), (5, 5, 14, 1, 0, 9)]
    assert lines["ntotal"].tolist() == [18, 2, 1, 0, 5]
    assert [tuple(s) for s in segs[3:]] == [(0, 0, 2, 2, 1, 0), (-2, -2, -1, -1, 2, 0), (10, 10, 10, 10, 3, 0), (10, 10, 10, 15, 4, 0)]
    assert lines["flags"].tolist() == [0, RAISE | CONN4, RAISE | CONN4, RAISE, CONN4]
    assert np.isnan(lines["z0"][[0, 3, 4]]).all() and np.isnan(lines["z1"][[0, 3, 4]]).all()
    assert lines["z0"][1:3].tolist() == [3.0, 3.0] and lines["z1"][1:3].tolist() == [4.5, 4.5]
    e = lines_from_features([], GT, (40, 40))
    assert e[0].size == 0 and e[1].size == 0 and e[0].dtype == _lib.BURN_LINE_DTYPE


def test_value_errors_come_before_the_library(monkeypatch):
    from malstroem_amd import _lib, adaptations
    from malstroem_amd.adaptations import burn_lines, lines_from_features

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    ok = [[1001.0, 4999.0], [1009.9, 4999.0]]
    with pytest.raises(ValueError, match="feature 1: .*Polygon"):
        lines_from_features([feature(ok), feature([[ok[0], ok[1], ok[0]]], "Polygon", )], GT, (40, 40))
    with pytest.raises(ValueError, match="feature 0 \\(id 'a7'\\)"):
        lines_from_features([dict(feature(ok[0], "Point"), id="a7")], GT, (40, 40))
    with pytest.raises(ValueError, match="north-up"):
        lines_from_features([feature(ok)], (1000.0, 2.0, 0.1, 5000.0, 0.0, -2.0), (40, 40))
    for props in (dict(mode="dig"), dict(connectivity=6), dict(z_from="3"), dict(z_to=float("inf")), dict(z_to=1e39)):
        with pytest.raises(ValueError, match="feature 0"):
            lines_from_features([feature(ok, **props)], GT, (40, 40))
    with pytest.raises(ValueError, match="2\\*\\*29"):
        lines_from_features([feature([ok[0], [3e9, 4999.0]])], GT, (40, 40))
    dem = np.zeros((8, 8), dtype=np.float32)
    lines, segs = _burn.polylines([[(1, 1), (5, 6)], [(2, 2), (2, 7)]], 1.0, 2.0)

    def broken(what, field, index, value):
        l2, s2 = lines.copy(), segs.copy()
        (l2 if what == "line" else s2)[field][index] = value
        return l2, s2
    for args in (("seg", "line", 1, 2), ("seg", "line", 0, -1), ("seg", "r1", 0, 2 ** 29 + 1), ("seg", "c0", 1, -2 ** 29 - 1), ("seg", "koff", 0, -1),
                 ("seg", "koff", 1, 1), ("line", "ntotal", 0, 4), ("line", "ntotal", 1, -1), ("line", "z0", 0, np.inf), ("line", "z1", 1, -1e39),
                 ("line", "flags", 0, 4), ("line", "flags", 1, -1)):
        with pytest.raises(ValueError):
            burn_lines(dem, *broken(*args))
    with pytest.raises(ValueError, match="dtype mismatch"):
        burn_lines(dem.astype(np.float64), lines, segs)
    with pytest.raises(ValueError):
        burn_lines(dem, lines.astype([("z0", "<f8"), ("z1", "<f8"), ("ntotal", "<i8"), ("flags", "<i4")]), segs)
    with pytest.raises(ValueError):
        burn_lines(dem, lines, segs, nodata="none")
    assert adaptations.check_lines(lines, segs)[1].tobytes() == segs.tobytes()


def test_the_library_refuses_the_same_arguments_before_any_device_work():
    """straight at the C-ABI, past the checks of the Python layer: MHIP_EINVAL, with or without a device"""
    from malstroem_amd import _lib
    _lib.build()
    lib = _lib.load()
    dem = np.zeros((8, 8), dtype=np.float32)
    lines, segs = _burn.polylines([[(1, 1), (5, 6)], [(2, 2), (2, 7)]], 1.0, 2.0)
    res = np.zeros(2, dtype=_lib.BURN_RESULT_DTYPE)

    def rc(l, s, nseg=None, nline=None):
        return lib.mhip_burn_lines_f32(_lib.ptr(dem), _lib.i64(8), _lib.i64(8), _lib.i64(len(s) if nseg is None else nseg), _lib.ptr(s),
                                       _lib.i64(len(l) if nline is None else nline), _lib.ptr(l), ctypes.c_double(np.nan), _lib.ptr(res))
    for what, field, index, value in (("seg", "line", 1, 2), ("seg", "r1", 0, 2 ** 29 + 1), ("seg", "koff", 0, -1), ("seg", "koff", 1, 1),
                                      ("line", "z0", 0, np.inf), ("line", "z1", 1, -1e39), ("line", "flags", 0, 4), ("line", "ntotal", 1, -1)):
        l2, s2 = lines.copy(), segs.copy()
        (l2 if what == "line" else s2)[field][index] = value
        assert rc(l2, s2) == _lib.EINVAL, (what, field)
    assert rc(lines, segs, nseg=-1) == _lib.EINVAL and rc(lines, segs, nline=-1) == _lib.EINVAL
    # no segment: nothing to do, no device asked for; the records say what a line without a vertex gets
    lines["z0"][1] = np.nan
    res["cells"] = 7
    assert rc(lines, segs, nseg=0) == _lib.OK
    assert res["status"].tolist() == [0, 1] and res["cells"].tolist() == [0, 0] and res["z0"][0] == 1.0 and np.isnan(res["z0"][1])
    assert res.tobytes() == _burn.burn(dem, lines, segs[:0])[1].tobytes() and not dem.any()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    from malstroem_amd import _lib
    from malstroem_amd.adaptations import burn_lines
    _lib.build()
    lines, segs = _burn.polylines([[(1, 1), (5, 6)]], 1.0, 2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        burn_lines(np.zeros((8, 8), dtype=np.float32), lines, segs)


def test_tools_take_the_new_arguments_as_keywords_at_the_end():
    import inspect
    from malstroem_amd.complete import process_all
    from malstroem_amd.dem import DemTool
    p = list(inspect.signature(DemTool.__init__).parameters)
    assert p[:6] == ["self", "input_dem", "output_filled", "output_flowdir", "output_depths", "output_accum"]      # reference dem.py:33
    assert p[-3:] == ["input_adaptations", "output_adapted", "output_adaptation_report"]
    assert list(inspect.signature(process_all).parameters)[-1] == "adaptations"
    with pytest.raises(NotImplementedError, match="adaptations on row bands"):
        import types
        process_all("dem.tif", "out", [10], comm=types.SimpleNamespace(size=2, rank=0), adaptations="lines.geojson")
