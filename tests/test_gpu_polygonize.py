"""GPU: the polygonizer (csrc/polygonize.hip, malstroem_amd/vector.py) against its definition, the model
tests/_polygonize.py, byte for byte; at 1024 x 1024, where the model is too slow, against its three invariants (rasterizing the rings
gives the raster back, the areas are the cell counts, one exterior ring per label); the context; and ``complete`` with ``vector=True``.
Everything is exact: nothing here has a tolerance."""
import ctypes

import numpy as np
import pytest

import _polygonize as P
from _cases import fbm, fixtures

pytestmark = pytest.mark.gpu


def same(got, want):
    for g, w, dtype in zip(got, want, (np.int32, np.int64, np.int32)):
        assert g.dtype == w.dtype == dtype and g.shape == w.shape, (g.dtype, g.shape, w.shape)
    (gx, go, gl), (wx, wo, wl) = got, want
    assert go.tobytes() == wo.tobytes(), (len(go), len(wo), np.flatnonzero(go[:min(len(go), len(wo))] != wo[:min(len(go), len(wo))])[:5])
    assert gl.tobytes() == wl.tobytes(), np.flatnonzero(gl != wl)[:5]
    assert gx.tobytes() == wx.tobytes(), (np.argwhere(gx != wx)[:5], gx[(gx != wx).any(axis=1)][:5], wx[(gx != wx).any(axis=1)][:5])


def check(labels):
    from malstroem_amd.vector import polygonize
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    want = P.polygonize(lab)
    same(polygonize(lab), want)
    return want


# ---- against the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rings,verts", [("labelled", 119, 2528), ("wsheds", 105, 6144)])
def test_fixtures(name, rings, verts):
    xy, off, rl = check(fixtures()[name])
    assert (len(rl), len(xy)) == (rings, verts)


@pytest.mark.parametrize("shape", [(130, 257), (130, 256), (65, 129), (64, 64), (1, 300), (200, 1)])
def test_random_components(shape):
    """tile edges at 64, ragged tiles, single rows; more than one block of vertices and of edges"""
    lab = P.random_components(shape, 11 + shape[1])
    xy, off, rl = check(lab)
    assert len(rl) >= lab.max() > 10
    # ... and arbitrary labels (several components of one label, neighbours of other labels without background between them)
    check(np.random.default_rng(shape[0]).integers(0, 4, shape))


def test_every_interior_vertex_a_pinch():
    rr, cc = np.mgrid[0:66, 0:67]
    xy, off, rl = check(((rr + cc) % 2 == 0).astype(np.int32) * 9)
    assert set(rl.tolist()) == {9} and (P.ring_areas(xy, off) > 0).sum() == 1


def test_a_spiral_through_every_tile():
    """one ring of 17 000 edges that crosses every 64 x 64 tile many times: the longest list at this size, 16 rounds of the doubling"""
    sp = P.spiral(130)
    xy, off, rl = check(sp)
    assert len(rl) == 1 and off.tolist() == [0, len(xy)] and len(xy) > 250
    check(sp.T * 3)
    check(sp[::-1, ::-1])


def test_nested_frames():
    """holes within holes; the hole of one label and the exterior ring of the next share their start vertex"""
    for n, width in ((9, 1), (70, 1), (131, 3)):
        fr = P.frames(n, width)
        xy, off, rl = check(fr)
        start = xy[off[:-1]]
        shared = np.flatnonzero((start[1:] == start[:-1]).all(axis=1))
        assert len(shared) >= 3 and np.all(P.ring_areas(xy, off)[shared] > 0) and np.all(P.ring_areas(xy, off)[shared + 1] < 0)


def test_whole_raster_two_components_and_nothing():
    from malstroem_amd.vector import polygonize
    xy, off, rl = check(np.full((67, 130), 5))
    assert xy.tolist() == [[0, 0], [130, 0], [130, 67], [0, 67]] and rl.tolist() == [5]
    check(np.full((1, 1), 2))
    two = np.zeros((70, 140), dtype=np.int32)
    two[3:20, 5:50] = 4
    two[40:66, 60:139] = 4
    two[45:50, 70:80] = 0
    xy, off, rl = check(two)
    assert rl.tolist() == [4, 4, 4] and P.ring_areas(xy, off).tolist() == [17 * 45, 26 * 79, -50]
    xy, off, rl = polygonize(np.zeros((33, 65), dtype=np.int32))
    assert xy.shape == (0, 2) and off.tolist() == [0] and rl.shape == (0,)


def test_a_negative_label_is_refused():
    from malstroem_amd import _lib
    from malstroem_amd.vector import polygonize
    lab = P.random_components((40, 300), 5)
    lab[33, 257] = -1
    with pytest.raises(ValueError, match="negative"):
        polygonize(lab)
    # ... by the library itself as well (the `bad` word of the counting kernel)
    handle = ctypes.c_void_p()
    with pytest.raises(ValueError, match="negative"):
        _lib.call("mhip_polygonize_i32", _lib.ptr(lab), _lib.i64(40), _lib.i64(300), ctypes.byref(handle))
    assert not handle


# ---- 1024 x 1024: the invariants ------------------------------------------------------------------------------------------------------
def invariants(labels, xy, off, rl, counts):
    from malstroem_amd.objects import rasterize
    nlab = len(counts) - 1
    assert rasterize(labels.shape, xy, off, rl, nlab).tobytes() == labels.tobytes()
    area = P.ring_areas(xy, off)
    assert np.array_equal(np.bincount(rl, weights=area, minlength=nlab + 1).astype(np.int64)[1:], counts[1:])
    ext = np.bincount(rl[area > 0], minlength=nlab + 1)
    assert np.array_equal(ext[1:], (counts[1:] > 0).astype(ext.dtype))


@pytest.fixture(scope="module")
def terrain():
    """fbm at 1024 x 1024 through the pipeline; -> (pipeline, labels, watersheds), closed when the module is done"""
    from malstroem_amd.pipeline import HydroPipeline
    p = HydroPipeline((1024, 1024))
    p.upload("dem", fbm(1024))
    p.run("fill", "noflat", "flowdir", "label")
    p.apply_keep(None)
    p.run("watershed")
    yield p, p.download("labels"), p.download("watersheds")
    p.close()


@pytest.mark.parametrize("source", ["labels", "watersheds"])
def test_invariants_at_1024(terrain, source):
    from malstroem_amd.algorithms import label
    from malstroem_amd.vector import polygonize
    p, labels, wsheds = terrain
    raster = labels if source == "labels" else wsheds
    nlab = p.get_int("nlabels")
    assert nlab > 1000
    got = p.polygonize(source)
    counts = np.zeros(nlab + 1, dtype=np.int64)
    got_counts = np.asarray(label.label_count(raster), dtype=np.int64)
    counts[:len(got_counts)] = got_counts
    invariants(raster, *got, counts)
    # the context's call equals the stateless call on the downloaded raster
    same(polygonize(raster), got)


def test_a_handle_keeps_its_snapshot(terrain):
    from malstroem_amd import _lib
    from malstroem_amd.vector import take_polygons
    p, labels, wsheds = terrain
    want = p.polygonize("labels")
    handle = ctypes.c_void_p()
    _lib.call("mhip_ctx_polygonize", p._ctx, ctypes.c_int32(_lib.R_LABELS), ctypes.byref(handle))
    # a source without a raster, an unfiltered labelling and a source that is none: the errors of the getters; then a re-run
    with pytest.raises(ValueError, match="source"):
        p.polygonize("depths")
    other = ctypes.c_void_p()
    with pytest.raises(ValueError, match="MHIP_R_LABELS or MHIP_R_WATERSHEDS"):
        _lib.call("mhip_ctx_polygonize", p._ctx, ctypes.c_int32(_lib.R_DEPTHS), ctypes.byref(other))
    p.run("label")
    with pytest.raises(ValueError, match="apply_keep"):
        p.polygonize("labels")
    raw = p.raw_stats()
    keep = raw["max"] > 0.05
    keep[0] = False
    assert 0 < p.apply_keep(keep) < p.get_int("nlabels_raw")
    fewer = p.polygonize("labels")
    assert len(fewer[2]) < len(want[2])
    same(take_polygons(handle), want)
    # back to the module's state
    p.run("label")
    p.apply_keep(None)
    p.run("watershed")
    same(p.polygonize("labels"), want)


def test_a_context_without_the_raster_and_a_row_band_refuse():
    from malstroem_amd import _lib
    from malstroem_amd.distributed import HipBand
    from malstroem_amd.pipeline import HydroPipeline
    with HydroPipeline((8, 9)) as p:
        p.upload("dem", np.zeros((8, 9), dtype=np.float32))
        for source in ("labels", "watersheds"):
            with pytest.raises(ValueError, match="has not been computed"):
                p.polygonize(source)
        lab = np.zeros((8, 9), dtype=np.int32)
        lab[2:5, 3:8] = 6
        p.upload("labels", lab)       # (uploaded labels are final)
        same(p.polygonize("labels"), P.polygonize(lab))
    band = HipBand(64, 48, 0, 32, device=0, rank=0, size=2)
    try:
        band.upload("labels", np.ones((32, 48), dtype=np.int32))
        handle = ctypes.c_void_p()
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_polygonize", band._ctx, ctypes.c_int32(_lib.R_LABELS), ctypes.byref(handle))
    finally:
        band.close()


# ---- tools -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt,nlabels", [("area > 20.5 and maxdepth > 0.5 or volume > 2.5", 486), (None, 523)])
def test_complete_with_vector(tmp_path, flt, nlabels):
    import _zones
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterReader, RasterWriter, VectorReader
    from malstroem_amd.objects import rings_from_features
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(fx["dtm"])
    (tmp_path / "plain").mkdir()
    (tmp_path / "vector").mkdir()
    r0 = process_all(src, str(tmp_path / "plain"), [10, 100], filter=flt)
    r1 = process_all(src, str(tmp_path / "vector"), [10, 100], filter=flt, vector=True)
    assert r1["nlabels"] == nlabels and "bluespots_vector" not in r0
    d0, d1 = tmp_path / "plain", tmp_path / "vector"
    names0 = sorted(str(f.relative_to(d0)) for f in d0.rglob("*") if f.is_file())
    names1 = sorted(str(f.relative_to(d1)) for f in d1.rglob("*") if f.is_file())
    assert sorted(n for n in names1 if n not in names0) == ["vector/bluespots.geojson", "vector/watersheds.geojson"] and len(names0) >= 9
    for n in names0:
        assert (d0 / n).read_bytes() == (d1 / n).read_bytes(), n
    for key, tif in (("bluespots_vector", "bluespots.tif"), ("watersheds_vector", "watersheds.tif")):
        feats = VectorReader(r1[key]).read_geojson_features()
        raster = RasterReader(str(d1 / tif)).read()
        assert len(feats) == nlabels and [f["properties"]["bspot_id"] for f in feats] == list(range(1, nlabels + 1))
        assert all(f["geometry"]["type"] == "Polygon" for f in feats)
        xy, off, zone, nzone = rings_from_features(feats, gt)
        assert _zones.rasterize(raster.shape, xy, off, zone, nzone).tobytes() == np.ascontiguousarray(raster, dtype=np.int32).tobytes()


def test_vectorize_labels_and_the_file_form(tmp_path):
    """the reference's entry point: a label raster file, read through io.RasterReader, to features"""
    from malstroem_amd import vector
    from malstroem_amd.io import RasterWriter
    fx = fixtures()
    lab = np.ascontiguousarray(fx["labelled"], dtype=np.int32)
    gt = tuple(float(v) for v in fx["geotransform"])
    want = vector.features_from_rings(*P.polygonize(lab), gt, "spot")
    assert vector.vectorize_labels(lab, gt, "spot") == want and len(want) == 104
    path = str(tmp_path / "labelled.tif")
    RasterWriter(path, gt, None, 0).write(lab)
    gen = vector.vectorize_labels_file(path, id_attribute="spot")
    assert iter(gen) is gen and list(gen) == want
    assert [f["properties"]["bspot_id"] for f in vector.vectorize_labels_file(path)] == [f["id"] for f in want]
    # a uint8 raster is a label raster too; a float raster is not
    small = str(tmp_path / "small.tif")
    RasterWriter(small, gt, None).write((lab % 7).astype(np.uint8))
    assert list(vector.vectorize_labels_file(small)) == vector.features_from_rings(*P.polygonize(lab % 7), gt)
    floats = str(tmp_path / "floats.tif")
    RasterWriter(floats, gt, None).write(fx["depths"])
    with pytest.raises(ValueError, match="integers"):
        next(vector.vectorize_labels_file(floats))
