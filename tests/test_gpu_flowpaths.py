"""GPU: the flow paths (csrc/flowpaths.hip, malstroem_amd/flowpaths.py) against their definition, the model
tests/_flowpaths.py, bit for bit: ``xy``, ``reach_offsets``, every field of the records and ``unresolved``; the context against the
stateless call; the handle's lifetime; the refusals; and ``complete`` with ``flowpaths=``.  Everything is exact: nothing here has a
tolerance."""
import ctypes

import numpy as np
import pytest

import _flowpaths as F
from _cases import assert_same_bits, fixtures

pytestmark = pytest.mark.gpu


def same(got, want, what=""):
    """a result of the library (xy, reach_offsets, records, unresolved) against a result of the model"""
    xy, off, rec, unresolved = got
    assert_same_bits(off, want["reach_offsets"], what + " reach_offsets")
    assert_same_bits(rec, want["records"], what + " records")
    assert_same_bits(xy, want["xy"], what + " xy")
    assert unresolved == want["unresolved"], (what, unresolved, want["unresolved"])


# ---- against the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", F.CASE_IDS)
def test_against_the_model(case_id):
    from malstroem_amd.flowpaths import extract
    fd, acc, thr, lab, _ = F.case(case_id)
    want = F.model(case_id)
    same(extract(fd, acc, thr, lab), want, case_id)
    name = case_id.split("-")[0]
    if name.startswith("random") and thr == 1:
        assert int(want["stream"].sum()) + int((acc == 0).sum()) == fd.size      # every cell is a stream cell, the cycles hold 0
    if name in ("meander", "zigzag") and thr in (8, 64):
        assert F.count_confluences(want) >= (1000 if thr == 8 else 100)
    if name == "serpentine":
        assert len(want["records"]) == 1 and len(want["chains"][0]) == (24960 if thr == 1 else 19961) and len(want["xy"]) > 300
    if name == "synthetic":
        assert want["unresolved"] > 0
    if name == "cycles":
        assert np.any(want["records"]["end_kind"] == F.BLUESPOT) and want["unresolved"] == 0


def test_algorithms_alias_and_an_empty_mask():
    from malstroem_amd.algorithms import flow
    fd, acc, thr, lab, _ = F.case("fixture_labels-500")
    same(flow.flow_paths(fd, acc, thr, lab), F.model("fixture_labels-500"), "alias")
    xy, off, rec, unresolved = flow.flow_paths(fd, acc, 1e9)
    assert xy.shape == (0, 2) and xy.dtype == np.int32 and off.tolist() == [0] and off.dtype == np.int64 and rec.shape == (0,) and unresolved == 0
    # a mask of nothing but a cycle that nothing flows into: no reach either
    two = np.array([[2, 6]], dtype=np.uint8)
    xy, off, rec, unresolved = flow.flow_paths(two, np.ones((1, 2)), 1)
    assert xy.shape == (0, 2) and off.tolist() == [0] and rec.shape == (0,) and unresolved == 2
    same((xy, off, rec, unresolved), F.flow_paths(two, np.ones((1, 2)), 1), "2-cycle")


# ---- on a context -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def uploaded():
    """the reference fixture's rasters uploaded into a context; -> (pipeline, flowdir, accum, labels), closed when the module is done"""
    from malstroem_amd.pipeline import HydroPipeline
    fd, acc, _, lab, _ = F.case("fixture_labels-50")
    p = HydroPipeline(fd.shape)
    p.upload("flowdir", fd)
    p.upload("accum", acc)
    p.upload("labels", lab)       # (uploaded labels are final)
    yield p, fd, acc, lab
    p.close()


@pytest.mark.parametrize("thr", [50, 500])
@pytest.mark.parametrize("stop", [False, True])
def test_the_context_equals_the_stateless_call(uploaded, thr, stop):
    from malstroem_amd.flowpaths import extract
    p, fd, acc, lab = uploaded
    got = p.flow_paths(thr, stop_at_bluespots=stop)
    want = F.model("%s-%d" % ("fixture_labels" if stop else "fixture", thr))
    same(got, want, "context")
    stateless = extract(fd, acc, thr, lab if stop else None)
    for g, s in zip(got[:3], stateless[:3]):
        assert_same_bits(g, s)
    assert got[3] == stateless[3] == 0 and len(got[2]) > 10
    if stop:
        assert np.any(got[2]["end_kind"] == F.BLUESPOT) and np.any(got[2]["from_label"] > 0)


def test_a_handle_outlives_a_second_run_and_its_context():
    from malstroem_amd import _lib
    from malstroem_amd.flowpaths import take_flowpaths
    from malstroem_amd.pipeline import HydroPipeline
    fd, acc, _, lab, _ = F.case("fixture_labels-50")
    p = HydroPipeline(fd.shape)
    try:
        p.upload("flowdir", fd)
        p.upload("accum", acc)
        handle = ctypes.c_void_p()
        _lib.call("mhip_ctx_flowpaths", p._ctx, ctypes.c_double(50.0), ctypes.c_int32(0), ctypes.byref(handle))
        assert handle
        # a second run on other rasters, then the context goes
        p.upload("accum", np.ascontiguousarray(acc[::-1]))
        p.upload("flowdir", np.ascontiguousarray(fd[:, ::-1]))
        other = p.flow_paths(500)
        assert len(other[2]) != len(F.model("fixture-50")["records"])
    finally:
        p.close()
    same(take_flowpaths(handle), F.model("fixture-50"), "kept handle")


def test_a_band_and_a_context_without_the_rasters_refuse():
    from malstroem_amd import _lib
    from malstroem_amd.distributed import HipBand
    from malstroem_amd.pipeline import HydroPipeline
    lib = _lib.load()
    with HydroPipeline((8, 9)) as p:
        p.upload("flowdir", np.full((8, 9), 2, dtype=np.uint8))
        handle = ctypes.c_void_p()
        # the return code itself: nothing crosses the boundary but the code
        assert lib.mhip_ctx_flowpaths(p._ctx, ctypes.c_double(1.0), ctypes.c_int32(0), ctypes.byref(handle)) == _lib.EINVAL and not handle
        with pytest.raises(ValueError, match="has not been computed"):      # no ACCUM
            p.flow_paths(1)
        p.upload("accum", np.ones((8, 9)))
        with pytest.raises(ValueError, match="has not been computed"):      # no LABELS
            p.flow_paths(1, stop_at_bluespots=True)
        assert len(p.flow_paths(1)[2]) == 8
        assert lib.mhip_ctx_flowpaths(p._ctx, ctypes.c_double(0.0), ctypes.c_int32(0), ctypes.byref(handle)) == _lib.EINVAL and not handle
    band = HipBand(64, 48, 0, 32, device=0, rank=0, size=2)
    try:
        band.upload("flowdir", np.full((32, 48), 2, dtype=np.uint8))
        band.upload("accum", np.ones((32, 48)))
        handle = ctypes.c_void_p()
        assert lib.mhip_ctx_flowpaths(band._ctx, ctypes.c_double(1.0), ctypes.c_int32(0), ctypes.byref(handle)) == _lib.EINVAL and not handle
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_flowpaths", band._ctx, ctypes.c_double(1.0), ctypes.c_int32(0), ctypes.byref(handle))
    finally:
        band.close()


def test_argument_errors():
    from malstroem_amd import _lib
    lib = _lib.load()
    fd, acc = np.full((40, 300), 2, dtype=np.uint8), np.ones((40, 300))
    lab = np.zeros((40, 300), dtype=np.int32)
    lab[33, 257] = -1

    def rc(labels, h, w, thr):
        handle = ctypes.c_void_p()
        code = lib.mhip_flowpaths_f64(_lib.ptr(fd), _lib.ptr(acc), _lib.ptr(labels) if labels is not None else None, _lib.i64(h), _lib.i64(w),
                                      ctypes.c_double(thr), ctypes.byref(handle))
        assert not handle
        return code
    assert rc(None, 40, 300, 0.0) == _lib.EINVAL and b"threshold" in lib.mhip_last_error()
    assert rc(None, 40, 300, float("nan")) == _lib.EINVAL and rc(None, 40, 300, float("inf")) == _lib.EINVAL and rc(None, 40, 300, 0.5) == _lib.EINVAL
    assert rc(lab, 40, 300, 1.0) == _lib.EINVAL and b"negative" in lib.mhip_last_error()      # (the `bad` word of the class kernel)
    assert rc(None, 0, 300, 1.0) == _lib.EINVAL and rc(None, 40, 0, 1.0) == _lib.EINVAL
    from malstroem_amd.flowpaths import extract
    with pytest.raises(ValueError, match="negative"):
        extract(fd, acc, 1, lab)


# ---- tools -----------------------------------------------------------------------------------------------------------------------------
def test_complete_with_flowpaths(tmp_path):
    from malstroem_amd.complete import process_all
    from malstroem_amd.flowpaths import features_from_reaches
    from malstroem_amd.io import RasterReader, RasterWriter, VectorReader
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(fx["dtm"])
    (tmp_path / "with").mkdir()
    (tmp_path / "plain").mkdir()
    r1 = process_all(src, str(tmp_path / "with"), [10, 100], accum=True, flowpaths=50)
    r0 = process_all(src, str(tmp_path / "plain"), [10, 100], accum=True)
    d0, d1 = tmp_path / "plain", tmp_path / "with"
    names0 = sorted(str(f.relative_to(d0)) for f in d0.rglob("*") if f.is_file())
    names1 = sorted(str(f.relative_to(d1)) for f in d1.rglob("*") if f.is_file())
    assert sorted(n for n in names1 if n not in names0) == ["vector/flowpaths.geojson"] and len(names0) >= 10 and "flowpaths" not in r0
    for n in names0:
        assert (d0 / n).read_bytes() == (d1 / n).read_bytes(), n
    # the layer has exactly the model's features, the model run on the rasters the same run wrote
    fd = np.ascontiguousarray(RasterReader(str(d1 / "flowdir.tif")).read(), dtype=np.uint8)
    acc = np.ascontiguousarray(RasterReader(str(d1 / "accum.tif")).read(), dtype=np.float64)
    lab = np.ascontiguousarray(RasterReader(str(d1 / "bluespots.tif")).read(), dtype=np.int32)
    m = F.flow_paths(fd, acc, 50, lab)
    want = features_from_reaches(m["xy"], m["reach_offsets"], m["records"], gt)
    got = VectorReader(r1["flowpaths"]).read_geojson_features()
    assert len(got) == len(want) > 50
    strip = lambda f: (f["geometry"], f["properties"])
    assert [strip(f) for f in got] == [strip(f) for f in want]
    assert {f["properties"]["end"] for f in got} >= {"confluence", "bluespot", "edge"} and max(f["properties"]["order"] for f in got) >= 2


def test_complete_computes_the_accumulation_for_the_flow_paths_alone(tmp_path):
    """accum=False: no accum.tif, every other file as without the argument (the pour points too), and the same layer"""
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterWriter
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(fx["dtm"])
    for name in ("with", "plain", "accum"):
        (tmp_path / name).mkdir()
    r1 = process_all(src, str(tmp_path / "with"), [10], flowpaths=50)
    process_all(src, str(tmp_path / "plain"), [10])
    r2 = process_all(src, str(tmp_path / "accum"), [10], accum=True, flowpaths=50)
    d0, d1 = tmp_path / "plain", tmp_path / "with"
    names0 = sorted(str(f.relative_to(d0)) for f in d0.rglob("*") if f.is_file())
    names1 = sorted(str(f.relative_to(d1)) for f in d1.rglob("*") if f.is_file())
    assert sorted(n for n in names1 if n not in names0) == ["vector/flowpaths.geojson"] and "accum.tif" not in names1
    for n in names0:
        assert (d0 / n).read_bytes() == (d1 / n).read_bytes(), n
    with open(r1["flowpaths"], "rb") as a, open(r2["flowpaths"], "rb") as b:
        assert a.read() == b.read()
