"""GPU: the transfers of a resident context through `HydroPipeline` and `HipBand` -- whole rasters, row windows and the streaming
writers move the same bytes to the same rows for every element size, on an undivided context and on a band with both halo rows; the
two forms of the halo-row store agree; the flow-distance raster by rows is the raster.  Shapes: 5 x 7 (a width that is no multiple of
four; windows of 1 and of 2 rows, the last of these partial) and a band of 2 rows out of 6."""
import numpy as np
import pytest

import _flowdist as F
from _cases import assert_same_bits

pytestmark = pytest.mark.gpu

H, W = 5, 7
ELEMENT_SIZES = ["flowdir", "dem", "accum"]      # 1, 4 and 8 bytes a cell


def raster(name, shape, seed=0):
    """distinct values in every cell, none of them 0 and none the byte pattern of an unwritten block"""
    from malstroem_amd._lib import RASTER_DTYPE
    from malstroem_amd.pipeline import RASTERS
    n = shape[0] * shape[1]
    return (np.arange(1, n + 1).reshape(shape) + 40 * seed).astype(RASTER_DTYPE[RASTERS[name]])


def windows(n, step):
    return [(r, min(step, n - r)) for r in range(0, n, step)]


class Recorder(object):
    """a writer of `download_to`: keeps what it is handed"""

    def __init__(self):
        self.opened, self.closed, self.got = None, False, []

    def open(self, shape, dtype):
        self.opened = (tuple(shape), np.dtype(dtype))

    def write_window(self, row0, array):
        self.got.append((row0, np.array(array)))

    def close(self):
        self.closed = True


class WholeWriter(object):
    """a writer without windows: the fall-back of `download_to`"""

    def write(self, array):
        self.array = np.array(array)


@pytest.fixture()
def pipe():
    from malstroem_amd.pipeline import HydroPipeline
    with HydroPipeline((H, W)) as p:
        yield p


def check_every_way_out(p, name, a, step):
    assert_same_bits(p.download(name), a, "%s download" % name)
    rows = [p.download_rows(name, r, n) for r, n in windows(H, step)]
    assert [x.shape for x in rows] == [(n, W) for _, n in windows(H, step)]
    assert_same_bits(np.concatenate(rows), a, "%s download_rows by %d" % (name, step))
    rec = Recorder()
    p.download_to(name, rec, max_rows=2)
    assert rec.opened == ((H, W), a.dtype) and rec.closed
    assert [(r, x.shape[0]) for r, x in rec.got] == windows(H, 2)
    assert_same_bits(np.concatenate([x for _, x in rec.got]), a, "%s download_to" % name)
    whole = WholeWriter()
    p.download_to(name, whole, max_rows=2)
    assert_same_bits(whole.array, a, "%s download_to a writer without windows" % name)


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("name", ELEMENT_SIZES)
def test_upload_rows_then_every_way_out(pipe, name, step):
    a = raster(name, (H, W))
    for r, n in windows(H, step):
        pipe.upload_rows(name, r, a[r:r + n])
    check_every_way_out(pipe, name, a, step)


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("name", ELEMENT_SIZES)
def test_upload_then_every_way_out(pipe, name, step):
    a = raster(name, (H, W), seed=1)
    pipe.upload(name, a)
    check_every_way_out(pipe, name, a, step)


def test_labels_are_absent_until_the_last_window(pipe):
    lab = np.zeros((H, W), np.int32)
    lab[1, 2:4], lab[4, 5] = 3, 9
    pipe.upload("labels", np.ones((H, W), np.int32))      # present before the first window ...
    pipe.upload_rows("labels", 0, lab[:3])
    with pytest.raises(ValueError, match="has not been computed or uploaded"):      # ... absent after it
        pipe.download("labels")
    with pytest.raises(ValueError, match="has not been computed or uploaded"):
        pipe.download_rows("labels", 0, 1)
    pipe.upload_rows("labels", 3, lab[3:])
    assert_same_bits(pipe.download("labels"), lab, "labels after the last window")
    assert pipe.get_int("nlabels") == 9 == int(lab.max())


def test_window_bounds(pipe):
    pipe.upload("dem", raster("dem", (H, W)))
    for row0, nrows in [(4, 2), (0, H + 1), (0, 0), (2, 0), (-1, 1), (-1, 0)]:
        with pytest.raises(ValueError, match="ctx_download_rows"):
            pipe.download_rows("dem", row0, nrows)
    with pytest.raises(ValueError, match="ctx_upload_rows"):
        pipe.upload_rows("dem", 4, np.zeros((2, W), np.float32))
    assert_same_bits(pipe.download_rows("dem", 4, 1), raster("dem", (H, W))[4:], "the last row still comes out")


# ---- a band with a halo row on either side: rows [2, 4) of 6 -------------------------------------------------------------------
def new_band(name, band):
    from malstroem_amd.distributed import HipBand
    b = HipBand(6, W, 2, 2)
    assert b.shape == (2, W) and (b.W, b.nrows, b.row0, b.H_global) == (W, 2, 2, 6)
    b.zero_raster(name)      # the halo rows hold zeros, whatever the block held before
    b.upload(name, band)
    return b


@pytest.mark.parametrize("name", ELEMENT_SIZES)
def test_band_transfers_skip_the_halo_rows(name):
    band = raster(name, (2, W))
    top, bottom = raster(name, (1, W), seed=1)[0], raster(name, (1, W), seed=2)[0]
    b = new_band(name, band)
    try:
        assert_same_bits(b.download(name), band, "band download")
        assert_same_bits(b.download_rows(name, 0, 2), band, "band download_rows")
        assert_same_bits(b.download_rows(name, 1, 1), band[1:], "band download_rows of the last row")
        empty = b.download_rows(name, 0, 0)
        assert empty.shape == (0, W) and empty.dtype == band.dtype
        for row0, nrows in [(1, 2), (-1, 1)]:
            with pytest.raises(ValueError, match="ctx_download_rows"):
                b.download_rows(name, row0, nrows)
        assert_same_bits(b.get_edge_row(name, 0), band[0], "first owned row")
        assert_same_bits(b.get_edge_row(name, 1), band[1], "last owned row")
        first, last = b.get_edge_rows(name)
        assert_same_bits(first, band[0], "get_edge_rows first")
        assert_same_bits(last, band[1], "get_edge_rows last")
        assert b.get_edge_rows(name, first=False)[0] is None and b.get_edge_rows(name, last=False)[1] is None
        assert_same_bits(b.get_edge_rows(name, first=False)[1], band[1], "get_edge_rows last alone")
        assert b.set_halo_rows(name, top, bottom) == (True, True)
        assert_same_bits(b.get_edge_row(name, 2), top, "halo row above")
        assert_same_bits(b.get_edge_row(name, 3), bottom, "halo row below")
        assert b.set_halo_rows(name, top, bottom) == (False, False)
        assert_same_bits(b.download(name), band, "the owned rows after the halo rows were stored")
        with pytest.raises(ValueError, match="band raster must be"):
            b.upload(name, raster(name, (4, W)))
    finally:
        b.close()


@pytest.mark.parametrize("name", ELEMENT_SIZES)
def test_set_halo_row_agrees_with_set_halo_rows(name):
    band = raster(name, (2, W))
    top, bottom = raster(name, (1, W), seed=1)[0], raster(name, (1, W), seed=2)[0]
    other = top.copy()
    other[W - 1] += 1      # one cell, the last of the row
    two, one = new_band(name, band), new_band(name, band)
    try:
        for t, bt in [(top, bottom), (top, bottom), (other, bottom), (other, top)]:
            want = two.set_halo_rows(name, t, bt)
            assert (one.set_halo_row(name, 0, t), one.set_halo_row(name, 1, bt)) == want
            for side in (2, 3):
                assert_same_bits(one.get_edge_row(name, side), two.get_edge_row(name, side), "halo row, side %d" % side)
            assert_same_bits(one.get_edge_row(name, 2), t, "halo row above")
            assert_same_bits(one.get_edge_row(name, 3), bt, "halo row below")
        assert want == (False, True)
        assert two.set_halo_rows(name, None, bottom) == (False, True)      # one side alone, as set_halo_row passes it on
        assert_same_bits(two.get_edge_row(name, 2), other, "the side that was not given")
        assert_same_bits(one.download(name), band, "the owned rows")
    finally:
        two.close()
        one.close()


# ---- the flow-distance raster, which is no member of RASTERS ---------------------------------------------------------------------
def test_flow_distance_by_rows_is_the_raster(pipe):
    rng = np.random.default_rng(57)
    fd = rng.integers(0, 9, size=(H, W)).astype(np.uint8)
    lab = np.where(rng.random((H, W)) < 0.15, rng.integers(1, 5, size=(H, W)), 0).astype(np.int32)
    m = F.flow_distance(fd, lab, 1.0)
    pipe.upload("flowdir", fd)
    pipe.upload("labels", lab)
    assert pipe.flow_distance(1.0) == m["unresolved"]
    whole = pipe.download_flow_distance()
    assert_same_bits(whole, m["raster"], "flow distance against the model")
    rows = [pipe.download_flow_distance_rows(r, 1) for r in range(H)]
    assert_same_bits(np.concatenate(rows), whole, "flow distance a row at a time")
    rec = Recorder()
    pipe.download_flow_distance_to(rec, max_rows=2)
    assert rec.opened == ((H, W), np.dtype(np.float32)) and rec.closed and [(r, x.shape[0]) for r, x in rec.got] == windows(H, 2)
    assert_same_bits(np.concatenate([x for _, x in rec.got]), whole, "flow distance through a writer")
    for row0, nrows in [(4, 2), (0, 0), (-1, 1)]:
        with pytest.raises(ValueError, match="ctx_flow_distance_rows"):
            pipe.download_flow_distance_rows(row0, nrows)
