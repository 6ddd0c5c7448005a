"""CPU-only: the row-band protocol on inputs the chain never produces (tests/_band_cases.py) with the CPU stand-in backend
(tests/_cpu_band.CpuBand) over the in-process ThreadComm, against the oracle on the undivided raster, bit for bit.  The same
scenarios run on HipBand in tests/test_gpu_band_inputs.py."""
import numpy as np
import pytest

import _band_cases as bc
from _cpu_band import CpuBand

LABEL_CASES = [(shape, n, a) for shape, n in bc.LABEL_SHAPES for a in bc.align_choices(shape[0], n)]
FLOW_CASES = [(name, n, a) for name, f in bc.flow_fields_cached().items() for n, a in f["bands"]]


@pytest.mark.parametrize("shape,nbands,align", LABEL_CASES, ids=["%dx%d-%d-%s" % (s[0], s[1], n, "aligned" if a else "equal") for s, n, a in LABEL_CASES])
def test_band_labelling_statistics_and_filter_on_hard_masks(shape, nbands, align):
    bc.run_labelling(shape, nbands, align, CpuBand)


@pytest.mark.parametrize("name,nbands,align", FLOW_CASES, ids=["%s-%d-%s" % (f, n, "aligned" if a else "equal") for f, n, a in FLOW_CASES])
def test_band_accumulation_watersheds_and_stream_walk_on_uploaded_fields(name, nbands, align):
    bc.run_flow_field(name, nbands, align, CpuBand)


@pytest.mark.parametrize("nbands", bc.RECORD_BANDS)
@pytest.mark.parametrize("raster", ["tables", "rects", "dominant"])
def test_band_records_of_labels_that_are_no_components(raster, nbands):
    bc.run_records(raster, nbands, CpuBand)


def test_a_walker_on_a_cycle_across_a_seam_is_cut_after_one_visit_per_seam_cell():
    bc.run_trace_cut(CpuBand)


def test_the_scenarios_hold_what_they_claim():
    """the seams cut what the comments say they cut, and the hand-made field's rootless label is one"""
    import oracle
    fd, lab, _ = bc.handmade_field()
    ws = lab.copy()
    oracle.watersheds_from_labels(fd, ws, 0)
    assert ws[4, 1] == 0 and ws[3, 1] == 0 and ws[5, 1] == 7          # upstream of the rootless label: unassigned
    assert ws[3, 6] == 3 and ws[4, 6] == 3 and ws[2, 6] == 3
    for n in (2, 4, 5, 7):
        assert 6 in [r0 for r0, _ in bc.band_extents(12, n, False)]
    assert [r0 for r0, _ in bc.band_extents(320, 5, False)] == [0, 64, 128, 192, 256]
    assert [r0 for r0, _ in bc.band_extents(264, 4, True)] == [0, 63, 125, 187]
    assert [r0 for r0, _ in bc.band_extents(264, 7, False)] == [0, 38, 76, 114, 152, 190, 227]
    fields = bc.flow_fields_cached()
    cyc = fields["cycles-320x270"]["fd"]
    assert cyc[63, 10] == 4 and cyc[64, 10] == 0 and cyc[127, 191] == 3 and cyc[128, 192] == 7
    for shape, n in bc.LABEL_SHAPES:
        for a in bc.align_choices(shape[0], n):
            ext = bc.band_extents(shape[0], n, a)
            masks = bc.label_masks(shape[0], shape[1], ext)
            assert masks["u-shapes"].any() and masks["edge-singles"].any()
            # the arms of the first U are one component only through the neighbour band
            seam = ext[1][0]
            top = masks["u-shapes"][:seam]
            lab_top, _ = oracle.connected_components(top.astype(np.uint8))
            lab_all, _ = oracle.connected_components(masks["u-shapes"].astype(np.uint8))
            assert lab_top[seam - 1, 3] != lab_top[seam - 1, 9] and lab_all[seam - 1, 3] == lab_all[seam - 1, 9]
