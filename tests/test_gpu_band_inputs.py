"""GPU: the row-band path (HipBand contexts driven by threads over the in-process ThreadComm on one MI355X) on inputs the chain
never produces -- tests/_band_cases.py: hard masks through the labelling, its statistics and the filter; flow cycles, interior
sinks, inward edges and codes above 8 through the band accumulation, watersheds, watershed counts and the stream walk; records of
labels that are no components.  Everything against the oracle on the undivided raster, bit for bit (label sums by the rule of
_cases.assert_label_sums).  tests/test_band_inputs_cpu.py runs the same scenarios on the CPU stand-in."""
import pytest

import _band_cases as bc

pytestmark = pytest.mark.gpu

LABEL_CASES = [(shape, n, a) for shape, n in bc.LABEL_SHAPES for a in bc.align_choices(shape[0], n)]
FLOW_CASES = [(name, n, a) for name, f in bc.flow_fields_cached().items() for n, a in f["bands"]]


@pytest.mark.parametrize("shape,nbands,align", LABEL_CASES, ids=["%dx%d-%d-%s" % (s[0], s[1], n, "aligned" if a else "equal") for s, n, a in LABEL_CASES])
def test_band_labelling_statistics_and_filter_on_hard_masks(shape, nbands, align):
    bc.run_labelling(shape, nbands, align, None)


@pytest.mark.parametrize("name,nbands,align", FLOW_CASES, ids=["%s-%d-%s" % (f, n, "aligned" if a else "equal") for f, n, a in FLOW_CASES])
def test_band_accumulation_watersheds_and_stream_walk_on_uploaded_fields(name, nbands, align):
    """on acyclic fields every band's second accumulation pass must be the delta over the boundary pass's graph (accum_algorithm 1);
    where a flow cycle feeds a seam a band may take the full pass"""
    bc.run_flow_field(name, nbands, align, None, hip_engines=True)


@pytest.mark.parametrize("nbands", bc.RECORD_BANDS)
@pytest.mark.parametrize("raster", ["tables", "rects", "dominant"])
def test_band_records_of_labels_that_are_no_components(raster, nbands):
    bc.run_records(raster, nbands, None)


def test_a_walker_on_a_cycle_across_a_seam_is_cut_after_one_visit_per_seam_cell():
    bc.run_trace_cut(None)
