"""CPU: what a write of a resident raster does to every held product, as csrc/held_rules.hpp says it (printed by
tools/held_rules_check.cpp: the direct rule, then the cascade), against the table of DESIGN.md 4.5a -- tests/_ctx_shadow.py for the
products the shadow knows, stated here for the sea flood's three, which it does not.  Built with the host compiler, under
AddressSanitizer + UBSan where the compiler has them (a stand-alone program: nothing is preloaded)."""
import shutil
import subprocess
from pathlib import Path

import pytest

import _ctx_shadow as S

ROOT = Path(__file__).resolve().parents[1]
SHADOW = ("wet_at", "flow_distance", "travel_time", "hand", "reach_catchments", "inundation", "zones")      # the shadow's names are the program's
SEA = ("sea_level", "sea_depth", "sea_class")
VARIANTS = [(s, t) for s in ("filled", "dem") for t in (True, False)]


def _compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cc)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def says(tmp_path_factory):
    """(raster written, product, source, labels read) -> 'dropped' / 'survives', and ('call', product, other product) -> the same:
    every line the program printed"""
    cc = _compiler()
    assert cc, "no host C++ compiler"
    src, inc, exe = ROOT / "tools" / "held_rules_check.cpp", ROOT / "malstroem_amd" / "csrc", tmp_path_factory.mktemp("held") / "held_rules_check"
    base = [cc, "-std=c++17", "-O1", "-g", "-I", str(inc), str(src), "-o", str(exe)]
    r = subprocess.run(base[:4] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + base[4:], capture_output=True, text=True)
    if r.returncode != 0:       # a compiler without the sanitizers' run-time libraries: the plain build
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    out = {}
    for line in run.stdout.splitlines():
        writer, product, variant, verdict = line.split()
        assert verdict in ("dropped", "survives"), line
        if writer == "call":
            key = ("call", product, variant)
        else:
            source, labels = variant.split(":")
            assert labels in ("labels", "nolabels"), line
            key = (writer, product, source, labels == "labels")
        assert key not in out, line
        out[key] = verdict
    return out


def test_the_program_printed_every_product_and_the_test_has_a_row_for_each(says):
    writers, products = {k[0] for k in says} - {"call"}, {k[1] for k in says}
    assert products == set(SHADOW + SEA), products      # a product added to the header gets its expectation here
    assert writers == set(S.RASTERS) | {"ngdist"}, writers
    assert len(says) == len(writers) * len(products) * len(VARIANTS) + len(products) * (len(products) - 1)
    assert {res for res, v in S.columns()} >= set(SHADOW)


def test_every_cell_the_shadow_knows_is_the_headers(says):
    wrong = []
    for res, v in S.columns():
        if res not in SHADOW:      # (record sets and tables: validity bits of their own, no held product)
            continue
        for source, stop in VARIANTS:
            if v is not None and (v.get("source", source), v["stop"]) != (source, stop):
                continue      # (a result whose rule looks at no variant is asked under all four)
            for writer in S.UPLOADS:
                want = S.table_says(writer, res, v)
                if says[(writer, res, source, stop)] != want:
                    wrong.append((writer, S.column(res, v), source, stop, want))
    assert not wrong, wrong


def test_a_write_that_is_no_upload_of_the_shadow_drops_nothing(says):
    # NGDIST and FINALDEPTHS: no product is made from them (DESIGN 4.5a has no row for either)
    assert all(v == "survives" for k, v in says.items() if k[0] in ("ngdist", "finaldepths"))


def test_the_sea_flood_goes_with_the_dem_and_with_nothing_else(says):
    for key, verdict in says.items():
        if key[0] != "call" and key[1] in SEA:
            assert verdict == ("dropped" if key[0] == "dem" else "survives"), key


def test_what_goes_when_a_product_goes(says):
    """a drop for any reason, a new call of the product's own entry point included: the inundation goes with the hand and with the
    reach catchments (the shadow's GOES_WITH), the sea's depths and classes with its levels, and nothing else goes"""
    assert S.GOES_WITH == {"inundation": ("hand", "reach_catchments")}
    goes = {("hand", "inundation"), ("reach_catchments", "inundation"), ("sea_level", "sea_depth"), ("sea_level", "sea_class")}
    for key, verdict in says.items():
        if key[0] == "call":
            assert verdict == ("dropped" if key[1:] in goes else "survives"), key
