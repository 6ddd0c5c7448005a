"""CPU: the address arithmetic of the fused first visit (csrc/handover_addr.hpp, used by ng_handover_kernel) walked on the host by
tools/handover_addr_check.cpp -- every window of every shape the GPU tests use: loads inside the raster, level-table indices inside
the table and equal to the flood's own, border cells recognised, every cell stored exactly once.  Built with the host compiler,
under AddressSanitizer + UBSan where the compiler has them (a stand-alone program: nothing is preloaded)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cc)
        if path:
            return path
    return None


@pytest.mark.timeout(300)
def test_every_index_of_the_fused_first_visit_lies_inside_its_array(tmp_path):
    cc = _compiler()
    assert cc, "no host C++ compiler"
    src, inc, exe = ROOT / "tools" / "handover_addr_check.cpp", ROOT / "malstroem_amd" / "csrc", tmp_path / "handover_addr_check"
    base = [cc, "-std=c++17", "-O1", "-g", "-I", str(inc), str(src), "-o", str(exe)]
    r = subprocess.run(base[:4] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + base[4:], capture_output=True, text=True)
    if r.returncode != 0:       # a compiler without the sanitizers' run-time libraries: the assertions alone
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "assertions hold" in run.stdout
