"""DESIGN.md 12, "Measured": burn 100 000 random lines of 2 to 200 cells, half lower (sampled ends, 8-connected) and half raise (2 m
above the terrain at their first vertex, 4-connected), into the 16384^2 fBm DEM of the bench; host-clock time of mhip_ctx_burn_lines
with a warm pool, and the yardstick in the same process: download_rows + upload_rows of the whole DEM.  Also compares a 2048^2 window
of the adapted raster with the model (tests/_burn.py).  `python tools/lab/burn_measure.py out.json [size]`; under `rocprofv3
--kernel-trace --stats` the kernels' device time comes from tools/kernel_stats.py."""
import ctypes, json, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import bench, _burn
from malstroem_amd import _lib
from malstroem_amd.pipeline import HydroPipeline
from malstroem_amd.adaptations import check_lines

N = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
out = sys.argv[1]
dem = bench.fbm(N, 2.0, 42)
rng = np.random.default_rng(7)
nl = 100000
L = rng.integers(2, 201, nl)
r0 = rng.integers(0, N, nl); c0 = rng.integers(0, N, nl)
ang = rng.random(nl) * 2 * np.pi
dr = np.rint(np.sin(ang) * (L - 1)).astype(np.int64); dc = np.rint(np.cos(ang) * (L - 1)).astype(np.int64)
big = np.maximum(np.abs(dr), np.abs(dc)); scale = (L - 1) / np.maximum(big, 1)
dr = np.rint(dr * scale).astype(np.int64); dc = np.rint(dc * scale).astype(np.int64)
lines = np.zeros(nl, _lib.BURN_LINE_DTYPE); segs = np.zeros(nl, _lib.BURN_SEGMENT_DTYPE)
segs["r0"], segs["c0"], segs["r1"], segs["c1"], segs["line"] = r0, c0, r0 + dr, c0 + dc, np.arange(nl)
lines["ntotal"] = np.maximum(np.abs(dr), np.abs(dc))
raise_ = np.arange(nl) % 2 == 1
lines["flags"] = np.where(raise_, 3, 0)
lines["z0"] = np.where(raise_, dem[r0, c0].astype(np.float64) + 2.0, np.nan)
lines["z1"] = lines["z0"]
lines, segs = check_lines(lines, segs)
res = np.zeros(nl, _lib.BURN_RESULT_DTYPE)
rec = dict(size=N, lines=nl, steps=int(lines["ntotal"].sum() + nl), burn_call_ms=[], method_ms=[], yardstick_ms=[], yardstick_parts_ms=[])
with HydroPipeline((N, N)) as p:
    for rep in range(4):
        p.upload("dem", dem)
        t = time.perf_counter()
        _lib.call("mhip_ctx_burn_lines", p._ctx, _lib.i64(nl), _lib.ptr(segs), _lib.i64(nl), _lib.ptr(lines), ctypes.c_double(np.nan), _lib.ptr(res))
        rec["burn_call_ms"].append((time.perf_counter() - t) * 1e3)
    rec["cells"] = int(res["cells"].sum()); rec["status_counts"] = np.bincount(res["status"], minlength=3).tolist()
    adapted = p.download("dem")
    rec["cells_changed"] = int(np.sum(adapted != dem))
    for rep in range(2):
        p.upload("dem", dem)
        t = time.perf_counter(); p.burn_lines(lines, segs); rec["method_ms"].append((time.perf_counter() - t) * 1e3)
    for rep in range(3):
        t = time.perf_counter(); a = p.download_rows("dem", 0, N); t1 = time.perf_counter(); p.upload_rows("dem", 0, a); t2 = time.perf_counter()
        rec["yardstick_ms"].append((t2 - t) * 1e3); rec["yardstick_parts_ms"].append([(t1 - t) * 1e3, (t2 - t1) * 1e3])
    rec["copy_bandwidth_gbs"] = HydroPipeline.copy_bandwidth()
# the adapted raster against the model on a window the lines of which are all taken along
w = 2048
inwin = np.flatnonzero((np.minimum(segs["r0"], segs["r1"]) < w + 0) & (np.minimum(segs["c0"], segs["c1"]) < w + 0))
sel_l, sel_s = lines[inwin], segs[inwin].copy(); sel_s["line"] = np.arange(len(inwin))
# (levels sampled at vertices outside the window would differ: the model runs on the whole rows / columns the lines reach)
ext = int(max(sel_s["r0"].max(), sel_s["r1"].max(), sel_s["c0"].max(), sel_s["c1"].max())) + 1
ext = min(N, max(ext, w))
want, wres = _burn.burn(dem[:ext, :ext].copy(), sel_l, sel_s)
rec["model_window"] = dict(lines=int(len(inwin)), window=w, equal=bool(want[:w, :w].tobytes() == adapted[:w, :w].tobytes()),
                           cells_equal=bool(np.array_equal(wres["cells"][wres["status"] == 0], res["cells"][inwin][wres["status"] == 0])))
json.dump(rec, open(out, "w"), indent=1)
print(json.dumps(rec))
