"""DESIGN.md 15, "Measured": the flow paths of the 16384^2 fBm DEM of the bench, after the chain, at thresholds of 100, 1 000 and 10 000
cells.  Per threshold: reaches, vertices, stream cells (the cells of all paths less the appended ends), the longest reach in cells,
the Strahler orders, and the host-clock time of HydroPipeline.flow_paths to the arrays on the host (three calls); the yardstick in
the same process is download_to of MHIP_R_ACCUM into a writer that keeps nothing.  `python tools/lab/flowpaths_measure.py out.json
[size]`; under `rocprofv3 --kernel-trace --stats` the kernels' device time comes from tools/kernel_stats.py."""
import json, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import bench
from malstroem_amd.pipeline import HydroPipeline

out = sys.argv[1]
N = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
dem = bench.fbm(N, 2.0, 42)


class Sink(object):      # a raster writer that keeps nothing: the download alone
    def open(self, shape, dtype): pass
    def write_window(self, row0, data): pass
    def close(self): pass


def timed(fn, reps=3):
    ms = []
    for _ in range(reps):
        t = time.perf_counter(); r = fn(); ms.append((time.perf_counter() - t) * 1e3)
    return ms, r


rec = dict(size=N)
with HydroPipeline((N, N)) as p:
    p.upload("dem", dem)
    p.run("fill", "noflat", "flowdir", "accum", "label")
    rec["nlabels"] = p.apply_keep(None)
    p.run("watershed", "pourpoints")
    p.sync()
    rec["download_accum_ms"], _ = timed(lambda: p.download_to("accum", Sink()))
    for stop in (False, True):
        for thr in (100, 1000, 10000):
            r = {}
            r["flow_paths_ms"], (xy, off, reaches, unresolved) = timed(lambda: p.flow_paths(thr, stop_at_bluespots=stop))
            steps = reaches["n_orth"].astype(np.int64) + reaches["n_diag"]
            cells = steps + 1 - np.isin(reaches["end_kind"], (0, 3))
            r.update(reaches=int(len(reaches)), vertices=int(len(xy)), stream_cells=int(cells.sum()), longest_reach_cells=int(cells.max(initial=0)),
                     unresolved=int(unresolved), max_order=int(reaches["order"].max(initial=0)), order_0=int((reaches["order"] == 0).sum()),
                     end_kinds=np.bincount(reaches["end_kind"], minlength=5).tolist(),
                     result_bytes=int(xy.nbytes + off.nbytes + reaches.nbytes))
            r["ratio_fastest"] = min(r["flow_paths_ms"]) / min(rec["download_accum_ms"])
            r["ratio_slowest"] = max(r["flow_paths_ms"]) / max(rec["download_accum_ms"])
            rec["%s%d" % ("stop_" if stop else "t", thr)] = r
            print(stop, thr, json.dumps(r), flush=True)
    rec["download_accum_after_ms"], _ = timed(lambda: p.download_to("accum", Sink()))
    rec["copy_bandwidth_gbs"] = HydroPipeline.copy_bandwidth()
with open(out, "w") as fh:
    json.dump(rec, fh, indent=1)
print(json.dumps(rec))
