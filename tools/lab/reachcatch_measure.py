"""DESIGN.md 17, "Measured": HydroPipeline.reach_catchments(1000) on the 16384^2 fBm DEM of the bench, after the chain, three calls
by the host clock; the yardstick in the same process on the same context is flow_paths(1000, True) plus hand(1000) -- the new call
does the work of the first plus the tile and jump passes of the second.  Then three calls of inundate() at a uniform stage next to
the time mhip_copy_bandwidth gives for its 12 B/cell.  Also: the reaches, the assigned cells, the largest catchment, the wet cells.
`python tools/lab/reachcatch_measure.py out.json [size]`; under `rocprofv3 --kernel-trace --stats` the kernels' device time comes
from tools/kernel_stats.py."""
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


def timed(fn, reps=3):
    ms = []
    for _ in range(reps):
        t = time.perf_counter(); r = fn(); ms.append((time.perf_counter() - t) * 1e3)
    return ms, r


rec = dict(size=N)
with HydroPipeline((N, N)) as p:
    p.upload("dem", dem)
    del dem
    p.run("fill", "noflat", "flowdir", "accum", "label")
    rec["nlabels"] = p.apply_keep(None)
    p.run("watershed", "pourpoints")
    p.sync()
    rec["copy_bandwidth_gbs"] = HydroPipeline.copy_bandwidth()
    for stop in (True, False):
        r = {}
        r["flow_paths_ms"], fp = timed(lambda: p.flow_paths(1000, stop))
        r["hand_ms"], r["undrained"] = timed(lambda: p.hand(1000, stop_at_bluespots=stop))
        r["reach_catchments_ms"], rc = timed(lambda: p.reach_catchments(1000, stop))
        nreach = len(rc[2])
        r.update(reaches=nreach, vertices=len(rc[0]), unresolved=rc[3], assigned=rc[4])
        assert nreach == len(fp[2]) and np.array_equal(rc[0], fp[0])
        yard = min(r["flow_paths_ms"]) + min(r["hand_ms"])
        r["yardsticks_fastest_ms"] = yard
        r["pass_8B_ms"] = 8.0 * N * N / (rec["copy_bandwidth_gbs"] * 1e6)
        r["ratio_fastest"] = min(r["reach_catchments_ms"]) / yard
        stage = np.full(nreach + 1, 0.5, np.float32)
        r["inundate_ms"], zrec = timed(lambda: p.inundate(stage))
        r["inundate_floor_12B_ms"] = 12.0 * N * N / (rec["copy_bandwidth_gbs"] * 1e6)
        r.update(largest_catchment=int(zrec["cells"][1:].max(initial=0)), wet_cells=int(zrec["pos"][1:].sum()),
                 deepest=float(zrec["vmax"][1:].max(initial=0)))
        assert int(zrec["cells"][1:].sum()) == rc[4]
        rec["bluespots" if stop else "streams_only"] = r
        print(stop, json.dumps(r), flush=True)
    # algorithmic bytes a cell of the part that is new: reach cell pass 1 (class byte) in, 4 out; tile pass 1 + 8 [+ 4] in, 8 out; final
    # pass 8 scratch + 4 gathered in, 4 out; inundate 4 + 4 in, 4 gathered from a table that stays in cache, 4 out; its records 8 in
    rec["bytes_per_cell"] = dict(reachcell=5, tile_with_labels=21, tile_without_labels=17, final=16, inundate=12, inundate_records=8)
with open(out, "w") as fh:
    json.dump(rec, fh, indent=1)
print(json.dumps(rec))
