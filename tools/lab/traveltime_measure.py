"""DESIGN.md 18, "Measured": HydroPipeline.travel_time() on the 16384^2 fBm DEM of the bench, after the chain, pool warm, three calls
each by the host clock -- with the defaults (one class), with two classes (ACCUM read), with a time-area table; the yardsticks in the
same process on the same context are HydroPipeline.flow_distance() (with records) and the watershed stage, with the copy and read
rates of the process beside them.  `python tools/lab/traveltime_measure.py out.json [size]`; under `rocprofv3 --kernel-trace --stats`
the kernels' device time comes from tools/kernel_stats.py."""
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
    rec["watershed_stage_ms"] = p.stage_ms("watershed")
    p.travel_time(0.4)      # (warms the pool)
    rec["flow_distance_ms"], rec["flow_distance_unresolved"] = timed(lambda: p.flow_distance(0.4))
    rec["travel_time_ms"], rec["unresolved"] = timed(lambda: p.travel_time(0.4))
    rec["saturated"] = p.get_int("travel_time_saturated")
    tc = p.travel_time_records()["value"]
    rec["tc_max_s"], rec["tc_median_s"] = float(tc[1:].max()), float(np.median(tc[1:]))
    rec["travel_time_two_classes_ms"], _ = timed(lambda: p.travel_time(0.4, channel_threshold=1000.0, k_channel=6.0))
    rec["travel_time_table_ms"], _ = timed(lambda: p.travel_time(0.4, bins=(64, 60.0)))
    table = p.time_area()
    rec["table_cells"] = int(table.sum())
    rec["table_last_bin_cells"] = int(table[:, -1].sum())
    rec["flow_distance_after_ms"], _ = timed(lambda: p.flow_distance(0.4))
    rec["ratio_fastest"] = min(rec["travel_time_ms"]) / min(rec["flow_distance_ms"])
    # algorithmic bytes a cell.  cost pass: 1 (FLOWDIR) + 4 (FILLED) [+ 8 ACCUM] in, 4 out; tile pass: 1 + 4 (LABELS) + 4 (cost) in, 8
    # scratch out; final pass with records: 8 scratch + 4 gathered label in, 4 out; head pass: 8 + 4 in
    rec["bytes_per_cell"] = dict(cost_one_class=9, cost_two_classes=17, tile=17, final_rec=16, head=12, flow_distance_tile=13)
    rec["copy_bandwidth_gbs"] = HydroPipeline.copy_bandwidth()
    rec["read_bandwidth_gbs"] = HydroPipeline.read_bandwidth()
with open(out, "w") as fh:
    json.dump(rec, fh, indent=1)
print(json.dumps(rec))
