"""DESIGN.md 16, "Measured": HydroPipeline.hand(1000) on the 16384^2 fBm DEM of the bench, after the chain, with and without the
bluespots as drainage, three calls each by the host clock; the yardstick in the same process on the same context is
HydroPipeline.flow_distance() (the context's form of it, which also makes the per-label records).  Also: the undrained cells, and the
largest height and distance.  `python tools/lab/hand_measure.py out.json [size]`; under `rocprofv3 --kernel-trace --stats` the kernels'
device time comes from tools/kernel_stats.py."""
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
    rec["flow_distance_ms"], rec["flow_distance_unresolved"] = timed(lambda: p.flow_distance(1.0))
    for stop in (True, False):
        r = {}
        r["hand_ms"], r["undrained"] = timed(lambda: p.hand(1000, stop_at_bluespots=stop))
        r["ratio_fastest"] = min(r["hand_ms"]) / min(rec["flow_distance_ms"])
        r["ratio_slowest"] = max(r["hand_ms"]) / max(rec["flow_distance_ms"])
        hand_max = dist_max = 0.0
        for row0 in range(0, N, 2048):      # (windows: the host holds 2 x 64 MB at a time)
            n = min(2048, N - row0)
            h, d = p.download_hand_rows(row0, n), p.download_drain_distance_rows(row0, n)
            hand_max, dist_max = max(hand_max, float(h[d >= 0].max(initial=0))), max(dist_max, float(d.max(initial=0)))
        r.update(hand_max=hand_max, dist_max=dist_max)
        rec["bluespots" if stop else "streams_only"] = r
        print(stop, json.dumps(r), flush=True)
    rec["flow_distance_after_ms"], _ = timed(lambda: p.flow_distance(1.0))
    # algorithmic bytes a cell: tile pass 1 (FLOWDIR) + 8 (ACCUM) [+ 4 LABELS] in, 8 scratch out; final pass 8 scratch + 4 elevation + 4 gathered in, 4 + 4 out
    rec["bytes_per_cell"] = dict(hand_with_labels=45, hand_without_labels=41, flow_distance_raster=25)
    rec["copy_bandwidth_gbs"] = HydroPipeline.copy_bandwidth()
with open(out, "w") as fh:
    json.dump(rec, fh, indent=1)
print(json.dumps(rec))
