"""DESIGN.md 19, "Measured": HydroPipeline.sea_flood() on the 16384^2 fBm DEM of the bench, the sources the left raster column at the
DEM's 2nd percentile, max_level at its 10th, 30th and 100th percentile: three calls each by the host clock with the pool warm, with
the rounds, visits and re-checks of the last one, and the series pass for 16 levels; the copy rate of the process beside them.
`python tools/lab/seaflood_measure.py out.json [size]`.  The yardstick is the plain-fill stage with the iterative engine on the same
DEM -- the same operator with the raster border as its sources: `MHIP_DEVELOPER=1 MHIP_FILL=iterative python
tools/lab/seaflood_measure.py out.json [size] fill`, a process of its own (the engine is chosen once per process)."""
import json, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import bench
from malstroem_amd.pipeline import HydroPipeline

out = sys.argv[1]
N = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
mode = sys.argv[3] if len(sys.argv) > 3 else "sea"
dem = bench.fbm(N, 2.0, 42)


def timed(fn, reps=3):
    ms = []
    for _ in range(reps):
        t = time.perf_counter(); r = fn(); ms.append((time.perf_counter() - t) * 1e3)
    return ms, r


rec = dict(size=N, mode=mode, tiles=((N + 63) // 64) ** 2)
with HydroPipeline((N, N)) as p:
    p.upload("dem", dem)
    if mode == "fill":
        del dem
        ms = []
        for _ in range(4):      # (the first one warms the pool)
            p.upload_rows("dem", N - 1, p.download_rows("dem", N - 1, 1))      # a write of the DEM: the stage runs again
            p.run("fill"); p.sync()
            ms.append(p.stage_ms("fill"))
        rec.update(fill_stage_ms=ms[1:], fill_algorithm=p.get_int("fill_algorithm"), fill_rounds=p.get_int("fill_rounds"), fill_visits=p.get_int("fill_visits"),
                   fill_tiles=p.get_int("fill_tiles"))
    else:
        pct = {q: float(np.percentile(dem[::8, ::8], q)) for q in (2, 10, 30, 100)}
        pct[100] = float(dem.max())
        stage = np.full((N, N), np.nan, np.float32)
        stage[:, 0] = pct[2]
        del dem
        rec["percentiles"] = pct
        p.sea_flood(stage, pct[10])      # (warms the pool)
        for q in (10, 30, 100):
            ms, reached = timed(lambda: p.sea_flood(stage, pct[q]))
            r = dict(ms=ms, reached=reached, rounds=p.get_int("seaflood_rounds"), visits=p.get_int("seaflood_visits"), rechecks=p.get_int("seaflood_rechecks"))
            levels = np.linspace(pct[2], pct[q], 17)[1:]
            r["series16_ms"], s = timed(lambda: p.sea_levels(levels))
            r["series_wet_cells_last"] = int(s["wet_cells"][-1])
            r["depths_ms"], _ = timed(lambda: p.sea_depths(levels[-1]))
            r["classes_ms"], _ = timed(lambda: p.sea_classes(levels))
            rec["max_level_p%d" % q] = r
        # algorithmic bytes a cell.  prepare: 4 (DEM) + 4 (stage) in, 4 + 4 out; a visit: 4 (C) + 4 (L) in, 4 out where it moved; the proof:
        # 4 (L) + 4 (DEM) + 4 (stage) in, 4 out; series: 4 + 4 in
        rec["bytes_per_cell"] = dict(prepare=16, visit=12, proof=16, series=8)
        rec["copy_bandwidth_gbs"] = HydroPipeline.copy_bandwidth()
with open(out, "w") as fh:
    json.dump(rec, fh, indent=1)
print(json.dumps(rec))
