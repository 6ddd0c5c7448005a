"""DESIGN.md 20, "Measured": HydroPipeline.weighted_accumulation() alone on the 16384^2 fBm DEM of the bench after two runs of the
chain (the pool warm): the host clock around the whole call -- it uploads the weights, 4 B a cell, from the host --, one warm-up call
and then `reps` calls, with and without the sums per watershed; beside them the chain's stage times by HIP events (the accumulation
stage is the yardstick) and the upload of a 4-byte raster of the same shape through a context.  The kernels' own times come from the
same script under `rocprofv3 --kernel-trace --stats`, in a run of its own.
`python tools/lab/wacc_measure.py [size] [reps] [out.json]`."""
import json, os, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import bench
from malstroem_amd.pipeline import HydroPipeline

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
out = sys.argv[3] if len(sys.argv) > 3 else None
dem = bench.fbm(n)
rng = np.random.default_rng(1)
w = rng.integers(0, 2000001, size=(n, n), dtype=np.uint32)      # coefficients 0 .. 1 under a pattern of 0 .. 2
res = {"n": n, "reps": reps}
with HydroPipeline((n, n)) as p:
    p.upload("dem", dem)
    for _ in range(2):
        p.run("fill", "noflat", "flowdir", "accum", "label")
        nl = p.apply_keep(None)
        p.run("watershed", "pourpoints")
        p.sync()
    res["stage_ms"] = {s: p.stage_ms(s) for s in ("fill", "noflat", "flowdir", "accum", "label", "watershed", "pourpoints")}
    res["nlabels"] = nl
    with HydroPipeline((n, n)) as q:
        t = []
        for _ in range(3):
            t0 = time.perf_counter(); q.upload("labels", w.view(np.int32)); q.sync(); t.append((time.perf_counter() - t0) * 1e3)
        res["upload_4B_raster_ms"] = sorted(t)
    for name, by_ws in (("call_ms_with_watersheds", True), ("call_ms_without_watersheds", False)):
        t = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            wa = p.weighted_accumulation(w, by_watersheds=by_ws)
            t.append((time.perf_counter() - t0) * 1e3)
            res["unresolved"] = wa.unresolved
            wa.close()
        res[name] = [round(x, 3) for x in t[1:]]
        res[name + "_median"] = round(float(np.median(t[1:])), 3)
print(json.dumps(res))
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
