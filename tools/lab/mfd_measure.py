"""DESIGN.md 21, "Measured": HydroPipeline.mfd_accumulation() alone on the 16384^2 fBm DEM of the bench after two runs of the chain
(the pool warm): the host clock around the whole call with the default weight (nothing crosses the bus), one warm-up call and then
`reps` calls per exponent, with the rounds and tile visits of the schedule; beside it the yardstick, weighted_accumulation() of a
uint32 raster of UNIT on the same context in the same session (it uploads its weights, 4 B a cell; the upload of such a raster is
timed too), and the chain's stage times by HIP events.  The kernels' own times come from the same script under
`rocprofv3 --kernel-trace --stats`, in a run of its own.
`python tools/lab/mfd_measure.py [size] [reps] [out.json]`."""
import json, os, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import bench
from malstroem_amd.pipeline import HydroPipeline
from malstroem_amd.runoff import UNIT

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out = sys.argv[3] if len(sys.argv) > 3 else None
dem = bench.fbm(n)
w = np.full((n, n), UNIT, dtype=np.uint32)
res = {"n": n, "reps": reps}
with HydroPipeline((n, n)) as p:
    p.upload("dem", dem)
    for _ in range(2):
        p.run("fill", "noflat", "flowdir", "accum", "label")
        p.apply_keep(None)
        p.run("watershed", "pourpoints")
        p.sync()
    res["stage_ms"] = {s: p.stage_ms(s) for s in ("fill", "noflat", "flowdir", "accum", "label", "watershed", "pourpoints")}
    res["noflat_pending_before"] = p.get_int("noflat_pending")
    for e in (1, 4, 8):
        t = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            acc = p.mfd_accumulation(e)
            t.append((time.perf_counter() - t0) * 1e3)
            res["mfd_e%d_unresolved" % e] = acc.unresolved
            res["mfd_e%d_work" % e] = acc.work()
            acc.close()
        res["mfd_e%d_first_call_ms" % e] = round(t[0], 3)
        res["mfd_e%d_call_ms" % e] = [round(x, 3) for x in t[1:]]
        res["mfd_e%d_call_ms_median" % e] = round(float(np.median(t[1:])), 3)
    t = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        wa = p.weighted_accumulation(w, by_watersheds=False)
        t.append((time.perf_counter() - t0) * 1e3)
        wa.close()
    res["wacc_call_ms"] = [round(x, 3) for x in t[1:]]
    res["wacc_call_ms_median"] = round(float(np.median(t[1:])), 3)
    with HydroPipeline((n, n)) as q:
        t = []
        for _ in range(3):
            t0 = time.perf_counter(); q.upload("labels", w.view(np.int32)); q.sync(); t.append((time.perf_counter() - t0) * 1e3)
        res["upload_4B_raster_ms"] = sorted(round(x, 3) for x in t)
print(json.dumps(res))
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
