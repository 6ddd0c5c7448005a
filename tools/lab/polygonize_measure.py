"""DESIGN.md 14, "Measured": the outlines of the bluespots and of the watersheds of the 16384^2 fBm DEM of the bench, after the chain.
Per source: rings, vertices, the longest ring in vertices, the three invariants on the result (rasterized back on the device), the
host-clock time of HydroPipeline.polygonize (three calls, the first with a cold pool) and, the yardstick in the same process,
download_to of the same raster into a writer that keeps nothing.  `python tools/lab/polygonize_measure.py out.json [size]`; under
`rocprofv3 --kernel-trace --stats` the kernels' device time comes from tools/kernel_stats.py."""
import json, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import bench
from malstroem_amd import vector
from malstroem_amd.objects import rasterize
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
    for source in ("labels", "watersheds"):
        r = {}
        r["polygonize_ms"], (xy, off, rl) = timed(lambda: p.polygonize(source))
        r["download_to_ms"], _ = timed(lambda: p.download_to(source, Sink()))
        n = np.diff(off)
        area = vector.ring_areas(xy, off)
        r.update(rings=int(len(rl)), holes=int((area < 0).sum()), vertices=int(len(xy)), longest_ring_vertices=int(n.max(initial=0)))
        # edges: the perimeter of every ring
        nxt = np.arange(len(xy)) + 1
        nxt[off[1:] - 1] = off[:-1]
        r["edges"] = int(np.abs(xy[nxt].astype(np.int64) - xy).sum())
        per_ring = np.add.reduceat(np.abs(xy[nxt].astype(np.int64) - xy).sum(axis=1), off[:-1])
        r["longest_ring_edges"] = int(per_ring.max(initial=0))
        raster = p.download(source)
        t = time.perf_counter(); back = rasterize((N, N), xy, off, rl, rec["nlabels"]); r["rasterize_back_ms"] = (time.perf_counter() - t) * 1e3
        r["rasterized_back_equal"] = bool(back.tobytes() == raster.tobytes())
        counts = np.bincount(raster.ravel(), minlength=rec["nlabels"] + 1)
        r["areas_equal_counts"] = bool(np.array_equal(np.bincount(rl, weights=area, minlength=rec["nlabels"] + 1).astype(np.int64)[1:], counts[1:]))
        r["one_exterior_ring_per_label"] = bool(np.array_equal(np.bincount(rl[area > 0], minlength=rec["nlabels"] + 1)[1:], (counts[1:] > 0).astype(np.int64)))
        del raster, back
        rec[source] = r
        print(source, json.dumps(r), flush=True)
    rec["copy_bandwidth_gbs"] = HydroPipeline.copy_bandwidth()
with open(out, "w") as fh:
    json.dump(rec, fh, indent=1)
print(json.dumps(rec))
