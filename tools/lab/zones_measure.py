"""DESIGN.md 13, "Measured": 1 000 000 random footprints of 5 to 40 cells (rotated rectangles) over the 16384^2 fBm DEM of the bench,
after the chain with the final state of one event and wet_at of three.  Host-clock times, each ending in a synchronise, of
rasterize_zones (grow 0 and 1), of zone_stats per source, and of the yardstick in the same process: download_rows of the rasters a
join on the host would need.  apply_keep with a mask runs label_stats of DEPTHS by LABELS in the same process: its kernel stands
beside zone_stats_kernel in the kernel statistics.  Also compares a 2048^2 window (half the raster's edge when that is smaller) of
the zone raster and the statistics of the objects in it with the model (tests/_zones.py).  `python tools/lab/zones_measure.py out.json [size] [objects]`; under `rocprofv3
--kernel-trace --stats` the kernels' device time comes from tools/kernel_stats.py."""
import json, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import bench, _zones
from malstroem_amd.pipeline import HydroPipeline

out = sys.argv[1]
N = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
NOBJ = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
dem = bench.fbm(N, 2.0, 42)
rng = np.random.default_rng(7)
area = rng.uniform(5, 40, NOBJ); aspect = rng.uniform(1, 3, NOBJ)
w, h = np.sqrt(area * aspect), np.sqrt(area / aspect)
cx, cy = rng.uniform(0, N, NOBJ), rng.uniform(0, N, NOBJ)
ang = rng.uniform(0, np.pi, NOBJ)
ca, sa = np.cos(ang), np.sin(ang)
corners = np.array([(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)])
px = cx[:, None] + corners[None, :, 0] * w[:, None] * ca[:, None] - corners[None, :, 1] * h[:, None] * sa[:, None]
py = cy[:, None] + corners[None, :, 0] * w[:, None] * sa[:, None] + corners[None, :, 1] * h[:, None] * ca[:, None]
xy = np.ascontiguousarray(np.stack([px, py], axis=2).reshape(-1, 2))
off = np.arange(NOBJ + 1, dtype=np.int64) * 4
zone = np.arange(1, NOBJ + 1, dtype=np.int32)
W0, M = min(2048, N // 2), 64      # the window compared with the model, and its margin


def timed(fn, reps=3):
    ms = []
    for _ in range(reps):
        t = time.perf_counter(); r = fn(); ms.append((time.perf_counter() - t) * 1e3)
    return ms, r


rec = dict(size=N, objects=NOBJ, vertices=int(len(xy)))
with HydroPipeline((N, N)) as p:
    p.upload("dem", dem)
    p.run("fill", "noflat", "flowdir", "accum", "label")
    nraw = p.get_int("nlabels_raw")
    t = time.perf_counter(); n = p.apply_keep(np.ones(nraw + 1, dtype=bool)); rec["apply_keep_with_label_stats_ms"] = (time.perf_counter() - t) * 1e3
    p.run("watershed", "pourpoints")
    p.hypsometry(0.05)
    cap = p.stats()["sum"]
    p.final_depths(0.3 * cap)
    p.wet_at(np.stack([0.1 * cap, 0.3 * cap, 0.6 * cap]), [10.0, 30.0, 60.0])
    p.sync()
    rec["nlabels"] = n
    rec["rasterize_grow0_ms"], _ = timed(lambda: p.rasterize_zones(xy, off, zone, NOBJ, grow=0))
    z0 = p.download_zones_rows(0, W0 + M)[:, :W0 + M]
    rec["rasterize_grow1_ms"], _ = timed(lambda: p.rasterize_zones(xy, off, zone, NOBJ, grow=1))
    stats = {}
    for src in ("depths", "finaldepths", "wet_at", "dem"):
        rec["zone_stats_%s_ms" % src], stats[src] = timed(lambda: p.zone_stats(src))
    zr = p.download_zones()
    rec["cells_in_zones"] = int((zr > 0).sum()); rec["objects_with_cells"] = int((stats["depths"]["cells"][1:] > 0).sum())
    rec["objects_wet_in_bluespots"] = int((stats["depths"]["pos"][1:] > 0).sum()); rec["objects_wet_at_60mm"] = int((stats["wet_at"]["pos"][1:] > 0).sum())
    yard = {}
    for name, fn in (("depths", lambda: p.download_rows("depths", 0, N)), ("finaldepths", lambda: p.download_rows("finaldepths", 0, N)),
                     ("wet_at", lambda: p.download_wet_at_rows(0, N))):
        yard[name], a = timed(fn)
        if name == "depths":
            depths_win = a[:W0, :W0].copy()
        del a
    rec["yardstick_download_rows_ms"] = yard
    rec["copy_bandwidth_gbs"] = HydroPipeline.copy_bandwidth(); rec["read_bandwidth_gbs"] = HydroPipeline.read_bandwidth()
# the model on a window: every object that can reach it (half a diagonal is below 8 cells) is taken along
sel = np.flatnonzero((cx < W0 + M - 8) & (cy < W0 + M - 8))
sxy = xy.reshape(NOBJ, 4, 2)[sel].reshape(-1, 2)
want = _zones.rasterize((W0 + M, W0 + M), sxy, np.arange(len(sel) + 1, dtype=np.int64) * 4, zone[sel], NOBJ, 0)
rec["model_window"] = dict(window=W0, objects=int(len(sel)), zones_equal=bool(want[:W0, :W0].tobytes() == z0[:W0, :W0].tobytes()))
grown = _zones.grow_once(want)[:W0, :W0]
rec["model_window"]["grown_equal"] = bool(grown.tobytes() == zr[:W0, :W0].tobytes())
inside = sel[(cx[sel] > 9) & (cy[sel] > 9) & (cx[sel] < W0 - 9) & (cy[sel] < W0 - 9)]      # objects whose grown cells all lie in the window
ms = _zones.zone_stats(depths_win, grown, NOBJ)
rec["model_window"]["stats_objects"] = int(len(inside)); rec["model_window"]["stats_equal"] = bool(ms[inside + 1].tobytes() == stats["depths"][inside + 1].tobytes())
json.dump(rec, open(out, "w"), indent=1)
print(json.dumps(rec))
