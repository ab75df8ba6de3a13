"""Rates of the motion-blur ribbon leaf for docs/experiments.md "Motion blur of flat Bezier and B-spline curves": the tuft of
tools/curve_rates.py (the 4096 strands of tools/line_rates.py over bomberman's bounds as B-spline curves that share control points, 254
curves per strand) with two time steps - step 1 is step 0 rotated by 20 degrees about y through the centre, moved by 0.3 x the extent
along x, radii grown to 1.5 x (tools/line_mb_rates.py) - traced by 1 M random rays with random times at the default tessellation rate 4
under swept node boxes and under mb_bounds=linear, and the same curves at rest (step 0) under the static curve accel.  Closest hit and
occluded, one batch alone, timed as in tools/curve_rates.py; primTests (ribbon quads), leafVisits and nodeVisits per ray from one counted
batch each.  Needs a GPU.
    python tools/curve_mb_rates.py [robust]        (prints one line per case and a JSON line; `robust`: RTC_SCENE_FLAG_ROBUST scenes)"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
rtc = importlib.import_module("embree-compressed_amd").rtc
import pyoracle as po  # noqa: E402
import torch  # noqa: E402
import line_rates  # noqa: E402
from line_mb_rates import moved  # noqa: E402

line_rates.WARM, line_rates.REGIONS, line_rates.LAUNCHES = 3, 7, 4
M = line_rates.M


def main():
    d = np.load(os.path.join(ROOT, "assets", "bomberman.mesh.npz"))
    lo, hi = d["verts"].min(0), d["verts"].max(0)
    v, _ = line_rates.tuft(lo, hi)
    per = line_rates.PER + 1
    idx = (np.arange(line_rates.STRANDS)[:, None] * per + np.arange(per - 3)[None, :]).reshape(-1).astype(np.uint32)
    steps = [v, moved(v)]
    rays = po.make_random_rays(M, lo, hi, seed=3)
    rays["time"] = np.random.default_rng(5).random(M).astype(np.float32)
    flags = 4 if "robust" in sys.argv else 0
    out = {"curves": int(len(idx)), "rays": M, "robust": bool(flags), "regions": line_rates.REGIONS, "launches_per_region": line_rates.LAUNCHES}
    raw = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy())
    for key, cfg in (("moving.swept", ""), ("moving.linear", "mb_bounds=linear"), ("at_rest.static", "")):
        dev = rtc.Device(cfg)
        sc = rtc.Scene(dev, flags)
        t0 = time.perf_counter()
        if key.startswith("moving"):
            sc.add_curves_mb(steps, idx, basis="bspline")
        else:
            sc.add_curves(v, idx, basis="bspline")
        sc.commit()
        st = sc.stats()
        out[key + ".build_s"] = round(time.perf_counter() - t0, 2)
        out[key + ".accel"] = {k: st[k] for k in ("accelKind", "nodeCount", "nodeBytes", "primCount", "primBytes", "leafCount", "maxDepth", "totalBytes")}
        c = rtc.aligned_rayhits(M)
        c[:] = rays
        cnt = sc.intersect1M_counted(c)
        out[key + ".hits"] = int((c["geomID"] != 0xFFFFFFFF).sum())
        out[key + ".per_ray"] = {k: round(cnt[k] / M, 2) for k in ("primTests", "leafVisits", "nodeVisits")}
        for occluded in (False, True):
            src = (raw[:, :48].contiguous() if occluded else raw).cuda()
            mode = "occluded" if occluded else "closest"
            out[f"{key}.{mode}.alone"] = line_rates.timed(dev, sc, src, occluded, [torch.cuda.current_stream()])
            print(key, mode, out[key + ".hits"], out[key + ".per_ray"], out[f"{key}.{mode}.alone"], flush=True)
        sc.release()
        dev.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
