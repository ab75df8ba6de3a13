"""Rates of the motion-blur line leaf for docs/experiments.md "Motion blur of line segments": the tuft of tools/line_rates.py (4096 strands of
256 segments over bomberman's bounds) with two time steps - step 1 is step 0 rotated by 20 degrees about y through the centre, moved by
0.3 x the extent along x, radii grown to 1.5 x - traced by 1 M random rays with random times under swept node boxes and under
mb_bounds=linear, and the same segments at rest (step 0) under the static line accel.  Closest hit and occluded, one batch alone and four
in flight, timed as in tools/line_rates.py; primTests, leafVisits and nodeVisits per ray from one counted batch each.  Needs a GPU.
    python tools/line_mb_rates.py [robust]        (prints one line per case and a JSON line; `robust`: RTC_SCENE_FLAG_ROBUST scenes)"""
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
from line_rates import M, timed, tuft  # noqa: E402


def moved(v):
    """step 1 of the tuft: rotated by 20 degrees about y through its centre, moved by 0.3 x the extent along x, radii 1.5 x"""
    p = v[:, :3].astype(np.float64)
    ctr = (p.min(0) + p.max(0)) / 2
    a = np.deg2rad(20.0)
    c, s = np.cos(a), np.sin(a)
    q = (p - ctr) @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T + ctr
    q[:, 0] += 0.3 * (p[:, 0].max() - p[:, 0].min())
    return np.concatenate([q, 1.5 * v[:, 3:4]], 1).astype(np.float32)


def main():
    d = np.load(os.path.join(ROOT, "assets", "bomberman.mesh.npz"))
    lo, hi = d["verts"].min(0), d["verts"].max(0)
    v, idx = tuft(lo, hi)
    steps = [v, moved(v)]
    rays = po.make_random_rays(M, lo, hi, seed=3)
    rays["time"] = np.random.default_rng(5).random(M).astype(np.float32)
    flags = 4 if "robust" in sys.argv else 0
    out = {"segments": int(len(idx)), "rays": M, "robust": bool(flags)}
    for key, cfg in (("moving.swept", ""), ("moving.linear", "mb_bounds=linear"), ("at_rest.static", "")):
        dev = rtc.Device(cfg)
        sc = rtc.Scene(dev, flags)
        t0 = time.perf_counter()
        if key.startswith("moving"):
            sc.add_lines_mb(steps, idx)
        else:
            sc.add_lines(v, idx)
        sc.commit()
        st = sc.stats()
        out[key + ".build_s"] = round(time.perf_counter() - t0, 2)
        out[key + ".accel"] = {k: st[k] for k in ("accelKind", "nodeCount", "nodeBytes", "primCount", "leafCount", "maxDepth", "totalBytes")}
        c = rtc.aligned_rayhits(M)
        c[:] = rays
        cnt = sc.intersect1M_counted(c)
        out[key + ".hits"] = int((c["geomID"] != 0xFFFFFFFF).sum())
        out[key + ".per_ray"] = {k: round(cnt[k] / M, 2) for k in ("primTests", "leafVisits", "nodeVisits")}
        raw = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy())
        for occluded in (False, True):
            src = (raw[:, :48].contiguous() if occluded else raw).cuda()
            streams = [torch.cuda.Stream() for _ in range(4)]
            mode = "occluded" if occluded else "closest"
            out[f"{key}.{mode}.alone"] = timed(dev, sc, src, occluded, [torch.cuda.current_stream()])
            out[f"{key}.{mode}.four_in_flight"] = timed(dev, sc, src, occluded, streams)
            dev.set_stream(torch.cuda.current_stream().cuda_stream)
            print(key, mode, out[key + ".per_ray"], out[f"{key}.{mode}.alone"], out[f"{key}.{mode}.four_in_flight"], flush=True)
        sc.release()
        dev.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
