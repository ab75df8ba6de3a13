"""Rates of the ribbon leaf for docs/experiments.md "Flat Bezier and B-spline curves": the pinned hair of tests/curve_helpers.py (512 Bezier
curves in the unit cube) and one large tuft - the strands of tools/line_rates.py (4096 strands of 257 vertices over bomberman's bounds) as
B-spline curves that share control points, 254 curves per strand - traced by 1 M random rays at tessellation rates 4 and 16 in the lane form
and in the octet form of the leaf, closest hit and occluded, one batch alone.  Timed as in tools/line_rates.py (fewer regions); primTests,
leafVisits and nodeVisits per ray from one counted batch each.  Needs a GPU.
    python tools/curve_rates.py [robust]        (prints one line per case and a JSON line; `robust`: RTC_SCENE_FLAG_ROBUST scenes)"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
rtc = importlib.import_module("embree-compressed_amd").rtc
import pyoracle as po  # noqa: E402
import torch  # noqa: E402
import line_rates  # noqa: E402
from curve_helpers import hair_and_rays  # noqa: E402

line_rates.WARM, line_rates.REGIONS, line_rates.LAUNCHES = 3, 7, 4
M = line_rates.M
FORMS = {"lane": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "0", "RTAMD_OCT_LEAF": "0"},
         "octet": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "32", "RTAMD_OCT_LEAF": "1"}}


def main():
    d = np.load(os.path.join(ROOT, "assets", "bomberman.mesh.npz"))
    lo, hi = d["verts"].min(0), d["verts"].max(0)
    tv, _ = line_rates.tuft(lo, hi)
    per = line_rates.PER + 1
    tidx = (np.arange(line_rates.STRANDS)[:, None] * per + np.arange(per - 3)[None, :]).reshape(-1).astype(np.uint32)
    hv, hidx, _, _ = hair_and_rays()
    one = np.ones(3, np.float32)
    scenes = {"hair": (hv, hidx, "bezier", po.make_random_rays(M, 0 * one, one, seed=3)), "tuft": (tv, tidx, "bspline", po.make_random_rays(M, lo, hi, seed=3))}
    flags = 4 if "robust" in sys.argv else 0
    out = {"rays": M, "robust": bool(flags), "regions": line_rates.REGIONS, "launches_per_region": line_rates.LAUNCHES}
    for sname, (v, idx, basis, rays) in scenes.items():
        raw = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy())
        for N in (4, 16):
            for form, knobs in FORMS.items():
                os.environ.update(knobs)  # read when a device is created
                dev = rtc.Device("")
                sc = rtc.Scene(dev, flags)
                t0 = time.perf_counter()
                sc.add_curves(v, idx, basis=basis, tessellation_rate=N)
                sc.commit()
                key = f"{sname}.N{N}.{form}"
                st = sc.stats()
                out[key + ".build_s"] = round(time.perf_counter() - t0, 2)
                out[key + ".accel"] = {k: st[k] for k in ("accelKind", "nodeCount", "primCount", "leafCount", "maxDepth", "totalBytes")}
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
