"""Rates of the line leaf for docs/experiments.md "Line segments": 4096 strands of 256 segments over bomberman's bounds, 1 M random rays,
closest hit and occluded, one batch alone and four in flight; the triangle leaf on a scene of equal primitive count for comparison.
Timed regions: host clock around LAUNCHES launches per stream that end in a device synchronise, every launch on a batch of its own that is
restored (untimed) before the region; REGIONS regions per case after WARM untimed ones, median and range in Grays/s.  Needs a GPU.
    python tools/line_rates.py [robust-first]        (prints one line per case and a JSON line; `robust-first` swaps the order of the cases:
                                                      the first four-stream case of a process has come out at the one-batch rate, whichever it was)"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
rtc = importlib.import_module("embree-compressed_amd").rtc
import pyoracle as po  # noqa: E402
import torch  # noqa: E402

STRANDS, PER, M = 4096, 256, 1 << 20
WARM, REGIONS, LAUNCHES = 5, 15, 8


def tuft(lo, hi, seed=1):
    rng = np.random.default_rng(seed)
    ext = float(np.max(hi - lo))
    p = lo + rng.random((STRANDS, 3)) * (hi - lo)
    d = rng.normal(size=(STRANDS, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    v = np.zeros((STRANDS, PER + 1, 4), np.float32)
    for k in range(PER + 1):
        v[:, k, :3] = p
        v[:, k, 3] = ext * 5e-4 * (1.0 - 0.5 * k / PER)
        d = d + 0.25 * rng.normal(size=(STRANDS, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        p = p + d * ext * 0.004
    idx = (np.arange(STRANDS)[:, None] * (PER + 1) + np.arange(PER)[None, :]).reshape(-1).astype(np.uint32)
    return v.reshape(-1, 4), idx


def ribbons(v, idx):
    """one thin triangle per segment: v0, v1, v0 + 2 r * (a unit vector perpendicular to the segment)"""
    a, b = v[idx, :3].astype(np.float64), v[idx + 1, :3].astype(np.float64)
    t = b - a
    q = np.cross(t, np.array([0.3, 0.5, 0.81]))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c = a + q * 2.0 * v[idx, 3:4]
    tv = np.stack([a, b, c], 1).reshape(-1, 3).astype(np.float32)
    return tv, np.arange(len(tv), dtype=np.uint32).reshape(-1, 3)


def timed(dev, sc, src, occluded, streams):
    """a trace modifies the records in place: every launch of a region gets a working batch of its own, restored (untimed) from `src`"""
    call = sc.occluded1M if occluded else sc.intersect1M
    bufs = [[src.clone() for _ in range(LAUNCHES)] for _ in streams]

    def region():
        for row in bufs:
            for b in row:
                b.copy_(src)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(LAUNCHES):
            for row, s in zip(bufs, streams):
                if s is not None:
                    dev.set_stream(s.cuda_stream)
                call(row[k], check=False)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _ in range(WARM):
        region()
    rates = [LAUNCHES * len(streams) * M / region() / 1e9 for _ in range(REGIONS)]
    dev.check("timed")
    return {"median": round(float(np.median(rates)), 3), "min": round(float(np.min(rates)), 3), "max": round(float(np.max(rates)), 3)}


def main():
    d = np.load(os.path.join(ROOT, "assets", "bomberman.mesh.npz"))
    lo, hi = d["verts"].min(0), d["verts"].max(0)
    v, idx = tuft(lo, hi)
    tv, tt = ribbons(v, idx)
    rays = po.make_random_rays(M, lo, hi, seed=3)
    out = {"segments": int(len(idx)), "rays": M, "regions": REGIONS, "launches_per_region": LAUNCHES}
    order = ((4, "robust"), (0, "fast")) if "robust-first" in sys.argv else ((0, "fast"), (4, "robust"))
    for flags, fname in order:
        for what in ("lines", "triangles"):
            dev = rtc.Device("" if what == "lines" else ("tri_accel=bvh8.triangle4v" if flags else "tri_accel=bvh8.triangle4"))
            sc = rtc.Scene(dev, flags)
            t0 = time.perf_counter()
            if what == "lines":
                sc.add_lines(v, idx)
            else:
                sc.add_triangles(tv, tt)
            sc.commit()
            st = sc.stats()
            key = f"{what}.{fname}"
            out[key + ".build_s"] = round(time.perf_counter() - t0, 2)
            out[key + ".accel"] = {k: st[k] for k in ("accelKind", "nodeCount", "primCount", "leafCount", "maxDepth", "totalBytes")}
            raw = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy())
            for occluded in (False, True):
                src = (raw[:, :48].contiguous() if occluded else raw).cuda()
                streams = [torch.cuda.Stream() for _ in range(4)]
                if not occluded:
                    probe = src.clone()
                    sc.intersect1M(probe)
                    torch.cuda.synchronize()
                    out[key + ".hits"] = int((probe.cpu().numpy().reshape(-1).view(rays.dtype)["geomID"] != 0xFFFFFFFF).sum())
                mode = "occluded" if occluded else "closest"
                out[f"{key}.{mode}.alone"] = timed(dev, sc, src, occluded, [torch.cuda.current_stream()])
                out[f"{key}.{mode}.four_in_flight"] = timed(dev, sc, src, occluded, streams)
                dev.set_stream(torch.cuda.current_stream().cuda_stream)
                print(key, mode, out[f"{key}.{mode}.alone"], out[f"{key}.{mode}.four_in_flight"], flush=True)
            sc.release()
            dev.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
