"""Development measurement: bomberman as 727 quads vs as 1454 fan triangles, 1 M random rays (seed 0), both accel variants
(Pluecker / robust, Moeller / fast).  Prints Grays/s on ONE stream (steps strictly back to back) and IN FLIGHT (batches spread over
4 streams), one line per scene and variant.  Device-resident batches, restored from a pristine copy before every step (untimed).
usage: quad_rates.py [steps] [inflight]"""
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

rtc = importlib.import_module('embree-compressed_amd').rtc
raygen = importlib.import_module('embree-compressed_amd.raygen')
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
d = np.load(os.path.join(root, 'assets/bomberman.mesh.npz'))
v, fs, fi = d['verts'], d['face_sizes'], d['face_index']
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
nfl = int(sys.argv[2]) if len(sys.argv) > 2 else 4
n = 1 << 20
rays = raygen.make_random_rays(n, v.min(0), v.max(0), seed=0)
pristine = torch.from_numpy(rays.view(np.uint8).reshape(n, 80).copy()).cuda()


def measure(kind, variant):
    cfg = 'gpu=0,' + ('tri_accel=bvh8.triangle4v' if variant == 'pluecker' else 'tri_accel=bvh8.triangle4,quad_accel=bvh8.quad4v')
    dev = rtc.Device(cfg)
    sc = rtc.Scene(dev, rtc.RTC_SCENE_FLAG_ROBUST if variant == 'pluecker' else 0)
    if kind == 'quads':
        sc.add_quads(v, fi.reshape(-1, 4))
    else:
        sc.add_triangles(v, rtc.fan_triangulate(fs, fi))
    sc.commit()
    bufs = [pristine.clone() for _ in range(nfl)]
    streams = [torch.cuda.Stream() for _ in range(nfl)]
    for b in bufs:  # warm-up
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        sc.intersect1M(b)
    torch.cuda.synchronize()
    hits = int((bufs[0].view(torch.int32)[:, 18] != -1).sum().item())
    # one stream: K steps back to back, each on a restored batch
    one = 0.0
    st = torch.cuda.current_stream()
    dev.set_stream(st.cuda_stream)
    for _ in range(steps):
        bufs[0].copy_(pristine)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.intersect1M(bufs[0])
        dev.synchronize()
        one += time.perf_counter() - t0
    # in flight: K steps dealt round-robin over nfl streams
    for b in bufs:
        b.copy_(pristine)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        k = s % nfl
        if s >= nfl:  # the batch is re-used: restore it on its stream (its previous trace is ordered before)
            with torch.cuda.stream(streams[k]):
                bufs[k].copy_(pristine)
        dev.set_stream(streams[k].cuda_stream)
        sc.intersect1M(bufs[k])
    torch.cuda.synchronize()
    fl = time.perf_counter() - t0
    st = sc.stats()
    print(f'{kind:9s} {variant:8s}: {hits} hits, {st["nodeCount"]} nodes, {st["primCount"]} prims x {st["primBytes"]} B, '
          f'one stream {steps * n / one / 1e9:.2f} Grays/s ({one / steps * 1e3:.3f} ms/step), in flight x{nfl} {steps * n / fl / 1e9:.2f} Grays/s '
          f'(restores included)', flush=True)
    sc.release()
    dev.release()


for variant in ('pluecker', 'moeller'):
    for kind in ('triangles', 'quads'):
        measure(kind, variant)
