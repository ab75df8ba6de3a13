"""Development measurement of time-dependent top-level boxes (device config inst_bounds=linear, accel kinds 32 / 33) against the swept
boxes of the default: N moving instances of the bomberman triangles, 1 M random rays over the bounds of all instances and steps at
random times, device-resident, ONE stream, kernel time by HIP events around every step (the batch is restored from a pristine copy
before each step, untimed).  The two devices are built side by side and measured in alternation, repeat by repeat, so that drift of
the machine hits both; the records of the two must be equal byte for byte.  Scenes:
  mb      the moving case of tools/instance_mb_rates.py (docs/experiments.md "Instance motion blur"): step 1 = step 0 rotated by a further
          20 degrees about y and moved by 0.3 x the mesh extent
  fast    the same lattice, every instance moved by 8 x the mesh extent in a direction of its own: fast movers
  barely  moved by 0.01 x the extent: the costlier node step buys nothing
usage: instance_top_linear_rates.py [steps] [repeats] [scene:N ...]      (default: mb:16 mb:256 fast:64 barely:64)"""
import importlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

rtc = importlib.import_module('embree-compressed_amd').rtc
raygen = importlib.import_module('embree-compressed_amd.raygen')
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
d = np.load(os.path.join(root, 'assets/bomberman.mesh.npz'))
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cases = sys.argv[3:] or ['mb:16', 'mb:256', 'fast:64', 'barely:64']
n = 1 << 20


def snap(v):
    return (np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0).astype(np.float32)


tris = rtc.fan_triangulate(d['face_sizes'], d['face_index'])
mesh = snap(d['verts'] * 0.0625)
extent = float((mesh.max(0) - mesh.min(0)).max())


def roty(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def placements(scene, count):
    """(step 0, step 1) per instance, [3,4] row-major local-to-world: the lattice of tools/instance_mb_rates.py"""
    side = int(np.ceil(np.sqrt(count)))
    turn, move = {'mb': (20.0, 0.3), 'fast': (0.0, 8.0), 'barely': (0.0, 0.01)}[scene]
    out = []
    for i in range(count):
        s = 0.8 + 0.4 * ((i * 7) % 11) / 10.0
        m0, m1 = np.zeros((3, 4)), np.zeros((3, 4))
        m0[:, :3] = roty(37.0 * i) * s
        m0[:, 3] = (36.0 * (i % side), 0.25 * (i % 5), 36.0 * (i // side))
        m1[:, :3] = roty(37.0 * i + turn) * s
        b = np.deg2rad(73.0 * i)
        m1[:, 3] = m0[:, 3] + move * extent * np.array([np.cos(b), 0.2, np.sin(b)])
        out.append((m0.astype(np.float32), m1.astype(np.float32)))
    return out


class Side:
    def __init__(self, cfg, variant, xfms, pristine):
        self.dev = rtc.Device('gpu=0,' + cfg)
        flags = rtc.RTC_SCENE_FLAG_ROBUST if variant == 'pluecker' else 0
        self.sc = rtc.Scene(self.dev, flags)
        self.inner = rtc.Scene(self.dev, flags)
        self.inner.add_triangles(mesh, tris)
        self.inner.commit()
        for m0, m1 in xfms:
            self.sc.add_instance_mb(self.inner, [m0, m1])
        self.sc.commit()
        self.buf = pristine.clone()
        self.pristine = pristine
        self.st = torch.cuda.current_stream()
        self.dev.set_stream(self.st.cuda_stream)
        for _ in range(3):  # warm-up
            self.buf.copy_(pristine)
            self.sc.intersect1M(self.buf)
        torch.cuda.synchronize()
        self.meds = []

    def repeat(self):
        ms = []
        for _ in range(steps):
            self.buf.copy_(self.pristine)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self.st)
            self.sc.intersect1M(self.buf)
            e1.record(self.st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        self.meds.append(float(np.median(ms)))

    def release(self):
        self.sc.release()
        self.inner.release()
        self.dev.release()


print(f'library: {rtc.LIB_PATH}', flush=True)
for case in cases:
    scene, count = case.split(':')
    xfms = placements(scene, int(count))
    corners = np.array([[(mesh.min(0), mesh.max(0))[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
    world = np.concatenate([corners @ m[:, :3].astype(np.float64).T + m[:, 3] for pair in xfms for m in pair])
    rays = raygen.make_random_rays(n, world.min(0).astype(np.float32), world.max(0).astype(np.float32), seed=0).reshape(-1).view(rtc.RAYHIT_DTYPE).copy()
    rays['time'] = np.random.RandomState(1).rand(n).astype(np.float32)
    pristine = torch.from_numpy(rays.view(np.uint8).reshape(n, 80).copy()).cuda()
    for variant in ('pluecker', 'moeller'):
        sides = {cfg: Side(cfg, variant, xfms, pristine) for cfg in ('inst_bounds=swept', 'inst_bounds=linear')}
        same = bool(torch.equal(sides['inst_bounds=swept'].buf, sides['inst_bounds=linear'].buf))
        for _ in range(repeats):  # in alternation
            for s in sides.values():
                s.repeat()
        med = {}
        for cfg, s in sides.items():
            stt = s.sc.stats()
            hits = int((s.buf.view(torch.int32)[:, 18] != -1).sum().item())
            med[cfg] = float(np.median(s.meds))
            print(f'{case:10s} {variant:8s} {cfg:18s}: accel kind {stt["accelKind"]}, {stt["totalBytes"]} B, depth {stt["maxDepth"]}, {hits} hits; kernel {med[cfg]:.4f} ms per 1 M-ray '
                  f'batch (median of {repeats} repeats of {steps} steps; repeats {min(s.meds):.4f}..{max(s.meds):.4f}) = {n / med[cfg] / 1e3:.0f} Mrays/s', flush=True)
            s.release()
        print(f'{case:10s} {variant:8s}: swept / linear = {med["inst_bounds=swept"] / med["inst_bounds=linear"]:.2f}, records byte-identical: {same}', flush=True)
