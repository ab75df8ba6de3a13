"""Development measurement of time-dependent top-level boxes above moving SUBDIVISION instances (device config inst_subdiv_bounds=linear,
accel kinds 34 / 35) against the swept boxes of the default (kinds 24 / 25): N two-step instances (default 64) of bomberman as a
subdivision mesh at tessellation level L / compression level C (default 6 / 3) on the lattice of tools/instance_subdiv_rates.py, under
the eager accel and under subdiv_accel=bvh4.compressed.leaf; 1 M random rays over the bounds of all instances and steps at random times,
device-resident, ONE stream, kernel time by HIP events around every step (the batch is restored from a pristine copy before each step,
untimed).  The two devices are built side by side and measured in alternation, repeat by repeat, so that drift of the machine hits
both.  The eager records of the two must be equal byte for byte; bvh4.compressed.leaf closest hits depend on the visiting order where a
ray meets several blobs, so there the number of differing records is printed.  Regimes (step 1 = step 0 moved in a direction of the
instance's own):
  fast      by 8 x the mesh extent: displacement >> size
  moderate  by 1 x the extent: displacement about the size
  barely    by 0.01 x the extent: the costlier node step buys nothing
usage: instance_subdiv_top_linear_rates.py [steps] [repeats] [N] [L] [C] [regimes, default: fast moderate barely]"""
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
count = int(sys.argv[3]) if len(sys.argv) > 3 else 64
L = int(sys.argv[4]) if len(sys.argv) > 4 else 6
Cl = int(sys.argv[5]) if len(sys.argv) > 5 else 3
regimes = sys.argv[6:] or ['fast', 'moderate', 'barely']
n = 1 << 20
MOVE = {'fast': 8.0, 'moderate': 1.0, 'barely': 0.01}
KEYS = ('inst_subdiv_bounds=swept', 'inst_subdiv_bounds=linear')


def snap(v):
    return (np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0).astype(np.float32)


mesh = snap(d['verts'] * 0.0625)
fs, fi = d['face_sizes'], d['face_index']
extent = float((mesh.max(0) - mesh.min(0)).max())


def placements(regime):
    """(step 0, step 1) per instance, [3,4] row-major local-to-world: lattice spacing 72 (the mesh spans ~30, scaled by up to 2), uniform
    scales 1/2, 1, 2 as in tools/instance_subdiv_rates.py; step 1 moved by MOVE[regime] x the mesh extent"""
    side = int(np.ceil(np.sqrt(count)))
    out = []
    for i in range(count):
        s = (0.5, 1.0, 2.0)[i % 3]
        m0 = np.zeros((3, 4))
        m0[:, :3] = np.eye(3) * s
        m0[:, 3] = (72.0 * (i % side), 0.25 * (i % 5), 72.0 * (i // side))
        m1 = m0.copy()
        b = np.deg2rad(73.0 * i)
        m1[:, 3] = m0[:, 3] + MOVE[regime] * extent * np.array([np.cos(b), 0.2, np.sin(b)])
        out.append((m0.astype(np.float32), m1.astype(np.float32)))
    return out


class Side:
    def __init__(self, cfg, accel, xfms, pristine):
        self.dev = rtc.Device('gpu=0,subdiv_accel=' + accel + ',' + cfg)
        self.inner = rtc.Scene(self.dev)
        self.inner.add_subdiv(mesh, fs, fi)
        self.inner.set_levels(L, Cl)
        self.inner.commit()
        self.sc = rtc.Scene(self.dev)
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


print(f'library: {rtc.LIB_PATH}; {count} instances, L {L} / C {Cl}, {steps} steps x {repeats} repeats', flush=True)
for regime in regimes:
    xfms = placements(regime)
    corners = np.array([[(mesh.min(0), mesh.max(0))[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
    world = np.concatenate([corners @ m[:, :3].astype(np.float64).T + m[:, 3] for pair in xfms for m in pair])
    rays = raygen.make_random_rays(n, world.min(0).astype(np.float32), world.max(0).astype(np.float32), seed=0).reshape(-1).view(rtc.RAYHIT_DTYPE).copy()
    rays['time'] = np.random.RandomState(1).rand(n).astype(np.float32)
    pristine = torch.from_numpy(rays.view(np.uint8).reshape(n, 80).copy()).cuda()
    for accel in ('default', 'bvh4.compressed.leaf'):
        sides = {cfg: Side(cfg, accel, xfms, pristine) for cfg in KEYS}
        differ = int((sides[KEYS[0]].buf != sides[KEYS[1]].buf).any(1).sum().item())
        for _ in range(repeats):  # in alternation
            for s in sides.values():
                s.repeat()
        med = {}
        name = 'eager' if accel == 'default' else 'cbvh.leaf'
        for cfg, s in sides.items():
            stt = s.sc.stats()
            hits = int((s.buf.view(torch.int32)[:, 18] != -1).sum().item())
            med[cfg] = float(np.median(s.meds))
            print(f'{regime:9s} {name:9s} {cfg:25s}: accel kind {stt["accelKind"]}, {stt["totalBytes"]} B, depth {stt["maxDepth"]}, {hits} hits; kernel {med[cfg]:.4f} ms per 1 M-ray '
                  f'batch (median of {repeats} repeats of {steps} steps; repeats {min(s.meds):.4f}..{max(s.meds):.4f}) = {n / med[cfg] / 1e3:.0f} Mrays/s', flush=True)
        lo = min(sides[KEYS[0]].meds) / max(sides[KEYS[1]].meds)
        hi = max(sides[KEYS[0]].meds) / min(sides[KEYS[1]].meds)
        for s in sides.values():
            s.release()
        print(f'{regime:9s} {name:9s}: swept / linear = {med[KEYS[0]] / med[KEYS[1]]:.2f} ({lo:.2f}..{hi:.2f} over the repeats), records that differ: {differ}', flush=True)
