"""Development measurement of instance motion blur: N instances of the bomberman triangles (placed as tools/instance_rates.py places
them), 1 M random rays over the bounds of all instances and steps, device-resident, ONE stream, kernel time by HIP events around every
step (the batch is restored from a pristine copy before each step, untimed).  Both variants (Pluecker / Moeller).  Three cases:
  a  static       one time step per instance: the static kinds (14 / 15), the static kernel;
  b  same-steps   the same transforms given as two identical steps: kinds 18 / 19, the same boxes and the same hits, plus the inverse
                  of the interpolated transform at every instance entry - b / a is the price of the per-entry inverse;
  c  moving       step 1 = step 0 rotated by a further 20 degrees about y and moved by 0.3 x the mesh extent, rays at random times:
                  the top-level boxes are swept over the whole shutter - c / b is the price of the swept boxes.
The rays are the same in the three cases (bounds of case c, random times), so that a, b and c differ in the scene only.
usage: instance_mb_rates.py [steps] [repeats] [cases, e.g. abc] [N ...]      (default N: 16 256 1024)
(an older build of the library, RTAMD_LIB=..., serves case a only)"""
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
cases = sys.argv[3] if len(sys.argv) > 3 else 'abc'
counts = [int(a) for a in sys.argv[4:]] or [16, 256, 1024]
n = 1 << 20


def snap(v):
    return (np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0).astype(np.float32)


tris = rtc.fan_triangulate(d['face_sizes'], d['face_index'])
mesh = snap(d['verts'] * 0.0625)
extent = float((mesh.max(0) - mesh.min(0)).max())


def roty(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def placements(count):
    """(step 0, step 1) per instance, [3,4] row-major local-to-world: lattice spacing 36 (the mesh spans ~30), rotation about y, scale
    0.8..1.2; step 1: a further 20 degrees about y, moved by 0.3 x the extent in a direction that differs per instance"""
    side = int(np.ceil(np.sqrt(count)))
    out = []
    for i in range(count):
        s = 0.8 + 0.4 * ((i * 7) % 11) / 10.0
        m0, m1 = np.zeros((3, 4)), np.zeros((3, 4))
        m0[:, :3] = roty(37.0 * i) * s
        m0[:, 3] = (36.0 * (i % side), 0.25 * (i % 5), 36.0 * (i // side))
        m1[:, :3] = roty(37.0 * i + 20.0) * s
        b = np.deg2rad(73.0 * i)
        m1[:, 3] = m0[:, 3] + 0.3 * extent * np.array([np.cos(b), 0.2, np.sin(b)])
        out.append((m0.astype(np.float32), m1.astype(np.float32)))
    return out


def measure(case, variant, xfms, pristine):
    dev = rtc.Device('gpu=0')
    flags = rtc.RTC_SCENE_FLAG_ROBUST if variant == 'pluecker' else 0
    sc = rtc.Scene(dev, flags)
    inner = rtc.Scene(dev, flags)
    inner.add_triangles(mesh, tris)
    inner.commit()
    for m0, m1 in xfms:
        if case == 'a':
            sc.add_instance(inner, m0)
        else:
            sc.add_instance_mb(inner, [m0, m0 if case == 'b' else m1])
    sc.commit()
    buf = pristine.clone()
    st = torch.cuda.current_stream()
    dev.set_stream(st.cuda_stream)
    for _ in range(3):  # warm-up
        buf.copy_(pristine)
        sc.intersect1M(buf)
    torch.cuda.synchronize()
    hits = int((buf.view(torch.int32)[:, 18] != -1).sum().item())
    meds = []
    for _ in range(repeats):
        ms = []
        for _ in range(steps):
            buf.copy_(pristine)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            sc.intersect1M(buf)
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        meds.append(float(np.median(ms)))
    stt = sc.stats()
    med = float(np.median(meds))
    name = {'a': 'static', 'b': 'same-steps', 'c': 'moving'}[case]
    print(f'{len(xfms):5d} {case} {name:10s} {variant:8s}: accel kind {stt["accelKind"]}, {stt["nodeCount"]} nodes, {stt["totalBytes"]} B, depth {stt["maxDepth"]}, {hits} hits; '
          f'kernel {med:.4f} ms per 1 M-ray batch (median of {repeats} repeats of {steps} steps; repeats {min(meds):.4f}..{max(meds):.4f}) = {n / med / 1e3:.0f} Mrays/s', flush=True)
    sc.release()
    inner.release()
    dev.release()
    return med


print(f'library: {rtc.LIB_PATH}', flush=True)
if not hasattr(rtc.lib(), 'rtcamdGetGeometryWorld2Local'):
    cases = ''.join(c for c in cases if c == 'a')  # a build without instance motion blur
for count in counts:
    xfms = placements(count)
    corners = np.array([[(mesh.min(0), mesh.max(0))[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
    world = np.concatenate([corners @ m[:, :3].astype(np.float64).T + m[:, 3] for pair in xfms for m in pair])
    rays = raygen.make_random_rays(n, world.min(0).astype(np.float32), world.max(0).astype(np.float32), seed=0).reshape(-1).view(rtc.RAYHIT_DTYPE).copy()
    rays['time'] = np.random.RandomState(1).rand(n).astype(np.float32)
    pristine = torch.from_numpy(rays.view(np.uint8).reshape(n, 80).copy()).cuda()
    for variant in ('pluecker', 'moeller'):
        ms = {c: measure(c, variant, xfms, pristine) for c in cases}
        if 'a' in ms and 'b' in ms:
            print(f'{count:5d} {variant:8s}: same-steps / static = {ms["b"] / ms["a"]:.2f}', flush=True)
        if 'b' in ms and 'c' in ms:
            print(f'{count:5d} {variant:8s}: moving / same-steps = {ms["c"] / ms["b"]:.2f}', flush=True)
