"""Development measurement of motion-blur meshes below instances: 9 instances (a 3 x 3 lattice, placed as tools/instance_mb_rates.py
places them: general transforms - a rotation about y and a uniform scale of 0.8..1.2 per instance - with one step each) of the bomberman triangles with the two time steps of tests/test_gpu_motion_blur.py (`two_steps`: step 1 =
step 0 rotated by 20 degrees about y and moved by 0.3 x the extent along x), 1 M random rays at random times over the bounds of all
instances and both steps, device-resident, ONE stream, kernel time by HIP events around every step (the batch is restored from a
pristine copy before each step, untimed).  Both variants (Pluecker / Moeller).  Five cases:
  a  static       the mesh with one time step: the static kinds (14 / 15) - what the library traced before it took moving meshes here;
  b  at-rest      the mesh with two EQUAL steps: kinds 22 / 23, the same boxes and the same hits, through the MESHMB kernel and the
                  96-byte records - b / a is the price of the kernel form and of the interpolation;
  c  moving       the two steps of `two_steps`: the node boxes are swept over the whole shutter - c / b is the price of the swept boxes;
  d  at-rest      case b on a device with mb_bounds=linear,inst_mb_bounds=linear: kinds 30 / 31, time-dependent nodes (equal plane blocks)
     linear       below the instances, the NODEMB kernel - d / b is the price of the 144-byte nodes and of the per-lane node step;
  e  moving       case c on that device - e / c is what the time-dependent boxes save below an instance.
     linear
The rays are the same in all cases (bounds of case c), so that the cases differ in the scene and the device config only; all run on
the same build.
usage: instance_mesh_mb_rates.py [steps] [repeats] [cases, e.g. abcde]
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
cases = sys.argv[3] if len(sys.argv) > 3 else 'abcde'
n = 1 << 20
COUNT = 9


def snap(v):
    return (np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0).astype(np.float32)


def roty(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


tris = rtc.fan_triangulate(d['face_sizes'], d['face_index'])
s0 = snap(d['verts'] * 0.0625)
ext = s0.max(0) - s0.min(0)
ctr = (s0.min(0) + s0.max(0)) / 2
s1 = snap((s0.astype(np.float64) - ctr) @ roty(20.0).T + ctr + np.array([0.3 * ext[0], 0.0, 0.0]))


def placements(count):
    """[3,4] row-major local-to-world per instance: lattice spacing 36 (the mesh spans ~30), rotation about y, scale 0.8..1.2"""
    side = int(np.ceil(np.sqrt(count)))
    out = []
    for i in range(count):
        s = 0.8 + 0.4 * ((i * 7) % 11) / 10.0
        m = np.zeros((3, 4))
        m[:, :3] = roty(37.0 * i) * s
        m[:, 3] = (36.0 * (i % side), 0.25 * (i % 5), 36.0 * (i // side))
        out.append(m.astype(np.float32))
    return out


def measure(case, variant, xfms, pristine):
    dev = rtc.Device('gpu=0,mb_bounds=linear,inst_mb_bounds=linear' if case in 'de' else 'gpu=0')
    flags = rtc.RTC_SCENE_FLAG_ROBUST if variant == 'pluecker' else 0
    sc = rtc.Scene(dev, flags)
    inner = rtc.Scene(dev, flags)
    if case == 'a':
        inner.add_triangles(s0, tris)
    else:
        inner.add_triangles_mb([s0, s0 if case in 'bd' else s1], tris)
    inner.commit()
    for m in xfms:
        sc.add_instance(inner, m)
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
    name = {'a': 'static', 'b': 'at-rest', 'c': 'moving', 'd': 'at-rest linear', 'e': 'moving linear'}[case]
    print(f'{len(xfms):5d} {case} {name:14s} {variant:8s}: accel kind {stt["accelKind"]}, {stt["nodeCount"]} nodes, {stt["totalBytes"]} B, depth {stt["maxDepth"]}, {hits} hits; '
          f'kernel {med:.4f} ms per 1 M-ray batch (median of {repeats} repeats of {steps} steps; repeats {min(meds):.4f}..{max(meds):.4f}) = {n / med / 1e3:.0f} Mrays/s', flush=True)
    sc.release()
    inner.release()
    dev.release()
    return med


print(f'library: {rtc.LIB_PATH}', flush=True)
xfms = placements(COUNT)
both = np.concatenate([s0, s1])
corners = np.array([[(both.min(0), both.max(0))[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
world = np.concatenate([corners @ m[:, :3].astype(np.float64).T + m[:, 3] for m in xfms])
rays = raygen.make_random_rays(n, world.min(0).astype(np.float32), world.max(0).astype(np.float32), seed=0).reshape(-1).view(rtc.RAYHIT_DTYPE).copy()
rays['time'] = np.random.RandomState(1).rand(n).astype(np.float32)
pristine = torch.from_numpy(rays.view(np.uint8).reshape(n, 80).copy()).cuda()
for variant in ('pluecker', 'moeller'):
    ms = {}
    for c in cases:
        try:
            ms[c] = measure(c, variant, xfms, pristine)
        except rtc.RTCError as e:  # a build that refuses moving meshes below an instance
            print(f'{COUNT:5d} {c} {variant:8s}: refused ({e})', flush=True)
    if 'a' in ms and 'b' in ms:
        print(f'{COUNT:5d} {variant:8s}: at-rest / static = {ms["b"] / ms["a"]:.2f}', flush=True)
    if 'b' in ms and 'c' in ms:
        print(f'{COUNT:5d} {variant:8s}: moving / at-rest = {ms["c"] / ms["b"]:.2f}', flush=True)
    if 'b' in ms and 'd' in ms:
        print(f'{COUNT:5d} {variant:8s}: at-rest linear / at-rest = {ms["d"] / ms["b"]:.2f}', flush=True)
    if 'c' in ms and 'e' in ms:
        print(f'{COUNT:5d} {variant:8s}: moving linear / moving = {ms["e"] / ms["c"]:.2f}', flush=True)
