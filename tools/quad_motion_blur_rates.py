"""Development measurement of the motion-blur quad accel: bomberman as 727 quads (scaled and snapped as in
tests/test_gpu_quad_motion_blur.py), 1 M random rays at random times over the union of both steps' bounds, device-resident, ONE
stream, kernel time by HIP events around every step (the batch is restored from a pristine copy before each step, untimed).
  (a) static   the mesh committed static (step-0 vertices), traced by the static quad leaf
  (b) at-rest  2 steps with step 1 = step 0 (128-byte records + interpolation, boxes as tight as the static ones)
  (c) moving   2 steps: step 1 = step 0 rotated by 20 degrees about y and moved by 0.3 x extent along x
b / a = price of the records and the interpolation, c / b = price of the swept boxes.  Both variants (Pluecker / Moeller).
The triangle counterpart is motion_blur_rates.py.
`linear` as the third argument: the device is created with mb_bounds=linear (time-dependent node boxes, accel kinds 28 / 29) and only (b)
and (c) are measured.
usage: quad_motion_blur_rates.py [steps] [repeats] [linear]"""
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
linear = len(sys.argv) > 3 and sys.argv[3] == 'linear'
n = 1 << 20


def snap(v):
    return (np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0).astype(np.float32)


def rot_y(v, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    m = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    ctr = (v.min(0) + v.max(0)) / 2
    return (np.asarray(v, np.float64) - ctr) @ m.T + ctr


assert (d['face_sizes'] == 4).all()
quads = d['face_index'].reshape(-1, 4).astype(np.uint32)
s0 = snap(d['verts'] * 0.0625)
ext = s0.max(0) - s0.min(0)
s1 = snap(rot_y(s0, 20.0) + np.array([0.3 * ext[0], 0.0, 0.0]))
both = np.concatenate([s0, s1])
rays = raygen.make_random_rays(n, both.min(0), both.max(0), seed=0)
rays = rays.reshape(-1).view(rtc.RAYHIT_DTYPE).copy()
rays['time'] = np.random.RandomState(1).rand(n).astype(np.float32)
pristine = torch.from_numpy(rays.view(np.uint8).reshape(n, 80).copy()).cuda()


def measure(kind, variant):
    dev = rtc.Device('gpu=0,mb_bounds=linear' if linear else 'gpu=0')
    sc = rtc.Scene(dev, rtc.RTC_SCENE_FLAG_ROBUST if variant == 'pluecker' else 0)
    if kind == 'static':
        sc.add_quads(s0, quads)
    else:
        sc.add_quads_mb([s0, s1 if kind == 'moving' else s0], quads)
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
    print(f'{kind:8s} {variant:8s}: accel kind {stt["accelKind"]}, {stt["nodeCount"]} nodes, {stt["primCount"]} records x {stt["primBytes"]} B, {hits} hits; '
          f'kernel {med:.4f} ms (median of {repeats} repeats of {steps} steps; repeats {min(meds):.4f}..{max(meds):.4f}) = {n / med / 1e3:.0f} Mrays/s', flush=True)
    sc.release()
    dev.release()
    return med


print(f'library: {rtc.LIB_PATH}; mb_bounds={"linear" if linear else "swept"}', flush=True)
for variant in ('pluecker', 'moeller'):
    if linear:
        b, c = (measure(kind, variant) for kind in ('at-rest', 'moving'))
        print(f'{variant}: c/b (linear boxes) = {c / b:.2f}', flush=True)
        continue
    a, b, c = (measure(kind, variant) for kind in ('static', 'at-rest', 'moving'))
    print(f'{variant}: b/a (records + interpolation) = {b / a:.3f}, c/b (swept boxes) = {c / b:.2f}', flush=True)
