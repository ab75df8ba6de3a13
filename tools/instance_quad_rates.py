"""Development measurement of the instance accel with quad leaves (kinds 16 / 17), beside tools/instance_rates.py: N instances of
bomberman as 727 quads (scaled and snapped as in tests/instance_quads_helpers.py), placed as instance_rates.py places its triangles,
against the SAME geometry flattened by the caller into one top-level quad mesh (N x 727 transformed quads, traced by the static quad
kernel of trace_quad.hip) on the same build.  1 M random rays over the bounds of all instances, device-resident, ONE stream, kernel time
by HIP events around every step (the batch is restored from a pristine copy before each step, untimed).  Both variants.
instanced / flattened = price of the two-level traversal with the quad leaf's block loop (no octet form, 3 waves per SIMD for
closest-hit Pluecker) against a single BVH8 over everything.
usage: instance_quad_rates.py [steps] [repeats] [N ...]      (default N: 200)"""
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
counts = [int(a) for a in sys.argv[3:]] or [200]
n = 1 << 20


def snap(v):
    return (np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0).astype(np.float32)


assert (d['face_sizes'] == 4).all()
quads = d['face_index'].reshape(-1, 4).astype(np.uint32)
mesh = snap(d['verts'] * 0.0625)


def placements(count):
    """[3,4] row-major local-to-world of `count` instances: lattice spacing 36 (the mesh spans ~30), rotation about y, scale 0.8..1.2"""
    side = int(np.ceil(np.sqrt(count)))
    out = []
    for i in range(count):
        a = np.deg2rad(37.0 * i)
        s = 0.8 + 0.4 * ((i * 7) % 11) / 10.0
        m = np.zeros((3, 4))
        m[:, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) * s
        m[:, 3] = (36.0 * (i % side), 0.25 * (i % 5), 36.0 * (i // side))
        out.append(m.astype(np.float32))
    return out


def measure(kind, variant, xfms, pristine):
    dev = rtc.Device('gpu=0')
    flags = rtc.RTC_SCENE_FLAG_ROBUST if variant == 'pluecker' else 0
    sc = rtc.Scene(dev, flags)
    inner = None
    if kind == 'instanced':
        inner = rtc.Scene(dev, flags)
        inner.add_quads(mesh, quads)
        inner.commit()
        for m in xfms:
            sc.add_instance(inner, m)
    else:  # the caller's flattening: every instance's vertices transformed (float32 results of a float64 product), one quad mesh
        v = np.concatenate([(mesh.astype(np.float64) @ m[:, :3].astype(np.float64).T + m[:, 3]).astype(np.float32) for m in xfms])
        q = np.concatenate([quads + np.uint32(k * len(mesh)) for k in range(len(xfms))])
        sc.add_quads(v, q)
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
    print(f'{len(xfms):5d} {kind:9s} {variant:8s}: accel kind {stt["accelKind"]}, {stt["nodeCount"]} nodes, {stt["totalBytes"]} B, depth {stt["maxDepth"]}, {hits} hits; '
          f'kernel {med:.4f} ms per 1 M-ray batch (median of {repeats} repeats of {steps} steps; repeats {min(meds):.4f}..{max(meds):.4f}) = {n / med / 1e3:.0f} Mrays/s', flush=True)
    sc.release()
    if inner:
        inner.release()
    dev.release()
    return med


print(f'library: {rtc.LIB_PATH}', flush=True)
for count in counts:
    xfms = placements(count)
    corners = np.array([[(mesh.min(0), mesh.max(0))[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
    world = np.concatenate([corners @ m[:, :3].astype(np.float64).T + m[:, 3] for m in xfms])
    rays = raygen.make_random_rays(n, world.min(0).astype(np.float32), world.max(0).astype(np.float32), seed=0)
    pristine = torch.from_numpy(rays.reshape(-1).view(np.uint8).reshape(n, 80).copy()).cuda()
    for variant in ('pluecker', 'moeller'):
        a = measure('instanced', variant, xfms, pristine)
        b = measure('flattened', variant, xfms, pristine)
        print(f'{count:5d} {variant:8s}: instanced / flattened = {a / b:.2f}', flush=True)
