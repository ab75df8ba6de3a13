"""Development measurement of subdivision meshes below an instance: N instances (default 64) of bomberman as a subdivision mesh at
tessellation level L / compression level C (default 6 / 3) on a square lattice in the xz plane, each scaled by a power of two, under
subdiv_accel=bvh4.compressed.leaf and under the eager accel (trace_instance_subdiv.hip), against the SAME N copies flattened by the
caller into one un-instanced scene of N subdivision meshes, traced by the top-level kernels in quad form (the default) and, for
compressed.leaf, in the one-ray-per-lane form (RTAMD_CBVH_FORM=lane) - the blob walk the instance kernel runs.  1 M random rays over the
bounds of all instances, device-resident, ONE stream, kernel time by HIP events around every step (the batch is restored from a pristine
copy before each step, untimed).  Also printed: accel bytes and commit times of both.
usage: instance_subdiv_rates.py [steps] [repeats] [N] [L] [C] [variants: il ie fl fe, default all four]
       (fe - the flattened eager scene - needs N x 119 MB of grid cells at L = 6)"""
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
d = np.load(os.path.join(root, 'assets/bomberman.mesh.npz'))
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
count = int(sys.argv[3]) if len(sys.argv) > 3 else 64
L = int(sys.argv[4]) if len(sys.argv) > 4 else 6
Cl = int(sys.argv[5]) if len(sys.argv) > 5 else 3
variants = sys.argv[6:] or ['il', 'ie', 'fl', 'fe']
n = 1 << 20
LEAF = 'bvh4.compressed.leaf'


def snap(v):
    return (np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0).astype(np.float32)


mesh = snap(d['verts'] * 0.0625)
fs, fi = d['face_sizes'], d['face_index']


def placements():
    """[3,4] row-major local-to-world: lattice spacing 72 (the mesh spans ~30, scaled by up to 2), uniform scales 1/2, 1, 2"""
    side = int(np.ceil(np.sqrt(count)))
    out = []
    for i in range(count):
        s = (0.5, 1.0, 2.0)[i % 3]
        m = np.zeros((3, 4))
        m[:, :3] = np.eye(3) * s
        m[:, 3] = (72.0 * (i % side), 0.25 * (i % 5), 72.0 * (i // side))
        out.append(m.astype(np.float32))
    return out


def measure(rtc, kind, accel, form, xfms, pristine):
    if form == 'lane':
        os.environ['RTAMD_CBVH_FORM'] = 'lane'  # read when a device is created
    else:
        os.environ.pop('RTAMD_CBVH_FORM', None)
    dev = rtc.Device('gpu=0,subdiv_accel=' + accel)
    sc = rtc.Scene(dev)
    inner = None
    t0 = time.perf_counter()
    if kind == 'instanced':
        inner = rtc.Scene(dev)
        inner.add_subdiv(mesh, fs, fi)
        inner.set_levels(L, Cl)
        inner.commit()
        for m in xfms:
            sc.add_instance(inner, m)
    else:  # the caller's flattening: one subdivision mesh per copy, vertices transformed (exact: power-of-two scales, grid translations)
        for m in xfms:
            sc.add_subdiv((mesh.astype(np.float64) @ m[:, :3].astype(np.float64).T + m[:, 3]).astype(np.float32), fs, fi)
        sc.set_levels(L, Cl)
    sc.commit()
    commit = time.perf_counter() - t0
    nbytes = sc.stats()['totalBytes'] + (inner.stats()['totalBytes'] if inner else 0)
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
    med = float(np.median(meds))
    extra = f' (the instanced scene\'s own accel, counted in: {inner.stats()["totalBytes"]} B)' if inner else ''
    print(f'{count:4d} x L{L} C{Cl} {kind:9s} {accel:20s} {form:5s}: accel kind {sc.stats()["accelKind"]}, {nbytes} B in all{extra}, commit {commit:.2f} s, {hits} hits; '
          f'kernel {med:.4f} ms per 1 M-ray batch (median of {repeats} repeats of {steps} steps; repeats {min(meds):.4f}..{max(meds):.4f}) = {n / med / 1e3:.0f} Mrays/s', flush=True)
    sc.release()
    if inner:
        inner.release()
    dev.release()
    return med


def main():
    rtc = importlib.import_module('embree-compressed_amd').rtc
    raygen = importlib.import_module('embree-compressed_amd.raygen')
    print(f'library: {rtc.LIB_PATH}', flush=True)
    xfms = placements()
    corners = np.array([[(mesh.min(0), mesh.max(0))[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
    world = np.concatenate([corners @ m[:, :3].astype(np.float64).T + m[:, 3] for m in xfms])
    rays = raygen.make_random_rays(n, world.min(0).astype(np.float32), world.max(0).astype(np.float32), seed=0)
    pristine = torch.from_numpy(rays.reshape(-1).view(np.uint8).reshape(n, 80).copy()).cuda()
    res = {}
    if 'il' in variants:
        res['il'] = measure(rtc, 'instanced', LEAF, 'lane', xfms, pristine)
    if 'ie' in variants:
        res['ie'] = measure(rtc, 'instanced', 'default', 'lane', xfms, pristine)
    if 'fl' in variants:
        res['fl.quad'] = measure(rtc, 'flattened', LEAF, 'quad', xfms, pristine)
        res['fl.lane'] = measure(rtc, 'flattened', LEAF, 'lane', xfms, pristine)
    if 'fe' in variants:
        res['fe'] = measure(rtc, 'flattened', 'default', 'octet', xfms, pristine)
    for a, b in (('il', 'fl.quad'), ('il', 'fl.lane'), ('ie', 'fe')):
        if a in res and b in res:
            print(f'{a} / {b} = {res[a] / res[b]:.2f}', flush=True)


if __name__ == '__main__':
    main()
