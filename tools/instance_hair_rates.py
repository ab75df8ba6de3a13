"""Development measurement of hair below instances (device config inst_hair=1, kinds 22 / 23 with the hair form of the two-level kernel,
csrc/trace_instance_hair.hip), modelled on tools/instance_quad_rates.py: N instances (default 64, on a lattice, general transforms - a
rotation about y and a uniform scale of 0.8..1.2) of ONE hair scene - a tuft of flat Bezier curves at tessellation rate 4 and a tuft of
line segments, rooted in a square and growing upwards - against the SAME hair flattened by the caller into one top-level scene (N x the
control points and end points transformed, radii multiplied by the instance's scale; traced by the static curve and line kernels of
trace_curve.hip / trace_line.hip).  1 M random rays over the bounds of all instances, device-resident, ONE stream, kernel time by HIP
events around every step (the batch is restored from a pristine copy before each step, untimed), closest hit and any hit, both variants
(robust / fast traversal), instanced and flattened alternating.  Prints the accel bytes of both and instanced / flattened.
The flattened twin runs on any build (RTAMD_LIB=... selects another build of the library); the instanced one needs inst_hair=1.
"moving": the moving variant (inst_hair=1,inst_hair_mb=1, the HAIRMB form, csrc/trace_instance_hair_mb.hip) - the tuft of curves with TWO
time steps (step 1: every point swayed sideways in proportion to its height), then the tuft of line segments with two time steps, each
alone in the hair scene, rays at random times in [0, 1); the flattened twin is traced by trace_curve_mb.hip / trace_line_mb.hip.
usage: instance_hair_rates.py [steps] [repeats] [N ...] [flattened] [moving]      (default N: 64; "flattened": only the flattened twin)"""
import importlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

rtc = importlib.import_module('embree-compressed_amd').rtc
raygen = importlib.import_module('embree-compressed_amd.raygen')
args = [a for a in sys.argv[1:] if a not in ('flattened', 'moving')]
only_flat = 'flattened' in sys.argv[1:]
moving = 'moving' in sys.argv[1:]
steps = int(args[0]) if len(args) > 0 else 20
repeats = int(args[1]) if len(args) > 1 else 5
counts = [int(a) for a in args[2:]] or [64]
n = 1 << 20
CURVES, STRANDS, PER = 2048, 256, 8  # one hair scene: 2048 curves and 256 strands of 8 line segments


def hair(seed=1, extent=16.0):
    """(curve control points [4 c, 4], curve index, line vertices, line index): roots uniform in the square [0, extent]^2 of the plane
    y = 0, hair grows along +y with a random lean; lengths 2..5, radii 0.02..0.06"""
    rng = np.random.default_rng(seed)
    root = np.stack([rng.random(CURVES) * extent, np.zeros(CURVES), rng.random(CURVES) * extent], 1)
    lean = rng.normal(scale=0.35, size=(CURVES, 3)) + np.array([0.0, 1.0, 0.0])
    lean /= np.linalg.norm(lean, axis=1, keepdims=True)
    ln = rng.uniform(2.0, 5.0, CURVES)
    cv = np.zeros((4 * CURVES, 4), np.float32)
    for k in range(4):
        cv[k::4, :3] = root + lean * ln[:, None] * (k / 3.0) + (rng.normal(scale=0.15, size=(CURVES, 3)) if k else 0.0)
        cv[k::4, 3] = rng.uniform(0.02, 0.06, CURVES) * (1.0 - 0.2 * k)
    lv, li = [], []
    for _ in range(STRANDS):
        p = np.array([rng.random() * extent, 0.0, rng.random() * extent])
        d = rng.normal(scale=0.35, size=3) + np.array([0.0, 1.0, 0.0])
        for k in range(PER + 1):
            lv.append(np.concatenate([p, [rng.uniform(0.02, 0.06)]]))
            if k < PER:
                li.append(len(lv) - 1)
            d = d + 0.2 * rng.normal(size=3)
            p = p + 0.5 * d / np.linalg.norm(d)
    return cv, np.arange(0, 4 * CURVES, 4, dtype=np.uint32), np.array(lv, np.float32), np.array(li, np.uint32)


CV, CI, LV, LI = hair()


def placements(count):
    """[3,4] row-major local-to-world of `count` instances: lattice spacing 24 (the tuft spans 16), rotation about y, uniform scale 0.8..1.2"""
    side = int(np.ceil(np.sqrt(count)))
    out = []
    for i in range(count):
        a = np.deg2rad(37.0 * i)
        s = 0.8 + 0.4 * ((i * 7) % 11) / 10.0
        m = np.zeros((3, 4))
        m[:, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) * s
        m[:, 3] = (24.0 * (i % side), 0.25 * (i % 5), 24.0 * (i // side))
        out.append((m.astype(np.float32), s))
    return out


def moved(v4, m, s):
    """points transformed (float32 results of a float64 product), radii multiplied by the uniform scale"""
    out = np.zeros_like(v4)
    out[:, :3] = (v4[:, :3].astype(np.float64) @ m[:, :3].astype(np.float64).T + m[:, 3]).astype(np.float32)
    out[:, 3] = (v4[:, 3].astype(np.float64) * s).astype(np.float32)
    return out


def swayed(v4):
    """the second time step: every point moved sideways in proportion to its height (the roots stay), radii kept"""
    out = v4.copy()
    out[:, 0] += 0.25 * v4[:, 1] / 4.0
    out[:, 2] += 0.15 * v4[:, 1] / 4.0
    return out


def measure(kind, variant, xfms, pristine, occluded, hair_mb=None):
    """hair_mb: None (the static tufts), 'curves' or 'lines' (that tuft alone, with two time steps)"""
    dev = rtc.Device('gpu=0' + (',inst_hair=1' if kind == 'instanced' else '') + (',inst_hair_mb=1' if kind == 'instanced' and hair_mb else ''))
    flags = rtc.RTC_SCENE_FLAG_ROBUST if variant == 'robust' else 0
    sc = rtc.Scene(dev, flags)
    inner = None
    if hair_mb:
        v, idx = (CV, CI) if hair_mb == 'curves' else (LV, LI)
        add = (lambda s, st, ix: s.add_curves_mb(st, ix, basis='bezier', tessellation_rate=4)) if hair_mb == 'curves' else (lambda s, st, ix: s.add_lines_mb(st, ix))
        if kind == 'instanced':
            inner = rtc.Scene(dev, flags)
            add(inner, [v, swayed(v)], idx)
            inner.commit()
            for m, _ in xfms:
                sc.add_instance(inner, m)
        else:
            index = np.concatenate([idx + np.uint32(k * len(v)) for k in range(len(xfms))])
            add(sc, [np.concatenate([moved(w, m, s) for m, s in xfms]) for w in (v, swayed(v))], index)
    elif kind == 'instanced':
        inner = rtc.Scene(dev, flags)
        inner.add_curves(CV, CI, basis='bezier', tessellation_rate=4)
        inner.add_lines(LV, LI)
        inner.commit()
        for m, _ in xfms:
            sc.add_instance(inner, m)
    else:  # the caller's flattening: one curve geometry and one line geometry over all copies
        sc.add_curves(np.concatenate([moved(CV, m, s) for m, s in xfms]), np.concatenate([CI + np.uint32(k * len(CV)) for k in range(len(xfms))]), basis='bezier', tessellation_rate=4)
        sc.add_lines(np.concatenate([moved(LV, m, s) for m, s in xfms]), np.concatenate([LI + np.uint32(k * len(LV)) for k in range(len(xfms))]))
    sc.commit()
    rec = 48 if occluded else 80
    src = pristine[:, :48].contiguous() if occluded else pristine
    buf = src.clone()
    trace = sc.occluded1M if occluded else sc.intersect1M
    st = torch.cuda.current_stream()
    dev.set_stream(st.cuda_stream)
    for _ in range(3):  # warm-up
        buf.copy_(src)
        trace(buf)
    torch.cuda.synchronize()
    w = buf.view(torch.int32)
    hits = int((w[:, 8] < 0).sum().item()) if occluded else int((w[:, 18] != -1).sum().item())  # tfar = -inf / geomID set
    meds = []
    for _ in range(repeats):
        ms = []
        for _ in range(steps):
            buf.copy_(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            trace(buf)
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        meds.append(float(np.median(ms)))
    stt = sc.stats()
    med = float(np.median(meds))
    print(f'{len(xfms):5d} {kind:9s} {"moving " + hair_mb + " " if hair_mb else ""}{variant:6s} {"any hit" if occluded else "closest"}: {stt["totalBytes"]} accel bytes, depth {stt["maxDepth"]}, {hits} hits; '
          f'kernel {med:.4f} ms per 1 M-ray batch of {rec}-byte records (median of {repeats} repeats of {steps} steps; repeats {min(meds):.4f}..{max(meds):.4f}) = {n / med / 1e3:.0f} Mrays/s', flush=True)
    sc.release()
    if inner:
        inner.release()
    dev.release()
    return med


print(f'library: {rtc.LIB_PATH}', flush=True)
for count in counts:
    xfms = placements(count)
    pts = np.concatenate([np.concatenate([moved(CV, m, s)[:, :3], moved(LV, m, s)[:, :3]]) for m, s in xfms])
    rays = raygen.make_random_rays(n, pts.min(0).astype(np.float32), pts.max(0).astype(np.float32), seed=0)
    if moving:
        rays.view(np.float32).reshape(n, 20)[:, 7] = np.random.default_rng(2).random(n, dtype=np.float32)  # ray.time
    pristine = torch.from_numpy(rays.reshape(-1).view(np.uint8).reshape(n, 80).copy()).cuda()
    for hair_mb in (('curves', 'lines') if moving else (None,)):
        for variant in ('robust', 'fast'):
            for occluded in (False, True):
                b = measure('flattened', variant, xfms, pristine, occluded, hair_mb)
                if only_flat:
                    continue
                a = measure('instanced', variant, xfms, pristine, occluded, hair_mb)
                print(f'{count:5d} {"moving " + hair_mb + " " if hair_mb else ""}{variant:6s} {"any hit" if occluded else "closest"}: instanced / flattened = {a / b:.2f}', flush=True)
