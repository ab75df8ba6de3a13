"""Shared by tests/test_host_instance_mb.py and tests/test_gpu_instance_mb.py: instances with time steps (instance motion blur, accel
kinds 18..21).

An instance is described as (geomID, scene key, steps): steps is a list of local-to-world [3,4] matrices, one per time step; one step is
a static instance.  A ray at `time` sees the instance under world2local(time) = inverse(lerp(steps[itime], steps[itime + 1], ftime));
world2local_at restates embree-compressed_amd/csrc/instance_xfm.h in numpy float32, operation for operation (instance_helpers.fma32
for every fmaf), vectorised over rays.  Scenes are described as in instance_quads_helpers ({"tris": ..., "quads": ...}); the expected
records of an instance come from that instance's LOCAL rays under the per-ray matrices, as in instance_quads_helpers."""
import numpy as np

import instance_helpers as ih
import instance_quads_helpers as iq
from instance_helpers import INVALID, fma32

STEP_DT = np.dtype([("local2world", "<f4", 12), ("pad", "<u4", 4)])
ACCEL_INSTMB_TRI_PLUECKER, ACCEL_INSTMB_TRI_MOELLER, ACCEL_INSTMB_PLUECKER, ACCEL_INSTMB_MOELLER = 18, 19, 20, 21
F32 = np.float32


def kind(mode, quads):
    """mode 0: Pluecker / robust, mode 1: Moeller / fast"""
    if quads:
        return ACCEL_INSTMB_PLUECKER if mode == 0 else ACCEL_INSTMB_MOELLER
    return ACCEL_INSTMB_TRI_PLUECKER if mode == 0 else ACCEL_INSTMB_TRI_MOELLER


def static_kind(mode, quads):
    if quads:
        return iq.ACCEL_INST_PLUECKER if mode == 0 else iq.ACCEL_INST_MOELLER
    return ih.ACCEL_INST_TRI_PLUECKER if mode == 0 else ih.ACCEL_INST_TRI_MOELLER


def time_segment(times, segments):
    """(itime, ftime) as accel.h / trace_mb.hip.h time_segment, in float32: ts = time * S, itime = clamp(floor(ts), 0, S - 1)"""
    s = F32(segments)
    ts = (np.asarray(times, F32) * s).astype(F32)
    itf = np.minimum(np.maximum(np.floor(ts), F32(0)), s - F32(1)).astype(F32)
    return itf.astype(np.int64), (ts - itf).astype(F32)


def lerp_at(steps, times):
    """lerp(steps[itime], steps[itime + 1], ftime) per ray: [n,3,4] float32, madd(1 - f, a, f * b) per entry"""
    st = np.asarray(steps, F32).reshape(-1, 3, 4)
    it, f = time_segment(times, len(st) - 1)
    a, b = st[it], st[it + 1]
    f = f[:, None, None]
    g = (F32(1) - f).astype(F32)
    return fma32(np.broadcast_to(g, a.shape), a, (f * b).astype(F32))


def _cross(a, b):
    """cross(a, b) = (msub(a.y, b.z, a.z * b.y), msub(a.z, b.x, a.x * b.z), msub(a.x, b.y, a.y * b.x)) on [n,3] float32"""
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
    return np.stack([fma32(ay, bz, -(az * by).astype(F32)), fma32(az, bx, -(ax * bz).astype(F32)), fma32(ax, by, -(ay * bx).astype(F32))], 1)


def invert(m):
    """instance_invert of instance_xfm.h on [n,3,4] float32 matrices: (inverse [n,3,4], ok [n])"""
    m = np.asarray(m, F32)
    vx, vy, vz, p = m[:, :, 0], m[:, :, 1], m[:, :, 2], m[:, :, 3]
    c0, c1, c2 = _cross(vy, vz), _cross(vz, vx), _cross(vx, vy)
    det = fma32(vx[:, 0], c0[:, 0], fma32(vx[:, 1], c0[:, 1], (vx[:, 2] * c0[:, 2]).astype(F32)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = (F32(1) / det).astype(F32)
        out = np.zeros(m.shape, F32)
        cs = np.stack([c0, c1, c2], 1)  # cs[n, i, k] = c_i.k;  column k of the inverse = (c0.k, c1.k, c2.k) * r
        for k in range(3):
            out[:, :, k] = (cs[:, :, k] * r[:, None]).astype(F32)
        for k in range(3):  # p' = -(madd(p.x, vx', madd(p.y, vy', p.z * vz'))) per component
            out[:, k, 3] = -fma32(p[:, 0], out[:, k, 0], fma32(p[:, 1], out[:, k, 1], (p[:, 2] * out[:, k, 2]).astype(F32)))
    ok = (det != 0) & np.isfinite(out.reshape(len(out), -1)).all(1)
    return out, ok


def world2local_at(steps, times):
    """The matrix the kernel uses for a ray at each of `times`: (world2local [n,3,4] float32 row-major, ok [n]).  One step: the static
    path's matrix (float64 inverse rounded once, instance_helpers.world2local), for every time."""
    st = np.asarray(steps, F32).reshape(-1, 3, 4)
    n = len(np.asarray(times).reshape(-1))
    if len(st) == 1:
        return np.broadcast_to(ih.world2local(st[0]), (n, 3, 4)).copy(), np.ones(n, bool)
    return invert(lerp_at(st, np.asarray(times, F32).reshape(-1)))


def world2local_f64(steps, times):
    """float64 inverse of the float64 lerp (itime / ftime from the float32 time_segment, the lerp weights then in float64)"""
    st = np.asarray(steps, np.float64).reshape(-1, 3, 4)
    it, f = time_segment(times, len(st) - 1)
    f = f.astype(np.float64)[:, None, None]
    m = np.zeros((len(it), 4, 4))
    m[:, :3] = (1.0 - f) * st[it] + f * st[it + 1]
    m[:, 3, 3] = 1.0
    return np.linalg.inv(m)[:, :3]


def local_rays(rays, w2l, ok=None, exact=False):
    """instance_helpers.local_rays with one matrix PER RAY (w2l [n,3,4]).  Rays whose matrix is not ok get tnear = inf: they are
    skipped (tnear > tfar), as the kernel does not enter the instance.  exact=True: float64, asserted to be representable in float32."""
    out = rays.copy()
    o = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1)
    d = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1)
    if ok is None:
        ok = np.ones(len(rays), bool)
    m = np.where(ok[:, None, None], np.asarray(w2l, F32), F32(0)).astype(F32)
    if exact:
        m64 = m.astype(np.float64)
        lo = np.einsum("nkj,nj->nk", m64[:, :, :3], o.astype(np.float64)) + m64[:, :, 3]
        ld = np.einsum("nkj,nj->nk", m64[:, :, :3], d.astype(np.float64))
        assert np.array_equal(lo.astype(F32).astype(np.float64), lo), "local origins are not exact in fp32"
        assert np.array_equal(ld.astype(F32).astype(np.float64), ld), "local directions are not exact in fp32"
        lo, ld = lo.astype(F32), ld.astype(F32)
    else:
        lo = np.stack([fma32(o[:, 0], m[:, k, 0], fma32(o[:, 1], m[:, k, 1], fma32(o[:, 2], m[:, k, 2], m[:, k, 3]))) for k in range(3)], 1)
        ld = np.stack([fma32(d[:, 0], m[:, k, 0], fma32(d[:, 1], m[:, k, 1], (d[:, 2] * m[:, k, 2]).astype(F32))) for k in range(3)], 1)
    out["org_x"], out["org_y"], out["org_z"] = lo[:, 0], lo[:, 1], lo[:, 2]
    out["dir_x"], out["dir_y"], out["dir_z"] = ld[:, 0], ld[:, 1], ld[:, 2]
    out["tnear"][~ok] = np.inf
    return out


def _restore(sub, rays, ok):
    """the records of rays that did not enter the instance: untouched"""
    sub["tnear"][~ok] = rays["tnear"][~ok]
    for f in ("org_x", "org_y", "org_z", "dir_x", "dir_y", "dir_z"):
        sub[f] = rays[f]  # merge() copies the hit fields only; keep the world ray in every record
    return sub


# ---- building -------------------------------------------------------------------------------------------------------------------------
def build(rtc, mode, scenes, instances, cfg="", extra=None):
    """top scene of `instances` [(geomID, scene key, steps)]: add_instance for one step, add_instance_mb for more"""
    dev = rtc.Device(cfg)
    inner = {k: iq.add_scene(rtc, dev, d, mode) for k, d in scenes.items()}
    top = rtc.Scene(dev, iq.flags(mode))
    for gid, key, steps in instances:
        if len(steps) == 1:
            assert top.add_instance(inner[key], steps[0], geom_id=gid) == gid
        else:
            assert top.add_instance_mb(inner[key], steps, geom_id=gid) == gid
    if extra:
        extra(top)
    top.commit()
    return dev, top, inner


def swept_bounds(scenes, instances):
    """world bounds of all instances over all their steps"""
    meshes = iq.bounds_meshes(scenes)
    flat = [(g, k, s) for g, k, steps in instances for s in steps]
    return ih.instances_bounds(meshes, flat)


def rays_with_times(rtc, po, scenes, instances, m, seed, snapped=False, eighths=False):
    """random rays through the swept bounds; ray.time random in [0, 1], or k/8 (eighths)"""
    lo, hi = swept_bounds(scenes, instances)
    rays = rtc.aligned_rayhits(m)
    rays[:] = po.make_random_rays(m, lo.astype(F32), hi.astype(F32), seed=seed)
    if snapped:
        for f in ("org_x", "org_y", "org_z"):
            rays[f] = ih.snap(rays[f])
    rng = np.random.RandomState(seed + 1000)
    rays["time"] = (rng.randint(0, 9, m) / 8.0).astype(F32) if eighths else rng.rand(m).astype(F32)
    return rays


# ---- expected records ---------------------------------------------------------------------------------------------------------------------
def oracle_instances(rtc, po, scenes, instances, rays, mode, exact=False):
    """instance_quads_helpers.oracle_instances with the per-ray matrices of world2local_at: (want, per, isb, want_tri)"""
    orcs = {}
    for k, d in scenes.items():
        t = po.TriangleScene(d["tris"][0], d["tris"][1], mode, np.full(len(d["tris"][1]), d["tris"][2], np.uint32)) if d["tris"] is not None else None
        q = iq.split_oracle(po, d["quads"][0], d["quads"][1], mode, iq.SPLIT_A, iq.SPLIT_B) if d["quads"] is not None else None
        orcs[k] = (t, q)
    per, per_tri, per_b = [], [], []
    for gid, key, steps in instances:
        w, ok = world2local_at(steps, rays["time"])
        sub = rtc.aligned_rayhits(len(rays))
        sub[:] = local_rays(rays, w, ok, exact)
        t, q = orcs[key]
        if t is not None:
            t.intersect1M(sub, inst_id=gid, nthreads=16)
        isb = np.zeros(len(rays), bool)
        raw = sub.copy()
        if q is not None:
            q.intersect1M(sub, inst_id=gid, nthreads=16)  # on the same records: against the tfar the triangles left, equal t accepted
            raw = sub.copy()
            isb = iq.map_b(sub, scenes[key]["quads"][2], iq.SPLIT_A, iq.SPLIT_B)
            quad = (raw["geomID"] == iq.SPLIT_A) | (raw["geomID"] == iq.SPLIT_B)
            raw["geomID"][quad] = scenes[key]["quads"][2]
        per.append(_restore(sub, rays, ok))
        per_tri.append(_restore(raw, rays, ok))
        per_b.append(isb)
    for t, q in orcs.values():
        for s in (t, q):
            if s is not None:
                s.free()
    want, best = iq.merge(rays, per, instances)
    want_tri, _ = iq.merge(rays, per_tri, instances)
    hit = want["geomID"] != INVALID
    isb = np.stack(per_b)[best, np.arange(len(rays))] & hit
    return want, per, isb, want_tri


def direct_instances(rtc, inner, instances, rays):
    """leg 2, no oracle arithmetic: every instance's scene traced directly with the EXACT local rays under the per-ray matrices, merged by
    smallest t.  Asserts that the mirror's matrices equal a float64 computation (the inputs make world2local(time) exact)."""
    per = []
    for gid, key, steps in instances:
        w, ok = world2local_at(steps, rays["time"])
        assert ok.all()
        if len(steps) > 1:
            assert np.array_equal(w.astype(np.float64), world2local_f64(steps, rays["time"])), "world2local(time) is not exact for these inputs"
        sub = rtc.aligned_rayhits(len(rays))
        sub[:] = local_rays(rays, w, ok, exact=True)
        inner[key].intersect1M(sub)
        per.append(sub)
    want, _ = iq.merge(rays, per, instances)
    return want, per


# ---- pinned inputs ------------------------------------------------------------------------------------------------------------------------
PERMS = [np.array(p, np.float64) for p in (
    [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
    [[-1, 0, 0], [0, 0, 1], [0, 1, 0]], [[0, 1, 0], [0, 0, -1], [-1, 0, 0]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]])]


def exact_instances(n, keys=("m",), moving=True):
    """n instances whose world2local(time) is exact for times k/8: the linear part - a signed axis permutation times a uniform
    power-of-two scale - is the same in all steps of an instance, the translations lie on the 2^-10 grid; 2, 3 and 5 steps mixed
    (segment counts 1, 2, 4).  moving=False: step 0 only."""
    out = []
    for i in range(n):
        s = (0.5, 1.0, 2.0)[i % 3]
        t0 = np.array([40.0 * (i % 4) + 0.125 * i, 40.0 * ((i // 4) % 5) + 5.0 / 1024.0 * i, 40.0 * (i // 20) + 1.0 / 1024.0 * i])
        nsteps = (2, 3, 5)[i % 3] if moving else 1
        steps = []
        for j in range(nsteps):
            dt = j * np.array([3.0 + 0.25 * i, -2.5 + 7.0 / 1024.0 * i, 1.75 - 0.125 * i]) + (j * j) * np.array([0.5, 0.0, -1.0 / 1024.0])
            steps.append(ih.affine(t0 + dt, (s, s, s), PERMS[i % len(PERMS)]))
        out.append((i, keys[i % len(keys)], steps))
    return out


GENERAL_SEED = 23
GENERAL_RAYS = 20000


def general_instances(keys=("m",)):
    """instance_quads_helpers.general_instances as step 0; step 1: the instance rotated by a further 20..50 degrees about its own axis and
    moved by up to 0.3 x its extent; a third step for every other instance"""
    out = []
    for g, key, m0 in iq.general_instances(keys):
        m0 = np.asarray(m0, np.float64)
        axis = (1.0 + g, 2.0, 0.5 * g - 1.0)
        extent = 2.0 * 16.0  # the mesh spans less than +-16, scales are about 1
        steps = [m0.astype(F32)]
        for j in range(1, 3 if g % 2 == 0 else 2):
            rot = ih.rotation(axis, j * (20.0 + 30.0 * ((g * 3) % 9) / 8.0))
            m = np.zeros((3, 4))
            m[:, :3] = rot @ m0[:, :3]
            frac = 0.3 * ((g * 5) % 9 + 1) / 9.0
            m[:, 3] = m0[:, 3] + j * frac * extent * np.array([0.6, -0.3, 0.74]) * (1 if g % 3 else -1)
            steps.append(m.astype(F32))
        out.append((g, key, steps))
    return out
