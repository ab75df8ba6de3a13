"""Shared by tests/test_host_instances.py and tests/test_gpu_instances.py: transforms, local rays, and the expected records of a scene
of instances.

The oracle has no instancing.  The expected records come from po.TriangleScene on the LOCAL mesh, once per instance, traced with that
instance's local rays (org' = world2local * org, dir' = world2local-linear * dir) and the ORIGINAL tfar - t is common to both spaces -
and are then merged: the hit with the smallest t wins and carries that instance's geomID as instID.  Ng, u, v stay as computed in
local space (the reference does not transform Ng)."""
import numpy as np

INVALID = 0xFFFFFFFF
HITF = ["Ng_x", "Ng_y", "Ng_z", "u", "v", "primID", "geomID", "instID"]
SCALE = 0.0625  # bomberman spans +-246: below 16 after scaling, so that scaled-by-two instances stay below 64 before translation

# accel records (embree-compressed_amd/csrc/accel.h)
NODE_DT = np.dtype([("origin", "<f4", 3), ("exp", "u1", 3), ("pad", "u1"), ("child", "<u4", 8), ("q", "u1", (6, 8))])
TRI_DT = np.dtype([("a", "<f4", 3), ("geomID", "<u4"), ("b", "<f4", 3), ("primID", "<u4"), ("c", "<f4", 3), ("pad", "<u4")])
INST_DT = np.dtype([("world2local", "<f4", 12), ("geomID", "<u4"), ("root", "<u4"), ("pad", "<u4", 2)])
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF
ACCEL_INST_TRI_PLUECKER, ACCEL_INST_TRI_MOELLER = 14, 15


def snap(v):
    """to the 2^-10 grid (as the motion-blur tests do)"""
    return (np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0).astype(np.float32)


def affine(t=(0, 0, 0), s=(1, 1, 1), rot=None):
    """local-to-world as a float32 [3,4] row-major matrix: x -> R * diag(s) * x + t"""
    m = np.zeros((3, 4), np.float64)
    r = np.eye(3) if rot is None else np.asarray(rot, np.float64)
    m[:, :3] = r @ np.diag(np.broadcast_to(np.asarray(s, np.float64), 3))
    m[:, 3] = t
    return m.astype(np.float32)


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def world2local(l2w):
    """inverse of a [3,4] local-to-world, computed in float64 and rounded once to float32 (what the library documents)"""
    m = np.eye(4)
    m[:3] = np.asarray(l2w, np.float64)
    return np.linalg.inv(m)[:3].astype(np.float32)


def xfm_points(m34, p):
    m = np.asarray(m34, np.float64)
    return np.asarray(p, np.float64) @ m[:, :3].T + m[:, 3]


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded: the product of two float32 is exact in float64; the float64 sum is corrected
    where it lies exactly half way between two float32 values and the part lost by the float64 addition (TwoSum) decides the side."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # exact: s + err == p + c
    bits = s.view(np.uint64) if s.ndim else np.array([s]).view(np.uint64)
    half = (bits & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)  # a tie of the float64 -> float32 rounding (normal range)
    out = s.astype(np.float32)
    fix = half & (err != 0)
    if fix.any():
        lo = np.nextafter(s, -np.inf).astype(np.float32)  # the float32 neighbours of the tie
        hi = np.nextafter(s, np.inf).astype(np.float32)
        out = np.where(fix, np.where(err > 0, hi, lo), out).astype(np.float32)
    return out


def local_rays(rays, w2l, exact=False):
    """The rays in the instance's space, computed in numpy float32 in the reference's operation order: org' = xfmPoint(world2local, org)
    = madd(x, vx, madd(y, vy, madd(z, vz, p))) (affinespace.h:110), dir' = xfmVector = madd(x, vx, madd(y, vy, z * vz))
    (linearspace3.h:169), every madd one fused multiply-add.  The order matters to the check: a local origin that is rounded differently
    by a few 1e-6 moves t by that much over the cosine of the angle of incidence, which is beyond 1e-4 relative for near or grazing hits.
    exact=True: computed in float64 and asserted to be exactly representable in float32, so that the operation order cannot matter."""
    out = rays.copy()
    o = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1)
    d = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1)
    if exact:
        m = np.asarray(w2l, np.float64)
        lo = o.astype(np.float64) @ m[:, :3].T + m[:, 3]
        ld = d.astype(np.float64) @ m[:, :3].T
        assert np.array_equal(lo.astype(np.float32).astype(np.float64), lo), "local origins are not exact in fp32"
        assert np.array_equal(ld.astype(np.float32).astype(np.float64), ld), "local directions are not exact in fp32"
        lo, ld = lo.astype(np.float32), ld.astype(np.float32)
    else:
        m = np.asarray(w2l, np.float32)
        n = len(rays)
        col = lambda k, j: np.full(n, m[k, j], np.float32)  # noqa: E731
        lo = np.stack([fma32(o[:, 0], col(k, 0), fma32(o[:, 1], col(k, 1), fma32(o[:, 2], col(k, 2), col(k, 3)))) for k in range(3)], 1)
        ld = np.stack([fma32(d[:, 0], col(k, 0), fma32(d[:, 1], col(k, 1), (d[:, 2] * col(k, 2)).astype(np.float32))) for k in range(3)], 1)
    out["org_x"], out["org_y"], out["org_z"] = lo[:, 0], lo[:, 1], lo[:, 2]
    out["dir_x"], out["dir_y"], out["dir_z"] = ld[:, 0], ld[:, 1], ld[:, 2]
    return out


def oracle_instances(rtc, po, meshes, instances, rays, mode, exact=False):
    """meshes: {key: (verts, tris, geomID inside the instanced scene)}; instances: [(instance geomID, mesh key, l2w [3,4])].
    Returns (want, per) - the merged records, and per[i] = that instance's own oracle records for all rays (local-frame hits)."""
    scenes = {k: po.TriangleScene(v, t, mode, np.full(len(t), g, np.uint32)) for k, (v, t, g) in meshes.items()}
    per = []
    for gid, key, l2w in instances:
        sub = rtc.aligned_rayhits(len(rays))
        sub[:] = local_rays(rays, world2local(l2w), exact)
        scenes[key].intersect1M(sub, inst_id=gid, nthreads=16)
        per.append(sub)
    for s in scenes.values():
        s.free()
    t = np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf) for p in per])  # [instances, rays]
    best = np.argmin(t, axis=0)
    want = rays.copy()
    for i, p in enumerate(per):
        sel = (best == i) & np.isfinite(t[i])
        want["tfar"][sel] = p["tfar"][sel]
        for f in HITF:
            want[f][sel] = p[f][sel]
        want["instID"][sel] = instances[i][0]
    return want, per


def equal_t_ties(per):
    """rays for which two instances report the same t"""
    t = np.sort(np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf) for p in per]), axis=0)
    if t.shape[0] < 2:
        return 0
    return int((np.isfinite(t[0]) & (t[0] == t[1])).sum())


def set_aside(want, per):
    """The rays the general-transform GPU test may set aside: the winning local-frame oracle hit lies within 1e-4 of a triangle edge
    (min(u, v, 1 - u - v) < 1e-4), or a second instance's hit lies within 1e-4 relative in t."""
    hit = want["geomID"] != INVALID
    u, v = want["u"].astype(np.float64), want["v"].astype(np.float64)
    edge = hit & (np.minimum(np.minimum(u, v), 1.0 - u - v) < 1e-4)
    t = np.sort(np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf).astype(np.float64) for p in per]), axis=0)
    close = np.zeros(len(want), bool)
    if t.shape[0] >= 2:
        both = np.isfinite(t[1])
        close[both] = (t[1][both] - t[0][both]) <= 1e-4 * np.abs(t[0][both])
    return edge | close


# ---- the pinned inputs of the general-transform test (test_host_instances.py pins them on the CPU, test_gpu_instances.py traces them)
GENERAL_SEED = 11
GENERAL_RAYS = 20000


def general_instances():
    """9 instances with rotations and non-uniform scales on a 3 x 3 grid in the xz plane"""
    out = []
    for i in range(9):
        rot = rotation((1.0 + i, 2.0, 0.5 * i - 1.0), 25.0 + 37.0 * i)
        s = (0.6 + 0.15 * i, 1.3 - 0.08 * i, 0.8 + 0.05 * ((i * 5) % 9))
        t = (40.0 * (i % 3) - 40.0 + 0.37 * i, 3.0 * i - 12.0, 40.0 * (i // 3) - 40.0 - 0.21 * i)
        out.append((i, "m", affine(t, s, rot)))
    return out


def instances_bounds(meshes, instances):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for _, key, l2w in instances:
        v = meshes[key][0]
        c = np.array([[(v.min(0), v.max(0))[(k >> a) & 1][a] for a in range(3)] for k in range(8)])
        w = xfm_points(l2w, c)
        lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
    return lo, hi


def general_rays(rtc, po, meshes, instances, snapped=False, m=GENERAL_RAYS, seed=GENERAL_SEED):
    lo, hi = instances_bounds(meshes, instances)
    rays = rtc.aligned_rayhits(m)
    rays[:] = po.make_random_rays(m, lo.astype(np.float32), hi.astype(np.float32), seed=seed)
    if snapped:
        for f in ("org_x", "org_y", "org_z"):
            rays[f] = snap(rays[f])
    return rays
