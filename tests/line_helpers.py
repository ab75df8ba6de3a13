"""Shared by tests/test_host_lines.py and tests/test_gpu_lines.py: line segment inputs (RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE) and the truth
the GPU leaf is held to.

The oracle has no line intersector, so the truth is a NumPy restatement of LineIntersector1::intersect with its Precalculations
(kernels/geometry/line_intersector.h:53-98, frame() of common/math/linearspace3.h:126-133): every segment against every ray, no BVH.  The
closest hit is the minimum of t over all segments, whatever the leaf order, unless two segments tie.  `dtype` selects the arithmetic:
float64 (the truth) or float32 (the arithmetic of the kernel, csrc/trace_line.hip: fused multiply-adds where the reference has madd /
msub, 1 / sqrt for rsqrt, a true division for rcp)."""
import numpy as np

from mb_linear_helpers import LEAF, NODE_DT, fma32, scales, walk_paths  # noqa: F401  (re-exported for the tests)

INVALID = 0xFFFFFFFF
ROBUST = 4  # RTC_SCENE_FLAG_ROBUST
ACCEL_LINE_ROBUST, ACCEL_LINE_FAST = 36, 37
LINE_DT = np.dtype([("v0", "<f4", 3), ("r0", "<f4"), ("v1", "<f4", 3), ("r1", "<f4"), ("geomID", "<u4"), ("primID", "<u4"), ("pad", "<u4", 2)])
assert LINE_DT.itemsize == 48
LEAF_MAX = 28  # TRI_LEAF_MAX: records per leaf


def _fma(a, b, c, dt):
    if dt == np.float32:
        return fma32(a, b, c)
    return a * b + c


def _dot3(ax, ay, az, bx, by, bz, dt):
    """vec3.h:193: madd(a.x, b.x, madd(a.y, b.y, a.z * b.z))"""
    return _fma(ax, bx, _fma(ay, by, (az * bz).astype(dt), dt), dt)


def ray_space(dirs, dt):
    """Precalculations: (s [m], dx [m,3], dy [m,3], N [m,3]) - the rows of frame(s * dir).transposed() and the depth scale"""
    d = np.asarray(dirs, dt)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    one = dt(1)
    s = (one / np.sqrt((x * x + y * y + z * z).astype(dt))).astype(dt)
    nx, ny, nz = (s * x).astype(dt), (s * y).astype(dt), (s * z).astype(dt)
    zero = np.zeros_like(nx)
    l0 = (zero * zero + nz * nz + ny * ny).astype(dt)
    l1 = (nz * nz + zero * zero + nx * nx).astype(dt)
    first = l0 > l1
    ax, ay, az = np.where(first, zero, -nz), np.where(first, nz, zero), np.where(first, -ny, nx)
    ra = (one / np.sqrt((ax * ax + ay * ay + az * az).astype(dt))).astype(dt)
    dx = np.stack([ax * ra, ay * ra, az * ra], 1).astype(dt)
    cx = _fma(ny, dx[:, 2], -(nz * dx[:, 1]).astype(dt), dt)
    cy = _fma(nz, dx[:, 0], -(nx * dx[:, 2]).astype(dt), dt)
    cz = _fma(nx, dx[:, 1], -(ny * dx[:, 0]).astype(dt), dt)
    rc = (one / np.sqrt((cx * cx + cy * cy + cz * cz).astype(dt))).astype(dt)
    dy = np.stack([cx * rc, cy * rc, cz * rc], 1).astype(dt)
    return s, dx, dy, np.stack([nx, ny, nz], 1).astype(dt)


def candidates(v0, v1, org, dirs, tnear, tfar, dtype=np.float64, chunk=256, self_rule=True):
    """LineIntersector1::intersect of all n segments (v0, v1: [n, 4] = x, y, z, radius) against all m rays.
    Returns valid [m, n] bool, t [m, n], u [m, n], and margin [m, n] = |d2 - r2| / r2 (inf where r2 == 0).
    self_rule=False leaves the self-intersection rule `t > tnear + 2 r s` out: a deliberately wrong side for the tests of the tests."""
    dt = np.float32 if dtype == np.float32 else np.float64
    v0, v1 = np.asarray(v0, np.float32).astype(dt), np.asarray(v1, np.float32).astype(dt)
    org, tnear, tfar = np.asarray(org, np.float32).astype(dt), np.asarray(tnear, np.float32).astype(dt), np.asarray(tfar, np.float32).astype(dt)
    m, n = org.shape[0], v0.shape[0]
    s, dx, dy, nn = ray_space(np.asarray(dirs, np.float32), dt)
    valid, T, U, margin = np.zeros((m, n), bool), np.zeros((m, n), dt), np.zeros((m, n), dt), np.zeros((m, n), dt)
    nonzero = ((v1[:, :3] - v0[:, :3]) != 0).any(1)
    with np.errstate(all="ignore"):
        for a in range(0, m, chunk):
            b = min(m, a + chunk)
            o = org[a:b, None, :]
            rows = [r[a:b, None, :] for r in (dx, dy, nn)]
            p = []
            for v in (v0, v1):
                d = (v[None, :, :3] - o).astype(dt)  # [c, n, 3]
                p.append([_dot3(d[..., 0], d[..., 1], d[..., 2], r[..., 0], r[..., 1], r[..., 2], dt) for r in rows])
            (p0x, p0y, p0z), (p1x, p1y, p1z) = p
            vx, vy, vz, vw = (p1x - p0x).astype(dt), (p1y - p0y).astype(dt), (p1z - p0z).astype(dt), (v1[None, :, 3] - v0[None, :, 3]).astype(dt)
            wx, wy = -p0x, -p0y
            d0 = _fma(wx, vx, (wy * vy).astype(dt), dt)
            d1 = _fma(vx, vx, (vy * vy).astype(dt), dt)
            u = np.fmin(np.fmax((d0 * (dt(1) / d1).astype(dt)).astype(dt), dt(0)), dt(1))
            px, py, pz = _fma(u, vx, p0x, dt), _fma(u, vy, p0y, dt), _fma(u, vz, p0z, dt)
            pw = _fma(u, np.broadcast_to(vw, u.shape), np.broadcast_to(v0[None, :, 3], u.shape), dt)
            sc = s[a:b, None]
            t = (pz * sc).astype(dt)
            d2 = _fma(px, px, (py * py).astype(dt), dt)
            r2 = (pw * pw).astype(dt)
            tn, tf = tnear[a:b, None], tfar[a:b, None]
            ok = (d2 <= r2) & (tn < t) & (t <= tf) & nonzero[None, :]
            if self_rule:
                ok &= t > (tn + ((dt(2) * pw).astype(dt) * sc).astype(dt)).astype(dt)
            valid[a:b], T[a:b], U[a:b] = ok, t, u
            margin[a:b] = np.where(r2 > 0, np.abs(d2 - r2) / np.where(r2 > 0, r2, 1), np.inf)
    return valid, T, U, margin


def closest(v0, v1, org, dirs, tnear, tfar, dtype=np.float64, self_rule=True):
    """-> dict: hit [m] bool, seg [m] (index of the nearest valid segment, lowest index on equal t), t, u, Ng [m, 3] float32 = v1 - v0 in
    float32, near_edge [m] (some segment has |d2 - r2| <= 1e-4 r2), near_tie [m] (the two nearest candidates within 1e-4 relative in t)"""
    valid, T, U, margin = candidates(v0, v1, org, dirs, tnear, tfar, dtype, self_rule=self_rule)
    tt = np.where(valid, T, np.inf)
    seg = tt.argmin(1)
    m = tt.shape[0]
    t = tt[np.arange(m), seg]
    hit = np.isfinite(t)
    two = np.sort(tt, 1)[:, :2] if tt.shape[1] > 1 else np.concatenate([tt, np.full((m, 1), np.inf)], 1)
    with np.errstate(all="ignore"):
        near_tie = np.isfinite(two[:, 1]) & (np.abs(two[:, 1] - two[:, 0]) <= 1e-4 * np.abs(two[:, 0]))
    ng = (np.asarray(v1, np.float32)[:, :3] - np.asarray(v0, np.float32)[:, :3]).astype(np.float32)
    return {"hit": hit, "seg": seg, "t": t, "u": U[np.arange(m), seg], "Ng": ng[seg], "near_edge": (margin <= 1e-4).any(1), "near_tie": near_tie}


def leaf_rule(records, org, direction, tnear, tfar):
    """The leaf's block rule on ONE ray and the LineRecords of one leaf in their stored order (csrc/trace_line.hip): blocks of four from
    the leaf start, all four tested against the tfar at block entry, the lowest lane with the block's minimum t wins, a later block wins an
    equal t (`t <= tfar`).  -> (primID, t) of the hit or (None, tfar)."""
    best = None
    v0 = np.concatenate([records["v0"], records["r0"][:, None]], 1)
    v1 = np.concatenate([records["v1"], records["r1"][:, None]], 1)
    for b in range(0, len(records), 4):
        valid, T, _, _ = candidates(v0[b:b + 4], v1[b:b + 4], np.asarray([org], np.float32), np.asarray([direction], np.float32), [tnear], [tfar], np.float32)
        tt = np.where(valid[0], T[0], np.inf)
        k = int(tt.argmin())  # the first (lowest) lane with the minimum
        if np.isfinite(tt[k]):
            best, tfar = int(records["primID"][b + k]), np.float32(tt[k])
    return best, tfar


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
TUFT_SEGMENTS, TUFT_RAYS, TUFT_HITS = 2048, 4096, 3239  # the pinned input and the hits its float64 truth has


def tuft_and_rays(n=TUFT_SEGMENTS, m=TUFT_RAYS, seed=1):
    """The pinned random tuft and its rays, all from ONE numpy.random.default_rng(seed) in this order of draws: starts uniform in the unit
    cube, directions (normal, normalised), lengths uniform in [0.02, 0.1], radii uniform in [0.004, 0.012] of the first ends, then of
    the second ends; ray origins (normal, normalised, on the sphere of radius 2 about the cube's centre), then their targets uniform in
    the cube.  Directions are not normalised; every segment has vertices of its own.
    -> (verts4 [2n, 4], first_index [n], org [m, 3], dirs [m, 3])"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ln = rng.uniform(0.02, 0.1, n)
    r0, r1 = rng.uniform(0.004, 0.012, n), rng.uniform(0.004, 0.012, n)
    v = np.zeros((2 * n, 4), np.float32)
    v[0::2, :3], v[1::2, :3] = p, p + d * ln[:, None]
    v[0::2, 3], v[1::2, 3] = r0, r1
    o = rng.normal(size=(m, 3))
    o = 0.5 + 2.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    to = rng.random((m, 3))
    return v, np.arange(0, 2 * n, 2, dtype=np.uint32), o.astype(np.float32), (to - o).astype(np.float32)


def ends(verts4, first_index):
    """(v0 [n, 4], v1 [n, 4]) of the segments"""
    v, i = np.asarray(verts4, np.float32).reshape(-1, 4), np.asarray(first_index, np.int64)
    return v[i], v[i + 1]


def decode_children(node):
    """(lo [8, 3], hi [8, 3]) of a QNode8's children with the node step's arithmetic: plane = fmaf(float(q), scale, origin)"""
    q = node["q"].astype(np.float32)  # [6, 8]
    s, o = np.repeat(scales(node), 2)[:, None], np.repeat(node["origin"], 2)[:, None]
    p = fma32(q, s, o)
    return p[0::2].T.copy(), p[1::2].T.copy()


def segment_box(rec):
    """LineMi::bounds in float32: merge(p0, p1) enlarged on every side by max(r0, r1)"""
    r = np.maximum(rec["r0"], rec["r1"]).astype(np.float32)
    return (np.minimum(rec["v0"], rec["v1"]) - r).astype(np.float32), (np.maximum(rec["v0"], rec["v1"]) + r).astype(np.float32)


def rays_of(rtc, org, dirs, tnear=0.0, tfar=np.inf):
    from helpers import fill_rays
    rh = rtc.aligned_rayhits(len(org))
    fill_rays(rh, np.asarray(org, np.float32), np.asarray(dirs, np.float32), tnear, tfar)
    return rh


def occ_of(rtc, rh):
    occ = rtc.aligned_rays(len(rh))
    for f in occ.dtype.names:
        occ[f] = rh[f]
    return occ
