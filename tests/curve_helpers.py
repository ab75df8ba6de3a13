"""Shared by tests/test_host_curves.py and tests/test_gpu_curves.py: flat cubic curve inputs (RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE /
_FLAT_BSPLINE_CURVE) and the truth the GPU leaf is held to.

The oracle has no curve intersector, so the truth is a NumPy restatement of Ribbon1Intersector1 + intersect_ribbon (kernels/geometry/
bezier_ribbon_intersector.h:80-201) + intersect_quad_backface_culling (quad_intersector.h:28-90) without the cylinder culling test: every
segment of every curve against every ray, no BVH.  The closest hit is the minimum of t over all segments of all curves, whatever the leaf
order, unless two candidates tie.  `dtype` selects the arithmetic: float64 (the truth) or float32 (the arithmetic of the kernel,
csrc/trace_curve.hip: fused multiply-adds where the reference has madd / msub, 1 / sqrt for rsqrt, a true division for rcp)."""
import numpy as np

from line_helpers import INVALID, LEAF, NODE_DT, ROBUST, _dot3, _fma, decode_children, fma32, occ_of, ray_space, rays_of, walk_paths  # noqa: F401  (re-exported)

ACCEL_CURVE_ROBUST, ACCEL_CURVE_FAST = 42, 43
CURVE_DT = np.dtype([("v", "<f4", (4, 4)), ("geomID", "<u4"), ("primID", "<u4"), ("N", "<u4"), ("pad", "<u4")])  # v[k] = (x, y, z, radius) of control point k
assert CURVE_DT.itemsize == 80


def _f(x, dt):
    return np.asarray(x).astype(dt)


def bezier_basis(u, dt):
    """BezierBasis::eval (kernels/subdiv/bezier_curve.h:27-37), the products in the reference's order"""
    t1 = _f(u, dt)
    t0 = (dt(1) - t1).astype(dt)
    return [((t0 * t0).astype(dt) * t0).astype(dt), ((dt(3) * t1).astype(dt) * (t0 * t0).astype(dt)).astype(dt),
            ((dt(3) * (t1 * t1).astype(dt)).astype(dt) * t0).astype(dt), ((t1 * t1).astype(dt) * t1).astype(dt)]


def bezier_derivative(u, dt):
    """BezierBasis::derivative (bezier_curve.h:39-49)"""
    t1 = _f(u, dt)
    t0 = (dt(1) - t1).astype(dt)
    t01, t00, t11 = (t0 * t1).astype(dt), (t0 * t0).astype(dt), (t1 * t1).astype(dt)
    b = [-t00, _fma(dt(-2), t01, t00, dt), _fma(dt(2), t01, -t11, dt), t11]
    return [(dt(3) * x).astype(dt) for x in b]


def bezier_derivative2(u, dt):
    t1 = _f(u, dt)
    t0 = (dt(1) - t1).astype(dt)
    return [(dt(6) * x).astype(dt) for x in (t0, _fma(dt(-2), t0, t1, dt), _fma(dt(-2), t1, t0, dt), t1)]


def combine(b, p0, p1, p2, p3, dt):
    """madd(b.x, v0, madd(b.y, v1, madd(b.z, v2, b.w * v3)))"""
    return _fma(b[0], p0, _fma(b[1], p1, _fma(b[2], p2, (b[3] * p3).astype(dt), dt), dt), dt)


def bspline_basis64(u):
    """BSplineBasis2 eval / derivative / derivative2 (kernels/subdiv/bspline_curve.h:28-62) in float64"""
    t, s = np.float64(u), 1.0 - np.float64(u)
    n = [s ** 3, 4 * s ** 3 + t ** 3 + 12 * s * s * t + 6 * s * t * t, 4 * t ** 3 + s ** 3 + 12 * t * t * s + 6 * t * s * s, t ** 3]
    d = [-s * s, -t * t - 4 * t * s, s * s + 4 * s * t, t * t]
    return [x / 6 for x in n], [x / 2 for x in d], [s, t - 2 * s, s - 2 * t, t]


def bspline_to_bezier(cp, dt=np.float32):
    """convert(BSplineCurveT, BezierCurveT) (bspline_curve.h:180-187) on control points [n, 4, 4], all four components"""
    cp = _f(np.asarray(cp, np.float32), dt)
    a, b, c, d = cp[:, 0], cp[:, 1], cp[:, 2], cp[:, 3]
    s6, s3, t3 = dt(np.float32(1.0) / np.float32(6.0)), dt(np.float32(1.0) / np.float32(3.0)), dt(np.float32(2.0) / np.float32(3.0))
    if dt == np.float64:
        s6, s3, t3 = 1.0 / 6.0, 1.0 / 3.0, 2.0 / 3.0
    out = np.zeros_like(cp)
    out[:, 0] = _fma(s6, a, _fma(t3, b, (s6 * c).astype(dt), dt), dt)
    out[:, 1] = _fma(t3, b, (s3 * c).astype(dt), dt)
    out[:, 2] = _fma(s3, b, (t3 * c).astype(dt), dt)
    out[:, 3] = _fma(s6, b, _fma(t3, c, (s6 * d).astype(dt), dt), dt)
    return out


def control_points(verts4, first_index):
    """[n, 4, 4]: the four vertices first_index[i] .. + 3 of every curve"""
    v, i = np.asarray(verts4, np.float32).reshape(-1, 4), np.asarray(first_index, np.int64)
    return np.stack([v[i], v[i + 1], v[i + 2], v[i + 3]], 1)


def native(verts4, first_index, basis="bezier"):
    """the Bezier control points the records hold, float32 [n, 4, 4]"""
    cp = control_points(verts4, first_index)
    return bspline_to_bezier(cp, np.float32) if basis == "bspline" else cp


def tessellated_bounds(cp, N, dt=np.float32):
    """BezierCurve3fa::tessellatedBounds(N) (bezier_curve.h:298-331): the box of eval0(j, N), j < N, and v3, enlarged by the largest |radius|
    among them.  cp [n, 4, 4] -> (lo [n, 3], hi [n, 3])"""
    cp = _f(np.asarray(cp, np.float32), dt)
    u = (np.arange(N).astype(dt) / dt(N)).astype(dt)
    b = [x[None, :, None] for x in bezier_basis(u, dt)]  # [1, N, 1]
    p = combine(b, cp[:, None, 0], cp[:, None, 1], cp[:, None, 2], cp[:, None, 3], dt)  # [n, N, 4]
    p = np.concatenate([p, cp[:, None, 3]], 1)
    r = np.abs(p[..., 3]).max(1)[:, None]
    return (p[..., :3].min(1) - r).astype(dt), (p[..., :3].max(1) + r).astype(dt)


def candidates(cp, N, org, dirs, tnear, tfar, dtype=np.float64, chunk=64):
    """intersect_ribbon of all n curves (cp [n, 4, 4] native control points, N segments each) against all m rays.
    Returns valid [m, n, N] bool, t, u, v [m, n, N] (the hit's u = (j + U) / N and v = 2 V - 1), margin [m, n, N] = |max(U, V) / den| and
    again [m, n, N] bool: the candidate passes the depth test once more with its own t as tfar, `T <= absDen * t` - true in exact
    arithmetic, in float32 only where absDen * fl(T / den) does not round below T."""
    dt = np.float32 if dtype == np.float32 else np.float64
    cp = np.asarray(cp, np.float32).astype(dt)
    org, tnear, tfar = np.asarray(org, np.float32).astype(dt), np.asarray(tnear, np.float32).astype(dt), np.asarray(tfar, np.float32).astype(dt)
    m, n = org.shape[0], cp.shape[0]
    s, dx, dy, nn = ray_space(np.asarray(dirs, np.float32), dt)
    nz = (nn * s[:, None]).astype(dt)  # ray_space.vz *= depth_scale
    shape = (m, n, N)
    valid, T, U, V, margin = np.zeros(shape, bool), np.zeros(shape, dt), np.zeros(shape, dt), np.zeros(shape, dt), np.zeros(shape, dt)
    again = np.zeros(shape, bool)
    uu = (np.arange(N + 1).astype(dt) / dt(N)).astype(dt)
    bas = [x[None, None, :] for x in bezier_basis(uu, dt)]
    der = [x[None, None, :] for x in bezier_derivative(uu, dt)]
    jj = np.arange(N).astype(dt)[None, None, :]
    with np.errstate(all="ignore"):
        for a in range(0, m, chunk):
            b = min(m, a + chunk)
            o = org[a:b, None, :]
            rows = [r[a:b, None, :] for r in (dx, dy, nz)]
            w = []  # ray-space control points: [c, n, 1] per component
            for k in range(4):
                d = (cp[None, :, k, :3] - o).astype(dt)
                w.append([_dot3(d[..., 0], d[..., 1], d[..., 2], r[..., 0], r[..., 1], r[..., 2], dt)[..., None] for r in rows] + [np.broadcast_to(cp[None, :, k, 3, None], (b - a, n, 1))])
            px, py, pz, pw = (combine(bas, w[0][c], w[1][c], w[2][c], w[3][c], dt) for c in range(4))  # [c, n, N + 1]
            ddx, ddy = (combine(der, w[0][c], w[1][c], w[2][c], w[3][c], dt) for c in range(2))
            nx, ny = ddy, -ddx
            rs = (dt(1) / np.sqrt(_fma(nx, nx, _fma(ny, ny, np.zeros_like(nx), dt), dt))).astype(dt)
            nnx, nny = (nx * rs).astype(dt), (ny * rs).astype(dt)
            lx, ly, ux, uy = _fma(pw, nnx, px, dt), _fma(pw, nny, py, dt), _fma(-pw, nnx, px, dt), _fma(-pw, nny, py, dt)
            A = {k: v[..., :-1] for k, v in (("lx", lx), ("ly", ly), ("ux", ux), ("uy", uy), ("z", pz), ("w", pw))}
            B = {k: v[..., 1:] for k, v in (("lx", lx), ("ly", ly), ("ux", ux), ("uy", uy), ("z", pz), ("w", pw))}
            edbx, edby = (B["lx"] - A["ux"]).astype(dt), (B["ly"] - A["uy"]).astype(dt)
            WW = _fma(A["ux"], edby, -(A["uy"] * edbx).astype(dt), dt)
            first = WW <= 0
            v0x, v0y, v0z = np.where(first, A["lx"], B["ux"]), np.where(first, A["ly"], B["uy"]), np.where(first, A["z"], B["z"])
            v1x, v1y, v1z = np.where(first, B["lx"], A["ux"]), np.where(first, B["ly"], A["uy"]), np.where(first, B["z"], A["z"])
            v2x, v2y, v2z = np.where(first, A["ux"], B["lx"]), np.where(first, A["uy"], B["ly"]), np.where(first, A["z"], B["z"])
            e0x, e0y, e0z = (v2x - v0x).astype(dt), (v2y - v0y).astype(dt), (v2z - v0z).astype(dt)
            e1x, e1y, e1z = (v0x - v1x).astype(dt), (v0y - v1y).astype(dt), (v0z - v1z).astype(dt)
            Ue = _fma(v0x, e0y, -(v0y * e0x).astype(dt), dt)
            Ve = _fma(v1x, e1y, -(v1y * e1x).astype(dt), dt)
            mx = np.where(Ue > Ve, Ue, Ve)
            ngx = _fma(e1y, e0z, -(e1z * e0y).astype(dt), dt)
            ngy = _fma(e1z, e0x, -(e1x * e0z).astype(dt), dt)
            den = _fma(e1x, e0y, -(e1y * e0x).astype(dt), dt)
            absden = np.abs(den)
            Tn = _dot3(v0x, v0y, v0z, ngx, ngy, den, dt)
            Ts = np.where(np.signbit(den), -Tn, Tn)
            tn, tf, sc = tnear[a:b, None, None], tfar[a:b, None, None], s[a:b, None, None]
            ok = (mx <= 0) & ((absden * tn).astype(dt) < Ts) & (Ts <= (absden * tf).astype(dt)) & (den != 0)
            rcp = (dt(1) / den).astype(dt)
            t, u, v = (Tn * rcp).astype(dt), (Ue * rcp).astype(dt), (Ve * rcp).astype(dt)
            u, v = np.where(first, u, (dt(1) - u).astype(dt)), np.where(first, v, (dt(1) - v).astype(dt))
            rad = _fma((dt(1) - u).astype(dt), A["w"], (u * B["w"]).astype(dt), dt)
            ok &= t > (tn + ((dt(2) * rad).astype(dt) * sc).astype(dt)).astype(dt)
            valid[a:b], T[a:b] = ok, t
            U[a:b] = (((jj % 8 + u).astype(dt) + (jj - jj % 8)).astype(dt) * (dt(1) / dt(N))).astype(dt)  # (step + U + float(i)) * (1 / N)
            V[a:b] = _fma(dt(2), v, np.full_like(v, -1), dt)
            margin[a:b] = np.abs(mx / den)
            again[a:b] = ok & (Ts <= (absden * t).astype(dt))
    return valid, T, U, V, margin, again


def closest(groups, org, dirs, tnear, tfar, dtype=np.float64):
    """groups: [(cp [n, 4, 4], N, geomID)].  -> dict: hit [m], geomID [m], primID [m] (index in its group), t, u, v, Ng [m, 3] (eval_du(u) of the
    world control points, in `dtype`), near_edge [m] (some segment has |max(U, V) / den| <= 1e-4), near_tie [m] (the two nearest candidates
    within 1e-4 relative in t), again [m] (candidates(): a coincident copy of the winner tested later would pass `T <= absDen * tfar`).
    On an equal t the first group, lowest curve, lowest segment wins."""
    dt = np.float32 if dtype == np.float32 else np.float64
    m = len(org)
    tt, uu, vv, gg, pp, cps, ag = [], [], [], [], [], [], []
    near_edge = np.zeros(m, bool)
    for cp, N, gid in groups:
        valid, T, U, V, margin, again = candidates(cp, N, org, dirs, tnear, tfar, dtype)
        n = len(cp)
        ag.append(again.reshape(m, -1))
        tt.append(np.where(valid, T, np.inf).reshape(m, -1))
        uu.append(U.reshape(m, -1))
        vv.append(V.reshape(m, -1))
        gg.append(np.full(n * N, gid, np.int64))
        pp.append(np.repeat(np.arange(n), N))
        cps.append(np.asarray(cp, np.float32))
        near_edge |= (margin <= 1e-4).reshape(m, -1).any(1)
    tt, uu, vv, gg, pp = np.concatenate(tt, 1), np.concatenate(uu, 1), np.concatenate(vv, 1), np.concatenate(gg), np.concatenate(pp)
    k = tt.argmin(1)
    ar = np.arange(m)
    t = tt[ar, k]
    hit = np.isfinite(t)
    two = np.sort(tt, 1)[:, :2] if tt.shape[1] > 1 else np.concatenate([tt, np.full((m, 1), np.inf)], 1)
    with np.errstate(all="ignore"):
        near_tie = np.isfinite(two[:, 1]) & (np.abs(two[:, 1] - two[:, 0]) <= 1e-4 * np.abs(two[:, 0]))
    u = uu[ar, k]
    allcp = np.concatenate(cps, 0).astype(dt)
    base = np.cumsum([0] + [len(c) for c in cps])[:-1]
    gidx = {g[2]: b for g, b in zip(groups, base)}
    row = np.array([gidx[int(g)] for g in gg[k]]) + pp[k]
    c = allcp[row]  # [m, 4, 4]
    d = [x[:, None] for x in bezier_derivative(u, dt)]
    ng = combine(d, c[:, 0, :3], c[:, 1, :3], c[:, 2, :3], c[:, 3, :3], dt)
    return {"hit": hit, "geomID": gg[k], "primID": pp[k], "t": t, "u": u, "v": vv[ar, k], "Ng": ng, "near_edge": near_edge, "near_tie": near_tie,
            "again": np.concatenate(ag, 1)[ar, k], "cp": c}


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
HAIR_CURVES, HAIR_RAYS = 512, 2048  # the pinned input


def hair_and_rays(n=HAIR_CURVES, m=HAIR_RAYS, seed=1):
    """The pinned random hair and its rays, all from ONE numpy.random.default_rng(seed) in this order of draws: starts uniform in the unit
    cube; a unit direction per curve (normal, normalised); a length per curve uniform in [0.05, 0.2]; then for each of the four control
    points k in turn its position start + dir * length * k / 3 plus, for k > 0, a normal offset of sigma 0.015, and its radius uniform in
    [0.004, 0.012]; ray origins (normal, normalised, on the sphere of radius 2 about the cube's centre), then their targets uniform in the
    cube.  Directions are not normalised; every curve has vertices of its own.
    -> (verts4 [4n, 4], first_index [n], org [m, 3], dirs [m, 3])"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ln = rng.uniform(0.05, 0.2, n)
    v = np.zeros((4 * n, 4), np.float32)
    for k in range(4):
        q = p + d * ln[:, None] * (k / 3.0)
        if k > 0:
            q = q + rng.normal(scale=0.015, size=(n, 3))
        v[k::4, :3] = q
        v[k::4, 3] = rng.uniform(0.004, 0.012, n)
    o = rng.normal(size=(m, 3))
    o = 0.5 + 2.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    to = rng.random((m, 3))
    return v, np.arange(0, 4 * n, 4, dtype=np.uint32), o.astype(np.float32), (to - o).astype(np.float32)


# hits of the float64 truth on hair_and_rays() per tessellation rate, and the rays its two exclusion rules leave out
HAIR_HITS = {1: 932, 3: 1072, 4: 1078, 8: 1087, 9: 1086, 16: 1091}
HAIR_LEFT_OUT = {1: 0, 3: 3, 4: 0, 8: 0, 9: 0, 16: 3}
_TRUTH = {}


def hair_truth(N):
    """closest() in float64 of the pinned hair at rate N, tnear 0 and tfar inf; computed once per process and never changed"""
    if N not in _TRUTH:
        v, idx, org, dirs = hair_and_rays()
        m = len(org)
        _TRUTH[N] = closest([(native(v, idx), N, 0)], org, dirs, np.zeros(m, np.float32), np.full(m, np.inf, np.float32), np.float64)
    return _TRUTH[N]


def compare(got_hit, got_geom, got_prim, got_t, got_u, got_v, want, what=""):
    """The tolerances of the line tests on the rays the truth `want` (closest(), float64) does not leave out: hit / miss, geomID and primID
    exact, t within 1e-4 relative, u and v within 1e-4 absolute.  Prints the figures, asserts the cap of 0.5 % on the rays left out and
    returns (rays left out, max t error, max u error, max v error)."""
    out = want["near_edge"] | want["near_tie"]
    keep = ~out
    m = len(out)
    h = want["hit"] & keep
    flips = int((got_hit[keep] != want["hit"][keep]).sum())
    both = h & got_hit
    ids = int(((got_geom[both] != want["geomID"][both]) | (got_prim[both] != want["primID"][both])).sum())
    same = both & (got_geom == want["geomID"]) & (got_prim == want["primID"])
    with np.errstate(all="ignore"):
        et = np.abs(got_t[same].astype(np.float64) - want["t"][same]) / np.abs(want["t"][same])
    eu = np.abs(got_u[same].astype(np.float64) - want["u"][same])
    ev = np.abs(got_v[same].astype(np.float64) - want["v"][same])
    mt, mu, mv = (float(e.max()) if e.size else 0.0 for e in (et, eu, ev))
    print("%s: %d hits, %d rays left out, %d hit flips, %d id differences, t %.1e u %.1e v %.1e" % (what, int(want["hit"].sum()), int(out.sum()), flips, ids, mt, mu, mv))
    assert out.sum() <= 0.005 * m, (what, int(out.sum()))
    assert flips == 0 and ids == 0, (what, flips, ids)
    assert mt <= 1e-4 and mu <= 1e-4 and mv <= 1e-4, (what, mt, mu, mv)
    return int(out.sum()), mt, mu, mv


def curve_box(rec):
    """tessellated_bounds of CurveRecords, float32"""
    lo, hi = np.zeros((len(rec), 3), np.float32), np.zeros((len(rec), 3), np.float32)
    for N in np.unique(rec["N"]):
        sel = rec["N"] == N
        lo[sel], hi[sel] = tessellated_bounds(rec["v"][sel], int(N), np.float32)
    return lo, hi
