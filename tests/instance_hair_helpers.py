"""Shared by tests/test_host_instance_hair.py and tests/test_gpu_instance_hair.py: instanced scenes that hold line segments and flat
curves (device config inst_hair=1), alone or beside triangle and quad meshes - the kinds 22 / 23 with the hair form of the two-level
kernel (embree-compressed_amd/csrc/trace_instance_hair.hip).

An instanced scene is described as instance_mesh_mb_helpers describes one, with two more entries:
    {"tris": ..., "quads": ..., "tris_mb": ..., "quads_mb": ...,
     "curves": [(verts4, first_index, basis, tessellation rate, geomID), ...] or None, "lines": (verts4, first_index, geomID) or None}
Instances are (geomID, scene key, [local-to-world per step]) as in instance_mb_helpers.

The layout (csrc/accel.h InstanceRecord / InstanceSceneRecord): `blobs` = the general layout of instance_mesh_mb_helpers, then zero
padding to a multiple of 80 bytes and every scene's CurveRecords, then zero padding to a multiple of 48 bytes and every scene's
LineRecords; a scene record holds six roots in visiting order - triangles, motion-blur triangles, quads, motion-blur quads, curves,
lines - with REF_EMPTY for a missing tree."""
import numpy as np

import curve_helpers as ch
import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
import line_helpers as lh
from instance_helpers import EMPTY, LEAF

HOST_CFG = "gpu=none,inst_accel=default,hair_accel=default,quad_accel=default,tri_accel_mb=default,inst_hair=1"
GPU_CFG = "inst_hair=1"
SCENE_DT = np.dtype([("triRoot", "<u4"), ("triMBRoot", "<u4"), ("quadRoot", "<u4"), ("quadMBRoot", "<u4"), ("curveRoot", "<u4"), ("lineRoot", "<u4"), ("pad", "<u4", 10)])
TREE_CURVE, TREE_LINE = 4, 5
VISIT = imm.VISIT + (("curveRoot", TREE_CURVE), ("lineRoot", TREE_LINE))
F32 = np.float32
REFUSE_MOTION = "motion blur of line segments and flat curves inside an instanced scene is not supported"
REFUSE_LINEAR = ("inst_hair=1: line segments and flat curves below an instance are traced over swept boxes only (kinds 22 / 23); not beside "
                 "inst_bounds=linear or inst_mb_bounds=linear trees")
REFUSE_FILTER = "inst_hair=1: geometry filter functions below the instances of a scene with instanced line segments or flat curves are not supported"
REFUSE_CONTEXT = "inst_hair=1: RTCIntersectContext::filter is not supported on a scene with instanced line segments or flat curves"
OLD_CURVES = "flat Bezier and B-spline curves inside an instanced scene are not supported"
OLD_ONLY = "an instanced scene may hold triangle and quad meshes only (no subdivision meshes or instances)"


def desc(tris=None, quads=None, tris_mb=None, quads_mb=None, curves=None, lines=None):
    return {"tris": tris, "quads": quads, "tris_mb": tris_mb, "quads_mb": quads_mb, "curves": curves, "lines": lines}


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def strands(n_strands=12, per=8, seed=3, extent=8.0, step=1.0, radius=(0.1, 0.3)):
    """n_strands x per line segments, the segments of a strand share their end points: (verts4, first_index)"""
    rng = np.random.default_rng(seed)
    verts, idx = [], []
    for _ in range(n_strands):
        p = rng.random(3) * extent
        d = rng.normal(size=3)
        for k in range(per + 1):
            verts.append(np.concatenate([p, [rng.uniform(*radius)]]))
            if k < per:
                idx.append(len(verts) - 1)
            d = d + 0.5 * rng.normal(size=3)
            p = p + step * d / np.linalg.norm(d)
    return np.array(verts, F32), np.array(idx, np.uint32)


def tuft(n=24, seed=4, extent=8.0, length=(2.0, 5.0), radius=(0.1, 0.3), sigma=0.4):
    """n cubic curves with control points of their own, curve_helpers.hair_and_rays scaled up: (verts4, first_index)"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * extent
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ln = rng.uniform(*length, n)
    v = np.zeros((4 * n, 4), F32)
    for k in range(4):
        q = p + d * ln[:, None] * (k / 3.0)
        if k > 0:
            q = q + rng.normal(scale=sigma, size=(n, 3))
        v[k::4, :3] = q
        v[k::4, 3] = rng.uniform(*radius, n)
    return v, np.arange(0, 4 * n, 4, dtype=np.uint32)


def curve_geometries(first_gid=0, n=24, seed=10):
    """Bezier and B-spline geometries at the tessellation rates 1, 4, 9 and 16 (rates above 8 take the leaf's second pass)"""
    out = []
    for k, (basis, rate) in enumerate((b, r) for r in (1, 4, 9, 16) for b in ("bezier", "bspline")):
        v, idx = tuft(n, seed + k)
        out.append((v, idx, basis, rate, first_gid + k))
    return out


def coincident_meshes(gid_tris=1, gid_quads=2, n=6, seed=8, extent=8.0):
    """n squares as two triangles each and the same squares as quads: the quad tree comes later and wins the bit-identical t"""
    rng = np.random.default_rng(seed)
    c = ih.snap(rng.random((n, 3)) * extent)
    e = 1.5
    v = np.concatenate([c[:, None, :] + np.array([[0, 0, 0], [e, 0, 0], [e, e, 0], [0, e, 0]])[None] for _ in range(1)], 0).reshape(-1, 3).astype(F32)
    q = (np.arange(n)[:, None] * 4 + np.arange(4)[None]).astype(np.uint32)
    t = np.concatenate([q[:, [0, 1, 3]], q[:, [2, 3, 1]]], 1).reshape(-1, 3).astype(np.uint32)  # the quad's own split: A = (v0, v1, v3), B = (v2, v3, v1)
    return (v, t, gid_tris), (v, q, gid_quads)


def moving_triangles(gid=3, n=40, seed=9, extent=8.0):
    """a small soup with two time steps on the 2^-10 grid"""
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3)) * extent
    v0 = ih.snap((c + rng.normal(scale=0.8, size=(n, 3, 3))).reshape(-1, 3))
    v1 = ih.snap(v0 + np.array([0.5, -0.25, 0.375]))
    return ([v0.astype(F32), v1.astype(F32)], np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), gid)


def scenes(which):
    """the five inner scenes of the short-ray leg: (a) lines, (b) curves, (c) curves + lines, (d) triangles + quads + curves + lines,
    (e) motion-blur triangles + lines"""
    ls = strands() + (0,)
    if which == "a":
        return {"m": desc(lines=ls)}
    if which == "b":
        return {"m": desc(curves=curve_geometries())}
    if which == "c":
        return {"m": desc(curves=curve_geometries(first_gid=1, n=12), lines=ls)}
    if which == "d":
        t, q = coincident_meshes(gid_tris=1, gid_quads=2)
        return {"m": desc(tris=t, quads=q, curves=curve_geometries(first_gid=3, n=12)[2:6], lines=ls)}
    if which == "e":
        return {"m": desc(tris_mb=moving_triangles(gid=3), lines=ls)}
    raise KeyError(which)


def points(d):
    """every point of a scene description with the radii added on all sides (curves: the control points, whose hull holds the curve)"""
    out = []
    for p in ("tris", "quads"):
        if d.get(p) is not None:
            out.append(np.asarray(d[p][0], np.float64))
    for p in ("tris_mb", "quads_mb"):
        if d.get(p) is not None:
            out += [np.asarray(s, np.float64) for s in d[p][0]]
    hair = list(d.get("curves") or []) + ([d["lines"]] if d.get("lines") is not None else [])
    for g in hair:
        v = np.asarray(g[0], np.float64).reshape(-1, 4)
        r = np.abs(v[:, 3]).max()  # (a curve's box is enlarged by the largest radius among its points)
        out += [v[:, :3] - r, v[:, :3] + r]
    return np.concatenate(out)


def bounds_meshes(scs):
    """{key: (points,)} as instance_subdiv_helpers.mesh_box and instance_helpers.instances_bounds read it"""
    return {k: (points(d),) for k, d in scs.items()}


# ---- building ---------------------------------------------------------------------------------------------------------------------------
def add_scene(rtc, dev, d, mode):
    sc = rtc.Scene(dev, iq.flags(mode))
    for part, add in (("tris", sc.add_triangles), ("tris_mb", sc.add_triangles_mb), ("quads", sc.add_quads), ("quads_mb", sc.add_quads_mb)):
        if d.get(part) is not None:
            v, idx, gid = d[part]
            assert add(v, idx, geom_id=gid) == gid
    for v, idx, basis, rate, gid in (d.get("curves") or []):
        assert sc.add_curves(v, idx, basis=basis, tessellation_rate=rate, geom_id=gid) == gid
    if d.get("lines") is not None:
        v, idx, gid = d["lines"]
        assert sc.add_lines(v, idx, geom_id=gid) == gid
    sc.commit()
    return sc


def build(rtc, mode, scs, instances, cfg=GPU_CFG, extra=None, commit=True):
    dev = rtc.Device(cfg)
    inner = {k: add_scene(rtc, dev, d, mode) for k, d in scs.items()}
    top = rtc.Scene(dev, iq.flags(mode))
    for gid, key, steps in instances:
        if len(steps) == 1:
            assert top.add_instance(inner[key], steps[0], geom_id=gid) == gid
        else:
            assert top.add_instance_mb(inner[key], steps, geom_id=gid) == gid
    keep = extra(top, dev) if extra else None
    if commit:
        top.commit()
    top._extra_keep = keep
    return dev, top, inner


def release(dev, top, inner):
    top.release()
    for s in inner.values():
        s.release()
    for s in (getattr(top, "_extra_keep", None) or []):
        s.release()
    dev.release()


# ---- decoding the accel -------------------------------------------------------------------------------------------------------------------
def split_blobs(blobs, n_inst, n_quads, n_steps, n_scenes, n_trimb, n_quadmb, n_curves, n_lines):
    """the sections of `blobs`: (InstanceRecords, QuadRecords, steps, scene records, TriMBRecords, QuadMBRecords, CurveRecords, LineRecords,
    byte offset of the curve section, byte offset of the line section); asserts alignment, zero padding and the total size"""
    o = 64 * (n_inst + n_quads + n_steps + n_scenes)
    recs = blobs[: 64 * n_inst].view(ih.INST_DT)
    quads = blobs[64 * n_inst: 64 * (n_inst + n_quads)].view(iq.QUAD_DT)
    steps = blobs[64 * (n_inst + n_quads): 64 * (n_inst + n_quads + n_steps)].view(im.STEP_DT)
    scs = blobs[o - 64 * n_scenes: o].view(SCENE_DT)
    out = []
    for size, n in ((96, n_trimb), (128, n_quadmb), (80, n_curves), (48, n_lines)):
        off = (o + size - 1) // size * size
        assert not blobs[o:off].any() and off % size == 0
        out.append((off, blobs[off: off + size * n]))
        o = off + size * n
    assert o == len(blobs), (o, len(blobs))
    return (recs, quads, steps, scs, out[0][1].view(ds.TRIMB_DT), out[1][1].view(ds.QUADMB_DT), out[2][1].view(ch.CURVE_DT), out[3][1].view(lh.LINE_DT),
            out[2][0], out[3][0])


def leaf_records(nodes, root):
    """the record indices of every leaf below root, in the order met, and the depth"""
    leaves, depth = imm.walk(nodes, root)
    idx = [i for first, count in leaves for i in range(first, first + count)]
    return idx, leaves, depth


# ---- the stack walk of a ray that hits nothing (static instances) --------------------------------------------------------------------------
def simulate_stack(nodes, root, blobs, n_inst, org, dirs):
    """The kernel's walk without primitive tests - the walk of a ray that hits nothing - for the kinds 22 / 23 with six roots per scene
    record: entering an instance stacks the exit marker and, in reverse visiting order, one marker per pending tree.  Closest-hit order
    (nearest child first, the others stacked far to near).  Returns per ray the deepest slot written."""
    lo, hi, child = ds.decode_nodes(nodes)
    recs = blobs[: 64 * n_inst].view(ih.INST_DT)
    words = blobs.view(np.uint32)
    out = []
    for i in range(len(org)):
        wo, wd = np.asarray(org[i], np.float64), np.asarray(dirs[i], np.float64)
        o, d = wo, wd
        stack, deepest, cur = [], -1, int(root)
        while True:
            if cur != EMPTY and not (cur & LEAF):
                with np.errstate(divide="ignore", invalid="ignore"):
                    t1, t2 = (lo[cur] - o) / d, (hi[cur] - o) / d
                tn = np.fmax(np.minimum(t1, t2).max(1), 0.0)
                tf = np.maximum(t1, t2).min(1)
                hits = [(tn[k], -k, int(child[cur][k])) for k in range(8) if int(child[cur][k]) != EMPTY and tn[k] <= tf[k]]
                hits.sort()
                if hits:
                    for h in reversed(hits[1:]):
                        stack.append(h[2])
                        deepest = max(deepest, len(stack) - 1)
                    cur = hits[0][2]
                    continue
            elif cur != EMPTY and o is wo and (cur & LEAF) and ((cur >> 26) & 31):  # an instance leaf of the top level
                r = recs[cur & 0x3FFFFFF]
                m = r["world2local"].astype(np.float64).reshape(4, 3)
                o, d = wo @ m[:3] + m[3], wd @ m[:3]
                stack.append(imm.REF_INST_EXIT)
                roots = [int(x) for x in words[int(r["root"]) * 16: int(r["root"]) * 16 + 6]]
                have = [x for x in roots if x != EMPTY]
                for x in reversed(have[1:]):
                    stack.append(x)  # (a marker; its root is continued at when popped)
                deepest = max(deepest, len(stack) - 1)
                cur = have[0] if have else EMPTY
                continue
            # a leaf below an instance (no test), a miss, or an empty tree: pop
            if not stack:
                break
            cur = stack.pop()
            if cur == imm.REF_INST_EXIT:
                o, d = wo, wd
                cur = EMPTY
        out.append(deepest)
    return np.array(out)


# ---- the float64 truth of the general-transform leg ---------------------------------------------------------------------------------------
# line_helpers.closest / curve_helpers.closest round their inputs to float32 first, which is right for the records of a scene but not for
# a float64 local ray and scaled radii.  The two closed forms restated in plain float64, all pairs, no BVH, tnear = 0 and tfar = inf:
# LineIntersector1::intersect (kernels/geometry/line_intersector.h:53-98) and intersect_ribbon + intersect_quad_backface_culling
# (bezier_ribbon_intersector.h:80-201, quad_intersector.h:28-90), as line_helpers.candidates / curve_helpers.candidates state them.
def ray_space64(dirs):
    """(s [m], dx, dy, n [m, 3]): the depth scale and the rows of frame(s * dir).transposed() (linearspace3.h:126-133)"""
    d = np.asarray(dirs, np.float64)
    s = 1.0 / np.linalg.norm(d, axis=1)
    n = d * s[:, None]
    zero = np.zeros(len(d))
    a0 = np.stack([zero, n[:, 2], -n[:, 1]], 1)
    a1 = np.stack([-n[:, 2], zero, n[:, 0]], 1)
    a = np.where(((a0 * a0).sum(1) > (a1 * a1).sum(1))[:, None], a0, a1)
    dx = a / np.linalg.norm(a, axis=1, keepdims=True)
    dy = np.cross(n, dx)
    dy /= np.linalg.norm(dy, axis=1, keepdims=True)
    return s, dx, dy, n


def _window(m, tnear, tfar):
    """tnear / tfar [m] in float64, 0 and inf by default"""
    return (np.zeros(m) if tnear is None else np.asarray(tnear, np.float64)), (np.full(m, np.inf) if tfar is None else np.asarray(tfar, np.float64))


def lines_truth64(v0, v1, org, dirs, tnear=None, tfar=None):
    """v0, v1 [n, 4] = (x, y, z, radius), org / dirs [m, 3], all float64 -> dict: hit [m], seg [m] (the nearest valid segment, the lowest
    index on an equal t), t, u, and near_edge / near_tie [m] as line_helpers.closest has them; tnear / tfar [m] default to 0 and inf"""
    v0, v1, org = np.asarray(v0, np.float64), np.asarray(v1, np.float64), np.asarray(org, np.float64)
    assert v0.dtype == np.float64 and org.dtype == np.float64
    tn, tf = (x[:, None] for x in _window(len(org), tnear, tfar))
    s, dx, dy, n = ray_space64(dirs)
    rows = np.stack([dx, dy, n], 1)  # [m, 3, 3]
    with np.errstate(all="ignore"):
        p0 = np.einsum("mnk,mrk->mnr", v0[None, :, :3] - org[:, None, :], rows)  # [m, n, 3]
        p1 = np.einsum("mnk,mrk->mnr", v1[None, :, :3] - org[:, None, :], rows)
        v = p1 - p0
        vw = (v1[:, 3] - v0[:, 3])[None, :]
        u = np.clip(-(p0[..., 0] * v[..., 0] + p0[..., 1] * v[..., 1]) / (v[..., 0] ** 2 + v[..., 1] ** 2), 0.0, 1.0)
        p = p0 + u[..., None] * v
        pw = v0[None, :, 3] + u * vw
        t = p[..., 2] * s[:, None]
        nonzero = ((v1[:, :3] - v0[:, :3]) != 0).any(1)[None, :]
        d2, r2 = p[..., 0] ** 2 + p[..., 1] ** 2, pw * pw
        ok = (d2 <= r2) & (t > tn) & (t <= tf) & (t > tn + 2.0 * pw * s[:, None]) & nonzero
        near_edge = (np.where(r2 > 0, np.abs(d2 - r2) / np.where(r2 > 0, r2, 1), np.inf) <= 1e-4).any(1)
    tt = np.where(ok, t, np.inf)
    seg = tt.argmin(1)
    ar = np.arange(len(org))
    two = np.sort(np.concatenate([tt, np.full((len(org), 1), np.inf)], 1), 1)[:, :2]  # (a single segment has no second candidate)
    with np.errstate(all="ignore"):
        near_tie = np.isfinite(two[:, 1]) & (np.abs(two[:, 1] - two[:, 0]) <= 1e-4 * np.abs(two[:, 0]))
    return {"hit": np.isfinite(tt[ar, seg]), "seg": seg, "t": tt[ar, seg], "u": u[ar, seg], "near_edge": near_edge, "near_tie": near_tie}


def _bezier64(u):
    t1, t0 = u, 1.0 - u
    return ([t0 ** 3, 3 * t1 * t0 * t0, 3 * t1 * t1 * t0, t1 ** 3], [-3 * t0 * t0, 3 * (t0 * t0 - 2 * t0 * t1), 3 * (2 * t0 * t1 - t1 * t1), 3 * t1 * t1])


def curves_truth64(groups, org, dirs, tnear=None, tfar=None):
    """groups: [(cp [n, 4, 4] native (Bezier) control points in float64, N, geomID)] -> dict: hit [m], geomID, primID (index in its group),
    t, u, v, and near_edge / near_tie [m] as curve_helpers.closest has them; on an equal t the first group, lowest curve, lowest segment
    wins; tnear / tfar [m] default to 0 and inf"""
    org = np.asarray(org, np.float64)
    m = len(org)
    tn, tf = (x[:, None, None] for x in _window(m, tnear, tfar))
    near_edge, two = np.zeros(m, bool), np.full((m, 2), np.inf)
    s, dx, dy, n = ray_space64(dirs)
    rows = np.stack([dx, dy, n * s[:, None]], 1)  # the z row scaled by s once more: a transformed z is a ray parameter
    best = {"hit": np.zeros(m, bool), "geomID": np.full(m, -1), "primID": np.full(m, -1), "t": np.full(m, np.inf), "u": np.zeros(m), "v": np.zeros(m)}
    ar = np.arange(m)
    for cp, N, gid in groups:
        cp = np.asarray(cp)
        assert cp.dtype == np.float64
        w = np.einsum("mnck,mrk->mncr", cp[None, :, :, :3] - org[:, None, None, :], rows)  # [m, n, 4 control points, 3]
        rad = cp[None, :, :, 3]
        bas, der = _bezier64(np.arange(N + 1) / float(N))  # each [N + 1]
        with np.errstate(all="ignore"):
            p = sum(b[None, None, :, None] * w[:, :, k, None, :] for k, b in enumerate(bas))        # [m, n, N + 1, 3]
            pw = sum(b[None, None, :] * rad[:, :, k, None] for k, b in enumerate(bas))              # [m or 1, n, N + 1]
            dd = sum(b[None, None, :, None] * w[:, :, k, None, :2] for k, b in enumerate(der))      # [m, n, N + 1, 2]
            nx, ny = dd[..., 1], -dd[..., 0]
            rs = 1.0 / np.sqrt(nx * nx + ny * ny)
            nx, ny = nx * rs, ny * rs
            lx, ly, ux, uy, z = p[..., 0] + pw * nx, p[..., 1] + pw * ny, p[..., 0] - pw * nx, p[..., 1] - pw * ny, p[..., 2]
            pw = np.broadcast_to(pw, z.shape)
            A = [x[..., :-1] for x in (lx, ly, ux, uy, z, pw)]
            B = [x[..., 1:] for x in (lx, ly, ux, uy, z, pw)]
            edbx, edby = B[0] - A[2], B[1] - A[3]
            first = A[2] * edby - A[3] * edbx <= 0
            v0 = [np.where(first, A[0], B[2]), np.where(first, A[1], B[3]), np.where(first, A[4], B[4])]
            v1 = [np.where(first, B[0], A[2]), np.where(first, B[1], A[3]), np.where(first, B[4], A[4])]
            v2 = [np.where(first, A[2], B[0]), np.where(first, A[3], B[1]), np.where(first, A[4], B[4])]
            e0 = [v2[k] - v0[k] for k in range(3)]
            e1 = [v0[k] - v1[k] for k in range(3)]
            Ue = v0[0] * e0[1] - v0[1] * e0[0]
            Ve = v1[0] * e1[1] - v1[1] * e1[0]
            ngx, ngy = e1[1] * e0[2] - e1[2] * e0[1], e1[2] * e0[0] - e1[0] * e0[2]
            den = e1[0] * e0[1] - e1[1] * e0[0]
            Tn = v0[0] * ngx + v0[1] * ngy + v0[2] * den
            Ts = np.where(den < 0, -Tn, Tn)
            ok = (np.maximum(Ue, Ve) <= 0) & (Ts > np.abs(den) * tn) & (Ts <= np.abs(den) * tf) & (den != 0)
            t, u, v = Tn / den, Ue / den, Ve / den
            u, v = np.where(first, u, 1.0 - u), np.where(first, v, 1.0 - v)
            ok &= t > tn + 2.0 * ((1.0 - u) * A[5] + u * B[5]) * s[:, None, None]
            near_edge |= (np.abs(np.maximum(Ue, Ve) / den) <= 1e-4).reshape(m, -1).any(1)
        tt = np.where(ok, t, np.inf).reshape(m, -1)
        two = np.sort(np.concatenate([two, tt], 1), 1)[:, :2]
        k = tt.argmin(1)
        sel = tt[ar, k] < best["t"]
        U = ((np.arange(N)[None, None, :] + u) / float(N)).reshape(m, -1)
        V = (2.0 * v - 1.0).reshape(m, -1)
        for key, val in (("geomID", np.full(m, gid)), ("primID", k // N), ("t", tt[ar, k]), ("u", U[ar, k]), ("v", V[ar, k])):
            best[key][sel] = val[sel]
        best["hit"] |= sel
    with np.errstate(all="ignore"):
        best["near_tie"] = np.isfinite(two[:, 1]) & (np.abs(two[:, 1] - two[:, 0]) <= 1e-4 * np.abs(two[:, 0]))
    best["near_edge"] = near_edge
    return best
