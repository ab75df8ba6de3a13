"""Shared by tests/test_host_deep_stack.py and tests/test_gpu_deep_stack.py: scenes whose rays carry deep traversal stacks, and a CPU walk
of the product's own node arrays that measures how deep.

Every traversal kernel keeps the first entries of a ray's stack in LDS (16 in the lane kernels, 8 in the ray-pool kernel) and the rest in
an HBM overflow area of 7 * (maxDepth + 1) + 2 entries in all.  Meshes of ordinary shape never leave the LDS part: a ray enters few of
the children of a node and finds its hit early.  The scenes here are soups of NEEDLES - triangles (or quads) as long as the cube they
lie in and 2 % of that wide: the box of a needle is cube sized, its area almost nil, so the node boxes of the BVH8 overlap everywhere, a
ray enters most children of most nodes, misses most leaves and really descends into what it stacked.

simulate_stack() walks the QNode8 array of a committed scene (read back from a `gpu=none` device) in float64 with the kernels' rules:
children entered in ascending entry distance, equal distances to the higher child index (four hit children with a tie: the
reference's sorting network, trace_common.hip.h sort4_network), the nearest entered and the others stacked, popped entries culled by
`dist > tfar`, Moeller-Trumbore in float64 on the leaf records to shrink tfar.  It is a measurement of the INPUTS (how many rays reach
which stack slot), not a reference for hits: its float64 slab tests may enter a child the fp32 kernels skip and the other way round."""
from collections import namedtuple

import numpy as np

NODE_DT = np.dtype([("origin", "<f4", 3), ("exp", "u1", 3), ("pad", "u1"), ("child", "<u4", 8), ("q", "u1", (6, 8))])
TRI_DT = np.dtype([("a", "<f4", 3), ("geomID", "<u4"), ("b", "<f4", 3), ("primID", "<u4"), ("c", "<f4", 3), ("pad", "<u4")])
QUAD_DT = np.dtype([("v0", "<f4", 3), ("geomID", "<u4"), ("v1", "<f4", 3), ("primID", "<u4"), ("v2", "<f4", 3), ("pad0", "<u4"),
                    ("v3", "<f4", 3), ("pad1", "<u4")])
TRIMB_DT = np.dtype([("a0", "<f4", 3), ("geomID", "<u4"), ("b0", "<f4", 3), ("primID", "<u4"), ("c0", "<f4", 3), ("segment", "<u4"),
                     ("a1", "<f4", 3), ("numSegments", "<u4"), ("b1", "<f4", 3), ("pad0", "<u4"), ("c1", "<f4", 3), ("pad1", "<u4")])
QUADMB_DT = np.dtype([("v0a", "<f4", 3), ("pad0", "<u4"), ("v1a", "<f4", 3), ("primID", "<u4"), ("v2a", "<f4", 3), ("pad1", "<u4"),
                      ("v3a", "<f4", 3), ("geomID", "<u4"), ("v0b", "<f4", 3), ("pad2", "<u4"), ("v1b", "<f4", 3), ("segment", "<u4"),
                      ("v2b", "<f4", 3), ("pad3", "<u4"), ("v3b", "<f4", 3), ("numSegments", "<u4")])
INST_DT = np.dtype([("world2local", "<f4", 12), ("geomID", "<u4"), ("root", "<u4"), ("pad", "<u4", 2)])
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF
REF_INST_EXIT, REF_INST_QUADS = 0x80000000, 0x80000001
INVALID = 0xFFFFFFFF
ROBUST = 4  # RTC_SCENE_FLAG_ROBUST
LDS_STACK, POOL_STACK = 16, 8  # TRACE_LDS_STACK / TRACE_POOL_STACK: stack entries the lane kernels / the ray-pool kernel keep in LDS
TIMES = (0.0, 0.25, 0.5, 0.75, 1.0)

# the pinned inputs: tests/test_host_deep_stack.py measures them, tests/test_gpu_deep_stack.py traces them
# 4096 needles give trees of depth 3 on which 10 % of the rays pass slot 16 (measured: 60 of 600, 33 of 300) - on the bar and no margin;
# 8192 give depth 4 and 60 %.  The instanced scenes keep 4096: the top-level entries and the markers come on top (40-52 %).
N_SLIVERS, N_INSTANCED, SOUP_SEED = 8192, 4096, 7
HOST_RAYS, HOST_RAY_SEED = 300, 17
GPU_RAYS, GPU_RAY_SEED = 20000, 23


def stack_capacity(max_depth):
    """stack entries the host provides per ray, LDS and overflow area together (rt_trace.cpp launch_on, rt_service.cpp service_trace)"""
    return 7 * (max_depth + 1) + 2


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def snap(v):
    """to the 2^-10 grid, below 64 (as the motion-blur and instance tests do)"""
    s = np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0
    assert np.abs(s).max() < 64
    return s.astype(np.float32)


def sliver_soup(n, seed, extent=1.0, length=1.0, width=0.02, quads=False, snapped=False):
    """n needles with centres c uniform in [0, extent)^3 and random unit directions d: v0 = c - length/2 d, v1 = c + length/2 d,
    v2 = v1 + width p, (quads) v3 = v0 + width p with p a unit vector perpendicular to d; float32, every primitive with vertices of
    its own.  Returns (verts [3n or 4n, 3], indices [n, 3 or 4]); snapped=True: vertices on the 2^-10 grid."""
    rng = np.random.RandomState(seed)
    c = rng.rand(n, 3) * extent
    d = rng.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = np.cross(d, rng.randn(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    v0, v1 = c - 0.5 * length * d, c + 0.5 * length * d
    v2, v3 = v1 + width * p, v0 + width * p
    k = 4 if quads else 3
    verts = np.stack([v0, v1, v2, v3][:k], 1).reshape(-1, 3)
    verts = snap(verts) if snapped else verts.astype(np.float32)
    return verts, np.arange(k * n, dtype=np.uint32).reshape(n, k)


def rot_y(v, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    m = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    ctr = (v.min(0) + v.max(0)) / 2
    return (np.asarray(v, np.float64) - ctr) @ m.T + ctr


def sliver_soup_mb(n, seed, quads=False, deg=4.0, move=(0.05, 0.03, -0.04), **kw):
    """two time steps on the 2^-10 grid: step 0 = the snapped soup, step 1 = step 0 turned about y by `deg` degrees, moved by `move`
    and snapped - vertices lerped at times k/4 are then exact in fp32.  Returns ([step0, step1], indices)."""
    v, idx = sliver_soup(n, seed, quads=quads, snapped=True, **kw)
    return [v, snap(rot_y(v, deg) + np.asarray(move, np.float64))], idx


def at_time(steps, time, exact=True):
    """the mesh at `time` (getTimeSegment + lerp in float64; exact in fp32 for snapped steps and times k / (4 S))"""
    S = len(steps) - 1
    ts = np.float64(time) * S
    it = int(min(max(np.floor(ts), 0), S - 1))
    f = ts - it
    v = (1.0 - f) * steps[it].astype(np.float64) + f * steps[it + 1].astype(np.float64)
    assert not exact or np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v.astype(np.float32)


def bounds(*vert_arrays):
    a = np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v in vert_arrays])
    return a.min(0), a.max(0)


def deep_instances():
    """three instances of one soup with overlapping bounds, on the exact grid: snapped translations, uniform scales 1, 2 and 1/2"""
    import instance_helpers as ih
    return [(0, "m", ih.affine((0.0, 0.0, 0.0), (1.0,) * 3)),
            (1, "m", ih.affine((-0.375, -0.25, -0.5), (2.0,) * 3)),
            (2, "m", ih.affine((0.25, 0.375, 0.125), (0.5,) * 3))]


def instance_ray_box(scenes, inst):
    """the box the rays of the instance cases are drawn from: the world bounds of the first (unit-scale) instance, which lie inside
    the double-size instance and contain the half-size one - every instance gets its share of the hits"""
    import instance_helpers as ih
    import instance_quads_helpers as iq
    lo, hi = ih.instances_bounds(iq.bounds_meshes(scenes), inst[:1])
    return lo.astype(np.float32), hi.astype(np.float32)


def instanced_scene(kind, n=N_INSTANCED, seed=SOUP_SEED):
    """the instanced scene of the instance cases as instance_quads_helpers describes one: kind 't' = n needle triangles, 'q' = n needle
    quads, 'tq' = n / 2 of each (geomIDs 3 and 7)"""
    tv, tt = sliver_soup(n if kind == "t" else n // 2, seed, snapped=True)
    qv, qq = sliver_soup(n if kind == "q" else n // 2, seed + 1, quads=True, snapped=True)
    return {"m": {"tris": (tv, tt, 3) if "t" in kind else None, "quads": (qv, qq, 7) if "q" in kind else None}}


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------
Leaves = namedtuple("Leaves", "t0 t1 segment nseg")  # t0 / t1: [records, triangles per record, 3, 3] float64 (t1: None when static)
Instances = namedtuple("Instances", "records quads has_quads")  # InstanceRecords, the Leaves of the quad trees, kind 16 / 17
StackWalk = namedtuple("StackWalk", "deepest hit hit_slot from_overflow")


def tri_leaves(recs, pluecker):
    """TriRecords: Pluecker (a, b, c) = (v0, v1, v2), Moeller (v0, e1 = v0 - v1, e2 = v2 - v0)"""
    a, b, c = (recs[f].astype(np.float64) for f in ("a", "b", "c"))
    t = np.stack([a, b, c], 1) if pluecker else np.stack([a, a - b, a + c], 1)
    return Leaves(t[:, None], None, None, None)


def _split(v0, v1, v2, v3):
    return np.stack([np.stack([v0, v1, v3], 1), np.stack([v2, v1, v3], 1)], 1)  # A = (v0, v1, v3), B = (v2, v1, v3)


def quad_leaves(recs):
    return Leaves(_split(*(recs[f"v{k}"].astype(np.float64) for k in range(4))), None, None, None)


def tri_mb_leaves(recs):
    t0 = np.stack([recs[f].astype(np.float64) for f in ("a0", "b0", "c0")], 1)[:, None]
    t1 = np.stack([recs[f].astype(np.float64) for f in ("a1", "b1", "c1")], 1)[:, None]
    return Leaves(t0, t1, recs["segment"].astype(np.int64), recs["numSegments"].astype(np.int64))


def quad_mb_leaves(recs):
    t0 = _split(*(recs[f"v{k}a"].astype(np.float64) for k in range(4)))
    t1 = _split(*(recs[f"v{k}b"].astype(np.float64) for k in range(4)))
    return Leaves(t0, t1, recs["segment"].astype(np.int64), recs["numSegments"].astype(np.int64))


def decode_nodes(nodes):
    """child boxes of every node as the kernels decode them - lo = fmaf(float(q), scale, origin) in fp32, as
    test_host_accel.py:_decode_child - vectorised: (lo [N, 8, 3], hi [N, 8, 3]) float64, children [N][8] as Python ints"""
    scale = (nodes["exp"].astype(np.uint32) << 23).view(np.float32).astype(np.float64)  # [N, 3]
    org = nodes["origin"].astype(np.float64)
    q = nodes["q"].astype(np.float64)  # [N, 6, 8]
    # q * scale is exact (8-bit integer times a power of two): one rounding, like the fma
    lo = (q[:, 0::2, :] * scale[:, :, None] + org[:, :, None]).astype(np.float32).astype(np.float64).transpose(0, 2, 1)
    hi = (q[:, 1::2, :] * scale[:, :, None] + org[:, :, None]).astype(np.float32).astype(np.float64).transpose(0, 2, 1)
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi), nodes["child"].tolist()


def _order(hit, dist):
    """visiting order of the hit children `hit` (ascending child index) with entry distances `dist`"""
    if len(hit) == 4 and len(set(dist)) < 4:
        # sort4_network (trace_common.hip.h): s1 = the highest child index; a comparator swaps when the first is nearer
        s = [[dist[3], 3], [dist[2], 2], [dist[1], 1], [dist[0], 0]]
        for a, b in ((1, 0), (3, 2), (2, 0), (3, 1), (2, 1)):
            if s[a][0] < s[b][0]:
                s[a], s[b] = s[b], s[a]
        return [hit[q] for _, q in s]
    # ascending distance, equal distances -> the higher child index first
    return [k for _, _, k in sorted((d, -k, k) for k, d in zip(hit, dist))]


def _leaf_hit(leaves, first, count, o, d, tnear, tfar, time):
    """nearest Moeller-Trumbore hit (float64) of the records [first, first + count) within [tnear, tfar], or None"""
    t0 = leaves.t0[first:first + count]
    if leaves.t1 is not None:
        S = leaves.nseg[first:first + count]
        ts = time * S
        it = np.clip(np.floor(ts), 0, S - 1)
        use = it == leaves.segment[first:first + count]
        f = (ts - it)[use][:, None, None, None]
        t0 = (1.0 - f) * t0[use] + f * leaves.t1[first:first + count][use]
    tri = t0.reshape(-1, 3, 3)
    if not len(tri):
        return None
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = o - tri[:, 0]
        u = (tv * pv).sum(1) * inv
        qv = np.cross(tv, e1)
        v = (qv * d).sum(1) * inv
        t = (e2 * qv).sum(1) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tnear) & (t <= tfar)
    return float(t[ok].min()) if ok.any() else None


def _walk_one(lo, hi, child, root, leaves, o, d, tnear, tfar, time, threshold, inst):
    wo, wd = o, d
    with np.errstate(divide="ignore"):
        rd = 1.0 / d
    stack = []  # (reference, distance)
    deepest, hit, hit_slot = -1, False, -1
    cur, cur_slot = root, -1  # cur_slot: the slot `cur` was popped from, -1 while the ray descends
    inside, in_quads = inst is None, False
    if root == EMPTY:
        return StackWalk(-1, False, -1, False)
    while True:
        if cur != EMPTY and not cur & LEAF:
            # inner node: slab test of the 8 children (entry distance clamped to tnear, exit distance to the ray's current tfar)
            t1, t2 = (lo[cur] - o) * rd, (hi[cur] - o) * rd
            tn = np.maximum(np.minimum(t1, t2).max(1), tnear)
            tf = np.minimum(np.maximum(t1, t2).min(1), tfar)
            ch = child[cur]
            ks = [k for k in np.nonzero(tn <= tf)[0].tolist() if ch[k] != EMPTY]
            if not ks:
                cur = EMPTY
            elif len(ks) == 1:
                cur = ch[ks[0]]
            else:
                order = _order(ks, [float(tn[k]) for k in ks])
                cur = ch[order[0]]
                for k in reversed(order[1:]):  # the farthest at the bottom: they pop in visiting order
                    stack.append((ch[k], float(tn[k])))
                deepest = max(deepest, len(stack) - 1)
            if cur != EMPTY:
                cur_slot = -1  # descended, not popped
                continue
        elif cur != EMPTY and not inside:
            # instance leaf: the ray enters the instance; the exit marker, and the pending quad tree, go on the stack
            rec = inst.records[cur & 0x3FFFFFF]
            m = rec["world2local"].astype(np.float64).reshape(4, 3)  # vx, vy, vz, p
            o, d = wo @ m[:3] + m[3], wd @ m[:3]
            with np.errstate(divide="ignore"):
                rd = 1.0 / d
            stack.append((REF_INST_EXIT, 0.0))
            inside, in_quads = True, False
            cur, qroot = int(rec["root"]), int(rec["pad"][0]) if inst.has_quads else EMPTY
            if qroot != EMPTY:
                if cur != EMPTY:
                    stack.append((REF_INST_QUADS, qroot))
                else:
                    cur, in_quads = qroot, True
            deepest = max(deepest, len(stack) - 1)
            cur_slot = -1
            if cur != EMPTY:
                continue
        elif cur != EMPTY:
            lv = inst.quads if in_quads else leaves
            if lv is not None:
                t = _leaf_hit(lv, cur & 0x3FFFFFF, (cur >> 26) & 31, o, d, tnear, tfar, time)
                if t is not None:
                    tfar, hit, hit_slot = t, True, cur_slot
        # pop
        cur = EMPTY
        while stack:
            slot = len(stack) - 1
            ref, dist = stack.pop()
            if inst is not None and ref == REF_INST_EXIT:
                o, d, inside, in_quads = wo, wd, False, False
                with np.errstate(divide="ignore"):
                    rd = 1.0 / d
                continue
            if inst is not None and inst.has_quads and ref == REF_INST_QUADS:
                cur, in_quads, cur_slot = int(dist), True, slot
                break
            if dist > tfar:
                continue
            cur, cur_slot = ref, slot
            break
        if cur == EMPTY:
            return StackWalk(deepest, hit, hit_slot, hit and hit_slot >= threshold)


def simulate_stack(nodes, root, prims_or_none, org, dir, tfar=np.inf, threshold=LDS_STACK, time=0.0, instances=None):
    """Walk `nodes` (NODE_DT) from `root` for every ray (org, dir: [m, 3]; tnear = 0; `time` a scalar or [m]).  prims_or_none: the Leaves
    of the tree's records (tri_leaves, quad_leaves, tri_mb_leaves, quad_mb_leaves), or None - no primitive tests, tfar never shrinks.
    instances: an Instances for the node array of an instance accel - leaves met outside an instance are InstanceRecords, entering
    one stacks the exit marker (and the marker of the pending quad tree), prims_or_none are then the Leaves of the TriRecords.
    Returns a StackWalk of arrays: deepest = the highest stack slot the ray wrote (-1: none), hit, hit_slot = the slot the leaf of the
    final closest hit was popped from (-1: the ray descended into it), from_overflow = hit and hit_slot >= threshold."""
    lo, hi, child = decode_nodes(nodes)
    org, dir = np.asarray(org, np.float64), np.asarray(dir, np.float64)
    times = np.broadcast_to(np.asarray(time, np.float64), (len(org),))
    out = [_walk_one(lo, hi, child, int(root), prims_or_none, org[i], dir[i], 0.0, float(tfar), float(times[i]), threshold, instances)
           for i in range(len(org))]
    return StackWalk(np.array([w.deepest for w in out]), np.array([w.hit for w in out]), np.array([w.hit_slot for w in out]),
                     np.array([w.from_overflow for w in out]))


def rays_of(rtc, org, dirs, times=None):
    """RAYHIT records (16-byte aligned) of the rays, tnear 0, tfar inf, time = times[i % len(times)]"""
    from helpers import fill_rays
    rays = rtc.aligned_rayhits(len(org))
    fill_rays(rays, org, dirs)
    if times is not None:
        rays["time"] = np.asarray(times, np.float32)[np.arange(len(org)) % len(times)]
    return rays


def occ_of(rtc, rays):
    occ = rtc.aligned_rays(len(rays))
    for f in occ.dtype.names:
        occ[f] = rays[f]
    return occ


def copy_of(rtc, rays):
    out = rtc.aligned_rayhits(len(rays))
    out[:] = rays
    return out


# ---- expected records -------------------------------------------------------------------------------------------------------------------
def oracle_per_time(rtc, po, steps, idx, rays, mode, nthreads=8):
    """The rays traced by one static oracle scene per distinct ray time (tests/test_gpu_motion_blur.py, test_gpu_quad_motion_blur.py):
    po.TriangleScene on the mesh at that time for triangles, the split-triangle scene with the B mapping for quads (idx [n, 4]).
    Returns (records, mask of the hits that came from a B triangle)."""
    import instance_quads_helpers as iq
    quads = idx.shape[1] == 4
    want, isb = rays.copy(), np.zeros(len(rays), bool)
    for t in np.unique(rays["time"]):
        sel = np.nonzero(rays["time"] == t)[0]
        sub = rtc.aligned_rayhits(len(sel))
        sub[:] = rays[sel]
        v = at_time(steps, t)
        orc = iq.split_oracle(po, v, idx, mode) if quads else po.TriangleScene(v, idx, mode, np.zeros(len(idx), np.uint32))
        orc.intersect1M(sub, nthreads=nthreads)
        orc.free()
        if quads:
            isb[sel] = iq.map_b(sub)
        want[sel] = sub
    return want, isb


def quad_allowances(got, want, isb, mode, quad_gids=None, nonplanar=None):
    """The two allowances of test_bomberman_quads_1m_parity, applied to `want` in place before helpers.compare_hits: Moeller B-lane u / v
    within 4e-7 (the oracle maps after the division, the kernel before), and - capped at fewer than 1 % of the hits - the kernel's
    normal for hits within 1e-4 of the v1-v3 diagonal, where A and B are hit within ulps and may be ranked the other way.
    nonplanar: a mask of the non-planar quads, indexed by primID, or {geomID: such a mask} - the normal allowance (and its cap) then
    covers hits on those quads only: the two split normals of a planar quad agree, whichever triangle wins.  Returns the number of
    hits the normal allowance was applied to."""
    hit = want["geomID"] != INVALID
    if mode == 1:
        b = isb & hit & (got["geomID"] != INVALID)
        for f in ("u", "v"):
            assert np.all(np.abs(got[f][b].astype(np.float64) - want[f][b]) <= 4e-7 + 1e-4 * np.abs(want[f][b])), f
            want[f][b] = got[f][b]
    diag = hit & (np.abs(want["u"].astype(np.float64) + want["v"] - 1.0) < 1e-4)
    if quad_gids is not None:
        diag &= np.isin(want["geomID"], np.asarray(quad_gids, np.uint32))
    if nonplanar is not None:
        masks = nonplanar if isinstance(nonplanar, dict) else {int(g): nonplanar for g in np.unique(want["geomID"][hit])}
        bent = np.zeros(len(want), bool)
        for g, mask in masks.items():
            on = hit & (want["geomID"] == np.uint32(g))
            bent[on] = np.asarray(mask, bool)[want["primID"][on]]
        diag &= bent
    assert int(diag.sum()) < int(hit.sum()) // 100, int(diag.sum())
    for f in ("Ng_x", "Ng_y", "Ng_z"):
        want[f][diag] = got[f][diag]
    return int(diag.sum())
