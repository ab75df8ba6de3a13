"""Shared by tests/test_host_instance_subdiv.py and tests/test_gpu_instance_subdiv*.py: instanced scenes that hold subdivision meshes
(the second instance accel of a scene, kinds 24 / 25; csrc/accel.h InstanceRecord, csrc/trace_instance_subdiv.hip).

A mesh is described as (verts, face sizes, face indices, L, C): tessellation and compression level of its instanced scene.  Instances are
(geomID, mesh key, steps) with steps a list of local-to-world [3,4] matrices as in instance_mb_helpers (one step: static).  The expected
records of the byte-for-byte legs come from the instanced scene traced DIRECTLY (the subdivision kernels that exist without instancing)
with the instance's exact local rays and the instance's geomID as the context's instID."""
import numpy as np

import instance_helpers as ih
import instance_mb_helpers as im
import instance_quads_helpers as iq
from helpers import fill_rays
from instance_helpers import INVALID

ACCEL_GRIDSOA, ACCEL_CBVH_LEAF = 6, 4
ACCEL_INSTSUBDIV_GRID, ACCEL_INSTSUBDIV_CBVH_LEAF = 24, 25
EAGER, LEAF = "default", "bvh4.compressed.leaf"
FAMILIES = (EAGER, LEAF)
KIND = {EAGER: ACCEL_INSTSUBDIV_GRID, LEAF: ACCEL_INSTSUBDIV_CBVH_LEAF}
INNER_KIND = {EAGER: ACCEL_GRIDSOA, LEAF: ACCEL_CBVH_LEAF}
LEVELS = [(3, 2), (4, 1), (5, 4), (6, 5)]  # (L, C) of the 32-face mesh
HOST_CFG = "gpu=none,inst_accel=default,subdiv_accel="
F32 = np.float32


def cbvh_stride(C, mode=1):
    """accel.h cbvh_stride for the leaf mode"""
    elems = ((1 << (2 * C)) - 1) // 3
    payload = (160 + elems * 4 + 15) & ~15
    tail = (payload + (2 << (2 * C)) + 15) & ~15
    return (tail + 64 + 127) & ~127


def blob_stride(accel, C):
    return 160 if accel == EAGER else cbvh_stride(C)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def cube():
    """the cube of tests/test_gpu_subdiv.py (_cube): the displacement_geometry tutorial's"""
    v = np.array([[-1, -1, -1], [-1, -1, 1], [-1, 1, -1], [-1, 1, 1], [1, -1, -1], [1, -1, 1], [1, 1, -1], [1, 1, 1]], F32)
    fi = np.array([0, 4, 5, 1, 1, 5, 7, 3, 3, 7, 6, 2, 2, 6, 4, 0, 4, 6, 7, 5, 0, 1, 3, 2], np.uint32)
    return v, np.full(6, 4, np.uint32), fi


def bomberman_faces(bomberman, n=32):
    """the first n faces of bomberman (all 727 with n=None), scaled and snapped to the 2^-10 grid; vertices compacted to those in use"""
    v, fs, fi = bomberman
    assert (fs == 4).all()
    s = ih.snap(v * ih.SCALE)
    if n is None:
        return s, fs.copy(), fi.copy()
    idx = fi[: 4 * n]
    used, inv = np.unique(idx, return_inverse=True)
    return s[used].copy(), fs[:n].copy(), inv.astype(np.uint32)


def mesh_box(mesh):
    """a box that holds the limit surface: the control cage's (Catmull-Clark surfaces lie in the convex hull of their cage)"""
    v = mesh[0]
    return v.min(0).astype(np.float64), v.max(0).astype(np.float64)


# ---- instances ------------------------------------------------------------------------------------------------------------------------
def lattice_instances(n, keys=("m",), spacing=40.0, scales=(0.5, 1.0, 2.0), cols=4, rows=5):
    """instance_quads_helpers.grid_instances with the lattice spacing as a parameter: translations on the 2^-10 grid, uniform
    power-of-two scales, every component different from instance to instance; one step each"""
    out = []
    for i in range(n):
        s = scales[i % len(scales)]
        t = (spacing * (i % cols) + 0.125 * i, spacing * ((i // cols) % rows) + 5.0 / 1024.0 * i, spacing * (i // (cols * rows)) + 1.0 / 1024.0 * i)
        out.append((i, keys[i % len(keys)], [ih.affine(t, (s, s, s))]))
    return out


def static(instances):
    """[(g, key, m)] -> [(g, key, [m])]"""
    return [(g, k, [m]) for g, k, m in instances]


def world_boxes(meshes, instances):
    """per instance: (lo, hi) float64 of the union over its steps of the transformed corners of the mesh box"""
    out = []
    for _, key, steps in instances:
        lo, hi = mesh_box(meshes[key])
        c = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)])
        w = np.concatenate([ih.xfm_points(m, c) for m in steps])
        out.append((w.min(0), w.max(0)))
    return out


# ---- building -------------------------------------------------------------------------------------------------------------------------
def add_inner(rtc, dev, mesh):
    v, fs, fi, L, C = mesh
    sc = rtc.Scene(dev)
    assert sc.add_subdiv(v, fs, fi) == 0
    sc.set_levels(L, C)
    sc.commit()
    return sc


def build(rtc, accel, meshes, instances, cfg="", extra=None, commit=True):
    """device with subdiv_accel=`accel` (cfg: a prefix such as "gpu=none,inst_accel=default" or "service=1"), one instanced scene per
    mesh key, the top scene of `instances`; extra(top, dev) adds other geometry"""
    dev = rtc.Device((cfg + "," if cfg else "") + "subdiv_accel=" + accel)
    inner = {k: add_inner(rtc, dev, m) for k, m in meshes.items()}
    top = rtc.Scene(dev)
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


# ---- rays -----------------------------------------------------------------------------------------------------------------------------
def _slab(o, d, lo, hi):
    """entry / exit parameter of the lines o + t d through the box [lo, hi] (float64; inf / nan free for d == 0 components outside)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
    par = d == 0
    inside = (o >= lo) & (o <= hi)
    tn = np.where(par, np.where(inside, -np.inf, np.inf), tn)
    tf = np.where(par, np.where(inside, np.inf, -np.inf), tf)
    return tn.max(1), tf.min(1)


def inflate(box, frac):
    lo, hi = box
    e = (hi - lo) * frac
    return lo - e, hi + e


def short_rays(rtc, meshes, instances, per_instance, seed, times=None):
    """Rays built per instance, with a finite tfar: origins on the 2^-10 grid in the instance's world box grown on every side by a
    quarter of its largest extent, directions on the 2^-8 grid towards the box, tfar at most 1.5 box diagonals and cut to 0.9 of the distance at which the ray would
    enter any OTHER instance's world box inflated by 2 % of its extent (rays that start inside such a box are dropped).  Returns
    (rays, owner [n] = index into `instances`).  times: ray.time values, cycled."""
    rng = np.random.RandomState(seed)
    boxes = world_boxes(meshes, instances)
    recs, owner = [], []
    for i, (lo, hi) in enumerate(boxes):
        n = per_instance
        grow = 0.25 * (hi - lo).max()
        blo, bhi = lo - grow, hi + grow
        o = ih.snap(blo + rng.rand(n, 3) * (bhi - blo)).astype(np.float64)
        target = lo + rng.rand(n, 3) * (hi - lo)
        d = target - o
        d = np.round(d / np.abs(d).max(1, keepdims=True) * 256.0) / 256.0  # on the 2^-8 grid, the largest component +-1
        tfar = np.full(n, 1.5 * np.linalg.norm(hi - lo))
        ok = np.ones(n, bool)
        for j, other in enumerate(boxes):
            if j == i:
                continue
            tn, tf = _slab(o, d, *inflate(other, 0.02))
            crosses = (tn <= tf) & (tf >= 0)
            ok &= ~(crosses & (tn <= 0))  # starts inside
            tfar = np.where(crosses & (tn > 0), np.minimum(tfar, 0.9 * tn), tfar)
        r = rtc.aligned_rayhits(int(ok.sum()))
        fill_rays(r, o[ok].astype(F32), d[ok].astype(F32), tfar=tfar[ok].astype(F32))
        recs.append(r)
        owner.append(np.full(int(ok.sum()), i))
    rays = rtc.aligned_rayhits(sum(len(r) for r in recs))
    rays[:] = np.concatenate(recs)
    owner = np.concatenate(owner)
    if times is not None:
        rays["time"] = np.asarray(times, F32)[np.arange(len(rays)) % len(times)]
    return rays, owner


def assert_cannot_reach_others(meshes, instances, rays, owner):
    """host-side condition of the short-ray legs: no segment [0, tfar] meets another instance's world box inflated by 2 % of its extent
    (the margin covers the quantized node boxes of the top-level tree)"""
    boxes = world_boxes(meshes, instances)
    o = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1).astype(np.float64)
    d = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1).astype(np.float64)
    tfar = rays["tfar"].astype(np.float64)
    assert np.isfinite(tfar).all()
    for j, other in enumerate(boxes):
        tn, tf = _slab(o, d, *inflate(other, 0.02))
        reach = (tn <= tf) & (tf >= 0) & (tn <= tfar) & (owner != j)
        assert not reach.any(), (j, int(reach.sum()))


def crossing_rays(rtc, meshes, instances, m, seed):
    """long rays (tfar = inf) through the lattice: origins on the 2^-10 grid in the bounds of all instances inflated by a tenth, aimed at
    a random point of a random instance's world box; directions on the 2^-8 grid"""
    rng = np.random.RandomState(seed)
    boxes = world_boxes(meshes, instances)
    lo = np.min([b[0] for b in boxes], 0)
    hi = np.max([b[1] for b in boxes], 0)
    blo, bhi = inflate((lo, hi), 0.1)
    o = ih.snap(blo + rng.rand(m, 3) * (bhi - blo)).astype(np.float64)
    pick = rng.randint(0, len(boxes), m)
    tl, th = np.array([boxes[k][0] for k in pick]), np.array([boxes[k][1] for k in pick])
    d = tl + rng.rand(m, 3) * (th - tl) - o
    d = np.round(d / np.abs(d).max(1, keepdims=True) * 256.0) / 256.0
    d[(d == 0).all(1)] = (0.25, -0.5, 1.0)
    rays = rtc.aligned_rayhits(m)
    fill_rays(rays, o.astype(F32), d.astype(F32))
    return rays


# ---- expected records -------------------------------------------------------------------------------------------------------------------
def direct(rtc, inner_scene, gid, steps, rays, tfar=None, coherent=False, occluded=False):
    """the instanced scene traced directly with the instance's EXACT local rays (per-ray matrices for a moving instance, asserted exact),
    instID = the instance's geomID; tfar: replaces the rays' (an array).  Returns RAYHIT records (occluded: RAY records) that keep the
    world ray in org / dir."""
    w, ok = im.world2local_at(steps, rays["time"])
    assert ok.all()
    if len(steps) > 1:
        assert np.array_equal(w.astype(np.float64), im.world2local_f64(steps, rays["time"])), "world2local(time) is not exact for these inputs"
    sub = rtc.aligned_rayhits(len(rays))
    sub[:] = im.local_rays(rays, w, ok, exact=True)
    if tfar is not None:
        sub["tfar"] = tfar
    ctx = rtc.make_context(inst_id=gid, coherent=coherent)
    if occluded:
        occ = iq.occ_of(rtc, sub)
        inner_scene.occluded1M(occ, ctx=ctx)
        out = iq.occ_of(rtc, rays)
        out["tfar"] = occ["tfar"]
        return out
    inner_scene.intersect1M(sub, ctx=ctx)
    for f in ("org_x", "org_y", "org_z", "dir_x", "dir_y", "dir_z"):
        sub[f] = rays[f]
    return sub


def direct_owned(rtc, inner, instances, rays, owner, **kw):
    """short-ray legs: every ray traced directly in its owner's scene only"""
    occluded = kw.get("occluded", False)
    want = iq.occ_of(rtc, rays) if occluded else iq.copy(rtc, rays)
    for i, (gid, key, steps) in enumerate(instances):
        sel = np.nonzero(owner == i)[0]
        if len(sel):
            sub = rtc.aligned_rayhits(len(sel))
            sub[:] = rays[sel]
            want[sel] = direct(rtc, inner[key], gid, steps, sub, **kw)
    return want


def direct_all(rtc, inner, instances, rays, tfar=None):
    """crossing legs: per[i] = instance i's direct records for all rays"""
    return [direct(rtc, inner[key], gid, steps, rays, tfar=tfar) for gid, key, steps in instances]


def merge(rays, per, instances):
    want, _ = iq.merge(rays, per, instances)
    return want


def differing(got, want):
    size = got.dtype.itemsize
    return int((got.view(np.uint8).reshape(-1, size) != want.view(np.uint8).reshape(-1, size)).any(1).sum())


# ---- accel layout (host tests) ----------------------------------------------------------------------------------------------------------
def decode(top, rtc):
    """(nodes, records + steps as INST_DT, blobs bytes, (number of blobs, first blob index)) of the subdivision instance accel"""
    sel = rtc.ACCEL_DATA_INSTSUBDIV
    nodes = top.accel_data(sel + 0).view(ih.NODE_DT)
    blobs = top.accel_data(sel + 2)
    off = top.accel_data(sel + 3).view(np.uint32)
    return nodes, blobs, (int(off[0]), int(off[1]))


def depth_of(nodes, root):
    """levels of inner nodes from `root` down (0 for a leaf root)"""
    if root == ih.EMPTY or root & ih.LEAF:
        return 0
    return 1 + max(depth_of(nodes, int(c)) for c in nodes[root]["child"])


# ---- compressed.leaf: what holds in any visiting order ------------------------------------------------------------------------------------
def order_free_classes(rtc, inner, instances, rays):
    """The fork's leaf mode is order dependent: a blob is entered with far = min(frustum exit, ray.tfar), so a hit found earlier changes
    what a later blob reports.  Two classes of rays get the same record whatever the order in which the kernel visits the instances,
    computed from direct traces only:
      none[r]   no instance hits r when traced directly with the original tfar;
      single[r] exactly one instance i hits r, and every other instance misses r when traced directly with tfar = t_i.
    Returns (none, single, want): want = for `single` rays the record of instance i's direct trace, for all others the untouched ray."""
    per = direct_all(rtc, inner, instances, rays)
    hit = np.stack([p["geomID"] != INVALID for p in per])
    nh = hit.sum(0)
    none, single = nh == 0, nh == 1
    want = iq.copy(rtc, rays)
    for i, p in enumerate(per):
        sel = single & hit[i]
        want[sel] = p[sel]
    ti = want["tfar"]
    for j, (gid, key, steps) in enumerate(instances):
        sel = np.nonzero(single & ~hit[j])[0]
        if not len(sel):
            continue
        sub = rtc.aligned_rayhits(len(sel))
        sub[:] = rays[sel]
        again = direct(rtc, inner[key], gid, steps, sub, tfar=ti[sel])
        single[sel[again["geomID"] != INVALID]] = False
    want[~single] = rays[~single]
    return none, single, want


def occluded_any(rtc, inner, instances, rays):
    """RAY records: tfar = -inf where any instance's direct any-hit trace of the local ray reports occluded"""
    occ = iq.occ_of(rtc, rays)
    for gid, key, steps in instances:
        o = direct(rtc, inner[key], gid, steps, rays, occluded=True)
        occ["tfar"][o["tfar"] == -np.inf] = -np.inf
    return occ
