"""Shared by tests/test_host_instance_quads.py and tests/test_gpu_instance_quads.py: instanced scenes that hold quad meshes, alone or
beside triangles (accel kinds 16 / 17).

An instanced scene is described as {"tris": (verts, tris, geomID) or None, "quads": (verts, quads, geomID) or None}.  The oracle has
neither instancing nor quads.  The expected records of one instance come from the instance's LOCAL rays (instance_helpers.local_rays)
traced through po.TriangleScene for the scene's triangles and then, ON THE SAME RECORDS - so that the tfar the triangles left applies, as
inside the kernel - through the split-triangle scene of its quads (A = (v0, v1, v3), B = (v2, v1, v3)) with the B mapping applied; the
instances are merged by smallest t."""
import numpy as np

import instance_helpers as ih
from instance_helpers import INVALID

QUAD_DT = np.dtype([("v0", "<f4", 3), ("geomID", "<u4"), ("v1", "<f4", 3), ("primID", "<u4"), ("v2", "<f4", 3), ("pad0", "<u4"),
                    ("v3", "<f4", 3), ("pad1", "<u4")])
ACCEL_INST_PLUECKER, ACCEL_INST_MOELLER = 16, 17
ROBUST = 4  # RTC_SCENE_FLAG_ROBUST
# geomIDs of the split oracle's A and B triangles while a record is between the quad pass and the B mapping (no test mesh uses them)
SPLIT_A, SPLIT_B = 0x7FFFFFF0, 0x7FFFFFF1


def flags(mode):
    return ROBUST if mode == 0 else 0  # mode 0: Pluecker / robust (kind 16), mode 1: Moeller / fast (kind 17)


# ---- the split oracle and the B mapping of tests/test_gpu_quads.py (_split_oracle, _map_b), with the A / B marks as parameters ----------
def split_oracle(po, verts, quads, mode, a_id=0, b_id=1):
    """TriangleScene on the split triangles: A of every quad, then B; geomID a_id = A, b_id = B; primID = quad index"""
    a = quads[:, [0, 1, 3]]
    b = quads[:, [2, 1, 3]]
    tris = np.concatenate([a, b]).astype(np.uint32)
    gids = np.concatenate([np.full(len(quads), a_id), np.full(len(quads), b_id)]).astype(np.uint32)
    pids = np.concatenate([np.arange(len(quads)), np.arange(len(quads))]).astype(np.uint32)
    return po.TriangleScene(verts, tris, mode, gids, pids)


def map_b(want, geom_id=0, a_id=0, b_id=1):
    """apply the B mapping to oracle records whose hit came from a B triangle (geomID b_id); hits on A or B get geom_id; returns the B mask"""
    isb = want["geomID"] == b_id
    u, v = want["u"][isb].copy(), want["v"][isb].copy()
    want["u"][isb] = np.float32(1) - v
    want["v"][isb] = np.float32(1) - u
    for f in ("Ng_x", "Ng_y", "Ng_z"):
        want[f][isb] = -want[f][isb]
    hit = isb | (want["geomID"] == a_id)
    want["geomID"][hit] = geom_id
    return isb


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def bomberman_quads(bomberman):
    """the 727 quads, scaled and snapped to the 2^-10 grid as the `mesh` of tests/test_gpu_instances.py"""
    v, fs, fi = bomberman
    assert (fs == 4).all() and len(fs) == 727
    s = ih.snap(v * ih.SCALE)
    assert np.abs(s).max() < 16
    return s, fi.reshape(-1, 4).astype(np.uint32)


def quads_only(bomberman, gid=0):
    v, q = bomberman_quads(bomberman)
    return {"m": {"tris": None, "quads": (v, q, gid)}}


def mixed_scenes(bomberman):
    """two scenes over the same faces: in "a" the even faces are triangles (two per face, geomID 3) and the odd ones quads (geomID 7), in
    "b" the other way round"""
    v, q = bomberman_quads(bomberman)

    def split(first):
        t = q[first::2]
        tris = np.concatenate([t[:, [0, 1, 2]], t[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.uint32)
        return {"tris": (v, tris, 3), "quads": (v, q[1 - first::2].copy(), 7)}

    return {"a": split(0), "b": split(1)}


def bounds_meshes(scenes):
    """{key: (all vertices,)} as instance_helpers.instances_bounds / general_rays read it"""
    out = {}
    for k, s in scenes.items():
        vs = [p[0] for p in (s["tris"], s["quads"]) if p is not None]
        out[k] = (np.concatenate(vs),)
    return out


def grid_instances(n, keys=("m",), scales=(0.5, 1.0, 2.0)):
    """n instances on the 2^-10 grid (as _grid_instances of tests/test_gpu_instances.py): translations on a lattice with spacing 40,
    uniform power-of-two scales, every component different from instance to instance; instance i uses scene keys[i % len(keys)]"""
    out = []
    for i in range(n):
        s = scales[i % len(scales)]
        t = (40.0 * (i % 4) + 0.125 * i, 40.0 * ((i // 4) % 5) + 5.0 / 1024.0 * i, 40.0 * (i // 20) + 1.0 / 1024.0 * i)
        out.append((i, keys[i % len(keys)], ih.affine(t, (s, s, s))))
    return out


def general_instances(keys=("m",)):
    """instance_helpers.general_instances (rotations, non-uniform scales), instance i over scene keys[i % len(keys)]"""
    return [(g, keys[g % len(keys)], m) for g, _, m in ih.general_instances()]


# ---- building ------------------------------------------------------------------------------------------------------------------------
def add_scene(rtc, dev, desc, mode):
    sc = rtc.Scene(dev, flags(mode))
    if desc["tris"] is not None:
        v, t, gid = desc["tris"]
        assert sc.add_triangles(v, t, geom_id=gid) == gid
    if desc["quads"] is not None:
        v, q, gid = desc["quads"]
        assert sc.add_quads(v, q, geom_id=gid) == gid
    sc.commit()
    return sc


def build(rtc, mode, scenes, instances, cfg="", extra=None):
    """top scene of `instances` [(geomID, scene key, l2w)] over one instanced scene per key; extra(top) adds other geometry"""
    dev = rtc.Device(cfg)
    inner = {k: add_scene(rtc, dev, d, mode) for k, d in scenes.items()}
    top = rtc.Scene(dev, flags(mode))
    for gid, key, l2w in instances:
        assert top.add_instance(inner[key], l2w, geom_id=gid) == gid
    if extra:
        extra(top)
    top.commit()
    return dev, top, inner


def release(dev, top, inner):
    top.release()
    for s in inner.values():
        s.release()
    dev.release()


# ---- expected records ------------------------------------------------------------------------------------------------------------------
def merge(rays, per, instances):
    """the hit with the smallest t wins and carries its instance's geomID as instID"""
    t = np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf) for p in per])  # [instances, rays]
    best = np.argmin(t, axis=0)
    want = rays.copy()
    for i, p in enumerate(per):
        sel = (best == i) & np.isfinite(t[i])
        want["tfar"][sel] = p["tfar"][sel]
        for f in ih.HITF:
            want[f][sel] = p[f][sel]
        want["instID"][sel] = instances[i][0]
    return want, best


def oracle_instances(rtc, po, scenes, instances, rays, mode, exact=False):
    """leg 1.  Returns (want, per, isb, want_tri): the merged records, per[i] = instance i's own records for all rays, isb = the merged hit
    came from a B triangle of a quad, want_tri = the merged records with u, v, Ng as the hit TRIANGLE has them (before the B mapping):
    what instance_helpers.set_aside measures edge distances on."""
    orcs = {}
    for k, d in scenes.items():
        t = po.TriangleScene(d["tris"][0], d["tris"][1], mode, np.full(len(d["tris"][1]), d["tris"][2], np.uint32)) if d["tris"] is not None else None
        q = split_oracle(po, d["quads"][0], d["quads"][1], mode, SPLIT_A, SPLIT_B) if d["quads"] is not None else None
        orcs[k] = (t, q)
    per, per_tri, per_b = [], [], []
    for gid, key, l2w in instances:
        sub = rtc.aligned_rayhits(len(rays))
        sub[:] = ih.local_rays(rays, ih.world2local(l2w), exact)
        t, q = orcs[key]
        if t is not None:
            t.intersect1M(sub, inst_id=gid, nthreads=16)
        isb = np.zeros(len(rays), bool)
        raw = sub.copy()
        if q is not None:
            q.intersect1M(sub, inst_id=gid, nthreads=16)  # on the same records: against the tfar the triangles left, equal t accepted
            raw = sub.copy()
            isb = map_b(sub, scenes[key]["quads"][2], SPLIT_A, SPLIT_B)
            quad = (raw["geomID"] == SPLIT_A) | (raw["geomID"] == SPLIT_B)
            raw["geomID"][quad] = scenes[key]["quads"][2]
        per.append(sub)
        per_tri.append(raw)
        per_b.append(isb)
    for t, q in orcs.values():
        for s in (t, q):
            if s is not None:
                s.free()
    want, best = merge(rays, per, instances)
    want_tri, _ = merge(rays, per_tri, instances)
    hit = want["geomID"] != INVALID
    isb = np.stack(per_b)[best, np.arange(len(rays))] & hit
    return want, per, isb, want_tri


def diagonal(want):
    """hits within 1e-4 of a quad's v1-v3 diagonal in the quad's parametrisation: A and B are hit within ulps there, the oracle's rcp
    (rcpps + Newton) may rank them the other way, and on a non-planar quad their normals differ (test_bomberman_quads_1m_parity)"""
    hit = want["geomID"] != INVALID
    return hit & (np.abs(want["u"].astype(np.float64) + want["v"] - 1.0) < 1e-4)


def quad_set_aside(want, per, want_tri, quad_gids):
    """instance_helpers.set_aside - within 1e-4 of an edge of the hit triangle, or a second instance within 1e-4 relative in t -
    extended by the diagonal band |u + v - 1| < 1e-4 of quad hits, where the kernel's normal is taken"""
    onq = np.isin(want["geomID"], np.asarray(quad_gids, np.uint32))
    return ih.set_aside(want_tri, per) | (diagonal(want) & onq)


def direct_instances(rtc, inner, instances, rays):
    """leg 2, no oracle arithmetic: every instance's scene traced directly (a plain scene: today's triangle + quad kernels) with the EXACT
    local rays, merged by smallest t.  Returns (want, per)."""
    per = []
    for gid, key, l2w in instances:
        sub = rtc.aligned_rayhits(len(rays))
        sub[:] = ih.local_rays(rays, ih.world2local(l2w), exact=True)
        inner[key].intersect1M(sub)
        per.append(sub)
    want, _ = merge(rays, per, instances)
    return want, per


def copy(rtc, rays):
    out = rtc.aligned_rayhits(len(rays))  # 16-byte aligned (rtcIntersect1 contract)
    out[:] = rays
    return out


def occ_of(rtc, rays):
    occ = rtc.aligned_rays(len(rays))
    for f in occ.dtype.names:
        occ[f] = rays[f]
    return occ


# ---- a scene whose quad leaves hold more than one block ---------------------------------------------------------------------------------
def overlapping_quads(n=40, seed=5):
    """n large quads on the 2^-10 grid whose boxes nearly coincide: no split pays, so the builder leaves them in leaves of 5 or more"""
    rng = np.random.RandomState(seed)
    c = rng.rand(n, 1, 3) * 0.25
    base = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float64)
    v = c + base + (rng.rand(n, 4, 3) - 0.5) * 0.5
    return ih.snap(v.reshape(-1, 3)), np.arange(4 * n, dtype=np.uint32).reshape(-1, 4)


# ---- pinned inputs (test_host_instance_quads.py checks them with the oracle alone, test_gpu_instance_quads.py traces them) -------------
PARITY_RAYS = 8192
PARITY_SEED = {1: 101, 2: 102, 9: 109}
GENERAL_SEED = 11
GENERAL_RAYS = 20000
