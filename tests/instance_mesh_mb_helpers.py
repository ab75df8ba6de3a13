"""Shared by tests/test_host_instance_mesh_mb.py and tests/test_gpu_instance_mesh_mb.py: instanced scenes that hold triangle and quad
meshes with time steps (accel kinds 22 / 23), alone or beside static meshes.

An instanced scene is described as instance_quads_helpers describes one, with two more entries:
    {"tris": (verts, tris, geomID) or None, "quads": (verts, quads, geomID) or None,
     "tris_mb": ([verts per step], tris, geomID) or None, "quads_mb": ([verts per step], quads, geomID) or None}
Instances are described as in instance_mb_helpers: (geomID, scene key, [local-to-world per step]).

The layout of the accel (embree-compressed_amd/csrc/accel.h, InstanceRecord): `blobs` = N InstanceRecords | QuadRecords | InstanceSteps |
one 64-byte scene record per distinct scene | padding | TriMBRecords from a multiple of 96 bytes | padding | QuadMBRecords from a
multiple of 128 bytes; an InstanceRecord's `root` is the index of its scene record in 64-byte units."""
import numpy as np

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mb_helpers as im
import instance_quads_helpers as iq
from instance_helpers import EMPTY, INVALID, LEAF

ACCEL_INSTMESHMB_PLUECKER, ACCEL_INSTMESHMB_MOELLER = 22, 23
SCENE_DT = np.dtype([("triRoot", "<u4"), ("triMBRoot", "<u4"), ("quadRoot", "<u4"), ("quadMBRoot", "<u4"), ("pad", "<u4", 12)])
# tree codes (accel.h INST_TREE_*) and the markers of the pending trees; visiting order: triangles, MB triangles, quads, MB quads
TREE_TRI, TREE_QUAD, TREE_TRIMB, TREE_QUADMB = 0, 1, 2, 3
VISIT = (("triRoot", TREE_TRI), ("triMBRoot", TREE_TRIMB), ("quadRoot", TREE_QUAD), ("quadMBRoot", TREE_QUADMB))
REF_INST_EXIT = 0x80000000
F32 = np.float32
PARTS = ("tris", "tris_mb", "quads", "quads_mb")


def kind(mode):
    """mode 0: Pluecker / robust, mode 1: Moeller / fast"""
    return ACCEL_INSTMESHMB_PLUECKER if mode == 0 else ACCEL_INSTMESHMB_MOELLER


def marker(code):
    return REF_INST_EXIT + code


def desc(tris=None, quads=None, tris_mb=None, quads_mb=None):
    return {"tris": tris, "quads": quads, "tris_mb": tris_mb, "quads_mb": quads_mb}


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
def second_step(v, deg=20.0, frac=0.3):
    """step 1 of the `two_steps` data of tests/test_gpu_motion_blur.py: the mesh rotated by `deg` degrees about y through its centre and
    moved by frac x its extent, snapped to the 2^-10 grid"""
    v = np.asarray(v, np.float64)
    ext = v.max(0) - v.min(0)
    return ih.snap(ds.rot_y(v, deg) + frac * ext * np.array([0.6, -0.3, 0.74]))


# (signed axis permutation, translation) of the four copies of the mesh in scene (c): on the 2^-10 grid
PART_PLACES = (([[1, 0, 0], [0, 1, 0], [0, 0, 1]], (0.0, -4.0, 0.0)), ([[0, -1, 0], [1, 0, 0], [0, 0, 1]], (0.5, 0.0, 0.25)),
               ([[1, 0, 0], [0, 0, -1], [0, 1, 0]], (0.25, 0.5, 0.0)), ([[1, 0, 0], [0, 1, 0], [0, 0, 1]], (0.75, 4.0, 0.5)))


def bomberman_parts(bomberman):
    """Four whole copies of the bomberman mesh (scaled, snapped) that penetrate each other, one per mesh kind with a geomID of its own:
    static triangles (geomID 3), triangles with two steps (5), static quads (7), quads with two steps (9).  (One mesh dealt out face by
    face would not do: its floor is most of what a ray sees, and whoever gets it gets the hits; four copies stacked along y would not
    do either: the top and the bottom floor would share the hits.)  The floors of the second and third copy are turned into the planes
    across x and across z, the first and the fourth lie 4 units below and above the centre, so that every copy is in front from a good
    share of all directions; no two copies share a plane, so no two trees meet at a bit-identical t by construction of the scene.  The
    moving ones leave the cluster over the shutter (second_step)."""
    v, q = iq.bomberman_quads(bomberman)
    t = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.uint32)
    c = [ih.snap(v.astype(np.float64) @ np.asarray(m, np.float64).T + np.asarray(o)) for m, o in PART_PLACES]
    return {"tris": (c[0], t, 3), "tris_mb": ([c[1], second_step(c[1])], t, 5), "quads": (c[2], q, 7), "quads_mb": ([c[3], second_step(c[3])], q, 9)}


def scenes_a(bomberman):
    """(a) MB triangles only: all faces as triangles with two steps"""
    v, q = iq.bomberman_quads(bomberman)
    t = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.uint32)
    return {"m": desc(tris_mb=([v, second_step(v)], t, 0))}


def scenes_b(bomberman):
    """(b) MB quads only"""
    v, q = iq.bomberman_quads(bomberman)
    return {"m": desc(quads_mb=([v, second_step(v)], q, 0))}


def scenes_c(bomberman):
    """(c) all four kinds in one scene, distinct geomIDs"""
    return {"m": desc(**bomberman_parts(bomberman))}


def scenes_d(bomberman):
    """(d) two distinct scenes: "s" static only (triangles + quads), "m" MB only (triangles + quads)"""
    p = bomberman_parts(bomberman)
    return {"s": desc(tris=p["tris"], quads=p["quads"]), "m": desc(tris_mb=p["tris_mb"], quads_mb=p["quads_mb"])}


def bounds_meshes(scenes):
    """{key: (all vertices of all steps,)} as instance_helpers.instances_bounds reads it"""
    out = {}
    for k, s in scenes.items():
        vs = [s[p][0] for p in ("tris", "quads") if s[p] is not None]
        vs += [st for p in ("tris_mb", "quads_mb") if s[p] is not None for st in s[p][0]]
        out[k] = (np.concatenate(vs),)
    return out


# ---- building ---------------------------------------------------------------------------------------------------------------------------
def add_scene(rtc, dev, d, mode):
    sc = rtc.Scene(dev, iq.flags(mode))
    for part, add in (("tris", sc.add_triangles), ("tris_mb", sc.add_triangles_mb), ("quads", sc.add_quads), ("quads_mb", sc.add_quads_mb)):
        if d.get(part) is not None:
            v, idx, gid = d[part]
            assert add(v, idx, geom_id=gid) == gid
    sc.commit()
    return sc


def build(rtc, mode, scenes, instances, cfg="", extra=None):
    dev = rtc.Device(cfg)
    inner = {k: add_scene(rtc, dev, d, mode) for k, d in scenes.items()}
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


def own_accels(rtc, cfg, d, mode):
    """the four accels of the scene `d` as scenes of their own export them, {part: (nodes, records, root, maxDepth) or None}"""
    dev = rtc.Device(cfg)
    out = {}
    for part, (data, dt) in zip(PARTS, ((1, ih.TRI_DT), (2, ds.TRIMB_DT), (2, iq.QUAD_DT), (2, ds.QUADMB_DT))):
        if d.get(part) is None:
            out[part] = None
            continue
        sc = add_scene(rtc, dev, desc(**{part: d[part]}), mode)
        out[part] = (sc.accel_data(0).view(ih.NODE_DT).copy(), sc.accel_data(data).view(dt).copy(), sc.accel_root(), sc.stats()["maxDepth"])
        sc.release()
    dev.release()
    return out


def aimed_rays(rtc, scenes, instances, m, seed, denom=8):
    """m rays on the 2^-10 grid, ray i aimed at instance i % n: from a point on a sphere around the instance's bounds over all its
    steps towards a random point of the inner half of these bounds; ray.time = k / denom.  Most of them hit something."""
    rng = np.random.RandomState(seed)
    meshes = bounds_meshes(scenes)
    boxes = [ih.instances_bounds(meshes, [(g, k, s) for s in steps]) for g, k, steps in instances]
    lo, hi = np.array([b[0] for b in boxes])[np.arange(m) % len(boxes)], np.array([b[1] for b in boxes])[np.arange(m) % len(boxes)]
    c, h = (lo + hi) / 2, (hi - lo) / 2
    u = rng.randn(m, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    org = ih.snap(c + 1.5 * np.linalg.norm(h, axis=1, keepdims=True) * u)
    tgt = ih.snap(c + (rng.rand(m, 3) - 0.5) * h)
    rays = rtc.aligned_rayhits(m)
    from helpers import fill_rays
    fill_rays(rays, org, (tgt - org).astype(F32))
    rays["time"] = (rng.randint(0, denom + 1, m) / float(denom)).astype(F32)
    return rays


def rays_with_times(rtc, po, scenes, instances, m, seed, snapped=False, denom=8):
    """random rays through the bounds of all instances over all their steps; ray.time = k / denom (denom=None: random in [0, 1])"""
    flat = [(g, k, s) for g, k, steps in instances for s in steps]
    lo, hi = ih.instances_bounds(bounds_meshes(scenes), flat)
    rays = rtc.aligned_rayhits(m)
    rays[:] = po.make_random_rays(m, lo.astype(F32), hi.astype(F32), seed=seed)
    if snapped:
        for f in ("org_x", "org_y", "org_z"):
            rays[f] = ih.snap(rays[f])
    rng = np.random.RandomState(seed + 1000)
    rays["time"] = rng.rand(m).astype(F32) if denom is None else (rng.randint(0, denom + 1, m) / float(denom)).astype(F32)
    return rays


# ---- decoding the accel -------------------------------------------------------------------------------------------------------------------
def split_blobs(blobs, n_inst, n_quads, n_steps, n_scenes, n_trimb, n_quadmb):
    """the sections of `blobs` per the documented layout: (InstanceRecords, QuadRecords, steps, scene records, TriMBRecords, QuadMBRecords,
    byte offset of the TriMB section, byte offset of the QuadMB section); asserts the alignment, the zero padding and the total size"""
    o = 0
    recs = blobs[o:o + 64 * n_inst].view(ih.INST_DT); o += 64 * n_inst
    quads = blobs[o:o + 64 * n_quads].view(iq.QUAD_DT); o += 64 * n_quads
    steps = blobs[o:o + 64 * n_steps].view(im.STEP_DT); o += 64 * n_steps
    scenes = blobs[o:o + 64 * n_scenes].view(SCENE_DT); o += 64 * n_scenes
    t_off = (o + 95) // 96 * 96
    assert not blobs[o:t_off].any()
    trimb = blobs[t_off:t_off + 96 * n_trimb].view(ds.TRIMB_DT)
    o = t_off + 96 * n_trimb
    q_off = (o + 127) // 128 * 128
    assert not blobs[o:q_off].any()
    quadmb = blobs[q_off:q_off + 128 * n_quadmb].view(ds.QUADMB_DT)
    assert q_off + 128 * n_quadmb == len(blobs), (q_off, n_quadmb, len(blobs))
    assert t_off % 96 == 0 and q_off % 128 == 0
    return recs, quads, steps, scenes, trimb, quadmb, t_off, q_off


def walk(nodes, root):
    """[(first record, count)] of the leaves reachable from root, and the number of levels of inner nodes above the deepest leaf"""
    if root == EMPTY:
        return [], 0
    if root & LEAF:
        return [(root & 0x3FFFFFF, (root >> 26) & 31)], 0
    out, todo, deepest = [], [(root, 1)], 0
    while todo:
        n, depth = todo.pop()
        deepest = max(deepest, depth)
        for c in nodes[n]["child"].tolist():
            if c == EMPTY:
                continue
            if c & LEAF:
                out.append((c & 0x3FFFFFF, (c >> 26) & 31))
            else:
                todo.append((c, depth + 1))
    return out, deepest


# ---- the stack walk with the tree markers ---------------------------------------------------------------------------------------------------
def simulate_stack(nodes, root, org, dirs, times, inst, tfar=np.inf):
    """deep_stack_helpers.simulate_stack restated for the kinds 22 / 23 (static instances): entering an instance stacks the exit marker
    and, in reverse visiting order, one marker per pending tree with its root in the distance word; popping a marker - before the
    distance cull - switches the leaf kind.  Returns per ray (deepest slot written, most markers stacked at once, deepest slot written
    while at least one tree marker was on the stack, highest slot a tree marker itself was written to; -1: none)."""
    lo, hi, child = ds.decode_nodes(nodes)
    out = []
    for i in range(len(org)):
        out.append(_walk_one(lo, hi, child, int(root), np.asarray(org[i], np.float64), np.asarray(dirs[i], np.float64), float(tfar), float(times[i]), inst))
    a = np.array(out)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3]


def _walk_one(lo, hi, child, root, wo, wd, tfar, time, inst):
    o, d = wo, wd
    with np.errstate(divide="ignore"):
        rd = 1.0 / d
    stack, deepest, most_markers, deepest_marked, marker_slot = [], -1, 0, -1, -1
    cur, inside, code = root, False, TREE_TRI

    def note():
        nonlocal deepest, most_markers, deepest_marked
        deepest = max(deepest, len(stack) - 1)
        nm = sum(1 for r, _ in stack if REF_INST_EXIT < r <= REF_INST_EXIT + 3)
        most_markers = max(most_markers, nm)
        if nm:
            deepest_marked = max(deepest_marked, len(stack) - 1)

    if root == EMPTY:
        return -1, 0, -1, -1
    while True:
        if cur != EMPTY and not cur & LEAF:
            t1, t2 = (lo[cur] - o) * rd, (hi[cur] - o) * rd
            tn = np.maximum(np.minimum(t1, t2).max(1), 0.0)
            tf = np.minimum(np.maximum(t1, t2).min(1), tfar)
            ch = child[cur]
            ks = [k for k in np.nonzero(tn <= tf)[0].tolist() if ch[k] != EMPTY]
            if not ks:
                cur = EMPTY
            elif len(ks) == 1:
                cur = ch[ks[0]]
            else:
                order = ds._order(ks, [float(tn[k]) for k in ks])
                cur = ch[order[0]]
                for k in reversed(order[1:]):
                    stack.append((ch[k], float(tn[k])))
                note()
            if cur != EMPTY:
                continue
        elif cur != EMPTY and not inside:
            rec = inst.records[cur & 0x3FFFFFF]
            m = rec["world2local"].astype(np.float64).reshape(4, 3)
            o, d = wo @ m[:3] + m[3], wd @ m[:3]
            with np.errstate(divide="ignore"):
                rd = 1.0 / d
            stack.append((REF_INST_EXIT, 0.0))
            inside = True
            sc = inst.scenes[int(rec["root"]) - inst.scene_base]
            have = [(int(sc[f]), c) for f, c in VISIT if int(sc[f]) != EMPTY]
            for r, c in reversed(have[1:]):
                stack.append((marker(c), r))
                marker_slot = max(marker_slot, len(stack) - 1)
            note()
            cur, code = have[0] if have else (EMPTY, TREE_TRI)
            if cur != EMPTY:
                continue
        elif cur != EMPTY:
            t = ds._leaf_hit(inst.leaves[code], cur & 0x3FFFFFF, (cur >> 26) & 31, o, d, 0.0, tfar, time)
            if t is not None:
                tfar = t
        cur = EMPTY
        while stack:
            ref, dist = stack.pop()
            if ref == REF_INST_EXIT:
                o, d, inside, code = wo, wd, False, TREE_TRI
                with np.errstate(divide="ignore"):
                    rd = 1.0 / d
                continue
            if REF_INST_EXIT < ref <= REF_INST_EXIT + 3:
                cur, code = int(dist), ref - REF_INST_EXIT
                break
            if dist > tfar:
                continue
            cur = ref
            break
        if cur == EMPTY:
            return deepest, most_markers, deepest_marked, marker_slot


class WalkInstances:
    """what simulate_stack needs of an accel of kind 22 / 23: decoded from the exported arrays"""

    def __init__(self, top, n_inst, counts, pluecker):
        n_quads, n_steps, n_scenes, n_trimb, n_quadmb = counts
        blobs = top.accel_data(2)
        recs, quads, _, scenes, trimb, quadmb, t_off, q_off = split_blobs(blobs, n_inst, n_quads, n_steps, n_scenes, n_trimb, n_quadmb)
        self.records, self.scenes = recs, scenes
        self.scene_base = n_inst + n_quads + n_steps
        prims = top.accel_data(1).view(ih.TRI_DT)

        def based(leaves, base):
            """Leaves indexed by the rebased first record"""
            pad = lambda a: None if a is None else np.concatenate([np.zeros((base,) + a.shape[1:], a.dtype), a])  # noqa: E731
            return ds.Leaves(pad(leaves.t0), pad(leaves.t1), pad(leaves.segment), pad(leaves.nseg))

        self.leaves = {TREE_TRI: ds.tri_leaves(prims, pluecker), TREE_QUAD: based(ds.quad_leaves(quads), n_inst),
                       TREE_TRIMB: based(ds.tri_mb_leaves(trimb), t_off // 96), TREE_QUADMB: based(ds.quad_mb_leaves(quadmb), q_off // 128)}


# ---- expected records -----------------------------------------------------------------------------------------------------------------------
def at_time(steps, time):
    """deep_stack_helpers.at_time: the mesh at `time`, asserted exact in fp32"""
    return ds.at_time(steps, time)


def oracle_instances(rtc, po, scenes, instances, rays, mode, exact=False):
    """Independent of the product's kernels.  Per distinct ray time (the times lie on a grid on which the lerped vertices are exact in
    fp32: at_time asserts it) every scene's parts become static oracle scenes - po.TriangleScene for triangle parts, the split-triangle
    scene with the B mapping for quad parts - and every instance's rays of that time are traced through them one after the other ON THE
    SAME RECORDS, in visiting order, with the local rays under the per-ray matrices of instance_mb_helpers.world2local_at (exact=True:
    asserted exact); the instances are merged by smallest t.  Returns (want, per, isb, want_tri) as instance_quads_helpers.oracle_instances."""
    subs, raws, isbs = [], [], []
    for gid, key, steps in instances:
        w, ok = im.world2local_at(steps, rays["time"])
        sub = rtc.aligned_rayhits(len(rays))
        sub[:] = im.local_rays(rays, w, ok, exact)
        subs.append(sub)
        raws.append(sub.copy())
        isbs.append(np.zeros(len(rays), bool))
    for t in np.unique(rays["time"]):
        sel = np.nonzero(rays["time"] == t)[0]
        for key, d in scenes.items():
            orcs = []
            for name in PARTS:
                if d.get(name) is None:
                    continue
                v, idx, g = d[name]
                v = at_time(v, t) if name.endswith("_mb") else v
                if idx.shape[1] == 3:
                    orcs.append((po.TriangleScene(v, idx, mode, np.full(len(idx), g, np.uint32)), g, False))
                else:
                    orcs.append((iq.split_oracle(po, v, idx, mode, iq.SPLIT_A, iq.SPLIT_B), g, True))
            for i, (gid, k, _) in enumerate(instances):
                if k != key:
                    continue
                part = rtc.aligned_rayhits(len(sel))
                part[:] = subs[i][sel]
                raw = part.copy()
                b = np.zeros(len(sel), bool)
                for orc, g, quad in orcs:
                    orc.intersect1M(part, inst_id=gid, nthreads=16)  # against the tfar the trees before left, equal t accepted
                    if quad:
                        onq = (part["geomID"] == iq.SPLIT_A) | (part["geomID"] == iq.SPLIT_B)
                        raw[onq] = part[onq]
                        raw["geomID"][onq] = g
                        nb = iq.map_b(part, g, iq.SPLIT_A, iq.SPLIT_B)
                        b = np.where(onq, nb, b)
                    else:
                        new = part["tfar"] != raw["tfar"]
                        raw[new] = part[new]
                subs[i][sel] = part
                raws[i][sel] = raw
                isbs[i][sel] = b
            for orc, _, _ in orcs:
                orc.free()
    per, per_tri = [], []
    for i in range(len(instances)):
        _, ok = im.world2local_at(instances[i][2], rays["time"])
        per.append(im._restore(subs[i], rays, ok))
        per_tri.append(im._restore(raws[i], rays, ok))
    want, best = iq.merge(rays, per, instances)
    want_tri, _ = iq.merge(rays, per_tri, instances)
    hit = want["geomID"] != INVALID
    return want, per, np.stack(isbs)[best, np.arange(len(rays))] & hit, want_tri


def quad_gids(scenes):
    return sorted({d[p][2] for d in scenes.values() for p in ("quads", "quads_mb") if d.get(p) is not None})


def general_case(rtc, po, bomberman, mode, seed):
    """the pinned inputs of the general-transform test: scene (c) under instance_mb_helpers.general_instances, random times on the k/8
    grid.  Returns (scenes, instances, rays, want, per, isb, aside)."""
    scenes = scenes_c(bomberman)
    inst = im.general_instances()
    rays = rays_with_times(rtc, po, scenes, inst, im.GENERAL_RAYS, seed, denom=8)
    want, per, isb, want_tri = oracle_instances(rtc, po, scenes, inst, rays, mode)
    aside = iq.quad_set_aside(want, per, want_tri, quad_gids(scenes))
    return scenes, inst, rays, want, per, isb, aside


GENERAL_SEED = 29


# ---- the needle scene of the stack tests ----------------------------------------------------------------------------------------------------------
DEEP_N = 2048  # needles per tree


def deep_scene(n=DEEP_N, seed=ds.SOUP_SEED):
    """deep_stack_helpers' needle soups in all four trees of one instanced scene: static triangles (geomID 3), triangles with two steps
    (5), static quads (7), quads with two steps (9), n needles each, on the 2^-10 grid"""
    tv, tt = ds.sliver_soup(n, seed, snapped=True)
    tm, tmi = ds.sliver_soup_mb(n, seed + 2)
    qv, qq = ds.sliver_soup(n, seed + 1, quads=True, snapped=True)
    qm, qmi = ds.sliver_soup_mb(n, seed + 3, quads=True)
    return {"m": desc(tris=(tv, tt, 3), tris_mb=(tm, tmi, 5), quads=(qv, qq, 7), quads_mb=(qm, qmi, 9))}


# ---- tree markers in the overflow area ---------------------------------------------------------------------------------------------------------
MARKER_N, MARKER_INSTANCES, MARKER_SEED = 8, 128, 41


def marker_spill_case():
    """A top level deep enough that the markers themselves leave LDS: 128 instances of one small scene (8 needles in each of the four
    trees) whose bounds nearly coincide - translations on the 2^-10 grid within a quarter of the scene's size, scale 1 - so that a ray
    enters most children of the three top-level levels and reaches an instance with up to 21 top-level entries below it; the exit
    marker and the three tree markers then land beyond the 16 slots in LDS.  Returns (scenes, instances)."""
    rng = np.random.RandomState(MARKER_SEED)
    inst = [(i, "m", [ih.affine(tuple(np.round(rng.rand(3) * 0.25 * 1024.0) / 1024.0))]) for i in range(MARKER_INSTANCES)]
    return deep_scene(MARKER_N, MARKER_SEED), inst


def marker_spill_rays(rtc, m, seed):
    """m rays on the 2^-10 grid from inside the instances' common box, random directions, times k / 4"""
    from helpers import fill_rays
    rng = np.random.RandomState(seed)
    rays = rtc.aligned_rayhits(m)
    fill_rays(rays, ds.snap(rng.rand(m, 3) * 1.25), rng.randn(m, 3).astype(F32))
    rays["time"] = np.asarray(ds.TIMES, F32)[np.arange(m) % len(ds.TIMES)]
    return rays
