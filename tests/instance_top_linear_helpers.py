"""Shared by tests/test_host_instance_top_linear.py and tests/test_gpu_instance_top_linear.py: moving instances under time-dependent
top-level boxes (device config inst_bounds=linear; accel kinds 32 / 33).

The accel (embree-compressed_amd/csrc/accel.h, InstanceRecord): `blobs` and `prims` are ALWAYS the general layout of the kinds 22 / 23
(instance_mesh_mb_helpers.split_blobs); the node buffer has the two sections of the kinds 30 / 31 (instance_mesh_mb_linear_helpers.
split_nodes) with the TOP-LEVEL tree in the second one: QNode8s of the instanced scenes' static trees | zero padding | QNodeMB8s - the
top-level tree, then the scenes' motion-blur trees.  The root and the inner references of the top-level tree index the buffer as one
array of QNodeMB8.

Instances are described as in instance_mb_helpers: (geomID, scene key, [local-to-world per step]); scenes as instance_mesh_mb_helpers.desc."""
import numpy as np

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import instance_mesh_mb_linear_helpers as iml
from helpers import random_soup
from instance_helpers import EMPTY, LEAF
from mb_linear_helpers import decode_children_mb, decode_nodes_mb, walk_paths

ACCEL_INSTTOP_LINEAR_PLUECKER, ACCEL_INSTTOP_LINEAR_MOELLER = 32, 33
KEY = "inst_bounds=linear"
ALL_KEYS = iml.LINEAR + "," + KEY
REF_INST_EXIT = imm.REF_INST_EXIT
TIMES33 = np.arange(33) / 32.0  # in [0, 1], every step time of 2, 3 and 5 steps included
F32 = np.float32


def kind(mode):
    """mode 0: Pluecker / robust, mode 1: Moeller / fast"""
    return ACCEL_INSTTOP_LINEAR_PLUECKER if mode == 0 else ACCEL_INSTTOP_LINEAR_MOELLER


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
def random_quads(n, seed, extent=10.0):
    rng = np.random.RandomState(seed)
    c = rng.rand(n, 1, 3) * extent
    base = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]], np.float64)
    v = ih.snap((c + base + (rng.rand(n, 4, 3) - 0.5) * 0.2).reshape(-1, 3))
    return v, np.arange(4 * n, dtype=np.uint32).reshape(-1, 4)


def soup_scene(nt=200, nq=100, seed=3):
    """one instanced scene: a random soup of nt triangles (geomID 0) and nq quads (geomID 1) in [0, 10]^3, on the 2^-10 grid"""
    d = imm.desc()
    if nt:
        v, t = random_soup(nt, seed)
        d["tris"] = (ih.snap(v), t, 0)
    if nq:
        v, q = random_quads(nq, seed + 1)
        d["quads"] = (v, q, 1)
    return d


def _t(x, y, z):
    return ih.affine((x, y, z))


RZ90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)


def instances(what):
    """the five containment scenes over one instanced scene "m" (soup_scene: [0, 10]^3); translations are whole numbers
    (a) a two-step translation, fast (2.4 x the scene's size), beside a static instance
    (b) a two-step 90 degree rotation about z - the lerped matrix shrinks the object in between - beside a static instance
    (c) three steps out and back: the middle step lies far outside the lerp of the end boxes
    (d) a five-step zig-zag
    (e) 40 instances, static and moving (2, 3 and 5 steps) mixed: the top-level tree has inner nodes below the root"""
    if what == "a":
        return [(0, "m", [_t(0, 0, 0), _t(24, 3, -2)]), (1, "m", [_t(0, 30, 0)])]
    if what == "b":
        return [(0, "m", [ih.affine((5, 5, 0)), ih.affine((5, 5, 0), rot=RZ90)]), (1, "m", [_t(40, 0, 0)])]
    if what == "c":
        return [(0, "m", [_t(0, 0, 0), _t(30, 0, 0), _t(2, 1, 0)]), (1, "m", [_t(0, 30, 0)])]
    if what == "d":
        return [(0, "m", [_t(0, 0, 0), _t(8, 12, 0), _t(16, 0, 0), _t(24, 12, 0), _t(32, 0, 0)]), (1, "m", [_t(0, -30, 0)])]
    if what == "e":
        return [(g, k, s if g % 4 else s[:1]) for g, k, s in im.exact_instances(40)]
    raise KeyError(what)


CASES = ("a", "b", "c", "d", "e")


def scene_bounds(d):
    """the instanced scene's bounds: every vertex of these soups is used"""
    vs = [d[p][0] for p in ("tris", "quads") if d.get(p) is not None]
    vs += [st for p in ("tris_mb", "quads_mb") if d.get(p) is not None for st in d[p][0]]
    v = np.concatenate(vs).astype(np.float64)
    return v.min(0), v.max(0)


def corners_at(lo, hi, steps, t):
    """float64 images [8, 3] of the eight corners of the box (lo, hi) under lerp(step[k], step[k + 1], f) at time t in [0, 1]"""
    c = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
    st = np.asarray(steps, np.float64).reshape(-1, 3, 4)
    if len(st) == 1:
        m = st[0]
    else:
        S = len(st) - 1
        ts = float(t) * S
        k = int(min(max(np.floor(ts), 0), S - 1))
        f = ts - k
        m = (1.0 - f) * st[k] + f * st[k + 1]
    return c @ m[:, :3].T + m[:, 3]


# ---- the exported accel -----------------------------------------------------------------------------------------------------------------------
def counts(scenes, inst):
    """(quads, steps, scenes, TriMBRecords, QuadMBRecords) of the general layout for instanced scenes WITHOUT moving meshes"""
    used = []
    for _, k, _ in inst:
        if k not in used:
            used.append(k)
    nq = sum(len(scenes[k]["quads"][1]) for k in used if scenes[k].get("quads") is not None)
    ns = sum(len(s) for _, _, s in inst if len(s) > 1)
    return nq, ns, len(used), 0, 0


def top_leaves(top):
    """[(path, record index)] of the top-level tree: path = [(QNodeMB8 index in 144-byte units, child slot), ...] from the root down"""
    _, image_mb, _, first = iml.split_nodes(top)
    root = top.accel_root()
    assert not root & LEAF and root >= first  # an inner node of the second section, even for a single instance
    out = []
    for path, rec, n in walk_paths(image_mb, root):
        assert n == 1 and all(node >= first for node, _ in path)
        out.append((path, rec))
    return image_mb, out


def path_boxes(image_mb, path, t):
    """[(lo[3], hi[3])] float64 of the boxes on `path` at ray time t, decoded with the kernel's fp32 formula"""
    out = []
    for node, slot in path:
        lo, hi = decode_children_mb(image_mb[node], t)
        out.append((lo[slot].astype(np.float64), hi[slot].astype(np.float64)))
    return out


def passes(boxes, org, dirs):
    """mask of the rays (float64 [m, 3]; tnear 0, tfar inf) whose slab test passes EVERY box of `boxes` [(lo[m or 1, 3], hi)]"""
    ok = np.ones(len(org), bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        rd = 1.0 / dirs
        for lo, hi in boxes:
            t1, t2 = (lo - org) * rd, (hi - org) * rd
            tn = np.maximum(np.fmax.reduce(np.minimum(t1, t2), axis=1), 0.0)
            tf = np.fmin.reduce(np.maximum(t1, t2), axis=1)
            ok &= tn <= tf
    return ok


# ---- the stack walk: the top level and the motion-blur trees over QNodeMB8s, the static trees over QNode8s ----------------------------------------
def _entry_matrix(inst, rec, time):
    """world2local as [4, 3] float64 rows vx, vy, vz, p: the record's for a static instance, the float64 inverse of the lerped steps
    (instance_mb_helpers.world2local_f64) for a moving one"""
    pad1 = int(rec["pad"][1])
    if pad1 == 0:
        return rec["world2local"].astype(np.float64).reshape(4, 3)
    S, first = pad1 >> 24, pad1 & 0xFFFFFF
    steps = inst.blobs64[first:first + S + 1]["local2world"].reshape(-1, 4, 3).transpose(0, 2, 1)  # [S + 1, 3, 4] row-major
    w = im.world2local_f64(steps, np.array([time], F32))[0]  # [3, 4]
    return np.ascontiguousarray(w.T)


def simulate_stack(top, org, dirs, times, inst, tfar=np.inf):
    """instance_mesh_mb_linear_helpers.simulate_stack for the kinds 32 / 33: a lane OUTSIDE an instance reads QNodeMB8s too.  `inst` is an
    instance_mesh_mb_helpers.WalkInstances with `blobs64` = the blobs as InstanceSteps.  Returns per ray (deepest slot written, most
    markers stacked at once)."""
    nodes8, image_mb, _, _ = iml.split_nodes(top)
    static = ds.decode_nodes(nodes8) if len(nodes8) else (None, None, None)
    times = np.asarray(times, F32)
    out = np.zeros((len(org), 2), np.int64)
    for t in np.unique(times):
        with np.errstate(over="ignore", invalid="ignore"):  # entries that overlay QNode8s decode to anything: no QNodeMB8 reference names them
            timed = decode_nodes_mb(image_mb, t)
        for i in np.nonzero(times == t)[0]:
            out[i] = _walk_one(static, timed, int(top.accel_root()), np.asarray(org[i], np.float64), np.asarray(dirs[i], np.float64), float(tfar), float(t), inst)
    return out[:, 0], out[:, 1]


def _walk_one(static, timed, root, wo, wd, tfar, time, inst):
    o, d = wo, wd
    with np.errstate(divide="ignore"):
        rd = 1.0 / d
    stack, deepest, most_markers = [], -1, 0
    cur, inside, code = root, False, imm.TREE_TRI

    def note():
        nonlocal deepest, most_markers
        deepest = max(deepest, len(stack) - 1)
        most_markers = max(most_markers, sum(1 for r, _ in stack if REF_INST_EXIT < r <= REF_INST_EXIT + 3))

    while True:
        if cur != EMPTY and not cur & LEAF:
            lo, hi, child = timed if (not inside or code in iml.MB_CODES) else static
            with np.errstate(invalid="ignore"):
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
            m = _entry_matrix(inst, rec, time)
            o, d = wo @ m[:3] + m[3], wd @ m[:3]
            with np.errstate(divide="ignore"):
                rd = 1.0 / d
            stack.append((REF_INST_EXIT, 0.0))
            inside = True
            sc = inst.scenes[int(rec["root"]) - inst.scene_base]
            have = [(int(sc[f]), c) for f, c in imm.VISIT if int(sc[f]) != EMPTY]
            for r, c in reversed(have[1:]):
                stack.append((imm.marker(c), r))
            note()
            cur, code = have[0] if have else (EMPTY, imm.TREE_TRI)
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
                o, d, inside, code = wo, wd, False, imm.TREE_TRI
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
            return deepest, most_markers


def walk_instances(top, scenes, inst, pluecker):
    w = imm.WalkInstances(top, len(inst), counts(scenes, inst), pluecker)
    w.blobs64 = top.accel_data(2).view(im.STEP_DT)
    return w


# ---- the deep chain: nested boxes at top level over a needle soup ----------------------------------------------------------------------------
CHAIN_N, CHAIN_NEEDLES = 30, 1024


def chain_case():
    """30 instances of one soup of 1024 needle triangles (deep_stack_helpers.sliver_soup) whose boxes are nested: instance i is the
    soup scaled by 1 + i / 32 about the centre of the unit cube, so box i lies inside box i + 1 and a ray through the middle enters all of
    them - up to 7 entries per top-level level on the stack, then the exit marker and the needles' own deep stack.  Instance 0 moves (two
    steps, by 1 / 16 along x), which makes the kind 32 / 33; everything lies on the 2^-10 grid."""
    v, t = ds.sliver_soup(CHAIN_NEEDLES, ds.SOUP_SEED, snapped=True)
    scenes = {"m": imm.desc(tris=(v, t, 3))}
    inst = []
    for i in range(CHAIN_N):
        s = 1.0 + i / 32.0
        m = ih.affine((0.5 - 0.5 * s,) * 3, (s,) * 3)
        inst.append((i, "m", [m, ih.affine((0.5 - 0.5 * s + 0.0625, 0.5 - 0.5 * s, 0.5 - 0.5 * s), (s,) * 3)] if i == 0 else [m]))
    return scenes, inst


def chain_rays(rtc, m, seed):
    """m rays on the 2^-10 grid from inside the unit cube, random directions, times k / 4"""
    from helpers import fill_rays
    rng = np.random.RandomState(seed)
    rays = rtc.aligned_rayhits(m)
    fill_rays(rays, ds.snap(0.25 + rng.rand(m, 3) * 0.5), rng.randn(m, 3).astype(F32))
    rays["time"] = np.asarray(ds.TIMES, F32)[np.arange(m) % len(ds.TIMES)]
    return rays
