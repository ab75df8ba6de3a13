"""CPU tests of time-dependent node boxes below instances (device config inst_mb_bounds=linear over scenes built under mb_bounds=linear;
accel kinds 30 / 31) on a `gpu=none` device that names every accel key: when the kinds are chosen and what stays byte for byte what it
was, the two-section node buffer as accel.h documents it, containment through the rebased image, the stack bound and the refusals.
Not tested: the builder's refusal of a QNodeMB8 index that would reach the leaf bit ("too many instanced motion blur nodes ..."), which
takes about 2^31 nodes."""
import ctypes as C

import numpy as np
import pytest

import instance_helpers as ih
import instance_mesh_mb_helpers as imm
import instance_mesh_mb_linear_helpers as iml
import instance_quads_helpers as iq
import deep_stack_helpers as ds
from helpers import random_soup
from instance_helpers import EMPTY, LEAF, NODE_DT, TRI_DT
from mb_linear_helpers import NODEMB_DT, QUAD_ENDS, QUADMB_DT, TRI_ENDS, TRIMB_DT, decode_children_mb, record_vertices, walk_paths

BASE = "gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,inst_accel=default"
SWEPT = BASE + ",mb_bounds=swept"
LIN = BASE + "," + iml.LINEAR
ERRFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)
REFUSAL = "an instanced scene with a motion blur accel built under mb_bounds=linear is not supported (instance accels hold swept node boxes: use mb_bounds=swept)"
FIELDS = {"tris": "triRoot", "tris_mb": "triMBRoot", "quads": "quadRoot", "quads_mb": "quadMBRoot"}
PART_DT = {"tris": (1, TRI_DT), "tris_mb": (2, TRIMB_DT), "quads": (2, iq.QUAD_DT), "quads_mb": (2, QUADMB_DT)}


class Errors:
    """the messages the device reports through rtcSetDeviceErrorFunction"""

    def __init__(self, dev):
        self.log = []
        self.fn = ERRFN(lambda user, code, msg: self.log.append((code, (msg or b"").decode())))
        dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(self.fn, C.c_void_p), None)
        self.dev = dev

    def expect(self, code, text):
        assert self.dev.error() == code, self.log
        assert self.log and self.log[-1][0] == code and text in self.log[-1][1], self.log
        self.log.clear()


def _random_quads(n, seed):
    rng = np.random.RandomState(seed)
    c = rng.rand(n, 1, 3) * 10.0
    base = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]], np.float64)
    v = (c + base + (rng.rand(n, 4, 3) - 0.5) * 0.2).reshape(-1, 3).astype(np.float32)
    return v, np.arange(4 * n, dtype=np.uint32).reshape(-1, 4)


def _moved(v, nsteps, seed):
    rng = np.random.RandomState(seed)
    shift = rng.rand(3).astype(np.float32) * 0.5
    return [(v + k * shift).astype(np.float32) for k in range(nsteps)]


def _desc(nt=0, ntm=0, nq=0, nqm=0, seed=3):
    """an instanced scene with nt static triangles (geomID 0), ntm moving ones (1, two steps), nq static quads (2), nqm moving ones (3,
    three steps)"""
    d = imm.desc()
    if nt:
        v, t = random_soup(nt, seed)
        d["tris"] = (v, t, 0)
    if ntm:
        v, t = random_soup(ntm, seed + 1)
        d["tris_mb"] = (_moved(v, 2, seed + 1), t, 1)
    if nq:
        v, q = _random_quads(nq, seed + 2)
        d["quads"] = (v, q, 2)
    if nqm:
        v, q = _random_quads(nqm, seed + 3)
        d["quads_mb"] = (_moved(v, 3, seed + 3), q, 3)
    return d


def _top(rtc, dev, inner, uses, flags=0, moving=()):
    top = rtc.Scene(dev, flags)
    ids = {}
    for i, k in enumerate(uses):
        m = ih.affine((30.0 * i, 0, 0))
        if i in moving:
            ids[top.add_instance_mb(inner[k], [m, ih.affine((30.0 * i, 1.0, 0)), ih.affine((30.0 * i, 2.0, 0.5))])] = k
        else:
            ids[top.add_instance(inner[k], m)] = k
    return top, ids


def _release(dev, top, inner):
    top.release()
    for s in inner.values():
        s.release()
    dev.release()


def _own(rtc, cfg, d, mode):
    """the accels of the scene `d` as scenes of their own export them on a device of config `cfg`:
    {part: (nodes, records, root, maxDepth, kind) or None}; the nodes of a kind 26..29 accel are QNodeMB8s"""
    dev = rtc.Device(cfg)
    out = {}
    for part in imm.PARTS:
        if d.get(part) is None:
            out[part] = None
            continue
        sc = imm.add_scene(rtc, dev, imm.desc(**{part: d[part]}), mode)
        st = sc.stats()
        data, dt = PART_DT[part]
        out[part] = (sc.accel_data(0).view(NODEMB_DT if st["nodeBytes"] == 144 else NODE_DT).copy(), sc.accel_data(data).view(dt).copy(), sc.accel_root(), st["maxDepth"],
                     st["accelKind"])
        sc.release()
    dev.release()
    return out


# ---- 1. the key, the kinds and what stays ---------------------------------------------------------------------------------------------------------
def test_unknown_inst_mb_bounds_is_an_invalid_argument(rtc):
    with pytest.raises(rtc.RTCError) as e:
        rtc.Device("gpu=none,inst_mb_bounds=bogus")
    assert e.value.code == rtc.RTC_ERROR_INVALID_ARGUMENT
    for ok in ("swept", "linear"):
        rtc.Device("gpu=none,inst_mb_bounds=" + ok).release()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(0, 20, 0, 0), (0, 0, 0, 20), (16, 20, 12, 20)])
def test_swept_keeps_the_refusal_and_linear_gives_the_kinds_30_31(rtc, mode, shape):
    for cfg in (BASE + ",mb_bounds=linear", BASE + ",mb_bounds=linear,inst_mb_bounds=swept",
                "gpu=none,quad_accel=default,mb_bounds=linear,inst_mb_bounds=linear"):  # (the last one: a host-only device that takes no moving meshes below instances)
        dev = rtc.Device(cfg)
        err = Errors(dev)
        if "inst_accel" not in cfg and (shape[2] or shape[3]):
            dev.release()
            continue
        inner = {"a": imm.add_scene(rtc, dev, _desc(*shape), mode)}
        top, _ = _top(rtc, dev, inner, "aa", iq.flags(mode))
        top.lib.rtcCommitScene(top.handle)
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, REFUSAL)
        _release(dev, top, inner)
    dev = rtc.Device(LIN)
    inner = {"a": imm.add_scene(rtc, dev, _desc(*shape), mode), "s": imm.add_scene(rtc, dev, _desc(16, 0, 12, 0, seed=9), mode)}
    for part, k in (("tris_mb", (26, 27)), ("quads_mb", (28, 29))):
        if shape[imm.PARTS.index(part)]:
            alone = imm.add_scene(rtc, dev, imm.desc(**{part: _desc(*shape)[part]}), mode)
            assert alone.stats()["accelKind"] == k[mode]
            alone.release()
    top, _ = _top(rtc, dev, inner, "sas", iq.flags(mode))
    top.commit()
    st = top.stats()
    assert st["accelKind"] == iml.kind(mode) == (30, 31)[mode] and st["leafCount"] == 3 and st["nodeBytes"] == 96
    _release(dev, top, inner)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["swept scenes", "static scenes", "static scenes, moving instances"])
def test_without_a_linear_accel_below_the_key_changes_no_byte(rtc, mode, what):
    """inst_mb_bounds=linear over scenes built under mb_bounds=swept, or over static scenes only: the kind and the four accel arrays of a
    device without the key"""
    got = []
    mesh_mb = what == "swept scenes"
    for cfg in (BASE + ",inst_mb_bounds=linear" if mesh_mb else LIN, BASE):
        dev = rtc.Device(cfg)
        inner = {"a": imm.add_scene(rtc, dev, _desc(40, 30 if mesh_mb else 0, 24, 20 if mesh_mb else 0), mode), "b": imm.add_scene(rtc, dev, _desc(24, 0, 0, 0, seed=5), mode)}
        top, _ = _top(rtc, dev, inner, "abab", iq.flags(mode), moving=(1, 2) if "moving" in what else ())
        top.commit()
        st = top.stats()
        got.append((st["accelKind"], top.accel_root(), st["maxDepth"], st["nodeCount"], st["nodeBytes"], st["totalBytes"], [top.accel_data(k).tobytes() for k in range(4)]))
        _release(dev, top, inner)
    want = imm.kind(mode) if mesh_mb else ((20, 21) if "moving" in what else (16, 17))[mode]
    assert got[0][0] == want
    assert got[0] == got[1]


# ---- 2. layout --------------------------------------------------------------------------------------------------------------------------------------
# name -> ({scene key: _desc arguments}, uses in instance order, indices of moving instances)
LAYOUTS = {
    "a single instance of a motion-blur tree: no QNode8 at all": ({"a": dict(ntm=60, seed=3)}, "a", ()),
    "a motion-blur tree whose root is a leaf: no QNodeMB8": ({"a": dict(ntm=3, seed=3)}, "aa", ()),
    "all four trees in one scene": ({"a": dict(nt=40, ntm=30, nq=24, nqm=20, seed=3)}, "aaa", (1,)),
    "two scenes, one instanced twice": ({"a": dict(ntm=44, nqm=36, seed=13), "b": dict(nt=100, ntm=50, seed=23)}, "aba", ()),
    "a static scene beside a moving one": ({"s": dict(nt=28, nq=32, seed=33), "m": dict(ntm=70, seed=43)}, "sm", (0,)),
    "a root-leaf tree beside a full one": ({"a": dict(nt=200, ntm=2, seed=5), "b": dict(nqm=40, nq=3, seed=7)}, "abba", (3,)),
}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_node_buffer_decodes_per_the_documented_layout(rtc, mode, name):
    """Against the kinds 22 / 23 build of the same scenes (mb_bounds=swept) and against the instanced scenes' own accels.  `prims` and the
    InstanceRecords, QuadRecords and InstanceSteps of `blobs` are the swept build's bytes and every section of `blobs` starts where it
    starts there; the scene records differ in their roots and the motion-blur records are those of the instanced scenes' own (midpoint
    built) accels, byte for byte - as a set the swept build's."""
    shapes, uses, moving = LAYOUTS[name]
    descs = {k: _desc(**a) for k, a in shapes.items()}
    order = list(dict.fromkeys(uses))
    own = {k: _own(rtc, LIN, descs[k], mode) for k in order}
    own_swept = {k: _own(rtc, SWEPT, descs[k], mode) for k in order}
    built = {}
    for cfg in (LIN, SWEPT):
        dev = rtc.Device(cfg)
        inner = {k: imm.add_scene(rtc, dev, d, mode) for k, d in descs.items()}
        top, ids = _top(rtc, dev, inner, uses, iq.flags(mode), moving)
        top.commit()
        built[cfg] = (dev, top, inner, ids)
    top, ids = built[LIN][1], built[LIN][3]
    top22 = built[SWEPT][1]
    assert top.stats()["accelKind"] == iml.kind(mode) and top22.stats()["accelKind"] == imm.kind(mode)
    n = len(uses)
    count = lambda part: sum(len(own[k][part][1]) for k in order if own[k][part] is not None)  # noqa: E731
    cat = lambda part: b"".join(own[k][part][1].tobytes() for k in order if own[k][part] is not None)  # noqa: E731
    counts = (n, count("quads"), 3 * len(moving), len(order), count("tris_mb"), count("quads_mb"))
    # -- prims and blobs
    assert top.accel_data(1).tobytes() == top22.accel_data(1).tobytes() == cat("tris")
    blobs, blobs22 = top.accel_data(2), top22.accel_data(2)
    assert len(blobs) == len(blobs22)
    recs, quads, steps, scenes, trimb, quadmb, t_off, q_off = imm.split_blobs(blobs, *counts)
    recs22, quads22, steps22, scenes22, trimb22, quadmb22, t_off22, q_off22 = imm.split_blobs(blobs22, *counts)
    assert (t_off, q_off) == (t_off22, q_off22)
    assert recs.tobytes() == recs22.tobytes() and quads.tobytes() == quads22.tobytes() and steps.tobytes() == steps22.tobytes()
    assert trimb.tobytes() == cat("tris_mb") and quadmb.tobytes() == cat("quads_mb")
    split = lambda a: sorted(a[i].tobytes() for i in range(len(a)))  # noqa: E731
    assert split(trimb) == split(trimb22) and split(quadmb) == split(quadmb22)
    assert not scenes["pad"].any()
    scene_base = n + len(quads) + len(steps)
    for r in recs:
        assert int(r["root"]) - scene_base == order.index(ids[int(r["geomID"])]) and r["pad"][0] == 0
    # -- the node buffer
    nodes8, image_mb, n_mb, first = iml.split_nodes(top)  # sizes, padding, blobOffsets, statistics
    assert first * 144 >= len(nodes8) * 96 > (first - 1) * 144 or len(nodes8) == 0 and first == 0
    st = top.stats()
    assert st["totalBytes"] == (first + n_mb) * 144 + len(top.accel_data(1)) + len(blobs) + 8
    if n == 1:
        assert top.accel_root() & LEAF and all(own[order[0]][p] is None for p in ("tris", "quads")) == (len(nodes8) == 0)
    bases = {"tris": 0, "quads": n, "tris_mb": t_off // 96, "quads_mb": q_off // 128}
    next_mb = first
    static_ranges, mb_ranges22 = [], []
    nodes22 = top22.accel_data(0).view(NODE_DT)
    for si, k in enumerate(order):
        for part in imm.PARTS:  # Scene::commit's order
            root, root22 = int(scenes[si][FIELDS[part]]), int(scenes22[si][FIELDS[part]])
            o = own[k][part]
            assert (root == EMPTY) == (o is None) == (root22 == EMPTY), (k, part)
            if o is None:
                continue
            onodes, orecs, oroot, _, okind = o
            base = bases[part]
            bases[part] += len(orecs)
            timed = part.endswith("_mb")
            assert (okind in (26, 27, 28, 29)) == timed and onodes.dtype == (NODEMB_DT if timed else NODE_DT)
            if timed and not root22 & LEAF:
                nb22 = root22 - own_swept[k][part][2]
                mb_ranges22.append((nb22, nb22 + len(own_swept[k][part][0])))
            if root & LEAF:  # the tree is one leaf: it contributes no node
                assert oroot & LEAF and root == oroot + base and len(onodes) == 0
                continue
            nb = root - oroot
            if timed:  # the roots point into the QNodeMB8 section, the trees lie there in order and without gaps
                assert nb == next_mb and first <= nb and nb + len(onodes) <= first + n_mb
                next_mb += len(onodes)
                run = image_mb[nb:nb + len(onodes)]
                assert run["q1"].tobytes() == onodes["q1"].tobytes()
                got = sorted((f, c) for _, f, c in walk_paths(image_mb, root))
                assert got == sorted((f + base, c) for _, f, c in walk_paths(onodes, oroot)) and sum(c for _, c in got) == len(orecs)
            else:
                assert nb + len(onodes) <= len(nodes8)
                static_ranges.append((nb, nb + len(onodes)))
                run = nodes8[nb:nb + len(onodes)]
            # the instanced scene's own nodes, byte for byte apart from the child words; every child word is the own word plus the base
            for f in ("origin", "exp", "pad", "q"):
                assert run[f].tobytes() == onodes[f].tobytes(), (k, part, f)
            oc = onodes["child"].astype(np.int64)
            want = np.where(oc == EMPTY, EMPTY, np.where(oc & LEAF, oc + base, oc + nb))
            assert np.array_equal(run["child"].astype(np.int64), want), (k, part)
    assert next_mb == first + n_mb
    # top-level tree first, then the static trees per scene, without gaps
    top_nodes = static_ranges[0][0] if static_ranges else len(nodes8)
    assert static_ranges == sorted(static_ranges) and all(a[1] == b[0] for a, b in zip(static_ranges, static_ranges[1:]))
    assert (static_ranges[-1][1] if static_ranges else top_nodes) == len(nodes8)
    leaves, _ = imm.walk(nodes8[:top_nodes], top.accel_root())
    assert sorted(f for f, _ in leaves) == list(range(n)) and all(c == 1 for _, c in leaves)
    # the QNode8 section is the node array of the kinds 22 / 23 build minus its motion-blur trees: the same nodes, inner child indices
    # moved down by the motion-blur nodes removed in front of them
    keep = np.ones(len(nodes22), bool)
    for a, b in mb_ranges22:
        keep[a:b] = False
    assert int(keep.sum()) == len(nodes8)
    new_index = np.cumsum(keep) - 1
    kept = nodes22[keep]
    for f in ("origin", "exp", "pad", "q"):
        assert kept[f].tobytes() == nodes8[f].tobytes(), f
    c22 = kept["child"].astype(np.int64)
    inner_ref = (c22 != EMPTY) & ((c22 & LEAF) == 0)
    assert keep[c22[inner_ref]].all()
    want = c22.copy()
    want[inner_ref] = new_index[c22[inner_ref]]
    assert np.array_equal(nodes8["child"].astype(np.int64), want)
    for dev, t, inner, _ in built.values():
        _release(dev, t, inner)


def test_the_layout_cases_put_0_1_and_2_mod_3_qnode8s_in_front_of_the_section(rtc):
    """the padding in front of the QNodeMB8 section is 0, 48 or 96 bytes: 96 n mod 144 = 0 for n = 0 mod 3, 96 for 1, 48 for 2"""
    seen = {}
    for name, (shapes, uses, moving) in LAYOUTS.items():
        dev = rtc.Device(LIN)
        inner = {k: imm.add_scene(rtc, dev, _desc(**a), 1) for k, a in shapes.items()}
        top, _ = _top(rtc, dev, inner, uses, 0, moving)
        top.commit()
        nodes8, _, n_mb, first = iml.split_nodes(top)
        seen[name] = (len(nodes8), n_mb, first * 144 - len(nodes8) * 96)
        _release(dev, top, inner)
    print(seen)
    assert {n8 % 3 for n8, _, _ in seen.values()} == {0, 1, 2}
    assert {pad for _, _, pad in seen.values()} == {0, 48, 96}
    assert seen["a single instance of a motion-blur tree: no QNode8 at all"][0] == 0
    assert seen["a motion-blur tree whose root is a leaf: no QNodeMB8"][1] == 0


# ---- 3. containment through the instance accel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_every_ancestor_box_in_the_rebased_image_holds_the_interpolated_vertices(rtc, mode):
    """test_host_mb_linear_bounds.py's assertion through the instance accel: every root-to-leaf path of every motion-blur tree reached
    through the scene records, decoded from the buffer as an array of QNodeMB8, holds the vertices its records produce at the times 0, 0.3,
    0.5 and 1.  At a time outside [0, 1] the node step clamps: the box is the one of the nearer end, bit for bit (a record extrapolates
    there; accel.h states that no containment is promised)."""
    descs = {"a": _desc(nt=40, ntm=90, nq=24, nqm=60, seed=3), "b": _desc(ntm=120, seed=11), "c": _desc(nt=9, nqm=80, seed=17)}
    dev = rtc.Device(LIN)
    inner = {k: imm.add_scene(rtc, dev, d, mode) for k, d in descs.items()}
    top, _ = _top(rtc, dev, inner, "abca", iq.flags(mode), moving=(2,))
    top.commit()
    assert top.stats()["accelKind"] == iml.kind(mode)
    _, image_mb, n_mb, first = iml.split_nodes(top)
    blobs = top.accel_data(2)
    as_array = lambda dt: blobs[:len(blobs) // dt.itemsize * dt.itemsize].view(dt)  # noqa: E731  (the kernel's view: ONE array of that record type)
    nq = sum(len(d["quads"][1]) for d in descs.values() if d["quads"] is not None)
    scenes = blobs[(4 + nq + 3) * 64:(4 + nq + 3 + 3) * 64].view(imm.SCENE_DT)
    checks, bad, trees, visited, nrecs = 0, [], 0, set(), 0
    for sc in scenes:
        for field, dt, ends in (("triMBRoot", TRIMB_DT, TRI_ENDS), ("quadMBRoot", QUADMB_DT, QUAD_ENDS)):
            root = int(sc[field])
            if root == EMPTY:
                continue
            assert not root & LEAF and first <= root < first + n_mb
            trees += 1
            recs = as_array(dt)
            for path, f0, count in walk_paths(image_mb, root):
                visited.update(n for n, _ in path)
                nrecs += count
                for r in recs[f0:f0 + count]:
                    assert int(r["numSegments"]) in (1, 2) and int(r["segment"]) < int(r["numSegments"])
                    for t in (0.0, 0.3, 0.5, 1.0):
                        p = record_vertices(r, ends, np.float32(t))
                        if p is None:  # another segment's record
                            continue
                        for node, slot in path:
                            lo, hi = decode_children_mb(image_mb[node], t)
                            checks += 1
                            if not ((lo[slot] <= p).all() and (p <= hi[slot]).all()):
                                bad.append((node, slot, t, lo[slot], hi[slot], p))
    assert trees == 4 and visited == set(range(first, first + n_mb))
    print(f"mode {mode}: {trees} motion-blur trees, {n_mb} QNodeMB8s from index {first}, {checks} box checks")
    assert nrecs == 90 + 120 + 2 * (60 + 80) and checks >= 2 * nrecs  # every record at two of the four times or more, under one ancestor or more
    assert not bad, bad[:3]
    for node in image_mb[first:first + n_mb]:
        for t, end in ((-0.5, 0.0), (1.5, 1.0), (np.nan, 0.0)):
            a, b = decode_children_mb(node, t), decode_children_mb(node, end)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    _release(dev, top, inner)


# ---- 4. stack bound -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,trees", [((0, 0, 0, 1500), 1), ((8, 1500, 0, 0), 2), ((8, 0, 40, 1500), 3), ((8, 1500, 40, 700), 4)])
def test_max_depth_equals_the_formula(rtc, shape, trees):
    """maxDepth = top-level depth + 1 (exit marker) + the most pending-tree markers of any scene (its trees - 1) + the deepest tree, with
    the depth of a linear accel as that accel reports it"""
    d = _desc(*shape, seed=9)
    own = _own(rtc, LIN, d, 1)
    deepest = max(o[3] for o in own.values() if o is not None)
    assert deepest >= 2
    dev = rtc.Device(LIN)
    inner = {"a": imm.add_scene(rtc, dev, d, 1), "one": imm.add_scene(rtc, dev, _desc(0, 4, 0, 0, seed=1), 1)}
    top = rtc.Scene(dev)
    for i in range(20):
        top.add_instance(inner["a"], ih.affine((12.0 * i, 0, 0)))
    top.add_instance(inner["one"], ih.affine((0, 40.0, 0)))  # a scene with fewer trees does not lower the bound
    top.commit()
    assert top.stats()["accelKind"] == iml.ACCEL_INSTMESHMB_LINEAR_MOELLER
    nodes8, image_mb, n_mb, first = iml.split_nodes(top)
    _, top_levels = imm.walk(nodes8, top.accel_root())  # (instance leaves end the walk)
    assert top_levels >= 2
    assert top.stats()["maxDepth"] == top_levels + 1 + (trees - 1) + deepest
    # the depth a linear accel reports is the depth of its tree in the image
    scenes = imm.split_blobs(top.accel_data(2), 21, shape[2], 0, 2, shape[1] + 4, 2 * shape[3])[3]
    for f, part in (("triMBRoot", "tris_mb"), ("quadMBRoot", "quads_mb")):
        if own[part] is not None:
            assert max(len(path) for path, _, _ in walk_paths(image_mb, int(scenes[0][f]))) == own[part][3]
    _release(dev, top, inner)


def test_the_walk_over_both_node_types_passes_slot_16_and_stacks_markers_there(rtc):
    """the preconditions of the GPU tests of the overflow area, on the host walk of instance_mesh_mb_linear_helpers alone: under
    deep_instances() rays of imm.deep_scene() write slots beyond the 16 in LDS while a tree marker is stacked, in
    imm.marker_spill_case() a tree marker itself is written beyond slot 16; no ray writes beyond stack_capacity(maxDepth)."""
    scenes = imm.deep_scene()
    inst = [(g, k, [m]) for g, k, m in ds.deep_instances()]
    dev, top, inner = imm.build(rtc, 1, scenes, inst, LIN)
    st = top.stats()
    assert st["accelKind"] == iml.ACCEL_INSTMESHMB_LINEAR_MOELLER
    lo, hi = ds.instance_ray_box({"m": {"tris": scenes["m"]["tris"], "quads": scenes["m"]["quads"]}}, ds.deep_instances())
    rng = np.random.RandomState(ds.HOST_RAY_SEED)
    m = 100
    org = lo + rng.rand(m, 3) * (hi - lo)
    dirs = rng.randn(m, 3)
    times = np.asarray(ds.TIMES)[np.arange(m) % len(ds.TIMES)]
    n = imm.DEEP_N
    w = imm.WalkInstances(top, 3, (n, 0, 1, n, n), pluecker=False)
    deepest, markers, marked, _ = iml.simulate_stack(top, org, dirs, times, w)
    share = float((marked >= ds.LDS_STACK).mean())
    print(f"deepest slot {deepest.max()} of {ds.stack_capacity(st['maxDepth'])}, most markers {markers.max()}, "
          f"{100 * share:.1f} % of the rays pass slot {ds.LDS_STACK} with a marker stacked")
    assert deepest.max() < ds.stack_capacity(st["maxDepth"]) and markers.max() == 3
    assert (marked >= ds.LDS_STACK).sum() >= 1
    iq.release(dev, top, inner)
    scenes, inst = imm.marker_spill_case()
    dev, top, inner = imm.build(rtc, 1, scenes, inst, LIN)
    st = top.stats()
    rays = imm.marker_spill_rays(rtc, 60, ds.HOST_RAY_SEED)
    org = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1)
    dirs = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1)
    n = imm.MARKER_N
    w = imm.WalkInstances(top, len(inst), (n, 0, 1, n, n), pluecker=False)
    deepest, markers, _, marker_slot = iml.simulate_stack(top, org, dirs, rays["time"], w)
    print(f"deepest slot {deepest.max()} of {ds.stack_capacity(st['maxDepth'])}, highest marker slot {marker_slot.max()}, "
          f"{int((marker_slot >= ds.LDS_STACK).sum())} of {len(rays)} rays write a tree marker beyond slot {ds.LDS_STACK}")
    assert deepest.max() < ds.stack_capacity(st["maxDepth"]) and markers.max() == 3
    assert (marker_slot >= ds.LDS_STACK).sum() >= 1
    iq.release(dev, top, inner)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_linear_accels_that_disagree_in_arithmetic_are_refused_with_the_present_messages(rtc):
    # within one scene: a robust scene under an explicit (Moeller) motion-blur accel beside its Pluecker triangles
    dev = rtc.Device(LIN.replace("tri_accel_mb=default", "tri_accel_mb=bvh8.triangle4imb"))
    err = Errors(dev)
    sc = rtc.Scene(dev, iq.ROBUST)
    v, t = random_soup(16, 1)
    sc.add_triangles(v, t)
    sc.add_triangles_mb(_moved(v, 2, 2), t)
    sc.commit()
    top = rtc.Scene(dev, iq.ROBUST)
    top.add_instance(sc)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "disagree in kind (Pluecker / robust: triangle; Moeller / fast: motion blur triangle)")
    top.release()
    sc.release()
    dev.release()
    # across scenes: a robust static scene beside a fast moving one; a robust moving one beside a fast moving one
    dev = rtc.Device(LIN)
    err = Errors(dev)
    a = rtc.Scene(dev, iq.ROBUST)
    a.add_triangles(v, t)
    a.commit()
    b = rtc.Scene(dev, 0)
    b.add_triangles_mb(_moved(v, 2, 2), t)
    b.commit()
    c = rtc.Scene(dev, iq.ROBUST)
    c.add_triangles_mb(_moved(v, 2, 2), t)
    c.commit()
    assert (b.stats()["accelKind"], c.stats()["accelKind"]) == (27, 26)
    text = "the instanced scenes of one scene disagree in accel kind (Pluecker / robust and Moeller / fast): the scene of instance 1 has "
    for order, want in (((a, b), "Moeller / fast accels (motion blur triangle), the scene of instance 0 Pluecker / robust ones (triangle)"),
                        ((b, a), "Pluecker / robust accels (triangle), the scene of instance 0 Moeller / fast ones (motion blur triangle)"),
                        ((c, b), "Moeller / fast accels (motion blur triangle), the scene of instance 0 Pluecker / robust ones (motion blur triangle)")):
        top = rtc.Scene(dev)
        for s in order:
            top.add_instance(s)
        top.lib.rtcCommitScene(top.handle)
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, text + want)
        top.release()
    for s in (a, b, c):
        s.release()
    dev.release()
