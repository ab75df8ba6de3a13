"""CPU tests of time-dependent top-level boxes above moving subdivision instances (device config inst_subdiv_bounds=linear; accel kinds
34 / 35) on a `gpu=none,inst_accel=default,subdiv_accel=<family>` device: the key, when the kinds are chosen and what stays byte for byte
what it was, the layout as accel.h documents it, containment of the moving instances at 33 times, tightness at both ends, how many rays
still enter a fast mover, the stack bound and the refusals, which keep their texts under the key.
Not tested: the refusal of a top-level node index that would reach the leaf bit, which takes about 2^31 nodes."""
import ctypes as C

import numpy as np
import pytest

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mb_helpers as im
import instance_subdiv_helpers as isd
import instance_subdiv_top_linear_helpers as stl
import instance_top_linear_helpers as itl
from helpers import random_soup
from instance_helpers import EMPTY, LEAF, NODE_DT
from mb_linear_helpers import decode_children_mb, walk_paths

ERRFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)
SQUARE = (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), np.array([4], np.uint32), np.array([0, 1, 2, 3], np.uint32))


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


def _meshes(bomberman, L=3, Cl=2):
    """two instanced scenes: the first 32 faces of bomberman at (L, Cl) and the cube one tessellation level higher"""
    return {"m": isd.bomberman_faces(bomberman) + (L, Cl), "c": isd.cube() + (L + 1, Cl)}


def _instances(moving=True):
    """five instances: three of "m" (one of them moving, three steps), two of "c" (one moving, two steps) - both scenes are shared"""
    inst = isd.lattice_instances(5, keys=("m", "c"))
    if moving:
        g, k, steps = inst[2]
        inst[2] = (g, k, [steps[0], ih.affine((85.0, 3.0, 1.0), (0.5,) * 3), ih.affine((90.0, -2.0, 4.0), (0.5,) * 3)])
        g, k, steps = inst[3]
        inst[3] = (g, k, [steps[0], ih.affine((125.0, 7.0, 2.0), (1.0,) * 3)])
    return inst


def _export(top):
    st = top.stats()
    return (st["accelKind"], top.accel_root(), st["maxDepth"], st["nodeCount"], st["nodeBytes"], st["leafCount"], st["totalBytes"], [top.accel_data(k).tobytes() for k in range(4)])


# ---- 1. the key and the kinds ---------------------------------------------------------------------------------------------------------------------
def test_unknown_inst_subdiv_bounds_is_an_invalid_argument(rtc):
    with pytest.raises(rtc.RTCError) as e:
        rtc.Device("gpu=none,inst_subdiv_bounds=bogus")
    assert e.value.code == rtc.RTC_ERROR_INVALID_ARGUMENT
    # the message of a failed rtcNewDevice is not handed out by the API (the error is kept per thread, as a code): its wording -
    # inst_subdiv_bounds=: unknown value '<v>' (swept or linear) - is looked up in the library
    import os
    with open(os.path.join(os.path.dirname(rtc.__file__), "lib", "libembree3.so"), "rb") as f:
        text = f.read()
    assert b"inst_subdiv_bounds=: unknown value '" in text and text.count(b"' (swept or linear)") >= 1
    for ok in ("swept", "linear"):
        rtc.Device("gpu=none,inst_subdiv_bounds=" + ok).release()


@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_static_instances_keep_their_kind_and_every_byte_under_the_key(rtc, bomberman, accel):
    got = []
    for cfg in (stl.HOST, stl.HOST_KEY, stl.HOST + ",inst_subdiv_bounds=swept"):
        built = isd.build(rtc, accel, _meshes(bomberman), _instances(moving=False), cfg)
        got.append(_export(built[1]))
        isd.release(*built)
    assert got[0][0] == isd.KIND[accel]
    assert got[0] == got[1] == got[2]


@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_swept_and_the_key_absent_give_the_same_bytes_for_moving_instances(rtc, bomberman, accel):
    got = []
    for cfg in (stl.HOST, stl.HOST + ",inst_subdiv_bounds=swept", stl.HOST + ",inst_bounds=linear"):  # (the mesh key does not reach this accel)
        built = isd.build(rtc, accel, _meshes(bomberman), _instances(), cfg)
        got.append(_export(built[1]))
        isd.release(*built)
    assert got[0][0] == isd.KIND[accel]
    assert got[0] == got[1] == got[2]


@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_a_moving_instance_gives_the_new_kind(rtc, bomberman, accel):
    for more in ("", ",inst_bounds=linear", ",inst_bounds=swept"):  # independent of the mesh key
        built = isd.build(rtc, accel, _meshes(bomberman), _instances(), stl.HOST_KEY + more)
        st = built[1].stats()
        assert st["accelKind"] == stl.KIND[accel] == {isd.EAGER: 34, isd.LEAF: 35}[accel] == getattr(rtc, "ACCEL_INSTSUBDIV_TOP_LINEAR_" + ("GRID" if accel == isd.EAGER else "CBVH_LEAF"))
        assert st["leafCount"] == 5 and st["nodeBytes"] == 96
        isd.release(*built)


@pytest.mark.parametrize("cfg,text", [
    ("gpu=none", "static triangle meshes only (no quads, time steps, subdivision meshes or instances)"),
    ("gpu=none,subdiv_accel=default", "static triangle meshes only (no quads, time steps, subdivision meshes or instances)"),
    ("gpu=none,inst_accel=default", "static triangle and quad meshes only (no time steps, subdivision meshes or instances)"),
    ("gpu=none,quad_accel=default,inst_accel=default", "static triangle and quad meshes only (no time steps, subdivision meshes or instances)"),
    ("gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,inst_accel=default", "triangle and quad meshes only (no subdivision meshes or instances)"),
])
@pytest.mark.parametrize("moving", [False, True])
def test_host_only_configs_without_both_keys_raise_todays_texts_under_the_key(rtc, cfg, text, moving):
    """a host-only device honours the key only where it takes moving subdivision instances at all: the commit's message is the one of
    the same config without the key"""
    logs = []
    for c in (cfg, cfg + "," + stl.KEY):
        dev = rtc.Device(c)
        err = Errors(dev)
        sub = isd.add_inner(rtc, dev, isd.cube() + (3, 1))
        top = rtc.Scene(dev)
        if moving:
            top.add_instance_mb(sub, [ih.affine((0, 0, 0)), ih.affine((3, 0, 0))])
        else:
            top.add_instance(sub)
        top.lib.rtcCommitScene(top.handle)
        assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION and err.log
        logs.append(err.log[-1])
        top.release(); sub.release(); dev.release()
    assert logs[0] == logs[1]
    if not moving:
        assert text in logs[0][1]


# ---- 2. layout ----------------------------------------------------------------------------------------------------------------------------------------
def _same_tree(nodes, ref, inner_nodes, inner_ref, leaf_base, node_base):
    """the rebased tree below `ref` is the instanced scene's tree below `inner_ref`: same boxes, children moved by node_base, leaf
    references by leaf_base; returns the number of leaves"""
    if inner_ref == EMPTY:
        assert ref == EMPTY
        return 0
    if inner_ref & LEAF:
        assert ref == inner_ref + leaf_base and ref != ds.REF_INST_EXIT and (ref & 0x7FFFFFFF) < (1 << 26)
        return 1
    assert ref == inner_ref + node_base
    n, m = nodes[ref], inner_nodes[inner_ref]
    for f in ("origin", "exp", "pad", "q"):
        assert n[f].tobytes() == m[f].tobytes()
    return sum(_same_tree(nodes, int(c), inner_nodes, int(d), leaf_base, node_base) for c, d in zip(n["child"], m["child"]))


@pytest.mark.parametrize("accel", isd.FAMILIES)
@pytest.mark.parametrize("what", ["five instances", "one instance"])
def test_layout(rtc, bomberman, accel, what):
    meshes = _meshes(bomberman)
    inst = _instances() if what == "five instances" else _instances()[2:3]
    swept, lin = stl.build_pair(rtc, accel, meshes, inst, stl.HOST)
    top, top_s, inner = lin[1], swept[1], lin[2]
    st = top.stats()
    assert st["accelKind"] == stl.KIND[accel] and top_s.stats()["accelKind"] == isd.KIND[accel]
    assert st["leafCount"] == len(inst)
    # -- the node buffer: the instanced trees (QNode8) | zero padding | the top-level tree (QNodeMB8); blobOffsets: four words
    nodes8, image_mb, n_mb, first, (nblobs, first_blob) = stl.split_nodes(top, rtc)
    assert top.accel_data(0).tobytes() == top.accel_data(rtc.ACCEL_DATA_INSTSUBDIV).tobytes()  # the scene holds nothing else
    _, blobs_s, (nblobs_s, first_blob_s) = isd.decode(top_s, rtc)
    assert len(top_s.accel_data(rtc.ACCEL_DATA_INSTSUBDIV + 3).view(np.uint32)) == 2  # the kinds 24 / 25 keep their two words
    assert (nblobs, first_blob) == (nblobs_s, first_blob_s)
    blobs = top.accel_data(2)
    assert st["totalBytes"] == (first + n_mb) * 144 + len(blobs) + 16 and len(top.accel_data(1)) == 0
    # the top-level tree fills the second section from its first node on; accel_root() indexes 144-byte units
    image_mb, leaves = stl.top_leaves(top, rtc)
    assert sorted(r for _, r in leaves) == list(range(len(inst)))  # every instance is reached exactly once
    visited = {n for path, _ in leaves for n, _ in path}
    assert visited == set(range(first, first + n_mb)) and min(visited) == first
    if what == "one instance":
        assert n_mb == 1 and top.accel_root() == first and [len(p) for p, _ in leaves] == [1]  # a root node of one child
    top_depth = max(len(p) for p, _ in leaves)
    # -- blobs: steps and leaf blobs byte for byte the swept device's, the records apart from `root`
    n = len(inst)
    assert len(blobs) == len(blobs_s) and blobs[64 * n:].tobytes() == blobs_s[64 * n:].tobytes()
    recs, recs_s = stl.records(top, rtc, n), blobs_s[:64 * n].view(ih.INST_DT)
    by_gid_s = {int(r["geomID"]): r for r in recs_s}
    assert sorted(by_gid_s) == sorted(int(r["geomID"]) for r in recs)
    # the instanced trees lead the buffer: scene by scene in order of first use, rebased from index 0
    key_of = {g: k for g, k, _ in inst}
    first_use = list(dict.fromkeys(key_of[int(r["geomID"])] for r in recs))
    inner_nodes = {k: inner[k].accel_data(0).view(NODE_DT) for k in first_use}
    assert len(nodes8) == sum(len(x) for x in inner_nodes.values())
    stride = isd.blob_stride(accel, 2)
    node_base, leaf_base, roots, depth = 0, first_blob, {}, 0
    for k in first_use:
        roots[k] = (node_base, leaf_base)
        node_base += len(inner_nodes[k])
        leaf_base += len(inner[k].accel_data(2)) // stride
        depth = max(depth, inner[k].stats()["maxDepth"])
    top_nodes_s = len(top_s.accel_data(0).view(NODE_DT)) - len(nodes8)  # the swept build keeps its top-level tree in front
    assert top_nodes_s >= (0 if n == 1 else 1)
    for r in recs:
        g = int(r["geomID"])
        rs = by_gid_s[g]
        for f in ("world2local", "geomID", "pad"):
            assert r[f].tobytes() == rs[f].tobytes(), f  # (the leaf order of both trees is the record order of each: compared by geomID)
        k = key_of[g]
        nb, lb = roots[k]
        iroot = inner[k].accel_root()
        assert int(r["root"]) == (iroot + (lb if iroot & LEAF else nb)) and int(rs["root"]) == (iroot + (lb if iroot & LEAF else nb + top_nodes_s))
    for k in first_use:
        nb, lb = roots[k]
        iroot = inner[k].accel_root()
        assert _same_tree(nodes8, iroot + (lb if iroot & LEAF else nb), inner_nodes[k], iroot, lb, nb) == inner[k].stats()["leafCount"]
    # -- maxDepth = the top-level depth + 1 for the exit marker + the deepest instanced tree
    assert st["maxDepth"] == top_depth + 1 + depth
    for b in (swept, lin):
        isd.release(*b)


# ---- 3. containment --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
@pytest.mark.parametrize("what", itl.CASES)
def test_every_box_above_an_instance_holds_it_at_33_times(rtc, accel, what):
    """every root-to-leaf path of the top-level tree, at 33 times in [0, 1]: the box decoded with the kernel's fp32 formula holds the
    float64 images of the eight corners of the instanced scene's bounds (rtcGetSceneBounds: what the builder transforms) under
    lerp(step[k], step[k + 1], f)."""
    meshes = {"m": stl.big_cube()}
    inst = itl.instances(what)
    steps_of = {g: s for g, _, s in inst}
    dev, top, inner = isd.build(rtc, accel, meshes, inst, stl.HOST_KEY)
    assert top.stats()["accelKind"] == stl.KIND[accel]
    lo, hi = (np.asarray(x, np.float64) for x in inner["m"].bounds())
    clo, chi = isd.mesh_box(meshes["m"])
    assert (lo >= clo - 1e-3).all() and (hi <= chi + 1e-3).all() and (hi - lo > 4).all()  # a real box inside the cage's
    image_mb, leaves = stl.top_leaves(top, rtc)
    recs = stl.records(top, rtc, len(inst))
    assert sorted(r for _, r in leaves) == list(range(len(inst)))
    checks, bad = 0, []
    for path, rec in leaves:
        steps = steps_of[int(recs[rec]["geomID"])]
        for t in itl.TIMES33:
            p = itl.corners_at(lo, hi, steps, t)
            for blo, bhi in itl.path_boxes(image_mb, path, np.float32(t)):
                checks += 1
                if not ((blo <= p).all() and (p <= bhi).all()):
                    bad.append((rec, float(t), blo, bhi, p.min(0), p.max(0)))
    print(f"({what}) {accel}: {len(leaves)} instances, {checks} box checks, deepest path {max(len(p) for p, _ in leaves)}")
    assert not bad, bad[:3]
    assert checks >= 33 * len(inst)
    if what == "e":
        assert len(inst) == 40 and max(len(p) for p, _ in leaves) >= 2  # inner QNodeMB8s below the root
    # times outside [0, 1] and NaN clamp: the box of the nearer end, bit for bit
    for node in {n for path, _ in leaves for n, _ in path}:
        for t, end in ((-0.5, 0.0), (1.5, 1.0), (np.nan, 0.0)):
            a, b = decode_children_mb(image_mb[node], t), decode_children_mb(image_mb[node], end)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    isd.release(dev, top, inner)


# ---- 4. tightness -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_leaf_boxes_are_one_to_two_grid_steps_outside_the_step_boxes(rtc, accel):
    """the QNodeMB8 guarantee at t = 0 and t = 1 for the leaf box of a two-step translating instance (its exact step box: the float64
    images of the corners of the scene's bounds); the static instance beside it has equal boxes at both ends"""
    meshes = {"m": stl.big_cube()}
    inst = itl.instances("a")
    steps_of = {g: s for g, _, s in inst}
    dev, top, inner = isd.build(rtc, accel, meshes, inst, stl.HOST_KEY)
    lo, hi = (np.asarray(x, np.float64) for x in inner["m"].bounds())
    image_mb, leaves = stl.top_leaves(top, rtc)
    recs = stl.records(top, rtc, len(inst))
    two_step = static = 0
    for path, rec in leaves:
        steps = steps_of[int(recs[rec]["geomID"])]
        node, slot = path[-1]
        s = (image_mb[node]["exp"].astype(np.uint32) << 23).view(np.float32).astype(np.float64)
        b0, b1 = (decode_children_mb(image_mb[node], t) for t in (0.0, 1.0))
        if len(steps) == 1:
            static += 1
            assert b0[0][slot].tobytes() == b1[0][slot].tobytes() and b0[1][slot].tobytes() == b1[1][slot].tobytes()
        else:
            two_step += 1
            for t, (blo, bhi) in ((0.0, b0), (1.0, b1)):
                p = itl.corners_at(lo, hi, steps, t)
                dlo, dhi = (p.min(0) - blo[slot].astype(np.float64)) / s, (bhi[slot].astype(np.float64) - p.max(0)) / s
                assert (dlo >= 1.0).all() and (dlo < 2.0).all() and (dhi >= 1.0).all() and (dhi < 2.0).all(), (rec, t, dlo, dhi)
    assert two_step == 1 and static == 1
    isd.release(dev, top, inner)


# ---- 5. fewer entries -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_a_fast_mover_is_entered_by_a_quarter_of_the_rays_the_swept_box_lets_in_at_most(rtc, accel):
    """isd.cube() at (4, 2), instanced once, translating by D = 10 scene widths along x over a two-step shutter; 4096 rays along -z from
    above, x uniform over the swept footprint, y over the scene's width, times uniform in [0, 1].  Counted: the rays whose slab test at
    their time passes the mover's leaf box and every box above it under the key, against the swept tree (a single instance: a bare
    leaf, no box at all, every ray enters) and against the float64 truth (rays that meet the scene's bounds at their time).
    Geometry: 1 / 11, and the quantizer pads by at most two steps of 1 / 255 of the node extent per side."""
    meshes = {"m": isd.cube() + (4, 2)}
    built = isd.build(rtc, accel, meshes, [(0, "m", [ih.affine((0, 0, 0))])], stl.HOST)
    lo, hi = (np.asarray(x, np.float64) for x in built[2]["m"].bounds())
    isd.release(*built)
    W = float(np.float32(hi[0] - lo[0]))
    D = 10.0 * W
    inst = [(0, "m", [ih.affine((0, 0, 0)), ih.affine((D, 0, 0))])]
    m = 4096
    rng = np.random.RandomState(3)
    org = np.stack([lo[0] + rng.rand(m) * (D + W), lo[1] + rng.rand(m) * (hi[1] - lo[1]), np.full(m, 5.0)], 1).astype(np.float32).astype(np.float64)
    dirs = np.tile(np.array([0.0, 0.0, -1.0]), (m, 1))
    times = rng.rand(m).astype(np.float32)
    shift = np.float64(np.float32(D)) * times.astype(np.float64)
    truth = int(((org[:, 0] >= lo[0] + shift) & (org[:, 0] <= hi[0] + shift) & (org[:, 1] >= lo[1]) & (org[:, 1] <= hi[1])).sum())
    swept_b, lin_b = stl.build_pair(rtc, accel, meshes, inst, stl.HOST)
    top = lin_b[1]
    assert top.stats()["accelKind"] == stl.KIND[accel]
    image_mb, leaves = stl.top_leaves(top, rtc)
    (path, rec), = leaves
    assert len(path) == 1  # a root of one child: the mover's box is tested although the tree is one leaf
    ok = np.ones(m, bool)
    for t in np.unique(times):
        sel = times == t
        ok[sel] = itl.passes([(l[None], h[None]) for l, h in itl.path_boxes(image_mb, path, t)], org[sel], dirs[sel])
    linear = int(ok.sum())
    top_s = swept_b[1]
    assert top_s.stats()["accelKind"] == isd.KIND[accel]
    nodes_s, _, _ = isd.decode(top_s, rtc)
    boxes = []
    for p, first, count in walk_paths(nodes_s, top_s.accel_root()):  # (a single instance: the root is the leaf, no path)
        assert (first, count) == (0, 1)
        l8, h8, _ = ds.decode_nodes(nodes_s)
        boxes = [(l8[n][s][None], h8[n][s][None]) for n, s in p]
    swept = int(itl.passes(boxes, org, dirs).sum())
    for bb in (swept_b, lin_b):
        isd.release(*bb)
    print(f"{accel}: rays that enter the mover: swept {swept}, linear {linear}, truly meeting the scene's bounds at their time {truth} of {m} (ratio {linear / swept:.3f}, geometry {1 / 11:.3f})")
    assert truth <= linear
    assert linear <= 0.25 * swept


# ---- 6. stack bound -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_max_depth_covers_the_deepest_path_of_a_chain_of_nested_moving_instances(rtc, accel):
    """stl.chain_instances(): nested moving instances over the needle patches.  maxDepth is the formula - top-level depth + 1 (exit
    marker) + the needle tree's depth - and no ray of the host walk writes a slot beyond the capacity sized from it; a tenth of the
    sampled rays or more pass the 16 slots in LDS (the precondition of the GPU test of the overflow area)."""
    meshes, inst = stl.needle_meshes(), stl.chain_instances()
    dev, top, inner = isd.build(rtc, accel, meshes, inst, stl.HOST_KEY)
    st = top.stats()
    assert st["accelKind"] == stl.KIND[accel]
    _, leaves = stl.top_leaves(top, rtc)
    top_depth = max(len(p) for p, _ in leaves)
    own = inner["m"].stats()["maxDepth"]
    assert top_depth >= 2 and st["maxDepth"] == top_depth + 1 + own
    assert ds.stack_capacity(st["maxDepth"]) > ds.LDS_STACK
    m = 60
    rng = np.random.RandomState(11)
    org = ds.snap(0.25 + rng.rand(m, 3) * 0.5).astype(np.float64)
    dirs = rng.randn(m, 3)
    times = np.asarray(ds.TIMES, np.float32)[np.arange(m) % len(ds.TIMES)]
    deepest = stl.simulate_stack(top, rtc, len(inst), org, dirs, times)
    deep = int((deepest >= ds.LDS_STACK).sum())
    print(f"{accel}: maxDepth {st['maxDepth']} (top level {top_depth}, needles {own}), capacity {ds.stack_capacity(st['maxDepth'])}, deepest slot {int(deepest.max())}, {deep} of {m} rays pass slot {ds.LDS_STACK}")
    assert deepest.max() < ds.stack_capacity(st["maxDepth"])
    assert deep >= m // 10
    isd.release(dev, top, inner)


# ---- 7. refusals keep their texts under the key ---------------------------------------------------------------------------------------------------------------------
CFG = stl.HOST_KEY
MOVE = [ih.affine((0, 0, 0)), ih.affine((3, 0, 0))]


def _commit_fails(rtc, top, err, text):
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, text)


@pytest.mark.parametrize("mode", ["box", "grid", "full"])
def test_other_compressed_modes_below_a_moving_instance_stay_refused(rtc, mode):
    dev = rtc.Device(f"{CFG},subdiv_accel=bvh4.compressed.{mode}")
    err = Errors(dev)
    sub = isd.add_inner(rtc, dev, isd.cube() + (3, 1))
    top = rtc.Scene(dev)
    top.add_instance_mb(sub, MOVE)
    _commit_fails(rtc, top, err, f"subdiv_accel=bvh4.compressed.{mode} below an instance is not supported (the eager accel and bvh4.compressed.leaf are)")
    top.release(); sub.release(); dev.release()


def test_mixed_compression_levels_are_refused_and_named(rtc):
    dev = rtc.Device(CFG + ",subdiv_accel=bvh4.compressed.leaf")
    err = Errors(dev)
    a, b = isd.add_inner(rtc, dev, isd.cube() + (4, 2)), isd.add_inner(rtc, dev, isd.cube() + (4, 3))
    top = rtc.Scene(dev)
    top.add_instance_mb(a, MOVE, geom_id=3)
    top.add_instance(b, ih.affine((10, 0, 0)), geom_id=7)
    _commit_fails(rtc, top, err, "the scene of instance 7 has bvh4.compressed.leaf at compression level 3, the scene of instance 3 bvh4.compressed.leaf at compression level 2")
    top.release(); a.release(); b.release(); dev.release()


@pytest.mark.parametrize("what", ["triangles", "quads", "instance"])
def test_subdivision_beside_anything_else_in_an_instanced_scene_is_refused(rtc, what):
    dev = rtc.Device(CFG + ",quad_accel=default,subdiv_accel=default")
    err = Errors(dev)
    v, t = random_soup(8, 1)
    leaf = rtc.Scene(dev)
    leaf.add_triangles(v, t)
    leaf.commit()
    inner = rtc.Scene(dev)
    inner.add_subdiv(*SQUARE)
    inner.set_levels(2, 1)
    if what == "triangles":
        inner.add_triangles(v, t)
        text = "may hold nothing else: the scene of instance 4 also enables a triangle mesh"
    elif what == "quads":
        inner.add_quads(SQUARE[0], np.array([[0, 1, 2, 3]], np.uint32))
        text = "may hold nothing else: the scene of instance 4 also enables a quad mesh"
    else:
        inner.add_instance(leaf)
        text = "may hold nothing else: the scene of instance 4 also enables an instance (instances below instances are not supported)"
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance_mb(inner, MOVE, geom_id=4)
    _commit_fails(rtc, top, err, text)
    top.release(); inner.release(); leaf.release(); dev.release()


def test_an_instance_below_an_instance_keeps_its_message(rtc):
    dev = rtc.Device(CFG + ",subdiv_accel=default")
    err = Errors(dev)
    sub = isd.add_inner(rtc, dev, isd.cube() + (3, 1))
    mid = rtc.Scene(dev)
    mid.add_instance_mb(sub, MOVE)
    mid.commit()
    assert mid.stats()["accelKind"] == 34
    top = rtc.Scene(dev)
    top.add_instance(mid)
    _commit_fails(rtc, top, err, "static triangle and quad meshes only (no time steps, subdivision meshes or instances)")
    top.release(); mid.release(); sub.release(); dev.release()


def test_a_filter_function_on_instanced_subdivision_geometry_is_refused(rtc):
    dev = rtc.Device(CFG + ",subdiv_accel=default")
    err = Errors(dev)
    inner = rtc.Scene(dev)
    gid = inner.add_subdiv(*SQUARE)
    inner.set_levels(2, 1)
    fn = rtc.FILTER_FUNC(lambda args: None)
    g = dev.lib.rtcGetGeometry(inner.handle, gid)
    dev.lib.rtcSetGeometryIntersectFilterFunction(g, C.cast(fn, C.c_void_p))
    dev.lib.rtcCommitGeometry(g)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance_mb(inner, MOVE, geom_id=1)
    _commit_fails(rtc, top, err, "subdivision geometry with a filter function inside an instanced scene is not supported (instance 1)")
    top.release(); inner.release(); dev.release()


def test_context_filter_and_counted_batches_are_refused_on_such_a_scene(rtc):
    dev, top, inner = isd.build(rtc, isd.EAGER, {"c": isd.cube() + (3, 1)}, [(0, "c", MOVE)], CFG)
    assert top.stats()["accelKind"] == 34
    err = Errors(dev)
    rh = rtc.aligned_rayhits(4)
    ctx = rtc.make_context()
    fn = rtc.FILTER_FUNC(lambda args: None)
    ctx.filter = C.cast(fn, C.c_void_p)
    top.intersect1M(rh, ctx=ctx, check=False)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "filter is not supported on a scene with instances")
    with pytest.raises(rtc.RTCError):
        top.intersect1M_counted(rh)
    assert "counted batches are not supported on a scene with instances" in err.log[-1][1]
    isd.release(dev, top, inner)
