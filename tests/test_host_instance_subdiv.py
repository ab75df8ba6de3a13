"""Instances of scenes that hold subdivision meshes, on the CPU: what rtcCommitScene builds on a host-only device whose config names
inst_accel= and subdiv_accel= (csrc/rt_instance_build.cpp build_instance_subdiv_accel; the layout is described at csrc/accel.h InstanceRecord),
what it refuses, and that every other host-only config keeps the messages it always raised."""
import ctypes as C

import numpy as np
import pytest

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mb_helpers as im
import instance_subdiv_helpers as isd
from helpers import random_soup
from instance_helpers import EMPTY, INST_DT, LEAF

ERRFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)
CFG = "gpu=none,inst_accel=default"
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
    """two instanced scenes: the first 32 faces of bomberman at (L, Cl) and the cube one tessellation level higher (L may differ)"""
    return {"m": isd.bomberman_faces(bomberman) + (L, Cl), "c": isd.cube() + (L + 1, Cl)}


def _instances():
    """five instances: three of "m" (one of them moving, three steps), two of "c" - both scenes are shared"""
    inst = isd.lattice_instances(5, keys=("m", "c"))
    g, k, steps = inst[2]
    inst[2] = (g, k, [steps[0], ih.affine((85.0, 3.0, 1.0), (0.5,) * 3), ih.affine((90.0, -2.0, 4.0), (0.5,) * 3)])
    return inst


def _top_leaves(nodes, root):
    """record indices of the top-level tree in leaf order, and its depth"""
    if root & LEAF:
        return [root & 0x3FFFFFF], 0
    out, depth = [], 0
    for c in nodes[root]["child"]:
        c = int(c)
        if c == EMPTY:
            continue
        assert not (c & LEAF) or (c >> 26) & 31 == 1  # one instance per leaf
        sub, d = _top_leaves(nodes, c)
        out += sub
        depth = max(depth, d)
    return out, depth + 1


def _same_tree(nodes, ref, inner_nodes, inner_ref, blobs, inner_blobs, stride, leaf_base, node_base):
    """the rebased tree below `ref` is the instanced scene's tree below `inner_ref`: same boxes, children moved by node_base, leaf
    references moved by leaf_base, and every leaf resolves to the bytes of the same blob; returns the number of leaves"""
    if inner_ref == EMPTY:
        assert ref == EMPTY
        return 0
    if inner_ref & LEAF:
        assert ref == inner_ref + leaf_base and ref & LEAF and ref != ds.REF_INST_EXIT
        a, b = (ref & 0x7FFFFFFF) * stride, (inner_ref & 0x7FFFFFFF) * stride
        assert (ref & 0x7FFFFFFF) < (1 << 26)
        assert blobs[a:a + stride].tobytes() == inner_blobs[b:b + stride].tobytes()
        return 1
    assert ref == inner_ref + node_base
    n, m = nodes[ref], inner_nodes[inner_ref]
    for f in ("origin", "exp", "q"):
        assert n[f].tobytes() == m[f].tobytes()
    return sum(_same_tree(nodes, int(c), inner_nodes, int(d), blobs, inner_blobs, stride, leaf_base, node_base) for c, d in zip(n["child"], m["child"]))


@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_kind_records_nodes_and_blobs(rtc, bomberman, accel):
    meshes, inst = _meshes(bomberman), _instances()
    dev, top, inner = isd.build(rtc, accel, meshes, inst, CFG)
    st = top.stats()
    assert st["accelKind"] == isd.KIND[accel] and st["leafCount"] == len(inst)
    assert all(s.stats()["accelKind"] == isd.INNER_KIND[accel] for s in inner.values())
    stride = isd.blob_stride(accel, 2)
    assert st["primBytes"] == stride == inner["m"].stats()["primBytes"]
    nodes, blobs, (nblobs, first) = isd.decode(top, rtc)
    assert top.accel_data(0).tobytes() == nodes.tobytes() and top.accel_data(2).tobytes() == blobs.tobytes()  # the scene holds nothing else
    assert len(top.accel_data(1)) == 0
    # blobs: the InstanceRecords, the InstanceSteps of the moving instance, zero padding, then the blob section from a multiple of the stride on
    nsteps = sum(len(s) for _, _, s in inst if len(s) > 1)
    assert first == -(-(len(inst) + nsteps) * 64 // stride) and len(blobs) == (first + nblobs) * stride
    assert not blobs[(len(inst) + nsteps) * 64: first * stride].any()
    recs = blobs[: len(inst) * 64].view(INST_DT)
    steps = blobs[len(inst) * 64: (len(inst) + nsteps) * 64].view(im.STEP_DT)
    order, top_depth = _top_leaves(nodes, top.accel_root())
    assert order == list(range(len(inst)))  # leaf order = record order
    assert sorted(int(g) for g in recs["geomID"]) == [g for g, _, _ in inst]
    # one copy of every distinct scene's blobs, in the order of first use
    by_gid = {g: (k, s) for g, k, s in inst}
    first_use = []
    for g in recs["geomID"]:
        k = by_gid[int(g)][0]
        if k not in first_use:
            first_use.append(k)
    inner_blobs = {k: inner[k].accel_data(2) for k in inner}
    assert nblobs * stride == sum(len(b) for b in inner_blobs.values())
    assert blobs[first * stride:].tobytes() == b"".join(inner_blobs[k].tobytes() for k in first_use)
    leaf_base, at = {}, first
    for k in first_use:
        leaf_base[k] = at
        at += len(inner_blobs[k]) // stride
    # every record: transform, root, steps; the rebased tree is the scene's own
    inner_nodes = {k: inner[k].accel_data(0).view(ih.NODE_DT) for k in inner}
    roots, depth = {}, 0
    for r in recs:
        key, st_ = by_gid[int(r["geomID"])]
        assert np.array_equal(r["world2local"], ih.world2local(st_[0]).T.reshape(-1))  # columns vx, vy, vz, p
        assert r["pad"][0] == 0
        if len(st_) > 1:
            s, f = int(r["pad"][1]) >> 24, int(r["pad"][1]) & 0xFFFFFF
            assert s == len(st_) - 1 and len(inst) <= f and f + len(st_) <= len(inst) + nsteps
            got = steps[f - len(inst): f - len(inst) + len(st_)]
            assert got["local2world"].tobytes() == b"".join(np.asarray(m, np.float32).T.reshape(-1).tobytes() for m in st_) and not got["pad"].any()
        else:
            assert r["pad"][1] == 0
        roots.setdefault(key, int(r["root"]))
        assert roots[key] == int(r["root"])  # instances of one scene share its tree
    node_base = len(nodes) - sum(len(n) for n in inner_nodes.values())
    for k in first_use:
        iroot = inner[k].accel_root()
        n = _same_tree(nodes, roots[k], inner_nodes[k], iroot, blobs, inner_blobs[k], stride, leaf_base[k], node_base)
        assert n == len(inner_blobs[k]) // stride == inner[k].stats()["leafCount"]
        depth = max(depth, isd.depth_of(inner_nodes[k], iroot))
        assert isd.depth_of(inner_nodes[k], iroot) == inner[k].stats()["maxDepth"]
        node_base += len(inner_nodes[k])
    # maxDepth = the top-level depth + 1 for the exit marker + the deepest instanced tree
    assert st["maxDepth"] == top_depth + 1 + depth
    isd.release(dev, top, inner)


@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_world_boxes(rtc, bomberman, accel):
    """the top-level node boxes hold the union over the time steps of xfmBounds(local2world, scene bounds), and no more than the
    quantization of a node allows (two steps of its 8-bit grid)"""
    meshes, inst = _meshes(bomberman), _instances()
    dev, top, inner = isd.build(rtc, accel, meshes, inst, CFG)
    nodes, blobs, _ = isd.decode(top, rtc)
    recs = blobs[: len(inst) * 64].view(INST_DT)
    lo, hi, child = ds.decode_nodes(nodes)
    by_gid = {g: (k, s) for g, k, s in inst}
    seen = 0

    def walk(n):
        nonlocal seen
        scale = (nodes[n]["exp"].astype(np.uint32) << 23).view(np.float32).astype(np.float64)
        for k, c in enumerate(child[n]):
            if c == EMPTY:
                continue
            if not c & LEAF:
                walk(c)
                continue
            key, steps = by_gid[int(recs[c & 0x3FFFFFF]["geomID"])]
            blo, bhi = (np.asarray(b, np.float64) for b in inner[key].bounds())
            corners = np.array([[(blo, bhi)[(j >> a) & 1][a] for a in range(3)] for j in range(8)])
            w = np.concatenate([ih.xfm_points(m, corners) for m in steps])
            eps = 1e-5 * np.abs(w).max()
            assert (lo[n][k] <= w.min(0) + eps).all() and (hi[n][k] >= w.max(0) - eps).all()
            assert (lo[n][k] >= w.min(0) - 2 * scale - eps).all() and (hi[n][k] <= w.max(0) + 2 * scale + eps).all()
            seen += 1

    root = top.accel_root()
    assert not root & LEAF
    walk(root)
    assert seen == len(inst)
    tlo, thi = top.bounds()
    assert (tlo <= lo[root].min(0) + 1.0).all() and (thi >= hi[root].max(0) - 1.0).all()
    isd.release(dev, top, inner)


@pytest.mark.parametrize("C_", [1, 2, 3, 4, 5])
def test_every_compression_level_is_placed(rtc, C_):
    meshes = {"c": isd.cube() + (5, C_)}
    dev, top, inner = isd.build(rtc, isd.LEAF, meshes, isd.lattice_instances(2, keys=("c",)), CFG)
    stride = isd.cbvh_stride(C_)
    _, blobs, (nblobs, first) = isd.decode(top, rtc)
    assert top.stats()["accelKind"] == isd.ACCEL_INSTSUBDIV_CBVH_LEAF and top.stats()["primBytes"] == stride
    assert nblobs == 6 * 4 ** (5 - C_) and first == -(-2 * 64 // stride)
    assert blobs[first * stride:].tobytes() == inner["c"].accel_data(2).tobytes()
    isd.release(dev, top, inner)


def test_a_top_scene_holds_both_classes_beside_geometry_of_its_own(rtc):
    """mesh instances stay in the first instance accel, byte for byte what it is without the subdivision instance"""
    v, t = random_soup(64, 3)

    def make(with_subdiv):
        dev = rtc.Device(CFG + ",quad_accel=default,subdiv_accel=default")
        tri = rtc.Scene(dev)
        tri.add_triangles(v, t)
        tri.commit()
        sub = isd.add_inner(rtc, dev, isd.cube() + (3, 1))
        top = rtc.Scene(dev)
        top.add_triangles(v + 100, t)
        top.add_instance(tri, ih.affine((5, 0, 0)))
        if with_subdiv:
            top.add_instance(sub, ih.affine((0, 50, 0), (2, 2, 2)))
        top.commit()
        return dev, top, [tri, sub]

    dev, top, keep = make(True)
    dev0, top0, keep0 = make(False)
    sel = rtc.ACCEL_DATA_INSTSUBDIV
    assert len(top0.accel_data(sel + 0)) == 0 and len(top0.accel_data(sel + 2)) == 0
    assert len(top.accel_data(sel + 0)) == len(keep[1].accel_data(0)) and len(top.accel_data(sel + 2)) == 160 + len(keep[1].accel_data(2))
    rec = top.accel_data(sel + 2)[:64].view(INST_DT)[0]
    assert rec["geomID"] == 2 and rec["root"] == keep[1].accel_root()  # a single instance: no top-level node, the tree starts at node 0
    for kind in (0, 1, 2, 3):  # stats() / accel_data() describe the triangle accel, as without the subdivision instance
        assert top.accel_data(kind).tobytes() == top0.accel_data(kind).tobytes()
    a, b = top.stats(), top0.stats()
    assert {k: a[k] for k in a if k != "totalBytes"} == {k: b[k] for k in b if k != "totalBytes"} and a["totalBytes"] > b["totalBytes"]
    for d, tp, ks in ((dev, top, keep), (dev0, top0, keep0)):
        tp.release()
        for s in ks:
            s.release()
        d.release()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _commit_fails(rtc, top, err, text):
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, text)


@pytest.mark.parametrize("mode", ["box", "grid", "full"])
def test_other_compressed_modes_below_an_instance_stay_refused(rtc, mode):
    dev = rtc.Device(f"{CFG},subdiv_accel=bvh4.compressed.{mode}")
    err = Errors(dev)
    sub = isd.add_inner(rtc, dev, isd.cube() + (3, 1))
    top = rtc.Scene(dev)
    top.add_instance(sub)
    _commit_fails(rtc, top, err, f"subdiv_accel=bvh4.compressed.{mode} below an instance is not supported")
    top.release(); sub.release(); dev.release()


def test_mixed_compression_levels_are_refused_and_named(rtc):
    dev = rtc.Device(CFG + ",subdiv_accel=bvh4.compressed.leaf")
    err = Errors(dev)
    a, b = isd.add_inner(rtc, dev, isd.cube() + (4, 2)), isd.add_inner(rtc, dev, isd.cube() + (4, 3))
    top = rtc.Scene(dev)
    top.add_instance(a, geom_id=3)
    top.add_instance(b, ih.affine((10, 0, 0)), geom_id=7)
    _commit_fails(rtc, top, err, "the scene of instance 7 has bvh4.compressed.leaf at compression level 3, the scene of instance 3 bvh4.compressed.leaf at compression level 2")
    top.release(); a.release(); b.release(); dev.release()
    # the tessellation level may differ, and the eager accel has no compression level to disagree in
    for accel, la, lb in ((isd.LEAF, (3, 2), (5, 2)), (isd.EAGER, (3, 1), (4, 3))):
        dev = rtc.Device(f"{CFG},subdiv_accel={accel}")
        a, b = isd.add_inner(rtc, dev, isd.cube() + la), isd.add_inner(rtc, dev, isd.cube() + lb)
        top = rtc.Scene(dev)
        top.add_instance(a)
        top.add_instance(b, ih.affine((10, 0, 0)))
        top.commit()
        assert top.stats()["accelKind"] == isd.KIND[accel]
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
    top.add_instance(inner, geom_id=4)
    _commit_fails(rtc, top, err, text)
    top.release(); inner.release(); leaf.release(); dev.release()


def test_an_instance_below_an_instance_keeps_its_message(rtc):
    dev = rtc.Device(CFG + ",subdiv_accel=default")
    err = Errors(dev)
    sub = isd.add_inner(rtc, dev, isd.cube() + (3, 1))
    mid = rtc.Scene(dev)
    mid.add_instance(sub)
    mid.commit()
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
    top.add_instance(inner, geom_id=1)
    _commit_fails(rtc, top, err, "subdivision geometry with a filter function inside an instanced scene is not supported")
    top.release(); inner.release(); dev.release()


@pytest.mark.parametrize("cfg,text", [
    ("gpu=none", "static triangle meshes only (no quads, time steps, subdivision meshes or instances)"),
    ("gpu=none,subdiv_accel=default", "static triangle meshes only (no quads, time steps, subdivision meshes or instances)"),
    ("gpu=none,inst_accel=default", "static triangle and quad meshes only (no time steps, subdivision meshes or instances)"),
    ("gpu=none,quad_accel=default,inst_accel=default", "static triangle and quad meshes only (no time steps, subdivision meshes or instances)"),
    ("gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,inst_accel=default", "triangle and quad meshes only (no subdivision meshes or instances)"),
])
def test_host_only_configs_without_both_keys_raise_todays_texts(rtc, cfg, text):
    dev = rtc.Device(cfg)
    err = Errors(dev)
    sub = isd.add_inner(rtc, dev, isd.cube() + (3, 1))
    top = rtc.Scene(dev)
    top.add_instance(sub)
    _commit_fails(rtc, top, err, text)
    top.release(); sub.release(); dev.release()


def test_context_filter_and_counted_batches_are_refused_on_such_a_scene(rtc):
    """hasInstances() is true for either instance accel; the refusals come before anything would touch a GPU"""
    dev, top, inner = isd.build(rtc, isd.EAGER, {"c": isd.cube() + (3, 1)}, isd.lattice_instances(1, keys=("c",)), CFG)
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
