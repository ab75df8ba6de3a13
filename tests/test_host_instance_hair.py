"""Line segments and flat curves below an instance (device config inst_hair=1), on a host-only device: the key, the kinds, the layout of
the accel (csrc/accel.h InstanceSceneRecord: six roots; CurveRecord and LineRecord sections behind the QuadMBRecords), the refusals, and
that a top scene without hair below it builds the bytes it built without the key.  tests/instance_hair_helpers.py."""
import ctypes as C
import os

import numpy as np
import pytest

import curve_helpers as ch
import instance_hair_helpers as ihh
import instance_helpers as ih
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
import line_helpers as lh
from instance_helpers import EMPTY, NODE_DT

CFG = ihh.HOST_CFG
IDENT = [ih.affine()]


def _log(dev):
    log = []
    fn = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda u, c, msg: log.append((c, msg.decode())))
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(fn, C.c_void_p), None)
    return log, fn


def _refused(rtc, mode, scs, inst, cfg, text, extra=None, gid=None):
    dev, top, inner = ihh.build(rtc, mode, scs, inst, cfg, extra=extra, commit=False)
    log, keep = _log(dev)
    with pytest.raises(rtc.RTCError) as e:
        top.commit()
    assert e.value.code == rtc.RTC_ERROR_INVALID_OPERATION
    assert log and log[-1][0] == rtc.RTC_ERROR_INVALID_OPERATION and text in log[-1][1], log
    if gid is not None:
        assert "instance %d" % gid in log[-1][1], log
    ihh.release(dev, top, inner)
    return log[-1][1]


def _decode(top, rtc, n_inst, n_scenes, counts):
    """(nodes, sections of ihh.split_blobs) of a committed top scene; counts = (quads, steps, triMB, quadMB, curves, lines)"""
    nodes = top.accel_data(0).view(NODE_DT)
    blobs = top.accel_data(2)
    return nodes, ihh.split_blobs(blobs, n_inst, counts[0], counts[1], n_scenes, *counts[2:])


def _own(rtc, d, mode, cfg=CFG):
    """the curve and line records, roots and depths of the scene `d` as a scene of its own exports them"""
    dev = rtc.Device(cfg)
    out = {}
    for part, dt in (("curves", ch.CURVE_DT), ("lines", lh.LINE_DT)):
        if d.get(part) is None:
            out[part] = None
            continue
        sc = ihh.add_scene(rtc, dev, ihh.desc(**{part: d[part]}), mode)
        out[part] = (sc.accel_data(0).view(NODE_DT).copy(), sc.accel_data(2).view(dt).copy(), sc.accel_root(), sc.stats()["maxDepth"], sc.stats()["accelKind"])
        sc.release()
    dev.release()
    return out


# ---- 1. the key -------------------------------------------------------------------------------------------------------------------------
def test_inst_hair_values_and_the_bad_value_message(rtc):
    for ok in ("0", "1"):
        rtc.Device("gpu=none,inst_hair=" + ok).release()
    with pytest.raises(rtc.RTCError) as e:
        rtc.Device("gpu=none,inst_hair=2")
    assert e.value.code == rtc.RTC_ERROR_INVALID_ARGUMENT
    # (the message of a failed rtcNewDevice is not handed out by the API: its wording is looked up in the library)
    with open(os.path.join(os.path.dirname(rtc.__file__), "lib", "libembree3.so"), "rb") as f:
        text = f.read()
    assert b"inst_hair=: unknown value '" in text


@pytest.mark.parametrize("cfg", [CFG.replace(",inst_hair=1", ""), CFG.replace("inst_hair=1", "inst_hair=0"),
                                 "gpu=none,hair_accel=default,quad_accel=default,inst_hair=1"])  # no key, key off, key without inst_accel=
def test_without_the_key_the_two_old_refusals_word_for_word(rtc, cfg):
    msg = _refused(rtc, 1, {"m": ihh.desc(curves=ihh.curve_geometries(n=4)[:1])}, [(0, "m", IDENT)], cfg, ihh.OLD_CURVES)
    assert msg.endswith(ihh.OLD_CURVES)
    only = ihh.OLD_ONLY if "inst_accel" in cfg and "tri_accel_mb" in cfg else None
    msg = _refused(rtc, 1, {"m": ihh.desc(lines=ihh.strands(2, 3) + (0,))}, [(0, "m", IDENT)], cfg, only or "an instanced scene may hold")
    assert only is None or msg.endswith(only)


def test_a_host_only_device_takes_curves_only_with_hair_accel_named(rtc):
    cfg = "gpu=none,inst_accel=default,inst_hair=1"
    dev, top, inner = ihh.build(rtc, 1, {"m": ihh.desc(lines=ihh.strands(2, 3) + (0,))}, [(0, "m", IDENT)], cfg)
    assert top.stats()["accelKind"] == 23
    ihh.release(dev, top, inner)
    # (without hair_accel= such a device refuses the curve types when the geometry is created: nothing to instance)
    dev = rtc.Device(cfg)
    sc = rtc.Scene(dev)
    with pytest.raises(rtc.RTCError):
        sc.add_curves(*ihh.tuft(2), basis="bezier")
    sc.release()
    dev.release()


# ---- 2. kinds and layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["a", "b", "c", "d", "e"])
def test_kind_roots_records_and_sections(rtc, mode, which):
    scs = ihh.scenes(which)
    d = scs["m"]
    # three instances share the scene, one of them moving: the scene is stored once
    moving = [ih.affine((1, 2, 3)), ih.affine((1.5, 2, 3))]
    inst = [(0, "m", IDENT), (1, "m", moving), (2, "m", [ih.affine((40, 0, 0), (2, 2, 2))])]
    dev, top, inner = ihh.build(rtc, mode, scs, inst, CFG)
    st = top.stats()
    assert st["accelKind"] == imm.kind(mode)  # 22 / 23, whatever moves
    own = _own(rtc, d, mode)
    n_curves = len(own["curves"][1]) if own["curves"] else 0
    n_lines = len(own["lines"][1]) if own["lines"] else 0
    mesh = imm.own_accels(rtc, CFG, d, mode)
    n_quads = len(mesh["quads"][1]) if mesh["quads"] else 0
    n_trimb = len(mesh["tris_mb"][1]) if mesh["tris_mb"] else 0
    nodes, (recs, quads, steps, scenes, trimb, quadmb, curves, lines, c_off, l_off) = _decode(top, rtc, 3, 1, (n_quads, 2, n_trimb, 0, n_curves, n_lines))
    assert c_off % 80 == 0 and l_off % 48 == 0
    assert len(scenes) == 1 and not scenes["pad"].any()
    scene_base = 3 + n_quads + 2
    assert (recs["root"] == scene_base).all() and sorted(recs["geomID"].tolist()) == [0, 1, 2]
    sc = scenes[0]
    have = {"triRoot": d["tris"], "triMBRoot": d["tris_mb"], "quadRoot": d["quads"], "quadMBRoot": d["quads_mb"], "curveRoot": d["curves"], "lineRoot": d["lines"]}
    for name, _ in ihh.VISIT:
        assert (int(sc[name]) == EMPTY) == (have[name] is None), name
    # the trees follow each other in the node array in visiting order: triangles, MB triangles, quads, MB quads, curves, lines
    first_nodes = [int(sc[n]) for n, _ in ihh.VISIT if int(sc[n]) != EMPTY and not int(sc[n]) & ih.LEAF]
    assert first_nodes == sorted(first_nodes)
    # walking from curveRoot / lineRoot reaches every record exactly once, and the records are the scene's own, byte for byte
    deepest = 0
    for part, root, got, off, size in (("curves", int(sc["curveRoot"]), curves, c_off, 80), ("lines", int(sc["lineRoot"]), lines, l_off, 48)):
        if own[part] is None:
            assert len(got) == 0
            continue
        o_nodes, o_recs, o_root, o_depth, o_kind = own[part]
        assert got.tobytes() == o_recs.tobytes(), part
        idx, leaves, depth = ihh.leaf_records(nodes, root)
        base = off // size
        assert sorted(idx) == list(range(base, base + len(o_recs))), part
        assert max(idx) < 1 << 26
        o_idx, o_leaves, o_d = ihh.leaf_records(o_nodes, o_root)
        assert [(f + base, c) for f, c in o_leaves] == leaves and depth == o_d  # the scene's own tree, rebased
        assert kind_robust(rtc, o_kind) == (mode == 0)
        deepest = max(deepest, o_depth)
    # maxDepth = top-level depth + 1 (exit marker) + pending-tree markers (trees - 1) + the deepest instanced tree
    trees = sum(v is not None for v in have.values())
    for p in ("tris", "tris_mb", "quads", "quads_mb"):
        if mesh[p]:
            deepest = max(deepest, mesh[p][3])
    top_depth = _top_depth(nodes, top.accel_root())
    assert st["maxDepth"] == top_depth + 1 + (trees - 1) + deepest, (st["maxDepth"], top_depth, trees, deepest)
    ihh.release(dev, top, inner)


def kind_robust(rtc, kind):
    return bool(rtc.accel_kind_row(kind)["robust"])


def _top_depth(nodes, root):
    """levels of inner nodes of the top-level tree: its leaves are instance records (count 1, index below the number of instances)"""
    def depth(ref):
        if ref == EMPTY or ref & ih.LEAF:
            return 0
        return 1 + max(depth(int(c)) for c in nodes[ref]["child"])
    return depth(int(root))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["a", "b", "c", "d", "e"])
def test_leaves_span_several_blocks_of_four(rtc, which, mode):
    """the condition of the short-ray leg of tests/test_gpu_instance_hair.py on every one of its scenes: below the instance, some leaf of
    every hair tree the scene has holds more than four records, so that the block loops of the two leaves run more than once"""
    dev, top, inner = ihh.build(rtc, mode, ihh.scenes(which), [(0, "m", IDENT)], CFG)
    nodes = top.accel_data(0).view(NODE_DT)
    sc = top.accel_data(2)[64:128].view(ihh.SCENE_DT)[0]  # one instance, no quads in front of the scene record unless the scene has some
    d = ihh.scenes(which)["m"]
    if d["quads"] is not None:
        sc = top.accel_data(2)[64 * (1 + len(d["quads"][1])):][:64].view(ihh.SCENE_DT)[0]
    for name, have in (("curveRoot", d["curves"]), ("lineRoot", d["lines"])):
        if have is None:
            assert int(sc[name]) == EMPTY
            continue
        leaves, _ = imm.walk(nodes, int(sc[name]))
        assert max(c for _, c in leaves) > 4, (which, name, leaves)
    ihh.release(dev, top, inner)


def test_six_trees_bound_the_depth(rtc):
    """all six trees in one scene: five markers wait above the exit marker"""
    t, q = ihh.coincident_meshes()
    d = ihh.desc(tris=t, quads=q, tris_mb=ihh.moving_triangles(gid=3), quads_mb=None, curves=ihh.curve_geometries(first_gid=5, n=8)[:2], lines=ihh.strands() + (9,))
    qv = [np.asarray(q[0], np.float32), (np.asarray(q[0]) + np.float32(0.5)).astype(np.float32)]
    d["quads_mb"] = (qv, q[1], 4)
    dev, top, inner = ihh.build(rtc, 1, {"m": d}, [(0, "m", IDENT)], CFG + ",quad_accel_mb=default")
    st = top.stats()
    assert st["accelKind"] == 23
    nodes = top.accel_data(0).view(NODE_DT)
    words = top.accel_data(2).view(np.uint32)
    rec = top.accel_data(2)[:64].view(ih.INST_DT)[0]
    roots = [int(x) for x in words[int(rec["root"]) * 16: int(rec["root"]) * 16 + 6]]
    assert all(r != EMPTY for r in roots)
    deepest = max(ihh.leaf_records(nodes, r)[2] for r in roots)
    assert st["maxDepth"] == _top_depth(nodes, top.accel_root()) + 1 + 5 + deepest
    ihh.release(dev, top, inner)


def test_two_scenes_fill_the_sections_in_order_of_first_use(rtc):
    scs = {"a": ihh.scenes("a")["m"], "c": ihh.scenes("c")["m"]}
    inst = [(0, "c", IDENT), (1, "a", [ih.affine((30, 0, 0))]), (2, "c", [ih.affine((0, 30, 0))])]
    dev, top, inner = ihh.build(rtc, 1, scs, inst, CFG)
    oa, oc = _own(rtc, scs["a"], 1), _own(rtc, scs["c"], 1)
    n_c, n_l = len(oc["curves"][1]), len(oc["lines"][1]) + len(oa["lines"][1])
    nodes, (recs, quads, steps, scenes, trimb, quadmb, curves, lines, c_off, l_off) = _decode(top, rtc, 3, 2, (0, 0, 0, 0, n_c, n_l))
    assert curves.tobytes() == oc["curves"][1].tobytes()
    assert lines.tobytes() == oc["lines"][1].tobytes() + oa["lines"][1].tobytes()  # "c" is used first
    assert int(scenes[1]["curveRoot"]) == EMPTY and int(scenes[0]["curveRoot"]) != EMPTY
    base = l_off // 48
    assert sorted(ihh.leaf_records(nodes, int(scenes[0]["lineRoot"]))[0]) == list(range(base, base + len(oc["lines"][1])))
    assert sorted(ihh.leaf_records(nodes, int(scenes[1]["lineRoot"]))[0]) == list(range(base + len(oc["lines"][1]), base + n_l))
    ihh.release(dev, top, inner)


def test_a_disabled_hair_geometry_does_not_count(rtc):
    dev = rtc.Device(CFG)
    sc = rtc.Scene(dev)
    t, _ = ihh.coincident_meshes()
    sc.add_triangles(t[0], t[1], geom_id=0)
    v, idx = ihh.strands(2, 3)
    sc.add_lines(v, idx, geom_id=1)
    sc.set_enabled(1, False)
    sc.commit()
    top = rtc.Scene(dev)
    top.add_instance(sc, ih.affine(), geom_id=0)
    top.commit()
    assert top.stats()["accelKind"] == 15  # ACCEL_INST_TRI_MOELLER: the triangle-only accel, as without the line geometry
    sc.set_enabled(1, True)  # ... and enabled again it counts: the general layout with a line tree
    sc.commit()
    top.commit()
    assert top.stats()["accelKind"] == 23
    scenes = top.accel_data(2)[64:128].view(ihh.SCENE_DT)
    assert int(scenes[0]["lineRoot"]) != EMPTY and int(scenes[0]["curveRoot"]) == EMPTY and int(scenes[0]["triRoot"]) != EMPTY
    top.release()
    sc.release()
    dev.release()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
def test_moving_hair_below_an_instance_is_refused(rtc):
    v, idx = ihh.strands(2, 3)
    cfg = CFG + ",line_accel_mb=default,hair_accel_mb=default"

    def build_and_refuse(add):
        dev = rtc.Device(cfg)
        log, keep = _log(dev)
        sc = rtc.Scene(dev)
        add(sc)
        sc.commit()
        top = rtc.Scene(dev)
        top.add_instance(sc, ih.affine(), geom_id=5)
        with pytest.raises(rtc.RTCError) as e:
            top.commit()
        assert e.value.code == rtc.RTC_ERROR_INVALID_OPERATION and ihh.REFUSE_MOTION in log[-1][1] and "instance 5" in log[-1][1], log
        top.release()
        sc.release()
        dev.release()
    build_and_refuse(lambda sc: sc.add_lines_mb([v, v + np.float32(0.25)], idx))
    cv, cidx = ihh.tuft(4)
    build_and_refuse(lambda sc: sc.add_curves_mb([cv, cv + np.float32(0.25)], cidx, basis="bspline"))


def test_hair_beside_the_linear_kinds_is_refused(rtc):
    scs = {"m": ihh.scenes("a")["m"]}
    moving = [ih.affine((1, 2, 3)), ih.affine((1.5, 2, 3))]
    _refused(rtc, 1, scs, [(0, "m", IDENT), (4, "m", moving)], CFG + ",inst_bounds=linear", ihh.REFUSE_LINEAR, gid=0)
    scs = {"m": ihh.scenes("e")["m"]}
    _refused(rtc, 1, scs, [(3, "m", IDENT)], CFG + ",mb_bounds=linear,inst_mb_bounds=linear", ihh.REFUSE_LINEAR, gid=3)


def test_geometry_filters_beside_instanced_hair_are_refused(rtc):
    t, _ = ihh.coincident_meshes()
    fn = rtc.FILTER_FUNC(lambda args: None)

    def filtered(dev):
        sc = rtc.Scene(dev)
        sc.add_triangles(t[0], t[1], geom_id=0)
        sc.set_filters(0, intersect=fn)
        sc.commit()
        return sc
    for cfg, text in ((CFG + ",inst_filters=1", ihh.REFUSE_FILTER), (CFG, "geometry filter functions inside an instanced scene are not supported")):
        dev = rtc.Device(cfg)
        log, keep = _log(dev)
        hair = ihh.add_scene(rtc, dev, ihh.scenes("a")["m"], 1)
        mesh = filtered(dev)
        top = rtc.Scene(dev)
        top.add_instance(hair, ih.affine(), geom_id=0)
        top.add_instance(mesh, ih.affine((30, 0, 0)), geom_id=7)
        with pytest.raises(rtc.RTCError) as e:
            top.commit()
        assert e.value.code == rtc.RTC_ERROR_INVALID_OPERATION and text in log[-1][1], log
        if text is ihh.REFUSE_FILTER:
            assert "instance 7" in log[-1][1]
        for s in (top, hair, mesh):
            s.release()
        dev.release()


def test_accels_that_disagree_in_arithmetic_are_refused_with_the_hair_accels_named(rtc):
    dev = rtc.Device(CFG)
    log, keep = _log(dev)
    a = ihh.add_scene(rtc, dev, ihh.scenes("a")["m"], 0)  # robust lines
    b = ihh.add_scene(rtc, dev, ihh.scenes("b")["m"], 1)  # fast curves
    top = rtc.Scene(dev)
    top.add_instance(a, ih.affine(), geom_id=0)
    top.add_instance(b, ih.affine((30, 0, 0)), geom_id=1)
    with pytest.raises(rtc.RTCError):
        top.commit()
    msg = log[-1][1]
    assert "disagree in accel kind" in msg and "(curve)" in msg and "(line)" in msg and "instance 1" in msg and "instance 0" in msg, msg
    for s in (top, a, b):
        s.release()
    dev.release()


def test_subdivision_beside_hair_in_one_instanced_scene_stays_refused(rtc):
    cfg = CFG + ",subdiv_accel=default"
    dev = rtc.Device(cfg)
    log, keep = _log(dev)
    sc = rtc.Scene(dev)
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    sc.add_subdiv(v, np.array([4], np.uint32), np.arange(4, dtype=np.uint32))
    lv, idx = ihh.strands(2, 3)
    sc.add_lines(lv, idx)
    sc.commit()
    top = rtc.Scene(dev)
    top.add_instance(sc, ih.affine(), geom_id=0)
    with pytest.raises(rtc.RTCError):
        top.commit()
    assert "an instanced scene that enables subdivision meshes may hold nothing else" in log[-1][1], log
    top.release()
    sc.release()
    dev.release()


# ---- 4. a top scene without hair builds the parent's bytes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_without_hair_below_it_a_top_scene_builds_the_same_bytes_with_and_without_the_key(rtc, bomberman, mode):
    moving = [ih.affine((1, 2, 3)), ih.affine((1.5, 2, 3))]
    cases = [(imm.scenes_c(bomberman), [(0, "m", IDENT), (1, "m", moving)], 22 + mode),  # the general layout: scene records with zero pad words
             (iq.mixed_scenes(bomberman), [(0, "a", IDENT), (1, "b", [ih.affine((40, 0, 0))])], 16 + mode)]
    for scs, inst, kind in cases:
        out = []
        for cfg in (CFG + ",quad_accel_mb=default", CFG.replace(",inst_hair=1", ",quad_accel_mb=default")):
            build = imm.build if "tris_mb" in next(iter(scs.values())) else iq.build
            dev, top, inner = build(rtc, mode, scs, [(g, k, s) if build is imm.build else (g, k, s[0]) for g, k, s in inst], cfg)
            st = top.stats()
            assert st["accelKind"] == kind
            out.append(([top.accel_data(k).tobytes() for k in range(4)], top.accel_root(), {k: v for k, v in st.items()}))
            iq.release(dev, top, inner)
        assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and out[0][2] == out[1][2]
    scs, inst, _ = cases[0]
    dev, top, inner = imm.build(rtc, mode, scs, inst, CFG + ",quad_accel_mb=default")
    blobs = top.accel_data(2)
    rec = blobs[:64].view(ih.INST_DT)[0]
    assert not blobs[int(rec["root"]) * 64 + 16: int(rec["root"]) * 64 + 64].any()  # words 4.. of the scene record stay zero
    iq.release(dev, top, inner)
