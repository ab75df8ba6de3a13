"""Line segments and flat curves with time steps below an instance (device config inst_hair=1,inst_hair_mb=1), on a host-only device:
the key, the kinds, the layout of the accel (csrc/accel.h InstanceSceneRecord: eight roots; CurveMBRecord and LineMBRecord sections behind
the LineRecords), the refusals, and that a top scene without moving hair below it builds the bytes it built without the key.
tests/instance_hair_mb_helpers.py."""
import ctypes as C
import os

import numpy as np
import pytest

import instance_hair_helpers as ihh
import instance_hair_mb_helpers as ihm
import instance_helpers as ih
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
from instance_helpers import EMPTY, NODE_DT

CFG = ihm.HOST_CFG
IDENT = [ih.affine()]


def _log(dev):
    log = []
    fn = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda u, c, msg: log.append((c, msg.decode())))
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(fn, C.c_void_p), None)
    return log, fn


def _refused(rtc, mode, scs, inst, cfg, text, gid=None):
    dev, top, inner = ihm.build(rtc, mode, scs, inst, cfg, commit=False)
    log, keep = _log(dev)
    with pytest.raises(rtc.RTCError) as e:
        top.commit()
    assert e.value.code == rtc.RTC_ERROR_INVALID_OPERATION
    assert log and log[-1][0] == rtc.RTC_ERROR_INVALID_OPERATION and text in log[-1][1], log
    if gid is not None:
        assert log[-1][1].endswith("(instance %d)" % gid), log
    ihm.release(dev, top, inner)
    return log[-1][1]


def _top_depth(nodes, root):
    def depth(ref):
        if ref == EMPTY or ref & ih.LEAF:
            return 0
        return 1 + max(depth(int(c)) for c in nodes[ref]["child"])
    return depth(int(root))


def _counts(rtc, d, mode):
    """(own static hair, own moving hair, own mesh accels, record counts in the order of ihm.split_blobs behind the scene count)"""
    static = {k: d.get(k) for k in ("tris", "quads", "tris_mb", "quads_mb", "curves", "lines")}
    own = ihm.own_hair(rtc, static, mode)
    own_mb = ihm.own_hair_mb(rtc, d, mode)
    mesh = imm.own_accels(rtc, CFG, static, mode)
    n = lambda o: len(o[1]) if o else 0  # noqa: E731
    return own, own_mb, mesh, (n(mesh["tris_mb"]), n(mesh["quads_mb"]), n(own["curves"]), n(own["lines"]), n(own_mb["curves_mb"]), n(own_mb["lines_mb"]))


# ---- 1. the key -------------------------------------------------------------------------------------------------------------------------
def test_inst_hair_mb_values_and_the_bad_value_message(rtc):
    for ok in ("0", "1"):
        rtc.Device("gpu=none,inst_hair_mb=" + ok).release()
        rtc.Device("gpu=none,inst_hair=1,inst_hair_mb=" + ok).release()
    for bad in ("gpu=none,inst_hair_mb=2", "gpu=none,inst_hair_mb=yes", "gpu=none,inst_hair=2"):  # a key of its own, not a value of inst_hair
        with pytest.raises(rtc.RTCError) as e:
            rtc.Device(bad)
        assert e.value.code == rtc.RTC_ERROR_INVALID_ARGUMENT
    # The full text with the value in it cannot be asserted through the API: a failed rtcNewDevice has no device to hold a message or an
    # error callback, and rtcGetDeviceError(NULL) hands out the per-thread CODE only (rtcore_api.cpp report()).  So the code is asserted
    # above for each bad value, and the wording - the key's own prefix, which no other message shares - is looked up in the library, as
    # tests/test_host_instance_hair.py does for inst_hair
    assert rtc.lib().rtcGetDeviceError(None) == rtc.RTC_ERROR_NONE  # (taken by the RTCError raised above)
    with open(os.path.join(os.path.dirname(rtc.__file__), "lib", "libembree3.so"), "rb") as f:
        text = f.read()
    assert b"inst_hair_mb=: unknown value '" in text and b"' (0 or 1)" in text


@pytest.mark.parametrize("cfg", [CFG.replace(",inst_hair_mb=1", ""), CFG.replace("inst_hair_mb=1", "inst_hair_mb=0")])
def test_without_the_key_the_old_refusal_word_for_word(rtc, cfg):
    for d in (ihm.desc(lines_mb=ihm.moving_strands(2, 2, 3)), ihm.desc(curves_mb=ihm.moving_curve_geometries(2, n=2)[:1])):
        msg = _refused(rtc, 1, {"m": d}, [(5, "m", IDENT)], cfg, ihh.REFUSE_MOTION, gid=5)
        assert msg.endswith(ihh.REFUSE_MOTION + " (instance 5)")


def test_the_key_acts_only_where_inst_hair_acts_and_without_its_motion_blur_accel_the_inner_commit_refuses_first(rtc):
    """A host-only device honours the key for a type only when the config names that type's motion-blur accel.  Without the name the
    top scene's refusal text ("motion blur of line segments and flat curves inside an instanced scene is not supported") CANNOT be
    reached: such a device does not build the motion-blur accel at all, so the instanced scene's OWN commit refuses the moving geometry
    first, with the text it always had, and there is no committed scene to instance.  That earlier refusal is what is asserted here."""
    lines, curves = ihm.desc(lines_mb=ihm.moving_strands(2, 2, 3)), ihm.desc(curves_mb=ihm.moving_curve_geometries(2, n=2)[:1])
    # inst_hair_mb=1 without inst_hair=1: the refusals of a device without either key
    cfg = CFG.replace(",inst_hair=1", "")
    _refused(rtc, 1, {"m": lines}, [(0, "m", IDENT)], cfg, ihh.OLD_ONLY)
    _refused(rtc, 1, {"m": curves}, [(0, "m", IDENT)], cfg, ihh.OLD_CURVES)
    # both keys, inst_accel= not named: a host-only device does not honour inst_hair=1 at all
    _refused(rtc, 1, {"m": lines}, [(0, "m", IDENT)], CFG.replace("inst_accel=default,", ""), "an instanced scene may hold")
    # both keys, the motion-blur accel of the type not named: the moving geometry is refused at its own scene's commit, before any top scene
    for cfg, d, text, other in ((CFG.replace(",line_accel_mb=default", ""), lines, "motion blur of line segments is not supported", curves),
                                (CFG.replace(",hair_accel_mb=default", ""), curves, "motion blur of flat Bezier and B-spline curves is not supported", lines)):
        dev = rtc.Device(cfg)
        log, keep = _log(dev)
        with pytest.raises(rtc.RTCError):
            ihm.add_scene(rtc, dev, d, 1)
        assert text in log[-1][1], log
        dev.release()
        dev, top, inner = ihm.build(rtc, 1, {"m": other}, [(0, "m", IDENT)], cfg)  # ... and takes the other type
        assert top.stats()["accelKind"] == 23
        ihm.release(dev, top, inner)


# ---- 2. kinds and layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["a", "b", "c", "d"])
def test_kind_eight_roots_records_and_sections(rtc, capfd, mode, which):
    scs = ihm.scenes(which)
    d = scs["m"]
    moving = [ih.affine((1, 2, 3)), ih.affine((1.5, 2, 3))]
    inst = [(0, "m", IDENT), (1, "m", moving), (2, "m", [ih.affine((40, 0, 0), (2, 2, 2))])]  # three instances share the scene: stored once
    capfd.readouterr()
    dev, top, inner = ihm.build(rtc, mode, scs, inst, CFG + ",verbose=2")
    err = capfd.readouterr().err
    st = top.stats()
    assert st["accelKind"] == imm.kind(mode)  # 22 / 23
    own, own_mb, mesh, counts = _counts(rtc, d, mode)
    # the verbose commit line is what exposes the hair level and the two new counts
    assert "instance accel kind %d: hair level 2, %d instanced motion blur curve segment records, %d instanced motion blur line segment records" % (st["accelKind"], counts[4], counts[5]) in err, err
    n_quads = len(mesh["quads"][1]) if mesh["quads"] else 0
    nodes = top.accel_data(0).view(NODE_DT)
    s = ihm.split_blobs(top.accel_data(2), 3, n_quads, 2, 1, *counts)
    assert s["curvemb_off"] % 160 == 0 and s["linemb_off"] % 80 == 0
    assert len(s["scenes"]) == 1 and not s["scenes"]["pad"].any()
    assert (s["recs"]["root"] == 3 + n_quads + 2).all() and sorted(s["recs"]["geomID"].tolist()) == [0, 1, 2]
    roots = ihm.scene_roots(top.accel_data(2), s["recs"][0])
    assert [n for n, _, _ in roots] == ["triRoot", "triMBRoot", "quadRoot", "quadMBRoot", "curveRoot", "curveMBRoot", "lineRoot", "lineMBRoot"]
    for name, _, root in roots:
        assert (root == EMPTY) == (d.get(ihm.PART_OF[name]) is None), name
    deepest = 0
    for part, name, got, off, size in (("curves_mb", "curveMBRoot", s["curvemb"], s["curvemb_off"], 160), ("lines_mb", "lineMBRoot", s["linemb"], s["linemb_off"], 80)):
        root = int(s["scenes"][0][name])
        if own_mb[part] is None:
            assert len(got) == 0
            continue
        o_nodes, o_recs, o_root, o_depth, o_kind = own_mb[part]
        assert got.tobytes() == o_recs.tobytes(), part  # byte-equal to the inner scene's own `blobs`
        idx, leaves, depth = ihh.leaf_records(nodes, root)
        base = off // size
        assert sorted(idx) == list(range(base, base + len(o_recs))), part  # the leaves cover exactly the scene's record range
        assert max(idx) < 1 << 26
        o_idx, o_leaves, o_d = ihh.leaf_records(o_nodes, o_root)
        assert [(f + base, c) for f, c in o_leaves] == leaves and depth == o_d  # the scene's own tree, rebased
        assert max(c for _, c in leaves) > 4, (part, leaves)  # leaves span several blocks of four
        assert bool(rtc.accel_kind_row(o_kind)["robust"]) == (mode == 0)
        deepest = max(deepest, o_depth)
    for o in list(own.values()) + [mesh[p] for p in ("tris", "tris_mb", "quads", "quads_mb")]:
        if o:
            deepest = max(deepest, o[3])
    trees = sum(r != EMPTY for _, _, r in roots)
    assert st["maxDepth"] == _top_depth(nodes, top.accel_root()) + 1 + (trees - 1) + deepest, (st["maxDepth"], trees, deepest)
    ihm.release(dev, top, inner)


def test_eight_trees_bound_the_depth_and_are_visited_in_slot_order(rtc):
    """all eight trees in one scene: seven markers wait above the exit marker; the host walk of a ray that hits nothing continues in the
    trees in the order triangles, motion-blur triangles, quads, motion-blur quads, curves, motion-blur curves, lines, motion-blur lines"""
    scs = ihm.scenes("c")
    inst = [(0, "m", IDENT), (1, "m", [ih.affine((40, 0, 0), (2, 2, 2))])]
    dev, top, inner = ihm.build(rtc, 1, scs, inst, CFG)
    st = top.stats()
    assert st["accelKind"] == 23
    nodes, blobs = top.accel_data(0).view(NODE_DT), top.accel_data(2)
    roots = ihm.scene_roots(blobs, blobs[:64].view(ih.INST_DT)[0])
    assert all(r != EMPTY for _, _, r in roots)
    deepest = max(ihh.leaf_records(nodes, r)[2] for _, _, r in roots)
    assert st["maxDepth"] == _top_depth(nodes, top.accel_root()) + 1 + 7 + deepest
    pts = ihm.points(scs["m"])
    c = (pts.min(0) + pts.max(0)) / 2
    org = np.array([c + (0, 0, -30), c + (40, 0, -30) + c, c + (0, -50, 0)])
    dirs = np.array([(0.01, 0.02, 1.0), (0.02, 0.01, 1.0), (0.01, 1.0, 0.02)])
    deep, visits = ihm.simulate_stack(nodes, top.accel_root(), blobs, 2, org, dirs)
    entered = [v for per in visits for v in per]
    assert len(entered) >= 3 and sorted({g for g, _ in entered}) == [0, 1]
    for _, codes in entered:
        assert codes == [0, 2, 1, 3, 4, 6, 5, 7], codes  # INST_TREE_*: tri, triMB, quad, quadMB, curve, curveMB, line, lineMB
    assert deep.max() < 7 * (st["maxDepth"] + 1) + 2
    ihm.release(dev, top, inner)


def test_two_scenes_fill_the_sections_in_order_of_first_use(rtc):
    scs = {"a": ihm.scenes("a")["m"], "c": ihm.scenes("c")["m"], "s": ihh.scenes("a")["m"]}  # "s": static lines only
    inst = [(0, "c", IDENT), (1, "a", [ih.affine((60, 0, 0))]), (2, "c", [ih.affine((0, 60, 0))]), (3, "s", [ih.affine((0, 0, 60))])]
    dev, top, inner = ihm.build(rtc, 1, scs, inst, CFG)
    (oa, ma, _, ca), (oc, mc, meshc, cc), (os_, ms, _, cs) = (_counts(rtc, scs[k], 1) for k in ("a", "c", "s"))
    total = tuple(x + y + z for x, y, z in zip(cc, ca, cs))
    s = ihm.split_blobs(top.accel_data(2), 4, len(meshc["quads"][1]), 0, 3, *total)
    nodes = top.accel_data(0).view(NODE_DT)
    assert s["linemb"].tobytes() == mc["lines_mb"][1].tobytes() + ma["lines_mb"][1].tobytes()  # "c" is used first
    assert s["curvemb"].tobytes() == mc["curves_mb"][1].tobytes()
    sc_c, sc_a, sc_s = s["scenes"]
    assert int(sc_a["curveMBRoot"]) == EMPTY and int(sc_c["curveMBRoot"]) != EMPTY
    assert int(sc_s["curveMBRoot"]) == EMPTY and int(sc_s["lineMBRoot"]) == EMPTY and int(sc_s["lineRoot"]) != EMPTY  # no moving hair: REF_EMPTY in words 6 / 7
    base, n_c = s["linemb_off"] // 80, len(mc["lines_mb"][1])
    assert sorted(ihh.leaf_records(nodes, int(sc_c["lineMBRoot"]))[0]) == list(range(base, base + n_c))
    assert sorted(ihh.leaf_records(nodes, int(sc_a["lineMBRoot"]))[0]) == list(range(base + n_c, base + n_c + len(ma["lines_mb"][1])))
    cbase = s["curvemb_off"] // 160
    assert sorted(ihh.leaf_records(nodes, int(sc_c["curveMBRoot"]))[0]) == list(range(cbase, cbase + len(mc["curves_mb"][1])))
    ihm.release(dev, top, inner)


def _bytes_of(rtc, build, mode, scs, inst, cfg):
    dev, top, inner = build(rtc, mode, scs, inst, cfg)
    out = ([top.accel_data(k).tobytes() for k in range(4)], top.accel_root(), dict(top.stats()))
    iq.release(dev, top, inner)
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_without_moving_hair_below_it_a_top_scene_builds_the_same_bytes_with_and_without_the_key(rtc, bomberman, mode):
    moving = [ih.affine((1, 2, 3)), ih.affine((1.5, 2, 3))]
    # static hair only: with and without inst_hair_mb=1
    scs, inst = ihh.scenes("d"), [(0, "m", IDENT), (1, "m", moving)]
    a = _bytes_of(rtc, ihh.build, mode, scs, inst, CFG)
    b = _bytes_of(rtc, ihh.build, mode, scs, inst, CFG.replace(",inst_hair_mb=1", ""))
    assert a == b and a[2]["accelKind"] == 22 + mode
    dev, top, inner = ihh.build(rtc, mode, scs, inst, CFG)
    blobs = top.accel_data(2)
    rec = blobs[:64].view(ih.INST_DT)[0]
    assert not blobs[int(rec["root"]) * 64 + 24: int(rec["root"]) * 64 + 64].any()  # words 6.. of the scene record stay zero
    ihh.release(dev, top, inner)
    # no hair at all: with both keys and without both
    for scs, inst, kind, build in ((imm.scenes_c(bomberman), [(0, "m", IDENT), (1, "m", moving)], 22 + mode, imm.build),
                                   (iq.mixed_scenes(bomberman), [(0, "a", IDENT[0]), (1, "b", ih.affine((40, 0, 0)))], 16 + mode, iq.build)):
        a = _bytes_of(rtc, build, mode, scs, inst, CFG)
        b = _bytes_of(rtc, build, mode, scs, inst, CFG.replace(",inst_hair=1", "").replace(",inst_hair_mb=1", ""))
        assert a == b and a[2]["accelKind"] == kind


def test_a_disabled_moving_hair_geometry_does_not_count(rtc):
    dev = rtc.Device(CFG)
    sc = rtc.Scene(dev)
    t, _ = ihh.coincident_meshes()
    sc.add_triangles(t[0], t[1], geom_id=0)
    steps, idx, _ = ihm.moving_strands(2, 2, 3)
    sc.add_lines_mb(steps, idx, geom_id=1)
    sc.set_enabled(1, False)
    sc.commit()
    top = rtc.Scene(dev)
    top.add_instance(sc, ih.affine(), geom_id=0)
    top.commit()
    assert top.stats()["accelKind"] == 15  # ACCEL_INST_TRI_MOELLER: the triangle-only accel, as without the line geometry
    sc.set_enabled(1, True)  # ... and enabled again it counts: the general layout with a motion-blur line tree
    sc.commit()
    top.commit()
    assert top.stats()["accelKind"] == 23
    roots = dict((n, r) for n, _, r in ihm.scene_roots(top.accel_data(2), top.accel_data(2)[:64].view(ih.INST_DT)[0]))
    assert roots["lineMBRoot"] != EMPTY and roots["triRoot"] != EMPTY and all(roots[n] == EMPTY for n in ("curveRoot", "lineRoot", "curveMBRoot", "quadRoot"))
    top.release()
    sc.release()
    dev.release()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
def test_moving_hair_built_under_linear_node_bounds_is_refused(rtc):
    for d in (ihm.scenes("a")["m"], ihm.desc(curves_mb=ihm.moving_curve_geometries(2, n=2)[:1])):
        msg = _refused(rtc, 1, {"m": d}, [(2, "m", IDENT), (4, "m", [ih.affine((40, 0, 0))])], CFG + ",mb_bounds=linear", ihm.REFUSE_MB_LINEAR, gid=2)
        assert msg.endswith(ihm.REFUSE_MB_LINEAR + " (instance 2)")


def test_the_inherited_refusals_with_moving_hair_as_the_trigger(rtc):
    scs = {"m": ihm.scenes("a")["m"]}
    moving = [ih.affine((1, 2, 3)), ih.affine((1.5, 2, 3))]
    # beside a time-dependent top level
    _refused(rtc, 1, scs, [(0, "m", IDENT), (4, "m", moving)], CFG + ",inst_bounds=linear", ihh.REFUSE_LINEAR, gid=0)
    # (beside inst_mb_bounds=linear trees the device's mb_bounds is linear and the moving hair itself holds time-dependent nodes: the
    # refusal of test_moving_hair_built_under_linear_node_bounds_is_refused comes first)
    # geometry filters below such a top scene, with and without inst_filters=1
    fn = rtc.FILTER_FUNC(lambda args: None)
    t, _ = ihh.coincident_meshes()
    for cfg, text in ((CFG + ",inst_filters=1", ihh.REFUSE_FILTER), (CFG, "geometry filter functions inside an instanced scene are not supported")):
        dev = rtc.Device(cfg)
        log, keep = _log(dev)
        hair = ihm.add_scene(rtc, dev, scs["m"], 1)
        mesh = rtc.Scene(dev)
        mesh.add_triangles(t[0], t[1], geom_id=0)
        mesh.set_filters(0, intersect=fn)
        mesh.commit()
        top = rtc.Scene(dev)
        top.add_instance(hair, ih.affine(), geom_id=0)
        top.add_instance(mesh, ih.affine((30, 0, 0)), geom_id=7)
        with pytest.raises(rtc.RTCError) as e:
            top.commit()
        assert e.value.code == rtc.RTC_ERROR_INVALID_OPERATION and text in log[-1][1], log
        if text is ihh.REFUSE_FILTER:
            assert log[-1][1].endswith("(instance 7)")
        for s in (top, hair, mesh):
            s.release()
        dev.release()
    # a filter on the moving-hair geometry itself
    dev = rtc.Device(CFG + ",inst_filters=1")
    log, keep = _log(dev)
    hair = rtc.Scene(dev)
    steps, idx, _ = ihm.moving_strands(2, 2, 3)
    hair.add_lines_mb(steps, idx, geom_id=0)
    hair.set_filters(0, occluded=fn)
    hair.commit()
    top = rtc.Scene(dev)
    top.add_instance(hair, ih.affine(), geom_id=3)
    with pytest.raises(rtc.RTCError):
        top.commit()
    assert ihh.REFUSE_FILTER in log[-1][1] and log[-1][1].endswith("(instance 3)"), log
    top.release()
    hair.release()
    dev.release()


def test_accels_that_disagree_in_arithmetic_are_refused_with_the_moving_hair_accels_named(rtc):
    dev = rtc.Device(CFG)
    log, keep = _log(dev)
    a = ihm.add_scene(rtc, dev, ihm.scenes("a")["m"], 0)  # robust moving lines
    b = ihm.add_scene(rtc, dev, ihm.scenes("b")["m"], 1)  # fast moving curves
    top = rtc.Scene(dev)
    top.add_instance(a, ih.affine(), geom_id=0)
    top.add_instance(b, ih.affine((30, 0, 0)), geom_id=1)
    with pytest.raises(rtc.RTCError):
        top.commit()
    msg = log[-1][1]
    assert "disagree in accel kind" in msg and "(motion blur curve)" in msg and "(motion blur line)" in msg and "instance 1" in msg and "instance 0" in msg, msg
    for s in (top, a, b):
        s.release()
    dev.release()
