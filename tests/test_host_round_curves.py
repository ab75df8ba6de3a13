"""CPU tests of round cubic curves (RTC_GEOMETRY_TYPE_ROUND_BEZIER_CURVE / _ROUND_BSPLINE_CURVE, device config round_curves=1) on a
`gpu=none,round_curves=1,hair_accel=default` device: the key's boundary and RTC_DEVICE_PROPERTY_CURVE_GEOMETRY_SUPPORTED, buffer formats,
curve validity, the CurveRecords (N = 0) and the BVH8 over the boxes of accurateBounds(), the two commit refusals, hair_accel= names,
rtcInterpolate, the accel slot beside the flat curves and meshes, and the float32 restatement of the tube leaf against the float64 truth
on the two pinned inputs of tests/test_gpu_round_curves.py (tests/round_curve_helpers.py)."""
import numpy as np
import pytest

import curve_helpers as ch
import round_curve_helpers as rh
from round_curve_helpers import ACCEL_CURVE_FAST, ACCEL_CURVE_ROBUST, CURVE_DT, NODE_DT, ROBUST, ROUND_BEZIER, ROUND_BSPLINE
from test_host_curves import Errors

HOST = "gpu=none,round_curves=1,hair_accel=default"
F = np.float32


def _hair(n=40, seed=3):
    v, idx, _, _ = ch.hair_and_rays(n, 1, seed)
    return v, idx


# ---- 1. the key's boundary -----------------------------------------------------------------------------------------------------------------
def test_with_the_key_both_round_types_are_taken_and_the_property_answers_one(rtc):
    dev = rtc.Device(HOST)
    err = Errors(dev)
    for t in (ROUND_BEZIER, ROUND_BSPLINE, 25, 33):
        g = dev.lib.rtcNewGeometry(dev.handle, t)
        assert g and dev.error() == rtc.RTC_ERROR_NONE
        dev.lib.rtcSetGeometryTessellationRate(g, 9.0)  # accepted, no effect on round curves
        assert dev.error() == rtc.RTC_ERROR_NONE
        dev.lib.rtcReleaseGeometry(g)
    assert not dev.lib.rtcNewGeometry(dev.handle, 120)  # RTC_GEOMETRY_TYPE_USER
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "RTC_GEOMETRY_TYPE_USER not supported")
    assert dev.get_property(99) == 1  # all five curve types are taken
    dev.release()


def test_without_hair_accel_a_host_device_takes_the_round_types_and_the_property_stays_zero(rtc):
    dev = rtc.Device("gpu=none,round_curves=1")
    err = Errors(dev)
    for t in (ROUND_BEZIER, ROUND_BSPLINE):
        g = dev.lib.rtcNewGeometry(dev.handle, t)
        assert g and dev.error() == rtc.RTC_ERROR_NONE
        dev.lib.rtcReleaseGeometry(g)
    for t in (25, 33):  # the flat cubic types are still refused there
        assert not dev.lib.rtcNewGeometry(dev.handle, t)
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "RTC_GEOMETRY_TYPE_*_CURVE not supported")
    assert dev.get_property(99) == 0
    dev.release()


@pytest.mark.parametrize("cfg", ["gpu=none", "gpu=none,hair_accel=default", "gpu=none,round_curves=0,hair_accel=default"])
def test_without_the_key_nothing_changes(rtc, cfg):
    dev = rtc.Device(cfg)
    err = Errors(dev)
    for t in (ROUND_BEZIER, ROUND_BSPLINE):
        assert not dev.lib.rtcNewGeometry(dev.handle, t)
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "RTC_GEOMETRY_TYPE_*_CURVE not supported")
    assert dev.get_property(99) == 0
    dev.release()


def test_an_unknown_value_of_the_key_is_an_invalid_argument(rtc):
    with pytest.raises(rtc.RTCError):
        rtc.Device("gpu=none,round_curves=2")


# ---- 2. buffer formats ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gtype", [ROUND_BEZIER, ROUND_BSPLINE])
def test_buffer_formats(rtc, gtype):
    dev = rtc.Device(HOST)
    lib = dev.lib
    g = lib.rtcNewGeometry(dev.handle, gtype)
    vb = np.zeros((8, 4), F)
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0, rtc.RTC_FORMAT_FLOAT3, vb.ctypes.data, 0, 16, 8)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION  # vertices are (x, y, z, radius)
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0, rtc.RTC_FORMAT_FLOAT4, vb.ctypes.data, 0, 16, 8)
    assert dev.error() == rtc.RTC_ERROR_NONE
    ib = np.zeros(4, np.uint32)
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_INDEX, 0, rtc.RTC_FORMAT_UINT4, ib.ctypes.data, 0, 16, 1)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION  # one word per curve
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_INDEX, 0, rtc.RTC_FORMAT_UINT, ib.ctypes.data, 0, 4, 4)
    assert dev.error() == rtc.RTC_ERROR_NONE
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_INDEX, 1, rtc.RTC_FORMAT_UINT, ib.ctypes.data, 0, 4, 4)
    assert dev.error() == rtc.RTC_ERROR_INVALID_ARGUMENT  # slot 0 only
    fb = np.zeros(3, np.uint8)
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_FLAGS, 0, rtc.RTC_FORMAT_UINT, fb.ctypes.data, 0, 1, 3)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_FLAGS, 0, rtc.RTC_FORMAT_UCHAR, fb.ctypes.data, 0, 1, 3)
    assert dev.error() == rtc.RTC_ERROR_NONE
    assert lib.rtcGetGeometryBufferData(g, rtc.RTC_BUFFER_TYPE_FLAGS, 0) == fb.ctypes.data
    assert lib.rtcGetGeometryBufferData(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0) == vb.ctypes.data
    p = lib.rtcSetNewGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0, rtc.RTC_FORMAT_FLOAT4, 16, 8)  # an owned buffer
    assert p and dev.error() == rtc.RTC_ERROR_NONE and lib.rtcGetGeometryBufferData(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0) == p
    lib.rtcReleaseGeometry(g)
    dev.release()


# ---- 3. validity ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_curves_get_no_record_and_keep_their_prim_ids(rtc):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    v = np.zeros((14, 4), F)
    v[:, 0] = np.arange(14)
    v[:, 3] = 0.1
    v[5, 1] = np.nan   # curves 2..5 use vertex 5
    v[12, 3] = -0.1    # curves 9, 10 use vertex 12
    idx = np.array([0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 12], np.uint32)  # the last two: index + 3 outside the vertex buffer
    sc.add_round_curves(v, idx, flags=np.arange(len(idx)) % 2)
    sc.commit()
    rec = sc.accel_data(2).view(CURVE_DT)
    assert sorted(rec["primID"].tolist()) == [0, 1, 4, 5, 6]
    assert sc.stats()["primCount"] == 5 and sc.stats()["primBytes"] == 80
    sc.release()
    sc = rtc.Scene(dev)
    v = np.zeros((8, 4), F)  # a radius of zero is valid, an infinite coordinate is not
    v[:, 0] = np.arange(8)
    v[7, 2] = np.inf
    sc.add_round_curves(v, np.array([0, 4], np.uint32))
    sc.commit()
    assert sc.accel_data(2).view(CURVE_DT)["primID"].tolist() == [0]
    sc.release()
    dev.release()


# ---- 4. / 5. records, boxes, tree ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,kind", [(0, ACCEL_CURVE_FAST), (ROBUST, ACCEL_CURVE_ROBUST)])
@pytest.mark.parametrize("basis", ["bezier", "bspline"])
def test_records_hold_the_native_points_and_the_boxes_are_accurate_bounds(rtc, flags, kind, basis):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev, flags)
    v, idx = _hair(300)
    gid = sc.add_round_curves(v, idx, basis=basis, geom_id=3)
    g = dev.lib.rtcGetGeometry(sc.handle, gid)
    dev.lib.rtcSetGeometryTessellationRate(g, 9.0)  # no effect: N stays 0
    dev.lib.rtcCommitGeometry(g)
    sc.commit()
    st = sc.stats()
    assert st["accelKind"] == kind and st["primCount"] == len(idx) and st["primBytes"] == 80 and st["nodeBytes"] == 96
    assert st["totalBytes"] == st["nodeCount"] * 96 + len(idx) * 80
    rec = sc.accel_data(2).view(CURVE_DT)
    nodes = sc.accel_data(0).view(NODE_DT)
    assert len(rec) == len(idx) and sorted(rec["primID"].tolist()) == list(range(len(idx))) and (rec["geomID"] == 3).all()
    assert (rec["pad"] == 0).all() and (rec["N"] == 0).all()
    want = ch.native(v, idx, basis)  # Bezier input verbatim, B-spline input converted (ch.bspline_to_bezier)
    assert rec["v"].tobytes() == want[rec["primID"]].tobytes()
    blo, bhi = rh.accurate_bounds(rec["v"], np.float32)
    seen, leaves = 0, 0
    for path, first, count in rh.walk_paths(nodes, sc.accel_root()):
        assert 1 <= count <= 28
        leaves += 1
        seen += count
        for k in range(first, first + count):
            for n, i in path:  # every node box on the way down, decoded as the kernel decodes it
                clo, chi = rh.decode_children(nodes[n])
                assert (clo[i] <= blo[k]).all() and (chi[i] >= bhi[k]).all(), (n, i, rec["primID"][k])
    assert seen == len(rec) and leaves == st["leafCount"]
    lo, hi = sc.bounds()
    assert np.array_equal(lo, blo.min(0)) and np.array_equal(hi, bhi.max(0))  # every record's box IS the restatement of accurateBounds
    # the box holds the tube: 4097 axis points of each curve, each with the sphere of its radius, which holds the disc of the surface
    a = rh.power_basis(rec["v"])
    u = np.linspace(0.0, 1.0, 4097)
    P, _, _ = rh._curve([x[:, None] for x in a], np.broadcast_to(u, (len(rec), 4097)))
    assert (blo[:, None] <= P[..., :3] - P[..., 3:] + 1e-6).all() and (bhi[:, None] >= P[..., :3] + P[..., 3:] - 1e-6).all()
    sc.release()
    dev.release()


def test_the_box_holds_sampled_surface_points(rtc):
    """4097 surface points of each curve - P(u) + r(u) (cos a n1 + sin a n2) with n1, n2 normal to P'(u), the angle a running with u - lie
    inside the record's box (bent, tapered curves; bounds of a committed scene)"""
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.normal(size=(80, 3)), rng.uniform(0.05, 0.6, (80, 1))], 1).astype(F)
    idx = np.arange(0, 80, 4, dtype=np.uint32)
    sc.add_round_curves(v, idx)
    sc.commit()
    rec = sc.accel_data(2).view(CURVE_DT)
    blo, bhi = rh.accurate_bounds(rec["v"], np.float32)
    a = rh.power_basis(rec["v"])
    u = np.linspace(0.0, 1.0, 4097)
    P, dP, _ = rh._curve([x[:, None] for x in a], np.broadcast_to(u, (len(rec), 4097)))
    T = dP[..., :3] / np.linalg.norm(dP[..., :3], axis=-1, keepdims=True)
    n1 = np.cross(T, np.array([0.3, -0.5, 0.81]))
    n1 /= np.linalg.norm(n1, axis=-1, keepdims=True)
    n2 = np.cross(T, n1)
    ang = (u * 2 * np.pi * 37)[None, :, None]
    S = P[..., :3] + P[..., 3:] * (np.cos(ang) * n1 + np.sin(ang) * n2)
    assert (blo[:, None] <= S + 1e-6).all() and (bhi[:, None] >= S - 1e-6).all()
    sc.release()
    dev.release()


# ---- 6. commit refusals, accel names ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis", ["bezier", "bspline"])
def test_time_steps_are_refused_at_commit(rtc, basis):
    dev = rtc.Device(HOST + ",hair_accel_mb=default")
    err = Errors(dev)
    sc = rtc.Scene(dev)
    v, idx = _hair(2)
    gid = sc.add_round_curves(v, idx, basis=basis)
    g = dev.lib.rtcGetGeometry(sc.handle, gid)
    dev.lib.rtcSetGeometryTimeStepCount(g, 2)
    assert dev.error() == rtc.RTC_ERROR_NONE
    dev.lib.rtcCommitGeometry(g)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "motion blur of round Bezier and B-spline curves is not supported")
    dev.release()


@pytest.mark.parametrize("cfg", [HOST, HOST + ",quad_accel=default,inst_accel=default", HOST + ",inst_accel=default,inst_hair=1",
                                 HOST + ",inst_accel=default,inst_hair=1,inst_hair_mb=1,hair_accel_mb=default,line_accel_mb=default",
                                 HOST + ",inst_accel=default,subdiv_accel=default,inst_filters=1"])
def test_round_curves_in_an_instanced_scene_are_refused(rtc, cfg):
    dev = rtc.Device(cfg)
    err = Errors(dev)
    inner = rtc.Scene(dev)
    inner.add_triangles(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], np.uint32))
    v, idx = _hair(2)
    curves = inner.add_round_curves(v, idx)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance(inner)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "round Bezier and B-spline curves inside an instanced scene are not supported")
    inner.set_enabled(curves, False)  # disabled, the round curve geometry does not count
    inner.commit()
    top.commit()
    assert top.stats()["accelKind"] != 0
    dev.release()


@pytest.mark.parametrize("name", ["default", "bvh4.bezier1v", "bvh4.bezier1i", "bvh4obb.bezier1v", "bvh4obb.bezier1i", "bvh8obb.bezier1v", "bvh8obb.bezier1i"])
def test_every_hair_accel_name_builds_the_one_accel(rtc, name):
    dev = rtc.Device("gpu=none,round_curves=1,hair_accel=" + name)
    sc = rtc.Scene(dev)
    v, idx = _hair()
    sc.add_round_curves(v, idx)
    sc.commit()
    assert sc.stats()["accelKind"] == ACCEL_CURVE_FAST and sc.stats()["primCount"] == len(idx)
    sc.release()
    dev.release()


def test_unknown_hair_accel_is_an_invalid_argument(rtc):
    dev = rtc.Device("gpu=none,round_curves=1,hair_accel=bvh8.bezier1v")
    err = Errors(dev)
    sc = rtc.Scene(dev)
    v, idx = _hair(2)
    sc.add_round_curves(v, idx)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_ARGUMENT, "unknown hair acceleration structure bvh8.bezier1v")
    dev.release()


# ---- 7. rtcInterpolate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis", ["bezier", "bspline"])
def test_interpolate_equals_the_flat_curve_of_the_same_vertices(rtc, basis):
    dev = rtc.Device(HOST)
    rng = np.random.default_rng(11)
    v = np.concatenate([rng.normal(size=(6, 3)), rng.uniform(0.1, 0.5, (6, 1))], 1).astype(F)
    attr = rng.normal(size=(6, 2)).astype(F)
    scenes = []
    for add in ("add_round_curves", "add_curves"):
        sc = rtc.Scene(dev)
        gid = getattr(sc, add)(v, np.array([0, 2], np.uint32), basis=basis)
        sc.set_vertex_attribute(gid, 1, attr)
        scenes.append((sc, gid))
    for prim, u in ((0, 0.0), (0, 0.25), (0, 1.0), (1, 0.5), (1, 0.8125)):
        for kw, count in (({}, 4), ({"buffer_type": rtc.RTC_BUFFER_TYPE_VERTEX_ATTRIBUTE, "slot": 1}, 2)):
            a = scenes[0][0].interpolate(scenes[0][1], prim, u, 0.375, count=count, **kw)
            b = scenes[1][0].interpolate(scenes[1][1], prim, u, 0.375, count=count, **kw)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0].any()
    pr, uu = np.array([0, 1, 0, 1], np.uint32), np.array([0.5, 0.25, 0.75, 1.0], F)
    a = scenes[0][0].interpolateN(scenes[0][1], pr, uu, np.zeros(4, F), count=4, valid=[-1, 0, -1, -1])
    b = scenes[1][0].interpolateN(scenes[1][1], pr, uu, np.zeros(4, F), count=4, valid=[-1, 0, -1, -1])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and not a[0][:, 1].any()
    for sc, _ in scenes:
        sc.release()
    dev.release()


# ---- 8. the restatement against the truth ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "b"])
def test_float32_restatement_meets_the_float64_truth_on_the_pinned_inputs(which):
    """The contract on the CPU before any GPU run: the leaf's arithmetic in float32 against the two-scan float64 truth under the rules of
    round_curve_helpers.compare.  Measured (hits / rays left out / t relative / u / Ng):  (a) 1127 / 8 (1 tie, 7 grazing misses) / 2.2e-7 /
    1.6e-6 / 1.7e-5;  (b) 685 / 8 (1 end, 7 grazing misses) / 1.2e-5 / 1.5e-5 / 2.7e-5; no hit or ID difference; no fold on either."""
    v, idx, org, dirs = rh.pinned(which)
    m = len(org)
    want = rh.pinned_truth(which)
    assert int(want["hit"].sum()) == rh.HAIR_HITS[which]
    got = rh.restate([(ch.native(v, idx), 0)], org, dirs, np.zeros(m, F), np.full(m, np.inf, F), np.float32)
    out, _, _, _ = rh.compare(got["hit"], got["geomID"], got["primID"], got["t"], got["u"], got["v"], got["Ng"], want, "float32 restatement, input (%s)" % which)
    assert out == rh.HAIR_LEFT_OUT[which] and out <= 0.005 * m
    # the u scan alone misses hits that the t scan finds (rays perpendicular to the tangent): the second scan is needed
    if which == "a":
        one = rh.truth([(ch.native(v, idx), 0)], org, dirs, np.zeros(m, F), np.full(m, np.inf, F), scan_t=False)
        assert int(one["hit"].sum()) <= int(want["hit"].sum()) and not (one["hit"] & ~want["hit"]).any()


def test_the_fold_rule_flags_rays_on_a_tube_that_runs_through_itself():
    """The first nine curves of the pinned hair under 1024 rays aimed at their middles: one of them bends more tightly than its radius, the
    hit point of a ray there has a second foot on the same curve inside that disc, and the rule leaves the ray out - on these rays, and
    on none of the two pinned inputs.  Every flagged ray is a hit whose point has another foot more than 0.005 away (the rule's own words,
    checked here from the curve alone), and the leaf's restatement is off the truth on some of them, which is what the rule is for."""
    v, idx, org, _ = ch.hair_and_rays(ch.HAIR_CURVES, 1024, 1)
    cp = ch.native(v, idx[:9])
    rng = np.random.default_rng(2)
    dirs = (cp[:, :, :3].mean(1)[np.arange(1024) % 9] + rng.normal(scale=0.001, size=(1024, 3)) - org).astype(F)
    want = rh.truth([(cp, 0)], org, dirs, np.zeros(1024, F), np.full(1024, np.inf, F))
    flagged = np.nonzero(want["fold"])[0]
    assert len(flagged) >= 5 and want["hit"][flagged].all() and len(set(want["primID"][flagged].tolist())) <= 2, flagged
    for i in flagged[:5]:  # the second foot, from the curve alone
        a = rh.power_basis(want["cp"][i:i + 1])
        u = np.linspace(0.0, 1.0, 20001)
        Q = want["org"][i] + want["t"][i] * want["dirs"][i]
        h, _ = rh._h([x for x in a], Q[None], u)
        far = (np.sign(h[:-1]) != np.sign(h[1:])) & (np.abs(u[:-1] - want["u"][i]) > 0.005)
        assert far.any() and (rh._G([x for x in a], Q[None], u)[:-1][far] < 1e-4).any(), i
    got = rh.restate([(cp, 0)], org, dirs, np.zeros(1024, F), np.full(1024, np.inf, F))
    off = np.abs(got["t"][flagged] - want["t"][flagged]) > 1e-4 * want["t"][flagged]
    print("fold rule: %d rays flagged on curves %s, the restatement is off the truth on %d of them" % (len(flagged), sorted(set(want["primID"][flagged].tolist())), int(off.sum())))
    assert not rh.pinned_truth("a")["fold"].any() and not rh.pinned_truth("b")["fold"].any()


def test_the_restatement_gives_the_closed_forms():
    straight = np.array([[[-1.5, 0, 0, .25], [-.5, 0, 0, .25], [.5, 0, 0, .25], [1.5, 0, 0, .25]]], F)
    org = np.array([[0, 0, -4], [0, 0, 0], [-4, 0, 0], [1.4, 0, -4], [0, .26, -4], [-4, 0, -4]], F)
    dirs = np.array([[0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 0, 1], [0, 0, 1], [1, 0, 1]], F)
    r = rh.restate([(straight, 5)], org, dirs, np.zeros(6, F), np.full(6, np.inf, F))
    assert r["hit"].tolist() == [True, True, False, True, False, True]
    assert r["t"][0] == F(3.75) and abs(r["t"][1] - 0.25) <= 1e-6 and abs(r["u"][3] - 29 / 30) <= 1e-6 and abs(r["u"][5] - 5 / 12) <= 1e-6
    taper = straight.copy()
    taper[0, :, 3] = [.1, .2, .3, .4]
    r = rh.restate([(taper, 5)], np.array([[.75, 0, -4], [-.75, 0, -4]], F), np.array([[0, 0, 1], [0, 0, 1]], F), np.zeros(2, F), np.full(2, np.inf, F))
    assert np.abs(r["t"] - [3.675, 3.825]).max() <= 1e-6 and np.abs(r["u"] - [.75, .25]).max() <= 1e-6


# ---- 9. the slot beside the others -----------------------------------------------------------------------------------------------------------
def test_flat_and_round_curves_and_triangles_make_three_accels(rtc):
    dev = rtc.Device(HOST)
    v, idx = _hair(30)
    tv = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    tri = np.array([[0, 1, 2]], np.uint32)
    tot = {}
    for parts in ("t", "c", "r", "cr", "tcr"):
        sc = rtc.Scene(dev)
        if "t" in parts:
            sc.add_triangles(tv, tri, geom_id=0)
        if "c" in parts:
            sc.add_curves(v, idx[:15], geom_id=1)
        if "r" in parts:
            sc.add_round_curves(v, idx[15:], geom_id=2)
        sc.commit()
        tot[parts] = (sc.stats()["accelKind"], sc.stats()["totalBytes"], sc.accel_data(2).tobytes(), sc.stats()["primCount"])
        sc.release()
    assert tot["t"][0] == 2 and tot["tcr"][0] == 2               # the inspection calls describe the triangles first, as before
    assert tot["c"][0] == ACCEL_CURVE_FAST and tot["r"][0] == ACCEL_CURVE_FAST
    assert tot["cr"][2] == tot["c"][2] and tot["cr"][3] == 15    # ... and the flat curves in front of the round ones: their records, unchanged
    assert tot["cr"][1] == tot["c"][1] + tot["r"][1] and tot["tcr"][1] == tot["t"][1] + tot["c"][1] + tot["r"][1]  # three accels
    rec = np.frombuffer(tot["r"][2], CURVE_DT)
    assert (rec["N"] == 0).all() and (rec["geomID"] == 2).all() and (np.frombuffer(tot["c"][2], CURVE_DT)["N"] == 4).all()
    dev.release()
