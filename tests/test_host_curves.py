"""CPU tests of flat cubic curves (RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE / _FLAT_BSPLINE_CURVE) on a `gpu=none,hair_accel=default` device:
the types and what stays refused, buffer formats, curve validity, the tessellation-rate clamp, the B-spline conversion, hair_accel=
names, accel kinds, the CurveRecords and the BVH8 over them, commit refusals, rtcInterpolate / rtcInterpolateN
(NativeCurvesISA::interpolate_helper, scene_bezier_curves.cpp:241-281), and the float32 restatement of the ribbon intersector against its
float64 truth on the pinned hair of tests/test_gpu_curves.py."""
import ctypes as C

import numpy as np
import pytest

import curve_helpers as ch
from curve_helpers import ACCEL_CURVE_FAST, ACCEL_CURVE_ROBUST, CURVE_DT, NODE_DT, ROBUST

HOST = "gpu=none,hair_accel=default"
BEZIER, BSPLINE = 25, 33
ERRFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)


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


def _hair(n=40, seed=3):
    """n curves with four vertices of their own: (verts4, first_index)"""
    v, idx, _, _ = ch.hair_and_rays(n, 1, seed)
    return v, idx


# ---- 1. the types, and what stays refused ------------------------------------------------------------------------------------------------
def test_the_flat_cubic_types_are_taken_and_round_curves_and_user_geometry_stay_refused(rtc):
    dev = rtc.Device(HOST)
    err = Errors(dev)
    for t in (BEZIER, BSPLINE):
        g = dev.lib.rtcNewGeometry(dev.handle, t)
        assert g and dev.error() == rtc.RTC_ERROR_NONE
        dev.lib.rtcReleaseGeometry(g)
    for t in (24, 32):  # ROUND_BEZIER, ROUND_BSPLINE
        assert not dev.lib.rtcNewGeometry(dev.handle, t)
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "RTC_GEOMETRY_TYPE_*_CURVE not supported")
    assert not dev.lib.rtcNewGeometry(dev.handle, 120)  # RTC_GEOMETRY_TYPE_USER
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "RTC_GEOMETRY_TYPE_USER not supported")
    assert dev.get_property(99) == 0  # RTC_DEVICE_PROPERTY_CURVE_GEOMETRY_SUPPORTED speaks for all five curve types
    dev.release()


def test_a_host_only_device_without_the_key_refuses_as_before(rtc):
    dev = rtc.Device("gpu=none")
    err = Errors(dev)
    for t in (BEZIER, BSPLINE):
        assert not dev.lib.rtcNewGeometry(dev.handle, t)
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "RTC_GEOMETRY_TYPE_*_CURVE not supported")
    dev.release()


@pytest.mark.parametrize("gtype", [BEZIER, BSPLINE])
def test_buffer_formats(rtc, gtype):
    dev = rtc.Device(HOST)
    lib = dev.lib
    g = lib.rtcNewGeometry(dev.handle, gtype)
    vb = np.zeros((8, 4), np.float32)
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


# ---- 2. validity, rate, conversion -------------------------------------------------------------------------------------------------------
def test_invalid_curves_get_no_record_and_keep_their_prim_ids(rtc):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    v = np.zeros((14, 4), np.float32)
    v[:, 0] = np.arange(14)
    v[:, 3] = 0.1
    v[5, 1] = np.nan   # curves 2..5 use vertex 5
    v[12, 3] = -0.1    # curves 9, 10 use vertex 12 (curve 10: 10..13)
    idx = np.array([0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 12], np.uint32)
    #               ok ok NaN NaN ok ok ok neg neg  index + 3 == nv: out of range   index + 3 > nv
    sc.add_curves(v, idx, flags=np.arange(len(idx)) % 2)
    sc.commit()
    rec = sc.accel_data(2).view(CURVE_DT)
    assert sorted(rec["primID"].tolist()) == [0, 1, 4, 5, 6]
    assert sc.stats()["primCount"] == 5 and sc.stats()["primBytes"] == 80
    sc.release()
    # a radius of zero and an infinite coordinate
    sc = rtc.Scene(dev)
    v = np.zeros((8, 4), np.float32)
    v[:, 0] = np.arange(8)
    v[7, 2] = np.inf
    sc.add_curves(v, np.array([0, 4], np.uint32))
    sc.commit()
    assert sc.accel_data(2).view(CURVE_DT)["primID"].tolist() == [0]
    sc.release()
    dev.release()


@pytest.mark.parametrize("rate,N", [(None, 4), (0.5, 1), (4.9, 4), (17, 16), (1, 1), (16, 16), (-3, 1)])
def test_the_tessellation_rate_is_clamped_at_commit(rtc, rate, N):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    v, idx = _hair(5)
    sc.add_curves(v, idx, tessellation_rate=rate)
    sc.commit()
    assert (sc.accel_data(2).view(CURVE_DT)["N"] == N).all()
    sc.release()
    dev.release()


def test_bspline_curves_are_converted_with_the_float32_madd_sequence(rtc):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    rng = np.random.default_rng(7)
    v = np.concatenate([rng.normal(size=(43, 3)) * 3, rng.uniform(0.01, 0.2, (43, 1))], 1).astype(np.float32)
    idx = np.arange(40, dtype=np.uint32)  # consecutive curves share three control points in the user's buffer
    sc.add_curves(v, idx, basis="bspline", geom_id=2)
    sc.commit()
    rec = sc.accel_data(2).view(CURVE_DT)
    rec = rec[np.argsort(rec["primID"])]
    want = ch.native(v, idx, "bspline")
    assert rec["v"].tobytes() == want.tobytes()  # bit-equal: four native points of its own per curve
    # and the conversion is right: both curves are the same function of u
    cp = ch.control_points(v, idx).astype(np.float64)
    for u in (0.0, 0.3, 1.0):
        b = ch.bspline_basis64(u)[0]
        p = sum(b[k] * cp[:, k] for k in range(4))
        q = ch.combine([x for x in ch.bezier_basis(u, np.float64)], *(want[:, k].astype(np.float64) for k in range(4)), np.float64)
        assert np.abs(p - q).max() <= 1e-5
    sc.release()
    dev.release()


# ---- 3. accel names and kinds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "bvh4.bezier1v", "bvh4.bezier1i", "bvh4obb.bezier1v", "bvh4obb.bezier1i", "bvh8obb.bezier1v", "bvh8obb.bezier1i"])
@pytest.mark.parametrize("flags,kind", [(0, ACCEL_CURVE_FAST), (ROBUST, ACCEL_CURVE_ROBUST)])
def test_every_hair_accel_name_builds_the_one_accel(rtc, name, flags, kind):
    dev = rtc.Device("gpu=none,hair_accel=" + name)
    sc = rtc.Scene(dev, flags)
    v, idx = _hair()
    sc.add_curves(v, idx)
    sc.commit()
    st = sc.stats()
    assert st["accelKind"] == kind and st["primCount"] == len(idx) and st["primBytes"] == 80 and st["nodeBytes"] == 96
    assert st["totalBytes"] == st["nodeCount"] * 96 + len(idx) * 80
    sc.release()
    dev.release()


def test_unknown_hair_accel_is_an_invalid_argument(rtc):
    dev = rtc.Device("gpu=none,hair_accel=bvh8.bezier1v")
    err = Errors(dev)
    sc = rtc.Scene(dev)
    v, idx = _hair(2)
    sc.add_curves(v, idx)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_ARGUMENT, "unknown hair acceleration structure bvh8.bezier1v")
    dev.release()


def test_curves_are_described_in_front_of_lines_and_instances_and_behind_meshes(rtc):
    dev = rtc.Device(HOST + ",quad_accel=default,inst_accel=default")
    v, idx = _hair(4)
    lv = np.array([[0, 0, 0, .1], [1, 0, 0, .1]], np.float32)
    tv = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    tri = np.array([[0, 1, 2]], np.uint32)
    inner = rtc.Scene(dev)
    inner.add_triangles(tv, tri)
    inner.commit()
    kinds = {}
    for parts in ("t", "c", "l", "i", "tc", "cl", "ci"):
        sc = rtc.Scene(dev)
        if "t" in parts:
            sc.add_triangles(tv, tri)
        if "c" in parts:
            sc.add_curves(v, idx)
        if "l" in parts:
            sc.add_lines(lv, np.array([0], np.uint32))
        if "i" in parts:
            sc.add_instance(inner)
        sc.commit()
        kinds[parts] = (sc.stats()["accelKind"], sc.stats()["totalBytes"])
        sc.release()
    assert kinds["t"][0] == 2 and kinds["tc"][0] == 2 and kinds["l"][0] == 37 and kinds["i"][0] == 15  # as before
    assert kinds["c"][0] == ACCEL_CURVE_FAST and kinds["cl"][0] == ACCEL_CURVE_FAST and kinds["ci"][0] == ACCEL_CURVE_FAST
    for a, b in (("t", "c"), ("c", "l"), ("c", "i")):
        assert kinds[a + b][1] == kinds[a][1] + kinds[b][1]
    inner.release()
    dev.release()


# ---- 4. records and tree ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, ROBUST])
@pytest.mark.parametrize("basis,rate", [("bezier", None), ("bezier", 9), ("bspline", 3)])
def test_records_hold_the_native_points_and_every_box_lies_inside_its_path(rtc, flags, basis, rate):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev, flags)
    v, idx = _hair(300)
    sc.add_curves(v, idx, basis=basis, tessellation_rate=rate, geom_id=3)
    sc.commit()
    rec = sc.accel_data(2).view(CURVE_DT)
    nodes = sc.accel_data(0).view(NODE_DT)
    N = 4 if rate is None else rate
    assert len(rec) == len(idx) and sorted(rec["primID"].tolist()) == list(range(len(idx))) and (rec["geomID"] == 3).all()
    assert (rec["pad"] == 0).all() and (rec["N"] == N).all()
    want = ch.native(v, idx, basis)
    assert np.array_equal(rec["v"], want[rec["primID"]])
    blo, bhi = ch.curve_box(rec)
    seen, leaves = 0, 0
    for path, first, count in ch.walk_paths(nodes, sc.accel_root()):
        assert 1 <= count <= 28
        leaves += 1
        seen += count
        for k in range(first, first + count):
            for n, i in path:  # every node box on the way down, decoded as the kernel decodes it
                clo, chi = ch.decode_children(nodes[n])
                assert (clo[i] <= blo[k]).all() and (chi[i] >= bhi[k]).all(), (n, i, rec["primID"][k])
    assert seen == len(rec) and leaves == sc.stats()["leafCount"]
    lo, hi = sc.bounds()
    assert np.array_equal(lo, blo.min(0)) and np.array_equal(hi, bhi.max(0))
    # the box holds every corner of every ribbon quad whatever the ray: all tessellation points, each with its radius around it
    p64 = want.astype(np.float64)
    for j in range(N + 1):
        b = ch.bezier_basis(j / N, np.float64)
        p = sum(b[k] * p64[:, k] for k in range(4))[rec["primID"]]
        assert (blo <= p[:, :3] - p[:, 3:] + 1e-6).all() and (bhi >= p[:, :3] + p[:, 3:] - 1e-6).all()
    sc.release()
    dev.release()


def test_two_geometries_carry_their_own_rate_in_the_records(rtc):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    v, idx = _hair(30)
    a = sc.add_curves(v, idx[:15], tessellation_rate=3)
    b = sc.add_curves(v, idx[15:], basis="bspline", tessellation_rate=9)
    sc.commit()
    rec = sc.accel_data(2).view(CURVE_DT)
    assert len(rec) == 30 and (rec["N"][rec["geomID"] == a] == 3).all() and (rec["N"][rec["geomID"] == b] == 9).all()
    # a disabled geometry leaves no records
    sc.set_enabled(a, False)
    sc.set_enabled(b, False)
    sc.commit()
    assert sc.stats()["accelKind"] == 0 and len(sc.accel_data(2)) == 0
    sc.release()
    dev.release()


# ---- 5. commit refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis", ["bezier", "bspline"])
def test_time_steps_are_refused_at_commit(rtc, basis):
    dev = rtc.Device(HOST)
    err = Errors(dev)
    sc = rtc.Scene(dev)
    v, idx = _hair(2)
    gid = sc.add_curves(v, idx, basis=basis)
    g = dev.lib.rtcGetGeometry(sc.handle, gid)
    dev.lib.rtcSetGeometryTimeStepCount(g, 2)
    assert dev.error() == rtc.RTC_ERROR_NONE
    dev.lib.rtcCommitGeometry(g)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "motion blur of flat Bezier and B-spline curves is not supported")
    dev.release()


@pytest.mark.parametrize("cfg", [HOST, HOST + ",quad_accel=default,inst_accel=default"])
def test_curves_in_an_instanced_scene_are_refused(rtc, cfg):
    dev = rtc.Device(cfg)
    err = Errors(dev)
    inner = rtc.Scene(dev)
    inner.add_triangles(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    v, idx = _hair(2)
    curves = inner.add_curves(v, idx)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance(inner)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "flat Bezier and B-spline curves inside an instanced scene are not supported")
    inner.set_enabled(curves, False)  # disabled, the curve geometry does not count
    inner.commit()
    top.commit()
    assert top.stats()["accelKind"] in (14, 15, 16, 17)
    dev.release()


# ---- 6. rtcInterpolate --------------------------------------------------------------------------------------------------------------------
def _basis64(basis, u):
    if basis == "bspline":
        return ch.bspline_basis64(u)
    return ch.bezier_basis(u, np.float64), ch.bezier_derivative(u, np.float64), ch.bezier_derivative2(u, np.float64)


def _strand(rtc, dev, basis):
    sc = rtc.Scene(dev)
    rng = np.random.default_rng(11)
    v = np.concatenate([rng.normal(size=(6, 3)), rng.uniform(0.1, 0.5, (6, 1))], 1).astype(np.float32)
    gid = sc.add_curves(v, np.array([0, 2], np.uint32), basis=basis)
    attr = rng.normal(size=(6, 2)).astype(np.float32)
    sc.set_vertex_attribute(gid, 1, attr)
    return sc, gid, v, attr


@pytest.mark.parametrize("basis", ["bezier", "bspline"])
def test_interpolate_evaluates_the_geometrys_own_basis(rtc, basis):
    dev = rtc.Device(HOST)
    sc, gid, v, attr = _strand(rtc, dev, basis)
    for prim, u in ((0, 0.0), (0, 0.25), (0, 1.0), (1, 0.5), (1, 0.8125)):
        b, d, dd = _basis64(basis, u)
        for buf, slot, src, count in ((None, 0, v, 4), (rtc.RTC_BUFFER_TYPE_VERTEX_ATTRIBUTE, 1, attr, 2)):
            c = src[2 * prim:2 * prim + 4].astype(np.float64)
            kw = {} if buf is None else {"buffer_type": buf, "slot": slot}
            P, du, dv, duu, dvv, duv = sc.interpolate(gid, prim, u, 0.375, count=count, **kw)
            for got, w in ((P, b), (du, d), (duu, dd)):
                assert np.abs(got - sum(w[k] * c[k] for k in range(4))).max() <= 2e-5, (prim, u, got)
            assert not dv.any() and not dvv.any() and not duv.any()
    if basis == "bezier":  # the end points of a Bezier curve are its first and last control point
        assert np.array_equal(sc.interpolate(gid, 1, 0.0, 0.0, count=4, derivs=0)[0], v[2])
        assert np.array_equal(sc.interpolate(gid, 1, 1.0, 0.0, count=4, derivs=0)[0], v[5])
    sc.lib.rtcCommitScene(sc.handle)  # (committing the scene changes nothing for rtcInterpolate)
    with pytest.raises(rtc.RTCError):
        sc.interpolate(gid, 2, 0.5, 0.0)  # an invalid primID is an error
    sc.release()
    dev.release()


@pytest.mark.parametrize("basis", ["bezier", "bspline"])
def test_interpolateN_honours_the_valid_mask(rtc, basis):
    dev = rtc.Device(HOST)
    sc, gid, v, attr = _strand(rtc, dev, basis)
    prim = np.array([0, 1, 0, 1], np.uint32)
    u = np.array([0.5, 0.25, 0.75, 1.0], np.float32)
    P, du, dv = sc.interpolateN(gid, prim, u, np.zeros(4, np.float32), count=4, valid=[-1, 0, -1, -1])
    for i in range(4):
        b, d, _ = _basis64(basis, float(u[i]))
        c = v[2 * prim[i]:2 * prim[i] + 4].astype(np.float64)
        if i == 1:
            assert not P[:, i].any() and not du[:, i].any()  # masked out: untouched
        else:
            assert np.abs(P[:, i] - sum(b[k] * c[k] for k in range(4))).max() <= 2e-5
            assert np.abs(du[:, i] - sum(d[k] * c[k] for k in range(4))).max() <= 2e-5 and not dv[:, i].any()
    sc.release()
    dev.release()


# ---- 7. the truth's two arithmetics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 4, 8, 9, 16])
def test_float32_restatement_agrees_with_the_float64_truth_on_the_pinned_hair(N):
    """The GPU parity test leaves a ray out only where the float64 truth has a segment with |max(U, V) / den| <= 1e-4 (an edge of a ribbon
    quad) or its two nearest candidates within 1e-4 relative in t, at most 0.5 % of the rays (tests/test_gpu_curves.py).  On the pinned
    hair the reference arithmetic in float32 stays inside that: same hits and IDs on the rays kept, t, u and v inside the 1e-4 contract.
    Measured (hits of 2048 rays / rays left out / t relative / u / v):  N 1: 932 / 0 / 4.4e-7 / 9.8e-6 / 3.8e-5;  N 3: 1072 / 3 / 3.5e-7 /
    1.2e-5 / 3.0e-5;  N 4: 1078 / 0 / 1.5e-6 / 3.1e-5 / 2.2e-5;  N 8: 1087 / 0 / 3.8e-7 / 6.8e-6 / 2.4e-5;  N 9: 1086 / 0 / 1.1e-6 / 1.1e-5 /
    2.5e-5;  N 16: 1091 / 3 / 5.8e-7 / 5.0e-5 / 3.4e-5; no hit or ID difference at any rate."""
    v, idx, org, dirs = ch.hair_and_rays()
    m = len(org)
    a = ch.hair_truth(N)
    b = ch.closest([(ch.native(v, idx), N, 0)], org, dirs, np.zeros(m, np.float32), np.full(m, np.inf, np.float32), np.float32)
    assert int(a["hit"].sum()) == ch.HAIR_HITS[N]
    out, _, _, _ = ch.compare(b["hit"], b["geomID"], b["primID"], b["t"], b["u"], b["v"], a, "float32 against float64, N = %d" % N)
    assert out == ch.HAIR_LEFT_OUT[N] and out <= 0.005 * m
