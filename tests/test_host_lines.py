"""CPU tests of line segments (RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE) on a `gpu=none` device: the type and what stays refused, buffer
formats, segment validity, line_accel= names, accel kinds, the LineRecords and the BVH8 over them, commit refusals, rtcInterpolate /
rtcInterpolateN (LineSegments::interpolate, scene_line_segments.cpp:228-263), and the float32 restatement of the intersector against its
float64 truth on the pinned tuft of tests/test_gpu_lines.py."""
import ctypes as C

import numpy as np
import pytest

import line_helpers as lh
from line_helpers import ACCEL_LINE_FAST, ACCEL_LINE_ROBUST, LINE_DT, NODE_DT, ROBUST

HOST = "gpu=none"
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


def _strands(n_strands=40, per=9, seed=3):
    """n_strands polylines of `per` vertices: (verts4, first_index) with per - 1 segments each that share vertices"""
    rng = np.random.RandomState(seed)
    v, idx = [], []
    for s in range(n_strands):
        p = rng.rand(3) * 4
        for k in range(per):
            if k + 1 < per:
                idx.append(len(v))
            v.append((*p, 0.01 + 0.02 * rng.rand()))
            p = p + (rng.rand(3) - 0.5) * 0.4
    return np.array(v, np.float32), np.array(idx, np.uint32)


# ---- 1. the type, and what stays refused --------------------------------------------------------------------------------------------------
def test_flat_linear_curves_are_taken_and_every_other_curve_type_stays_refused(rtc):
    dev = rtc.Device(HOST)
    err = Errors(dev)
    g = dev.lib.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE)
    assert g and dev.error() == rtc.RTC_ERROR_NONE
    dev.lib.rtcReleaseGeometry(g)
    for t in (24, 25, 32, 33):  # ROUND_BEZIER, FLAT_BEZIER, ROUND_BSPLINE, FLAT_BSPLINE
        assert not dev.lib.rtcNewGeometry(dev.handle, t)
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "RTC_GEOMETRY_TYPE_*_CURVE not supported")
    assert not dev.lib.rtcNewGeometry(dev.handle, 120)  # RTC_GEOMETRY_TYPE_USER
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "RTC_GEOMETRY_TYPE_USER not supported")
    assert dev.get_property(99) == 0  # RTC_DEVICE_PROPERTY_CURVE_GEOMETRY_SUPPORTED speaks for all five curve types
    dev.release()


def test_buffer_formats(rtc):
    dev = rtc.Device(HOST)
    lib = dev.lib
    g = lib.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE)
    vb = np.zeros((4, 4), np.float32)
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0, rtc.RTC_FORMAT_FLOAT3, vb.ctypes.data, 0, 16, 4)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION  # vertices are (x, y, z, radius)
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0, rtc.RTC_FORMAT_FLOAT4, vb.ctypes.data, 0, 16, 4)
    assert dev.error() == rtc.RTC_ERROR_NONE
    ib = np.zeros(3, np.uint32)
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_INDEX, 0, rtc.RTC_FORMAT_UINT3, ib.ctypes.data, 0, 4, 1)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION  # one word per segment
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_INDEX, 0, rtc.RTC_FORMAT_UINT, ib.ctypes.data, 0, 4, 3)
    assert dev.error() == rtc.RTC_ERROR_NONE
    fb = np.zeros(3, np.uint8)
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_FLAGS, 0, rtc.RTC_FORMAT_UINT, fb.ctypes.data, 0, 1, 3)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION
    lib.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_FLAGS, 0, rtc.RTC_FORMAT_UCHAR, fb.ctypes.data, 0, 1, 3)
    assert dev.error() == rtc.RTC_ERROR_NONE
    assert lib.rtcGetGeometryBufferData(g, rtc.RTC_BUFFER_TYPE_FLAGS, 0) == fb.ctypes.data
    assert lib.rtcGetGeometryBufferData(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0) == vb.ctypes.data
    # an owned buffer
    p = lib.rtcSetNewGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0, rtc.RTC_FORMAT_FLOAT4, 16, 8)
    assert p and dev.error() == rtc.RTC_ERROR_NONE and lib.rtcGetGeometryBufferData(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0) == p
    lib.rtcReleaseGeometry(g)
    dev.release()


# ---- 2. validity ----------------------------------------------------------------------------------------------------------------------------
def test_invalid_segments_get_no_record_and_a_zero_length_segment_gets_one(rtc):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    v = np.array([[0, 0, 0, .1], [1, 0, 0, .1], [2, 0, 0, .1], [np.nan, 0, 0, .1], [4, 0, 0, .1], [5, 0, 0, -.1], [6, 0, 0, .1],
                  [7, 0, 0, .1], [7, 0, 0, .2], [8, 0, 0, np.inf], [9, 0, 0, .1], [9, 1, 0, 0.0]], np.float32)
    #        0 ok  1 ok  2 NaN end  3 NaN start  4 negative radius at its end  5 negative radius at its start  6 ok  7 zero length: ok
    #        8 infinite radius at its end  9 at its start  10 ok (radius 0 is >= 0)  11 index at the last vertex
    idx = np.arange(12, dtype=np.uint32)
    sc.add_lines(v, idx, flags=np.arange(12) % 2)
    sc.commit()
    rec = sc.accel_data(2).view(LINE_DT)
    assert sorted(rec["primID"].tolist()) == [0, 1, 6, 7, 10]
    assert sc.stats()["primCount"] == 5 and sc.stats()["primBytes"] == 48
    z = rec[rec["primID"] == 7][0]
    assert np.array_equal(z["v0"], z["v1"])
    lo, hi = sc.bounds()
    assert np.allclose(lo, [-0.1, -0.2, -0.2]) and np.allclose(hi, [9.1, 1.1, 0.2])  # the enlarged boxes of the valid segments only (segment 7: radius 0.2)
    sc.release()
    dev.release()


# ---- 3. accel names and kinds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["", "line_accel=default", "line_accel=bvh8.line4i", "line_accel=bvh4.line4i"])
@pytest.mark.parametrize("flags,kind", [(0, ACCEL_LINE_FAST), (ROBUST, ACCEL_LINE_ROBUST)])
def test_every_line_accel_name_builds_the_one_accel(rtc, name, flags, kind):
    dev = rtc.Device(HOST + "," + name)
    sc = rtc.Scene(dev, flags)
    v, idx = _strands()
    sc.add_lines(v, idx)
    sc.commit()
    st = sc.stats()
    assert st["accelKind"] == kind and st["primCount"] == len(idx) and st["primBytes"] == 48 and st["nodeBytes"] == 96
    assert st["totalBytes"] == st["nodeCount"] * 96 + len(idx) * 48
    sc.release()
    dev.release()


def test_unknown_line_accel_is_an_invalid_argument(rtc):
    dev = rtc.Device("gpu=none,line_accel=bvh8.line8i")
    err = Errors(dev)
    sc = rtc.Scene(dev)
    v, idx = _strands(2)
    sc.add_lines(v, idx)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_ARGUMENT, "unknown line segment acceleration structure bvh8.line8i")
    dev.release()


def test_scenes_that_exist_today_answer_as_before_and_lines_come_before_instances(rtc):
    dev = rtc.Device("gpu=none,quad_accel=default,inst_accel=default")
    v, idx = _strands(4)
    tv = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    tri = np.array([[0, 1, 2]], np.uint32)
    inner = rtc.Scene(dev)
    inner.add_triangles(tv, tri)
    inner.commit()
    kinds = {}
    for parts in ("t", "l", "tl", "li", "i"):
        sc = rtc.Scene(dev)
        if "t" in parts:
            sc.add_triangles(tv, tri)
        if "l" in parts:
            sc.add_lines(v, idx)
        if "i" in parts:
            sc.add_instance(inner)
        sc.commit()
        kinds[parts] = (sc.stats()["accelKind"], sc.stats()["totalBytes"])
        sc.release()
    assert kinds["t"][0] == 2 and kinds["tl"][0] == 2          # the triangle accel is described when there is one
    assert kinds["l"][0] == ACCEL_LINE_FAST and kinds["li"][0] == ACCEL_LINE_FAST  # a top scene with lines of its own beside instances
    assert kinds["i"][0] == 15                                  # ACCEL_INST_TRI_MOELLER, as before
    assert kinds["tl"][1] == kinds["t"][1] + kinds["l"][1] and kinds["li"][1] == kinds["l"][1] + kinds["i"][1]
    inner.release()
    dev.release()


# ---- 4. records and tree ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, ROBUST])
def test_records_hold_the_input_and_every_box_lies_inside_its_path(rtc, flags):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev, flags)
    v, idx = _strands(60, 9)
    sc.add_lines(v, idx, geom_id=3)
    sc.commit()
    rec = sc.accel_data(2).view(LINE_DT)
    nodes = sc.accel_data(0).view(NODE_DT)
    assert len(rec) == len(idx) and sorted(rec["primID"].tolist()) == list(range(len(idx))) and (rec["geomID"] == 3).all()
    assert (rec["pad"] == 0).all()
    for r in rec:  # the pre-gathered vertices of segment primID
        a, b = v[idx[r["primID"]]], v[idx[r["primID"]] + 1]
        assert np.array_equal(r["v0"], a[:3]) and r["r0"] == a[3] and np.array_equal(r["v1"], b[:3]) and r["r1"] == b[3]
    seen, leaves = 0, 0
    for path, first, count in lh.walk_paths(nodes, sc.accel_root()):
        assert 1 <= count <= lh.LEAF_MAX
        leaves += 1
        seen += count
        for r in rec[first:first + count]:
            lo, hi = lh.segment_box(r)
            for n, i in path:  # every node box on the way down, decoded as the kernel decodes it
                clo, chi = lh.decode_children(nodes[n])
                assert (clo[i] <= lo).all() and (chi[i] >= hi).all(), (n, i, r["primID"])
    assert seen == len(rec) and leaves == sc.stats()["leafCount"]
    lo, hi = sc.bounds()
    blo, bhi = zip(*(lh.segment_box(r) for r in rec))
    assert np.array_equal(lo, np.min(blo, 0)) and np.array_equal(hi, np.max(bhi, 0))
    sc.release()
    dev.release()


def test_disabled_line_geometry_leaves_no_accel_and_update_is_seen(rtc):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    v, idx = _strands(3)
    gid = sc.add_lines(v, idx)
    sc.commit()
    assert sc.stats()["accelKind"] == ACCEL_LINE_FAST
    g = dev.lib.rtcGetGeometry(sc.handle, gid)
    dev.lib.rtcSetGeometryMask(g, 0xF)
    sc.set_user_data(gid, 0x1234)
    assert dev.lib.rtcGetGeometryUserData(g) == 0x1234
    # the shared vertex buffer changes: rtcUpdateGeometryBuffer + commits
    keep = [a for a in sc._keep if a.dtype == np.float32][0]
    keep[:, :3] += 10
    dev.lib.rtcUpdateGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0)
    dev.lib.rtcCommitGeometry(g)
    sc.commit()
    assert sc.bounds()[0].min() > 9
    sc.set_enabled(gid, False)
    sc.commit()
    assert sc.stats()["accelKind"] == 0 and len(sc.accel_data(2)) == 0
    sc.release()
    dev.release()


# ---- 5. commit refusals -------------------------------------------------------------------------------------------------------------------------
def test_time_steps_are_accepted_and_refused_at_commit(rtc):
    dev = rtc.Device(HOST)
    err = Errors(dev)
    sc = rtc.Scene(dev)
    v, idx = _strands(2)
    gid = sc.add_lines(v, idx)
    g = dev.lib.rtcGetGeometry(sc.handle, gid)
    dev.lib.rtcSetGeometryTimeStepCount(g, 2)
    assert dev.error() == rtc.RTC_ERROR_NONE
    dev.lib.rtcCommitGeometry(g)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "motion blur of line segments is not supported")
    dev.release()


@pytest.mark.parametrize("cfg,text", [("gpu=none", "static triangle meshes only"),
                                      ("gpu=none,quad_accel=default,inst_accel=default", "static triangle and quad meshes only"),
                                      ("gpu=none,quad_accel=default,tri_accel_mb=default,inst_accel=default", "triangle and quad meshes only")])
def test_lines_below_an_instance_are_refused(rtc, cfg, text):
    dev = rtc.Device(cfg)
    err = Errors(dev)
    inner = rtc.Scene(dev)
    inner.add_triangles(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    v, idx = _strands(2)
    lines = inner.add_lines(v, idx)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance(inner)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "an instanced scene may hold " + text)
    # disabled, the line geometry does not count
    inner.set_enabled(lines, False)
    inner.commit()
    top.commit()
    assert top.stats()["accelKind"] in (14, 15, 16, 17, 22, 23)
    dev.release()


# ---- 6. rtcInterpolate --------------------------------------------------------------------------------------------------------------------------
def _strand3(rtc, dev):
    sc = rtc.Scene(dev)
    v = np.array([[0, 0, 0, 0.5], [2, 4, -8, 0.25], [3, 4, 0, 1.0]], np.float32)
    gid = sc.add_lines(v, np.array([0, 1], np.uint32))
    attr = np.array([[1, 16], [5, 0], [-3, 8]], np.float32)
    sc.set_vertex_attribute(gid, 1, attr)
    return sc, gid, v, attr


def test_interpolate_closed_forms(rtc):
    dev = rtc.Device(HOST)
    sc, gid, v, attr = _strand3(rtc, dev)
    for prim, u in ((0, 0.0), (0, 0.25), (0, 1.0), (1, 0.5), (1, 0.75)):
        for vv in (0.0, 0.625):  # v is ignored
            P, du, dv, duu, dvv, duv = sc.interpolate(gid, prim, u, vv, count=4)
            a, b = v[prim], v[prim + 1]
            assert np.array_equal(P, (1 - u) * a + u * b) and np.array_equal(du, b - a)
            assert not dv.any() and not duu.any() and not dvv.any() and not duv.any()
            P, du, dv, duu, dvv, duv = sc.interpolate(gid, prim, u, vv, buffer_type=rtc.RTC_BUFFER_TYPE_VERTEX_ATTRIBUTE, slot=1, count=2)
            a, b = attr[prim], attr[prim + 1]
            assert np.array_equal(P, (1 - u) * a + u * b) and np.array_equal(du, b - a) and not dv.any() and not duu.any()
    sc.lib.rtcCommitScene(sc.handle)  # (committing the scene changes nothing for rtcInterpolate)
    assert np.array_equal(sc.interpolate(gid, 1, 0.5, 0.0, count=3, derivs=0)[0], [2.5, 4, -4])
    # an invalid primID is an error
    with pytest.raises(rtc.RTCError):
        sc.interpolate(gid, 2, 0.5, 0.0)
    sc.release()
    dev.release()


def test_interpolateN_honours_the_valid_mask(rtc):
    dev = rtc.Device(HOST)
    sc, gid, v, attr = _strand3(rtc, dev)
    prim = np.array([0, 1, 0, 1], np.uint32)
    u = np.array([0.5, 0.25, 0.75, 1.0], np.float32)
    P, du, dv = sc.interpolateN(gid, prim, u, np.zeros(4, np.float32), count=4, valid=[-1, 0, -1, -1])
    for i in range(4):
        a, b = v[prim[i]], v[prim[i] + 1]
        if i == 1:
            assert not P[:, i].any() and not du[:, i].any()  # masked out: untouched
        else:
            assert np.array_equal(P[:, i], (1 - u[i]) * a + u[i] * b) and np.array_equal(du[:, i], b - a) and not dv[:, i].any()
    sc.release()
    dev.release()


# ---- 7. the truth's two arithmetics ----------------------------------------------------------------------------------------------------------------
def test_float32_restatement_agrees_with_the_float64_truth_on_the_pinned_tuft():
    """The GPU parity test leaves a ray out only where the float64 truth is within 1e-4 of a decision (tests/test_gpu_lines.py).  On the
    pinned tuft the reference arithmetic in float32 needs none of that: same hits and IDs, t and u far inside the 1e-4 contract, no ray
    near a decision.  Measured: 3239 hits of 4096, 0 differing IDs, t to 5.3e-7 relative, u to 1.2e-5 absolute, 0 rays left out."""
    v, idx, org, dirs = lh.tuft_and_rays()
    v0, v1 = lh.ends(v, idx)
    m = len(org)
    tn, tf = np.zeros(m, np.float32), np.full(m, np.inf, np.float32)
    a, b = lh.closest(v0, v1, org, dirs, tn, tf, np.float64), lh.closest(v0, v1, org, dirs, tn, tf, np.float32)
    h = a["hit"]
    dt = float(np.max(np.abs(a["t"][h] - b["t"][h]) / np.abs(a["t"][h])))
    du = float(np.max(np.abs(a["u"][h] - b["u"][h])))
    out = int((a["near_edge"] | a["near_tie"]).sum())
    print(f"  {int(h.sum())} hits of {m}, {int((a['seg'][h] != b['seg'][h]).sum())} differing IDs, t to {dt:.3g} relative, u to {du:.3g}, {out} rays left out")
    assert int(h.sum()) == lh.TUFT_HITS and np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["seg"][h], b["seg"][h])
    assert dt <= 1e-4 and du <= 1e-4 and out == 0
