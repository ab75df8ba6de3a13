"""CPU tests of motion blur on flat Bezier and B-spline curves on a host-only device that names both hair accels
(`gpu=none,hair_accel=default,hair_accel_mb=default`): the key's names, what stays refused, the kinds 44..47, the 160-byte CurveMBRecords,
containment of the interpolated ribbon in the swept and in the time-dependent node boxes on every root-to-leaf path, a host walk of the
tree in the kernel's float32 arithmetic against the float64 truth on the pinned moving hair of tests/test_gpu_curve_motion_blur.py,
rtcInterpolate on a later time step, rtcGetSceneBounds, and the accels of the other builders of the generalised motion-blur frame, byte
for byte what the parent commit built."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import curve_helpers as ch
import curve_mb_helpers as mh
from curve_helpers import NODE_DT, ROBUST
from curve_mb_helpers import ACCEL_CURVEMB_FAST, ACCEL_CURVEMB_LINEAR_FAST, ACCEL_CURVEMB_LINEAR_ROBUST, ACCEL_CURVEMB_ROBUST, CURVEMB_DT
from mb_linear_helpers import NODEMB_DT, decode_nodes_mb, walk_paths

HOST = "gpu=none,hair_accel=default,hair_accel_mb=default"
ERRFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)
KIND = {(0, "swept"): ACCEL_CURVEMB_FAST, (ROBUST, "swept"): ACCEL_CURVEMB_ROBUST, (0, "linear"): ACCEL_CURVEMB_LINEAR_FAST, (ROBUST, "linear"): ACCEL_CURVEMB_LINEAR_ROBUST}


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


def _hair_steps(nsteps, n=40, seed=3):
    """n curves with four vertices of their own on a curved path with growing radii, coordinates and radii on multiples of 2^-16:
    ([nsteps arrays [4n, 4]], first_index)"""
    v, idx, _, _ = ch.hair_and_rays(n, 1, seed)
    v = v.astype(np.float64)
    steps = []
    for k in range(nsteps):
        xyz = v[:, :3] + np.array([0.75 * k, 0.1 * k * k, -0.3 * k]) + 0.05 * k * np.sin(v[:, :3] * 3.0)
        steps.append(np.concatenate([mh.snap16(xyz), mh.snap16(v[:, 3] * (1.0 + 0.25 * k))[:, None]], 1).astype(np.float32))
    return steps, idx


# ---- 1. keys and refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "bvh4.bezier1imb", "bvh8.bezier1imb"])
@pytest.mark.parametrize("flags,kind", [(0, ACCEL_CURVEMB_FAST), (ROBUST, ACCEL_CURVEMB_ROBUST)])
def test_every_name_of_the_key_builds_the_one_accel(rtc, name, flags, kind):
    dev = rtc.Device("gpu=none,hair_accel=default,hair_accel_mb=" + name)
    sc = rtc.Scene(dev, flags)
    steps, idx = _hair_steps(3)
    sc.add_curves_mb(steps, idx)
    sc.commit()
    st = sc.stats()
    assert st["accelKind"] == kind and st["primCount"] == 2 * len(idx) and st["primBytes"] == 160 and st["nodeBytes"] == 96
    assert st["totalBytes"] == st["nodeCount"] * 96 + 2 * len(idx) * 160
    sc.release()
    dev.release()


@pytest.mark.parametrize("flags,kind", [(0, ACCEL_CURVEMB_LINEAR_FAST), (ROBUST, ACCEL_CURVEMB_LINEAR_ROBUST)])
def test_linear_bounds_give_the_kinds_46_and_47_with_144_byte_nodes(rtc, flags, kind):
    dev = rtc.Device(HOST + ",mb_bounds=linear")
    sc = rtc.Scene(dev, flags)
    steps, idx = _hair_steps(2)
    sc.add_curves_mb(steps, idx)
    sc.commit()
    st = sc.stats()
    assert st["accelKind"] == kind and st["primCount"] == len(idx) and st["primBytes"] == 160 and st["nodeBytes"] == 144
    assert len(sc.accel_data(0)) == st["nodeCount"] * 144 and st["totalBytes"] == st["nodeCount"] * 144 + len(idx) * 160
    sc.release()
    dev.release()


def test_the_python_binding_has_the_four_kinds(rtc):
    assert (rtc.ACCEL_CURVEMB_ROBUST, rtc.ACCEL_CURVEMB_FAST, rtc.ACCEL_CURVEMB_LINEAR_ROBUST, rtc.ACCEL_CURVEMB_LINEAR_FAST) == (44, 45, 46, 47)


def test_unknown_name_is_an_invalid_argument(rtc):
    dev = rtc.Device("gpu=none,hair_accel=default,hair_accel_mb=bvh4obb.bezier1imb")
    err = Errors(dev)
    sc = rtc.Scene(dev)
    steps, idx = _hair_steps(2, 2)
    sc.add_curves_mb(steps, idx)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_ARGUMENT, "unknown motion blur hair acceleration structure bvh4obb.bezier1imb")
    dev.release()


@pytest.mark.parametrize("basis", ["bezier", "bspline"])
def test_without_the_key_a_host_only_device_refuses_as_before(rtc, basis):
    dev = rtc.Device("gpu=none,hair_accel=default")
    err = Errors(dev)
    sc = rtc.Scene(dev)
    steps, idx = _hair_steps(2, 2)
    sc.add_curves_mb(steps, idx, basis=basis)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "motion blur of flat Bezier and B-spline curves is not supported")
    dev.release()


def test_a_time_step_without_a_vertex_buffer_is_refused(rtc):
    dev = rtc.Device(HOST)
    err = Errors(dev)
    sc = rtc.Scene(dev)
    steps, idx = _hair_steps(2, 2)
    gid = sc.add_curves_mb(steps, idx)
    g = dev.lib.rtcGetGeometry(sc.handle, gid)
    dev.lib.rtcSetGeometryTimeStepCount(g, 3)  # step 2 has no buffer
    dev.lib.rtcCommitGeometry(g)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "motion blur geometry: a time step has no vertex buffer")
    dev.release()


@pytest.mark.parametrize("cfg", [HOST, HOST + ",quad_accel=default,tri_accel_mb=default,inst_accel=default"])
def test_moving_curves_in_an_instanced_scene_are_refused_with_the_message_of_static_ones(rtc, cfg):
    dev = rtc.Device(cfg)
    err = Errors(dev)
    inner = rtc.Scene(dev)
    inner.add_triangles(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    steps, idx = _hair_steps(2, 2)
    curves = inner.add_curves_mb(steps, idx)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance(inner)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "flat Bezier and B-spline curves inside an instanced scene are not supported")
    inner.set_enabled(curves, False)  # disabled, the curve geometry does not count
    inner.commit()
    top.commit()
    assert top.stats()["accelKind"] in (14, 15, 16, 17, 22, 23)
    dev.release()


def test_a_top_scene_may_hold_moving_curves_beside_instances(rtc):
    dev = rtc.Device(HOST + ",inst_accel=default")
    inner = rtc.Scene(dev)
    inner.add_triangles(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    inner.commit()
    steps, idx = _hair_steps(2, 4)
    kinds = {}
    for parts in ("c", "m", "cm", "ml", "mi"):
        sc = rtc.Scene(dev)
        if "c" in parts:
            sc.add_curves(steps[0], idx)
        if "m" in parts:
            sc.add_curves_mb(steps, idx)
        if "l" in parts:
            sc.add_lines(np.array([[0, 0, 0, .1], [1, 0, 0, .1]], np.float32), np.array([0], np.uint32))
        if "i" in parts:
            sc.add_instance(inner)
        sc.commit()
        kinds[parts] = (sc.stats()["accelKind"], sc.stats()["totalBytes"], sc.stats()["primBytes"])
        sc.release()
    assert kinds["c"][0] == 43 and kinds["m"][0] == ACCEL_CURVEMB_FAST and kinds["m"][2] == 160
    assert kinds["cm"][0] == 43 and kinds["cm"][1] == kinds["c"][1] + kinds["m"][1]  # both accels; the static one is described
    assert kinds["ml"][0] == ACCEL_CURVEMB_FAST and kinds["mi"][0] == ACCEL_CURVEMB_FAST  # in front of the line and instance accels
    inner.release()
    dev.release()


# ---- 2. records ---------------------------------------------------------------------------------------------------------------------
def test_the_record_is_160_bytes_laid_out_as_documented(rtc):
    """byte by byte: one curve, two steps, rate 9, every float a value of its own"""
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    s0 = np.arange(1, 17, dtype=np.float32).reshape(4, 4)
    s1 = np.arange(17, 33, dtype=np.float32).reshape(4, 4)
    sc.add_curves_mb([s0, s1], np.array([0], np.uint32), tessellation_rate=9, geom_id=6)
    sc.commit()
    raw = bytes(sc.accel_data(2))
    assert len(raw) == 160 and sc.accel_root() == (0x80000000 | (1 << 26))
    # the four points at step 0; the four at step 1; geomID, primID, segment, numSegments; N and three pad words
    want = np.arange(1, 33, dtype=np.float32).tobytes() + np.array([6, 0, 0, 1, 9, 0, 0, 0], np.uint32).tobytes()
    assert raw == want
    assert [CURVEMB_DT.fields[f][1] for f in CURVEMB_DT.names] == [0, 64, 128, 132, 136, 140, 144, 148]
    sc.release()
    dev.release()


@pytest.mark.parametrize("basis", ["bezier", "bspline"])
@pytest.mark.parametrize("nsteps,rate,N", [(2, None, 4), (4, 9, 9), (3, 40, 16)])
def test_records_hold_the_native_points_of_both_ends_of_their_time_segment(rtc, basis, nsteps, rate, N):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    steps, idx = _hair_steps(nsteps, 60)
    sc.add_curves_mb(steps, idx, basis=basis, tessellation_rate=rate, geom_id=3)
    sc.commit()
    raw = sc.accel_data(2)
    assert raw.dtype == np.uint8 and len(raw) == (nsteps - 1) * len(idx) * 160
    rec = raw.view(CURVEMB_DT)
    assert sc.stats()["primCount"] == len(rec) == (nsteps - 1) * len(idx)
    assert sorted(zip(rec["primID"].tolist(), rec["segment"].tolist())) == [(p, s) for p in range(len(idx)) for s in range(nsteps - 1)]
    assert (rec["geomID"] == 3).all() and (rec["numSegments"] == nsteps - 1).all() and (rec["N"] == N).all() and (rec["pad"] == 0).all()
    nat = mh.native_steps(steps, idx, basis)  # convert(BSplineCurveT, BezierCurveT) per time step, float32
    for s in range(nsteps - 1):
        sel = rec["segment"] == s
        assert np.array_equal(rec["va"][sel], nat[s][rec["primID"][sel]]) and np.array_equal(rec["vb"][sel], nat[s + 1][rec["primID"][sel]])
    sc.release()
    dev.release()


def test_a_curve_invalid_at_one_step_loses_the_adjacent_time_segments_only(rtc):
    """NativeCurves::valid(i, itime_range): 4 steps, curve 1 has a NaN vertex at step 1 and loses the segments 0 and 1, keeps segment 2;
    curve 2 has a negative radius at step 3 and loses segment 2; curve 3 starts too near the end of the buffer and is never valid"""
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    steps, _ = _hair_steps(4, 4)
    steps = [s[:15].copy() for s in steps]  # 15 vertices: curve 3 would need the vertices 12..15
    idx = np.array([0, 4, 8, 12], np.uint32)
    steps[1][6, 1] = np.nan
    steps[3][9, 3] = -0.25
    sc.add_curves_mb(steps, idx)
    sc.commit()
    rec = sc.accel_data(2).view(CURVEMB_DT)
    got = sorted(zip(rec["primID"].tolist(), rec["segment"].tolist()))
    assert got == [(0, 0), (0, 1), (0, 2), (1, 2), (2, 0), (2, 1)]
    assert sc.stats()["primCount"] == 6 and (rec["numSegments"] == 3).all()
    sc.release()
    dev.release()


def test_filter_flags_follow_the_static_curve_geometries(rtc):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    steps, idx = _hair_steps(2, 2)
    gid = sc.add_curves_mb(steps, idx)
    sc.commit()
    assert sc.filter_flags() == 0
    keep = rtc.FILTER_FUNC(lambda args: None)
    sc.set_filters(gid, intersect=keep, occluded=keep)
    sc.commit()
    assert sc.filter_flags() == rtc.RTCAMD_SCENE_FILTER_MESH_INTERSECT | rtc.RTCAMD_SCENE_FILTER_MESH_OCCLUDED
    sc.release()
    dev.release()


# ---- 3. containment -----------------------------------------------------------------------------------------------------------------
TIMES = np.linspace(0.0, 1.0, 17)


@pytest.mark.parametrize("N", [1, 4, 16])
@pytest.mark.parametrize("nsteps", [2, 5])
@pytest.mark.parametrize("bounds", ["swept", "linear"])
def test_the_interpolated_ribbon_lies_inside_every_node_box_on_its_path(rtc, bounds, nsteps, N):
    """At 17 times in [0, 1]: tessellated_bounds in float64 of the exactly interpolated control points of every record that accepts the
    time lies inside the decoded box of every node on the way down - the swept QNode8 boxes of the kinds 44 / 45, the QNodeMB8 boxes
    interpolated to that time with the node step's arithmetic in the kinds 46 / 47.  (The tessellation points and radii are linear in the
    control points; min is concave and max convex: the ribbon's box is inside the interpolated end boxes.)"""
    dev = rtc.Device(HOST + ",mb_bounds=" + bounds)
    sc = rtc.Scene(dev, ROBUST if N == 4 else 0)
    steps, idx = _hair_steps(nsteps, 150)
    sc.add_curves_mb(steps, idx, basis="bspline" if N == 16 else "bezier", tessellation_rate=N)
    sc.commit()
    linear = bounds == "linear"
    assert sc.stats()["accelKind"] == KIND[(ROBUST if N == 4 else 0, bounds)]
    nodes = sc.accel_data(0).view(NODEMB_DT if linear else NODE_DT)
    rec = sc.accel_data(2).view(CURVEMB_DT)
    assert len(rec) == (nsteps - 1) * len(idx) and (rec["N"] == N).all()
    paths = list(walk_paths(nodes, sc.accel_root()))
    assert sum(c for _, _, c in paths) == len(rec)
    static = None
    if not linear:
        lo8, hi8 = zip(*(ch.decode_children(n) for n in nodes))
        static = (np.array(lo8, np.float64), np.array(hi8, np.float64))
    slack = np.inf
    for t in TIMES:
        lo, hi, take = mh.record_box_at(rec, t)
        clo, chi = decode_nodes_mb(nodes, t)[:2] if linear else static
        for path, first, count in paths:
            sel = np.nonzero(take[first:first + count])[0] + first
            if not len(sel):
                continue
            for n, i in path:
                assert (clo[n, i] <= lo[sel]).all() and (chi[n, i] >= hi[sel]).all(), (n, i, t)
                slack = min(slack, float((lo[sel] - clo[n, i]).min()), float((chi[n, i] - hi[sel]).min()))
    print(f"  {bounds}, {nsteps} steps, N = {N}: smallest distance of a ribbon box from a node plane {slack:.3g}")
    # Scene::bounds holds the tessellated bounds of both ends of every record (the swept boxes, widened on the host)
    slo, shi = sc.bounds()
    ends = [ch.tessellated_bounds(rec[end], N, np.float64) for end in ("va", "vb")]
    lo, hi = np.minimum(ends[0][0].min(0), ends[1][0].min(0)), np.maximum(ends[0][1].max(0), ends[1][1].max(0))
    assert (slo <= lo).all() and (shi >= hi).all() and (lo - slo <= 1e-4).all() and (shi - hi <= 1e-4).all()
    sc.release()
    dev.release()


# ---- 4. a host walk of the tree -----------------------------------------------------------------------------------------------------
def _slab(lo, hi, org, dirs):
    """rays [m] against one box in float64: the ray's line segment [0, inf) meets the box"""
    with np.errstate(all="ignore"):
        inv = 1.0 / dirs
        t0, t1 = (lo - org) * inv, (hi - org) * inv
    near, far = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    return np.maximum(near, 0.0) <= far


@pytest.mark.parametrize("nsteps,N", [(2, 4), (5, 9)])
@pytest.mark.parametrize("bounds", ["swept", "linear"])
def test_a_host_walk_of_the_tree_meets_the_float64_truth_on_the_pinned_hair(rtc, bounds, nsteps, N):
    """Every ray of the pinned moving hair reaches the leaves whose node boxes, decoded at its time, it meets on the whole path; there the
    records of its time segment are interpolated and tested in the kernel's float32 arithmetic (curve_mb_helpers.interpolated_records,
    curve_helpers.candidates); the nearest candidate is held to the float64 truth under curve_helpers.compare."""
    truth = mh.hair_mb_truth(nsteps, N)
    assert int(truth["hit"].sum()) == mh.HAIR_MB_HITS[(nsteps, N)]
    assert int((truth["near_edge"] | truth["near_tie"]).sum()) == mh.HAIR_MB_LEFT_OUT[(nsteps, N)]
    dev = rtc.Device(HOST + ",mb_bounds=" + bounds)
    sc = rtc.Scene(dev)
    sc.add_curves_mb(truth["steps"], truth["idx"], tessellation_rate=N, geom_id=7)
    sc.commit()
    linear = bounds == "linear"
    nodes = sc.accel_data(0).view(NODEMB_DT if linear else NODE_DT)
    rec = sc.accel_data(2).view(CURVEMB_DT)
    paths = list(walk_paths(nodes, sc.accel_root()))
    org, dirs, times = truth["org"], truth["dirs"], truth["times"]
    m = len(org)
    o64, d64 = org.astype(np.float64), dirs.astype(np.float64)
    best = {k: np.full(m, v) for k, v in (("t", np.inf), ("u", 0.0), ("v", 0.0), ("prim", -1))}
    if not linear:
        lo8, hi8 = zip(*(ch.decode_children(n) for n in nodes))
        static = (np.array(lo8, np.float64), np.array(hi8, np.float64))
    for t in np.unique(times):
        rays = np.nonzero(times == t)[0]
        clo, chi = decode_nodes_mb(nodes, t)[:2] if linear else static
        cp, take = mh.interpolated_records(rec, t)
        for path, first, count in paths:
            sel = np.nonzero(take[first:first + count])[0] + first
            if not len(sel):
                continue
            reach = np.ones(len(rays), bool)
            for n, i in path:
                reach &= _slab(clo[n, i], chi[n, i], o64[rays], d64[rays])
            r = rays[reach]
            if not len(r):
                continue
            valid, T, U, V, _, _ = ch.candidates(cp[sel], N, org[r], dirs[r], np.zeros(len(r), np.float32), np.full(len(r), np.inf, np.float32), np.float32)
            tt = np.where(valid, T, np.inf).reshape(len(r), -1)
            k = tt.argmin(1)
            ar = np.arange(len(r))
            better = tt[ar, k] < best["t"][r]
            rb = r[better]
            best["t"][rb] = tt[ar, k][better]
            best["u"][rb] = U.reshape(len(r), -1)[ar, k][better]
            best["v"][rb] = V.reshape(len(r), -1)[ar, k][better]
            best["prim"][rb] = rec["primID"][sel][k // N][better]
    hit = np.isfinite(best["t"])
    ch.compare(hit, np.zeros(m, np.int64), best["prim"], best["t"], best["u"], best["v"], truth, f"host walk, {bounds}, {nsteps} steps, N = {N}")
    sc.release()
    dev.release()


# ---- 5. rtcInterpolate and rtcGetSceneBounds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis", ["bezier", "bspline"])
def test_interpolate_reads_the_vertex_slot_it_is_given(rtc, basis):
    """NativeCurvesISA::interpolate_helper on the buffer of a later time step: the geometry's own basis over the USER's control points"""
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    steps, idx = _hair_steps(3, 3)
    gid = sc.add_curves_mb(steps, idx, basis=basis)
    static = rtc.Scene(dev)
    sgid = [static.add_curves(s, idx, basis=basis) for s in steps]  # the same control points as three static geometries
    for slot in range(3):
        for prim, u in ((0, 0.0), (1, 0.25), (2, 0.625), (2, 1.0)):
            got = sc.interpolate(gid, prim, u, 0.375, slot=slot, count=4)
            want = static.interpolate(sgid[slot], prim, u, 0.375, slot=0, count=4)
            for a, b in zip(got, want):
                assert np.array_equal(a, b)
            cp = ch.control_points(steps[slot], idx)[prim].astype(np.float64)
            s = 1.0 - u
            if basis == "bezier":
                b64 = [s ** 3, 3 * u * s * s, 3 * u * u * s, u ** 3]
            else:
                b64 = ch.bspline_basis64(u)[0]
            assert np.abs(got[0] - sum(w * p for w, p in zip(b64, cp))).max() <= 1e-6
    assert not np.array_equal(sc.interpolate(gid, 1, 0.25, 0, slot=0, count=4)[0], sc.interpolate(gid, 1, 0.25, 0, slot=2, count=4)[0])
    static.release()
    sc.release()
    dev.release()


def test_scene_bounds_are_extended_by_the_swept_boxes(rtc):
    """a static triangle at the origin and one curve that moves from x = 10 to x = 20: the bounds hold the curve at both steps"""
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    sc.add_triangles(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    s0 = np.array([[10, 0, 0, .25], [11, 0, 0, .25], [12, 0, 0, .25], [13, 0, 0, .25]], np.float32)
    s1 = s0 + np.array([10, 2, 0, .25], np.float32)
    sc.add_curves_mb([s0, s1], np.array([0], np.uint32))
    sc.commit()
    lo, hi = sc.bounds()
    assert (np.abs(lo - np.array([0, -.25, -.5])) <= 1e-4).all() and (np.abs(hi - np.array([23.5, 2.5, .5])) <= 1e-4).all()
    assert lo[1] <= -.25 and lo[2] <= -.5 and hi[0] >= 23.5 and hi[1] >= 2.5 and hi[2] >= .5
    sc.release()
    dev.release()


# ---- 6. the other builders of the frame ---------------------------------------------------------------------------------------------
def _digest(sc):
    h = hashlib.sha256()
    for k in (0, 1, 2):
        h.update(bytes(sc.accel_data(k)))
    st = sc.stats()
    h.update(repr((sc.accel_root(), st["accelKind"], st["primCount"], st["leafCount"], st["maxDepth"])).encode())
    return h.hexdigest()[:16]


def accel_digests(rtc):
    """digests of the static triangle, motion-blur triangle, motion-blur quad and motion-blur line accels of a fixed input, swept and
    linear: nodes, records, root and counts"""
    rng = np.random.RandomState(11)
    tv = (rng.rand(300, 3) * 4).astype(np.float32)
    tris = rng.randint(0, 300, (500, 3)).astype(np.uint32)
    move = [np.array([0.5 * k, 0.125 * k * k, -0.25 * k], np.float32) for k in range(3)]
    qv = (rng.rand(200, 3) * 4).astype(np.float32)
    quads = rng.randint(0, 200, (300, 4)).astype(np.uint32)
    lv = np.concatenate([rng.rand(400, 3) * 4, 0.01 + 0.02 * rng.rand(400, 1)], 1).astype(np.float32)
    lidx = np.arange(0, 399, dtype=np.uint32)
    lsteps = [lv + np.append(move[k], np.float32(0.005 * k)) for k in range(3)]
    out = {}
    for bounds in ("swept", "linear"):
        dev = rtc.Device("gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,line_accel_mb=default,mb_bounds=" + bounds)
        for name, add in (("tri", lambda s: s.add_triangles(tv, tris)),
                          ("trimb", lambda s: s.add_triangles_mb([tv + m for m in move], tris)),
                          ("quadmb", lambda s: s.add_quads_mb([qv + m for m in move], quads)),
                          ("linemb", lambda s: s.add_lines_mb(lsteps, lidx))):
            for flags in (0, ROBUST):
                sc = rtc.Scene(dev, flags)
                add(sc)
                sc.commit()
                out[(name, bounds, flags)] = _digest(sc)
                sc.release()
        dev.release()
    return out


# accel_digests() of the parent commit's library, before build_mb_bvh8 was generalised over the geometries a Source takes
PARENT_DIGESTS = {
    ("tri", "swept", 0): "580b22026e99ffb8",
    ("tri", "swept", 4): "5e7cea8ad2a390e3",
    ("trimb", "swept", 0): "c5a3c637a7f36602",
    ("trimb", "swept", 4): "77ff6c0d1ed319a2",
    ("quadmb", "swept", 0): "41b5f69c198a0abe",
    ("quadmb", "swept", 4): "373119823b9cb9d3",
    ("linemb", "swept", 0): "249d3a0df49c1e80",
    ("linemb", "swept", 4): "effb739b0b70ff3c",
    ("tri", "linear", 0): "580b22026e99ffb8",
    ("tri", "linear", 4): "5e7cea8ad2a390e3",
    ("trimb", "linear", 0): "7b2b87c1b289880a",
    ("trimb", "linear", 4): "98ab69a076cdca8e",
    ("quadmb", "linear", 0): "81d66af70e326741",
    ("quadmb", "linear", 4): "bb601c0b75d17e17",
    ("linemb", "linear", 0): "d7852c74fe77b3d3",
    ("linemb", "linear", 4): "f526aa491e4bb44e",
}


def test_the_triangle_quad_and_line_accels_are_byte_identical_to_the_parents(rtc):
    got = accel_digests(rtc)
    assert len(PARENT_DIGESTS) == 16 and got == PARENT_DIGESTS, {k: (v, PARENT_DIGESTS.get(k)) for k, v in got.items() if PARENT_DIGESTS.get(k) != v}
