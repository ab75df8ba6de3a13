"""CPU tests of motion blur on line segments on a host-only device that names the accel (`gpu=none,line_accel_mb=default`): the key's
names, what stays refused, the kinds 38..41, the 80-byte LineMBRecords, containment of the interpolated segments in the swept and in
the time-dependent node boxes on every root-to-leaf path, rtcInterpolate on a later time step, and the two arithmetics of the truth on
the pinned moving tuft of tests/test_gpu_line_motion_blur.py."""
import ctypes as C

import numpy as np
import pytest

import line_helpers as lh
import line_mb_helpers as mh
from line_helpers import ACCEL_LINE_FAST, NODE_DT, ROBUST
from line_mb_helpers import ACCEL_LINEMB_FAST, ACCEL_LINEMB_LINEAR_FAST, ACCEL_LINEMB_LINEAR_ROBUST, ACCEL_LINEMB_ROBUST, LINEMB_DT
from mb_linear_helpers import NODEMB_DT, PAD_STEPS, decode_children_mb, scales, snap, walk_paths

HOST = "gpu=none,line_accel_mb=default"
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


def _strand_steps(nsteps, n_strands=40, per=9, seed=3):
    """n_strands polylines of `per` vertices (shared between neighbouring segments) on multiples of 2^-10, moved along a curved path with
    growing radii: ([nsteps arrays [nv, 4]], first_index)"""
    rng = np.random.RandomState(seed)
    v, idx = [], []
    for s in range(n_strands):
        p = rng.rand(3) * 4
        for k in range(per):
            if k + 1 < per:
                idx.append(len(v))
            v.append((*p, 0.01 + 0.02 * rng.rand()))
            p = p + (rng.rand(3) - 0.5) * 0.4
    v = np.array(v, np.float64)
    steps = []
    for k in range(nsteps):
        xyz = v[:, :3] + np.array([0.75 * k, 0.1 * k * k, -0.3 * k]) + 0.05 * k * np.sin(v[:, :3] * 3.0)
        steps.append(np.concatenate([snap(xyz), snap(v[:, 3] * (1.0 + 0.25 * k))[:, None]], 1).astype(np.float32))
    return steps, np.array(idx, np.uint32)


# ---- 1. keys and refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "bvh8.line4imb", "bvh4.line4imb"])
@pytest.mark.parametrize("flags,kind", [(0, ACCEL_LINEMB_FAST), (ROBUST, ACCEL_LINEMB_ROBUST)])
def test_every_name_of_the_key_builds_the_one_accel(rtc, name, flags, kind):
    dev = rtc.Device("gpu=none,line_accel_mb=" + name)
    sc = rtc.Scene(dev, flags)
    steps, idx = _strand_steps(3)
    sc.add_lines_mb(steps, idx)
    sc.commit()
    st = sc.stats()
    assert st["accelKind"] == kind and st["primCount"] == 2 * len(idx) and st["primBytes"] == 80 and st["nodeBytes"] == 96
    assert st["totalBytes"] == st["nodeCount"] * 96 + 2 * len(idx) * 80
    sc.release()
    dev.release()


@pytest.mark.parametrize("flags,kind", [(0, ACCEL_LINEMB_LINEAR_FAST), (ROBUST, ACCEL_LINEMB_LINEAR_ROBUST)])
def test_linear_bounds_give_the_kinds_40_and_41_with_144_byte_nodes(rtc, flags, kind):
    dev = rtc.Device(HOST + ",mb_bounds=linear")
    sc = rtc.Scene(dev, flags)
    steps, idx = _strand_steps(2)
    sc.add_lines_mb(steps, idx)
    sc.commit()
    st = sc.stats()
    assert st["accelKind"] == kind and st["primCount"] == len(idx) and st["primBytes"] == 80 and st["nodeBytes"] == 144
    assert len(sc.accel_data(0)) == st["nodeCount"] * 144 and st["totalBytes"] == st["nodeCount"] * 144 + len(idx) * 80
    sc.release()
    dev.release()


def test_unknown_name_is_an_invalid_argument(rtc):
    dev = rtc.Device("gpu=none,line_accel_mb=bvh8.line8imb")
    err = Errors(dev)
    sc = rtc.Scene(dev)
    steps, idx = _strand_steps(2, 2)
    sc.add_lines_mb(steps, idx)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_ARGUMENT, "unknown motion blur line segment acceleration structure bvh8.line8imb")
    dev.release()


def test_without_the_key_a_host_only_device_refuses_as_before(rtc):
    dev = rtc.Device("gpu=none")
    err = Errors(dev)
    sc = rtc.Scene(dev)
    steps, idx = _strand_steps(2, 2)
    sc.add_lines_mb(steps, idx)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "motion blur of line segments is not supported")
    dev.release()


def test_a_time_step_without_a_vertex_buffer_is_refused(rtc):
    dev = rtc.Device(HOST)
    err = Errors(dev)
    sc = rtc.Scene(dev)
    steps, idx = _strand_steps(2, 2)
    gid = sc.add_lines_mb(steps, idx)
    g = dev.lib.rtcGetGeometry(sc.handle, gid)
    dev.lib.rtcSetGeometryTimeStepCount(g, 3)  # step 2 has no buffer
    dev.lib.rtcCommitGeometry(g)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "motion blur geometry: a time step has no vertex buffer")
    dev.release()


@pytest.mark.parametrize("cfg,text", [(HOST, "static triangle meshes only"),
                                      (HOST + ",quad_accel=default,tri_accel_mb=default,inst_accel=default", "triangle and quad meshes only")])
def test_moving_lines_below_an_instance_are_refused_like_static_ones(rtc, cfg, text):
    dev = rtc.Device(cfg)
    err = Errors(dev)
    inner = rtc.Scene(dev)
    inner.add_triangles(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    steps, idx = _strand_steps(2, 2)
    lines = inner.add_lines_mb(steps, idx)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance(inner)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "an instanced scene may hold " + text)
    inner.set_enabled(lines, False)  # disabled, the line geometry does not count
    inner.commit()
    top.commit()
    assert top.stats()["accelKind"] in (14, 15, 22, 23)
    dev.release()


# ---- 2. kinds and layout ------------------------------------------------------------------------------------------------------------
def test_the_record_is_80_bytes_laid_out_as_documented(rtc):
    """byte by byte: one segment, two steps, every float a value of its own"""
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    s0 = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.float32)
    s1 = np.array([[9, 10, 11, 12], [13, 14, 15, 16]], np.float32)
    sc.add_lines_mb([s0, s1], np.array([0], np.uint32), geom_id=6)
    sc.commit()
    raw = bytes(sc.accel_data(2))
    assert len(raw) == 80 and sc.accel_root() == (0x80000000 | (1 << 26))
    want = np.arange(1, 17, dtype=np.float32).tobytes() + np.array([6, 0, 0, 1], np.uint32).tobytes()  # V0, V1 at step 0; V0, V1 at step 1; geomID, primID, segment, numSegments
    assert raw == want
    r = np.frombuffer(raw, LINEMB_DT)[0]
    assert [LINEMB_DT.fields[f][1] for f in LINEMB_DT.names] == [0, 12, 16, 28, 32, 44, 48, 60, 64, 68, 72, 76]
    assert r["r0a"] == 4 and r["r1a"] == 8 and r["r0b"] == 12 and r["r1b"] == 16 and r["numSegments"] == 1
    sc.release()
    dev.release()


def test_one_record_per_valid_segment_and_time_segment(rtc):
    """N - 1 records per segment; none for a (segment, time segment) pair that is invalid at either end (LineSegments::valid(i, itime))"""
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    base = np.array([[k, 0, 0, .1] for k in range(8)], np.float32)
    steps = [base.copy() for _ in range(4)]
    for k in range(4):
        steps[k][:, 1] += k
    steps[1][2, 0] = np.nan      # vertex 2 at step 1: segments 1 and 2 lose the time segments 0 and 1
    steps[3][5, 3] = -0.25       # negative radius at step 3: segments 4 and 5 lose time segment 2
    steps[0][7, 3] = np.inf      # vertex 7 at step 0: segment 6 loses time segment 0
    idx = np.arange(8, dtype=np.uint32)  # segment 7 starts at the last vertex: never valid
    sc.add_lines_mb(steps, idx)
    sc.commit()
    rec = sc.accel_data(2).view(LINEMB_DT)
    got = sorted(zip(rec["primID"].tolist(), rec["segment"].tolist()))
    lost = {(1, 0), (1, 1), (2, 0), (2, 1), (4, 2), (5, 2), (6, 0)}
    want = sorted((p, s) for p in range(7) for s in range(3) if (p, s) not in lost)
    assert got == want and (rec["numSegments"] == 3).all()
    for r in rec:  # the pre-gathered ends of the record's time segment
        p, s = int(r["primID"]), int(r["segment"])
        assert np.array_equal(np.append(r["v0a"], r["r0a"]), steps[s][p]) and np.array_equal(np.append(r["v1a"], r["r1a"]), steps[s][p + 1])
        assert np.array_equal(np.append(r["v0b"], r["r0b"]), steps[s + 1][p]) and np.array_equal(np.append(r["v1b"], r["r1b"]), steps[s + 1][p + 1])
    assert sc.stats()["primCount"] == len(want)
    sc.release()
    dev.release()


def test_static_and_moving_lines_in_one_scene_give_both_accels(rtc):
    dev = rtc.Device(HOST + ",inst_accel=default")
    steps, idx = _strand_steps(2, 4)
    kinds = {}
    tv, tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32)
    inner = rtc.Scene(dev)
    inner.add_triangles(tv, tri)
    inner.commit()
    for parts in ("l", "m", "lm", "tm", "mi"):
        sc = rtc.Scene(dev)
        if "t" in parts:
            sc.add_triangles(tv, tri)
        if "l" in parts:
            sc.add_lines(steps[0], idx)
        if "m" in parts:
            sc.add_lines_mb(steps, idx)
        if "i" in parts:
            sc.add_instance(inner)
        sc.commit()
        kinds[parts] = (sc.stats()["accelKind"], sc.stats()["totalBytes"], sc.stats()["primBytes"])
        sc.release()
    assert kinds["l"][0] == ACCEL_LINE_FAST and kinds["m"][0] == ACCEL_LINEMB_FAST and kinds["m"][2] == 80
    assert kinds["lm"][0] == ACCEL_LINE_FAST and kinds["lm"][1] == kinds["l"][1] + kinds["m"][1]  # both accels; the static one is described
    assert kinds["tm"][0] == 2                                                                    # the triangle accel is described when there is one
    assert kinds["mi"][0] == ACCEL_LINEMB_FAST                                                    # in front of the instance accel
    inner.release()
    dev.release()


def test_filter_flags_follow_the_static_line_geometries(rtc):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    steps, idx = _strand_steps(2, 2)
    gid = sc.add_lines_mb(steps, idx)
    sc.commit()
    assert sc.filter_flags() == 0
    keep = rtc.FILTER_FUNC(lambda args: None)
    sc.set_filters(gid, intersect=keep)
    sc.commit()
    assert sc.filter_flags() == rtc.RTCAMD_SCENE_FILTER_MESH_INTERSECT
    sc.set_filters(gid, intersect=keep, occluded=keep)
    sc.commit()
    assert sc.filter_flags() == rtc.RTCAMD_SCENE_FILTER_MESH_INTERSECT | rtc.RTCAMD_SCENE_FILTER_MESH_OCCLUDED
    sc.release()
    dev.release()


# ---- 3. containment -----------------------------------------------------------------------------------------------------------------
TIMES = np.linspace(0.0, 1.0, 33)


@pytest.mark.parametrize("nsteps", [2, 5])
@pytest.mark.parametrize("flags", [0, ROBUST])
@pytest.mark.parametrize("bounds", ["swept", "linear"])
def test_the_interpolated_segment_lies_inside_every_node_box_on_its_path(rtc, bounds, flags, nsteps):
    """At 33 times in [0, 1]: the box of the interpolated segment with interpolated radii (float64, exact) lies inside the decoded box of
    every node on the way down - the swept QNode8 boxes of the kinds 38 / 39, the QNodeMB8 boxes interpolated to that time with the node
    step's arithmetic in the kinds 40 / 41.  (min is concave and max convex: the segment's box is inside the interpolated end boxes.)"""
    dev = rtc.Device(HOST + ",mb_bounds=" + bounds)
    sc = rtc.Scene(dev, flags)
    steps, idx = _strand_steps(nsteps)
    sc.add_lines_mb(steps, idx)
    sc.commit()
    linear = bounds == "linear"
    want = {(0, False): ACCEL_LINEMB_FAST, (ROBUST, False): ACCEL_LINEMB_ROBUST, (0, True): ACCEL_LINEMB_LINEAR_FAST, (ROBUST, True): ACCEL_LINEMB_LINEAR_ROBUST}
    assert sc.stats()["accelKind"] == want[(flags, linear)]
    nodes = sc.accel_data(0).view(NODEMB_DT if linear else NODE_DT)
    rec = sc.accel_data(2).view(LINEMB_DT)
    assert len(rec) == (nsteps - 1) * len(idx)
    boxes = {t: mh.record_box_at(rec, t) for t in TIMES}
    decoded = {}
    seen = 0
    for path, first, count in walk_paths(nodes, sc.accel_root()):
        seen += count
        for t in TIMES:
            lo, hi, take = boxes[t]
            sel = np.nonzero(take[first:first + count])[0] + first
            if not len(sel):
                continue
            for n, i in path:
                key = (n, t if linear else 0.0)
                if key not in decoded:
                    decoded[key] = decode_children_mb(nodes[n], t) if linear else lh.decode_children(nodes[n])
                clo, chi = decoded[key]
                assert (clo[i].astype(np.float64) <= lo[sel]).all() and (chi[i].astype(np.float64) >= hi[sel]).all(), (n, i, t)
    assert seen == len(rec)
    # Scene::bounds: the union of the swept boxes
    lo0, hi0 = mh.segment_box64(*[np.concatenate([np.concatenate([rec[a], rec[r][:, None]], 1) for a, r in pair]) for pair in
                                  ((("v0a", "r0a"), ("v0b", "r0b")), (("v1a", "r1a"), ("v1b", "r1b")))])
    slo, shi = sc.bounds()
    assert np.array_equal(slo, lo0.min(0).astype(np.float32)) and np.array_equal(shi, hi0.max(0).astype(np.float32))
    sc.release()
    dev.release()


def test_root_linear_bounds_of_a_two_step_geometry_are_its_bounds_at_both_steps(rtc):
    """up to the quantizer's padding: at least one and less than PAD_STEPS grid steps per side (accel.h QNodeMB8)"""
    dev = rtc.Device(HOST + ",mb_bounds=linear")
    sc = rtc.Scene(dev)
    steps, idx = _strand_steps(2)
    sc.add_lines_mb(steps, idx)
    sc.commit()
    nodes = sc.accel_data(0).view(NODEMB_DT)
    root = nodes[sc.accel_root()]
    live = root["child"] != 0xFFFFFFFF
    step = scales(root).astype(np.float64)
    for t, s in ((0.0, steps[0]), (1.0, steps[1])):
        lo, hi = mh.segment_box64(*lh.ends(s, idx))
        clo, chi = decode_children_mb(root, t)
        glo, ghi = clo[live].min(0).astype(np.float64), chi[live].max(0).astype(np.float64)
        assert ((lo.min(0) - glo) >= step).all() and ((lo.min(0) - glo) < PAD_STEPS * step).all(), (t, lo.min(0) - glo, step)
        assert ((ghi - hi.max(0)) >= step).all() and ((ghi - hi.max(0)) < PAD_STEPS * step).all(), (t, ghi - hi.max(0), step)
    sc.release()
    dev.release()


# ---- 4. rtcInterpolate --------------------------------------------------------------------------------------------------------------
def test_interpolate_reads_the_vertex_slot_it_is_given(rtc):
    dev = rtc.Device(HOST)
    sc = rtc.Scene(dev)
    s0 = np.array([[0, 0, 0, 0.5], [2, 4, -8, 0.25], [3, 4, 0, 1.0]], np.float32)
    s1 = np.array([[8, 0, 0, 1.0], [10, 4, -8, 0.5], [11, 8, 0, 2.0]], np.float32)
    gid = sc.add_lines_mb([s0, s1], np.array([0, 1], np.uint32))
    for slot, v in ((0, s0), (1, s1)):
        for prim, u in ((0, 0.0), (0, 0.25), (1, 0.5), (1, 1.0)):
            P, du, dv, duu, dvv, duv = sc.interpolate(gid, prim, u, 0.375, slot=slot, count=4)
            a, b = v[prim], v[prim + 1]
            assert np.array_equal(P, (1 - u) * a + u * b) and np.array_equal(du, b - a)
            assert not dv.any() and not duu.any() and not dvv.any() and not duv.any()
    sc.release()
    dev.release()


# ---- 5. the truth's two arithmetics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsteps", [2, 5])
def test_float32_restatement_agrees_with_the_float64_truth_on_the_pinned_moving_tuft(nsteps):
    """The GPU tests leave a ray out only where the float64 truth is within 1e-4 of `d2 <= r2` or of a tie, at most 0.5 % of the rays.
    Measured on the pinned moving tuft (2 / 5 steps): 3317 / 2778 hits of 4096, 0 differing IDs, 1 / 0 rays near a decision."""
    steps, idx, org, dirs = mh.tuft_steps(nsteps)
    times = mh.round_robin_times(len(org), nsteps)
    assert len(np.unique(times)) == 4 * (nsteps - 1) + 1
    a = mh.moving_truth(steps, idx, org, dirs, times, np.float64)
    b = mh.moving_truth(steps, idx, org, dirs, times, np.float32)
    h = a["hit"]
    near = a["near_edge"] | a["near_tie"]
    print(f"  {nsteps} steps: {int(h.sum())} hits of {len(org)}, {int((a['seg'][h] != b['seg'][h]).sum())} differing IDs, {int(near.sum())} rays near a decision")
    assert int(h.sum()) == mh.TUFT_MB_HITS[nsteps] and int(near.sum()) == mh.TUFT_MB_NEAR[nsteps]
    assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["seg"][h], b["seg"][h])
    assert near.sum() <= 0.005 * len(org)
    assert (np.abs(a["t"][h] - b["t"][h]) <= 1e-4 * np.abs(a["t"][h])).all() and (np.abs(a["u"][h] - b["u"][h]) <= 1e-4).all()
