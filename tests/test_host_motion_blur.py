"""CPU tests of motion-blur triangle meshes (rtcSetGeometryTimeStepCount > 1) on a `gpu=none` device: accel choice (tri_accel_mb),
the TriMBRecord array (one 96-byte record per triangle and time segment), the swept boxes of the BVH8 over them, and that static
triangle meshes are built exactly as before."""
import numpy as np
import pytest

NODE_DT = np.dtype([("origin", "<f4", 3), ("exp", "u1", 3), ("pad", "u1"), ("child", "<u4", 8), ("q", "u1", (6, 8))])
TRIMB_DT = np.dtype([("a0", "<f4", 3), ("geomID", "<u4"), ("b0", "<f4", 3), ("primID", "<u4"), ("c0", "<f4", 3), ("segment", "<u4"),
                     ("a1", "<f4", 3), ("numSegments", "<u4"), ("b1", "<f4", 3), ("pad0", "<u4"), ("c1", "<f4", 3), ("pad1", "<u4")])
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF
ACCEL_TRI_MOELLER, ACCEL_TRIMB_PLUECKER, ACCEL_TRIMB_MOELLER = 2, 10, 11
ROBUST = 4  # RTC_SCENE_FLAG_ROBUST


def _grid_tris(n=8):
    """(n+1)^2 vertices of a warped grid, 2 n^2 triangles"""
    xs, ys = np.meshgrid(np.arange(n + 1, dtype=np.float32), np.arange(n + 1, dtype=np.float32))
    v = np.stack([xs.ravel(), ys.ravel(), (0.3 * np.sin(xs) * np.cos(ys)).ravel()], 1).astype(np.float32)
    t = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            t += [(a, a + 1, a + n + 2), (a, a + n + 2, a + n + 1)]
    return v, np.array(t, np.uint32)


def _steps(v, n, shift):
    """n time steps: step k = v moved by k * shift along a slightly bent path"""
    return [(v + np.float32(k) * np.asarray(shift, np.float32) + np.float32(0.05 * k * k) * np.array([0, 1, 0], np.float32)).astype(np.float32)
            for k in range(n)]


def _leaves(nodes, root):
    """[(first, count, node index or -1, child slot)] of every leaf reachable from root, and the inner (node, slot, child node) edges"""
    leaves, edges = [], []
    if root & LEAF:
        return [((root & 0x3FFFFFF), (root >> 26) & 31, -1, 0)], edges
    todo = [root]
    while todo:
        n = todo.pop()
        for i, c in enumerate(nodes[n]["child"]):
            c = int(c)
            if c == EMPTY:
                continue
            if c & LEAF:
                leaves.append((c & 0x3FFFFFF, (c >> 26) & 31, n, i))
            else:
                edges.append((n, i, c))
                todo.append(c)
    return leaves, edges


def _decode_child(node, i):
    lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for a in range(3):
        s = np.array([int(node["exp"][a]) << 23], np.uint32).view(np.float32)[0]
        o = node["origin"][a]
        # fmaf(q, s, o): q*s is exact (8-bit integer times a power of two), so one rounding like the kernel's fma
        lo[a] = np.float32(np.float64(node["q"][2 * a][i]) * np.float64(s) + np.float64(o))
        hi[a] = np.float32(np.float64(node["q"][2 * a + 1][i]) * np.float64(s) + np.float64(o))
    return lo, hi


# ---- 1. commit and accel kind ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsteps", [2, 5])
@pytest.mark.parametrize("cfg,flags,kind", [("", 0, ACCEL_TRIMB_MOELLER), ("", ROBUST, ACCEL_TRIMB_PLUECKER),
                                            ("tri_accel_mb=bvh8.triangle4imb", ROBUST, ACCEL_TRIMB_MOELLER),
                                            ("tri_accel_mb=bvh4.triangle4vmb", 0, ACCEL_TRIMB_MOELLER)])
def test_commit_builds_a_motion_blur_accel(rtc, nsteps, cfg, flags, kind):
    dev = rtc.Device("gpu=none" + ("," + cfg if cfg else ""))
    sc = rtc.Scene(dev, flags)
    v, t = _grid_tris(6)
    steps = _steps(v, nsteps, (0.5, 0.0, 1.0))
    # geometry 0 is static; the moving mesh is geometry 1
    sc.add_triangles(np.eye(3, dtype=np.float32) + 100, np.array([[0, 1, 2]], np.uint32))
    sc.lib.rtcDisableGeometry(sc.lib.rtcGetGeometry(sc.handle, 0))
    assert sc.add_triangles_mb(steps, t) == 1
    sc.commit()
    S = nsteps - 1
    st = sc.stats()
    assert st["accelKind"] == kind
    assert st["primCount"] == len(t) * S and st["primBytes"] == 96
    rec = sc.accel_data(2).view(TRIMB_DT)
    assert len(rec) == len(t) * S
    assert st["totalBytes"] == st["nodeCount"] * 96 + len(rec) * 96
    assert sorted(zip(rec["primID"].tolist(), rec["segment"].tolist())) == [(p, s) for p in range(len(t)) for s in range(S)]
    assert (rec["geomID"] == 1).all() and (rec["numSegments"] == S).all()
    for r in rec:
        p, s = t[r["primID"]], int(r["segment"])
        for k, f in enumerate("abc"):
            assert np.array_equal(r[f + "0"], steps[s][p[k]]) and np.array_equal(r[f + "1"], steps[s + 1][p[k]])
    # the leaves partition the record array
    nodes = sc.accel_data(0).view(NODE_DT)
    leaves, _ = _leaves(nodes, sc.accel_root())
    assert st["leafCount"] == len(leaves)
    covered = np.zeros(len(rec), np.int32)
    for first, count, _, _ in leaves:
        assert 1 <= count <= 28
        covered[first:first + count] += 1
    assert (covered == 1).all()
    # rtcGetSceneBounds covers the whole motion
    lo, hi = sc.bounds()
    allv = np.concatenate(steps)
    assert np.allclose(lo, allv.min(0)) and np.allclose(hi, allv.max(0))
    sc.release()
    dev.release()


def test_missing_time_step_buffer_is_an_invalid_operation(rtc):
    dev = rtc.Device("gpu=none")
    L = dev.lib
    sc = rtc.Scene(dev)
    v, t = _grid_tris(2)
    g = L.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_TRIANGLE)
    L.rtcSetGeometryTimeStepCount(g, 2)
    vpad = np.zeros((len(v) + 2, 3), np.float32)
    vpad[:len(v)] = v
    L.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0, rtc.RTC_FORMAT_FLOAT3, vpad.ctypes.data, 0, 12, len(v))
    L.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_INDEX, 0, rtc.RTC_FORMAT_UINT3, t.ctypes.data, 0, 12, len(t))
    L.rtcCommitGeometry(g)
    L.rtcAttachGeometry(sc.handle, g)
    L.rtcReleaseGeometry(g)
    assert dev.error() == rtc.RTC_ERROR_NONE
    L.rtcCommitScene(sc.handle)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION
    sc.release()
    dev.release()


def test_unknown_tri_accel_mb_is_an_invalid_argument(rtc):
    dev = rtc.Device("gpu=none,tri_accel_mb=bvh8.triangle9mb")
    sc = rtc.Scene(dev)
    v, t = _grid_tris(2)
    sc.add_triangles_mb(_steps(v, 2, (0, 0, 1)), t)
    dev.lib.rtcCommitScene(sc.handle)
    assert dev.error() == rtc.RTC_ERROR_INVALID_ARGUMENT
    sc.release()
    dev.release()


def test_a_triangle_invalid_at_one_step_loses_the_segments_that_touch_it(rtc):
    dev = rtc.Device("gpu=none")
    sc = rtc.Scene(dev)
    v, t = _grid_tris(3)
    steps = _steps(v, 4, (0, 0, 1))
    steps[3][5, 1] = np.nan          # vertex 5 is not finite at the last step: segment 2 of its triangles is dropped
    t = t.copy()
    t[1, 2] = len(v) + 7             # index out of range at every step: no record at all
    sc.add_triangles_mb(steps, t)
    sc.commit()
    rec = sc.accel_data(2).view(TRIMB_DT)
    uses5 = {p for p in range(len(t)) if 5 in t[p].tolist()}
    want = sorted((p, s) for p in range(len(t)) for s in range(3) if p != 1 and not (s == 2 and p in uses5))
    assert len(uses5) > 1 and sorted(zip(rec["primID"].tolist(), rec["segment"].tolist())) == want
    sc.release()
    dev.release()


# ---- 2. swept boxes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsteps", [2, 3])
def test_node_boxes_hold_both_ends_of_every_segment(rtc, nsteps):
    """Every leaf's child box holds both segment ends of every record in it, and every inner child box holds the boxes of its
    children - their exact boxes, as in tests/test_host_accel.py: a child node's DECODED boxes are rounded outwards on that node's own
    8-bit grid and may stick out of the parent's decoded box by a grid step, for static meshes too; what the traversal needs is that a
    box holds all geometry below it."""
    dev = rtc.Device("gpu=none")
    sc = rtc.Scene(dev)
    v, t = _grid_tris(12)
    extent = v.max(0) - v.min(0)
    steps = _steps(v, nsteps, 0.5 * extent)  # every step is translated by half the scene extent
    sc.add_triangles_mb(steps, t)
    sc.commit()
    nodes = sc.accel_data(0).view(NODE_DT)
    rec = sc.accel_data(2).view(TRIMB_DT)
    root = sc.accel_root()
    assert not root & LEAF
    leaves, edges = _leaves(nodes, root)
    assert len(leaves) > 8 and len(edges) > 0

    def walk(ref):
        """bounds of both segment ends of every record below ref; every child box on the way must hold what lies below it"""
        if ref & LEAF:
            first, count = ref & 0x3FFFFFF, (ref >> 26) & 31
            pts = np.concatenate([rec[f][first:first + count] for f in ("a0", "b0", "c0", "a1", "b1", "c1")])
            return pts.min(0), pts.max(0)
        lo, hi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
        for i, c in enumerate(nodes[ref]["child"]):
            if int(c) == EMPTY:
                continue
            clo, chi = walk(int(c))  # a leaf's records, or the boxes of an inner child's children
            blo, bhi = _decode_child(nodes[ref], i)
            assert (blo <= clo).all() and (bhi >= chi).all(), (ref, i, blo, clo, bhi, chi)
            lo, hi = np.minimum(lo, clo), np.maximum(hi, chi)
        return lo, hi

    lo, hi = walk(root)
    allv = np.concatenate(steps)
    assert np.array_equal(lo, allv.min(0)) and np.array_equal(hi, allv.max(0))
    sc.release()
    dev.release()


# ---- 3. static scenes unchanged -------------------------------------------------------------------------------------------------
def test_static_accel_is_unchanged_by_a_moving_mesh_in_the_scene(rtc):
    dev = rtc.Device("gpu=none")
    v, t = _grid_tris(7)
    mv, mt = _grid_tris(4)
    out = []
    for moving in (False, True):
        sc = rtc.Scene(dev)
        assert sc.add_triangles(v, t) == 0
        if moving:
            assert sc.add_triangles_mb(_steps(mv + 3, 3, (1, 0, 2)), mt) == 1
        sc.commit()
        st = sc.stats()
        assert st["accelKind"] == ACCEL_TRI_MOELLER  # the inspection calls describe the static triangle accel when there is one
        out.append((sc.accel_data(0).tobytes(), sc.accel_data(1).tobytes(), sc.accel_root(), st["primCount"], st["totalBytes"]))
        sc.release()
    assert out[0][:4] == out[1][:4]
    assert out[1][4] > out[0][4]  # ... and the moving mesh's accel is counted
    dev.release()


def test_a_mesh_with_one_time_step_lands_in_the_static_accel(rtc):
    dev = rtc.Device("gpu=none")
    v, t = _grid_tris(5)
    out = []
    for one_step in (False, True):
        sc = rtc.Scene(dev)
        if one_step:
            sc.add_triangles_mb([v], t)
        else:
            sc.add_triangles(v, t)
        sc.commit()
        assert sc.stats()["accelKind"] == ACCEL_TRI_MOELLER
        assert len(sc.accel_data(2)) == 0
        out.append((sc.accel_data(0).tobytes(), sc.accel_data(1).tobytes(), sc.accel_root()))
        sc.release()
    assert out[0] == out[1]
    dev.release()


def test_quads_with_time_steps_still_raise(rtc):
    dev = rtc.Device("gpu=none,quad_accel=default")
    L = dev.lib
    sc = rtc.Scene(dev)
    v = np.zeros((6, 3), np.float32)
    v[:4] = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]
    q = np.array([[0, 1, 2, 3]], np.uint32)
    g = L.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_QUAD)
    L.rtcSetGeometryTimeStepCount(g, 2)
    for slot in (0, 1):
        L.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_VERTEX, slot, rtc.RTC_FORMAT_FLOAT3, v.ctypes.data, 0, 12, 4)
    L.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_INDEX, 0, rtc.RTC_FORMAT_UINT4, q.ctypes.data, 0, 16, 1)
    L.rtcCommitGeometry(g)
    L.rtcAttachGeometry(sc.handle, g)
    L.rtcReleaseGeometry(g)
    assert dev.error() == rtc.RTC_ERROR_NONE
    L.rtcCommitScene(sc.handle)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION
    sc.release()
    dev.release()
