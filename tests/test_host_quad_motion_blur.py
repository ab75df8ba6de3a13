"""CPU tests of motion-blur quad meshes (RTC_GEOMETRY_TYPE_QUAD with rtcSetGeometryTimeStepCount > 1) on a
`gpu=none,quad_accel_mb=default` device: accel choice (quad_accel_mb), the QuadMBRecord array (one 128-byte record per quad and time
segment, the id words in the w of v1 and v3), the swept boxes of the BVH8 over them, and that every scene without such a mesh is
described as before."""
import numpy as np
import pytest

NODE_DT = np.dtype([("origin", "<f4", 3), ("exp", "u1", 3), ("pad", "u1"), ("child", "<u4", 8), ("q", "u1", (6, 8))])
QUADMB_DT = np.dtype([("v0a", "<f4", 3), ("pad0", "<u4"), ("v1a", "<f4", 3), ("primID", "<u4"), ("v2a", "<f4", 3), ("pad1", "<u4"),
                      ("v3a", "<f4", 3), ("geomID", "<u4"), ("v0b", "<f4", 3), ("pad2", "<u4"), ("v1b", "<f4", 3), ("segment", "<u4"),
                      ("v2b", "<f4", 3), ("pad3", "<u4"), ("v3b", "<f4", 3), ("numSegments", "<u4")])
VERTS = ["v0a", "v1a", "v2a", "v3a", "v0b", "v1b", "v2b", "v3b"]
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF
ACCEL_TRI_MOELLER, ACCEL_QUAD_MOELLER, ACCEL_TRIMB_MOELLER, ACCEL_QUADMB_PLUECKER, ACCEL_QUADMB_MOELLER = 2, 9, 11, 12, 13
ROBUST = 4  # RTC_SCENE_FLAG_ROBUST
CFG = "gpu=none,quad_accel_mb="


def _grid_quads(n=8):
    """(n+1)^2 vertices of a warped grid, n^2 non-planar quads"""
    xs, ys = np.meshgrid(np.arange(n + 1, dtype=np.float32), np.arange(n + 1, dtype=np.float32))
    v = np.stack([xs.ravel(), ys.ravel(), (0.3 * np.sin(xs) * np.cos(ys)).ravel()], 1).astype(np.float32)
    q = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            q.append((a, a + 1, a + n + 2, a + n + 1))
    return v, np.array(q, np.uint32)


def _steps(v, n, shift):
    """n time steps: step k = v moved by k * shift along a slightly bent path"""
    return [(v + np.float32(k) * np.asarray(shift, np.float32) + np.float32(0.05 * k * k) * np.array([0, 1, 0], np.float32)).astype(np.float32)
            for k in range(n)]


def _decode_child(node, i):
    lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for a in range(3):
        s = np.array([int(node["exp"][a]) << 23], np.uint32).view(np.float32)[0]
        o = node["origin"][a]
        # fmaf(q, s, o): q*s is exact (8-bit integer times a power of two), so one rounding like the kernel's fma
        lo[a] = np.float32(np.float64(node["q"][2 * a][i]) * np.float64(s) + np.float64(o))
        hi[a] = np.float32(np.float64(node["q"][2 * a + 1][i]) * np.float64(s) + np.float64(o))
    return lo, hi


def _leaves(nodes, root):
    """[(first, count, node index, child slot)] of every leaf below an inner root"""
    leaves, todo = [], [root]
    while todo:
        n = todo.pop()
        for i, c in enumerate(nodes[n]["child"]):
            c = int(c)
            if c == EMPTY:
                continue
            if c & LEAF:
                leaves.append((c & 0x3FFFFFF, (c >> 26) & 31, n, i))
            else:
                todo.append(c)
    return leaves


# ---- kinds, record layout, bounds -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsteps", [2, 5])
@pytest.mark.parametrize("name,flags,kind", [("default", 0, ACCEL_QUADMB_MOELLER), ("default", ROBUST, ACCEL_QUADMB_PLUECKER),
                                             ("bvh8.quad4imb", ROBUST, ACCEL_QUADMB_MOELLER), ("bvh4.quad4imb", 0, ACCEL_QUADMB_MOELLER)])
def test_commit_builds_a_motion_blur_quad_accel(rtc, nsteps, name, flags, kind):
    dev = rtc.Device(CFG + name)
    sc = rtc.Scene(dev, flags)
    v, q = _grid_quads(6)
    steps = _steps(v, nsteps, (0.5, 0.0, 1.0))
    # geometry 0 is disabled; the moving mesh is geometry 1
    sc.add_triangles(np.eye(3, dtype=np.float32) + 100, np.array([[0, 1, 2]], np.uint32))
    sc.lib.rtcDisableGeometry(sc.lib.rtcGetGeometry(sc.handle, 0))
    assert sc.add_quads_mb(steps, q) == 1
    sc.commit()
    S = nsteps - 1
    st = sc.stats()
    assert st["accelKind"] == kind
    assert st["primCount"] == len(q) * S and st["primBytes"] == 128
    assert len(sc.accel_data(1)) == 0  # no TriRecords
    rec = sc.accel_data(2).view(QUADMB_DT)
    assert len(rec) == len(q) * S
    assert st["totalBytes"] == st["nodeCount"] * 96 + len(rec) * 128
    assert sorted(zip(rec["primID"].tolist(), rec["segment"].tolist())) == [(p, s) for p in range(len(q)) for s in range(S)]
    assert (rec["geomID"] == 1).all() and (rec["numSegments"] == S).all()
    for f in ("pad0", "pad1", "pad2", "pad3"):
        assert (rec[f] == 0).all()
    for r in rec:
        p, s = q[r["primID"]], int(r["segment"])
        for k in range(4):
            assert np.array_equal(r[VERTS[k]], steps[s][p[k]]) and np.array_equal(r[VERTS[4 + k]], steps[s + 1][p[k]])
    # the leaves partition the record array, and every record's eight vertices lie inside the decoded child box of its leaf
    nodes = sc.accel_data(0).view(NODE_DT)
    root = sc.accel_root()
    assert not root & LEAF
    leaves = _leaves(nodes, root)
    assert st["leafCount"] == len(leaves)
    covered = np.zeros(len(rec), np.int32)
    for first, count, n, i in leaves:
        assert 1 <= count <= 28
        covered[first:first + count] += 1
        lo, hi = _decode_child(nodes[n], i)
        pts = np.concatenate([rec[f][first:first + count] for f in VERTS])
        assert (lo <= pts.min(0)).all() and (hi >= pts.max(0)).all(), (n, i, lo, hi)
    assert (covered == 1).all()
    # rtcGetSceneBounds covers all steps
    lo, hi = sc.bounds()
    allv = np.concatenate(steps)
    assert np.allclose(lo, allv.min(0)) and np.allclose(hi, allv.max(0))
    sc.release()
    dev.release()


def test_unknown_quad_accel_mb_is_an_invalid_argument(rtc):
    dev = rtc.Device(CFG + "bvh8.quad9mb")
    sc = rtc.Scene(dev)
    v, q = _grid_quads(2)
    sc.add_quads_mb(_steps(v, 2, (0, 0, 1)), q)
    dev.lib.rtcCommitScene(sc.handle)
    assert dev.error() == rtc.RTC_ERROR_INVALID_ARGUMENT
    sc.release()
    dev.release()


def test_missing_time_step_buffer_is_an_invalid_operation(rtc):
    dev = rtc.Device(CFG + "default")
    L = dev.lib
    sc = rtc.Scene(dev)
    v, q = _grid_quads(2)
    g = L.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_QUAD)
    L.rtcSetGeometryTimeStepCount(g, 2)
    vpad = np.zeros((len(v) + 2, 3), np.float32)
    vpad[:len(v)] = v
    L.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_VERTEX, 0, rtc.RTC_FORMAT_FLOAT3, vpad.ctypes.data, 0, 12, len(v))
    L.rtcSetSharedGeometryBuffer(g, rtc.RTC_BUFFER_TYPE_INDEX, 0, rtc.RTC_FORMAT_UINT4, q.ctypes.data, 0, 16, len(q))
    L.rtcCommitGeometry(g)
    L.rtcAttachGeometry(sc.handle, g)
    L.rtcReleaseGeometry(g)
    assert dev.error() == rtc.RTC_ERROR_NONE
    L.rtcCommitScene(sc.handle)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION
    sc.release()
    dev.release()


def test_a_quad_invalid_at_one_step_loses_the_segments_that_touch_it(rtc):
    dev = rtc.Device(CFG + "default")
    sc = rtc.Scene(dev)
    v, q = _grid_quads(3)
    steps = _steps(v, 4, (0, 0, 1))
    steps[2][5, 1] = np.nan          # vertex 5 is not finite at step 2: segments 1 and 2 of its quads are dropped
    q = q.copy()
    q[1, 2] = len(v) + 7             # index out of range at every step: no record at all
    sc.add_quads_mb(steps, q)
    sc.commit()
    rec = sc.accel_data(2).view(QUADMB_DT)
    uses5 = {p for p in range(len(q)) if 5 in q[p].tolist()}
    want = sorted((p, s) for p in range(len(q)) for s in range(3) if p != 1 and not (s in (1, 2) and p in uses5))
    assert len(uses5 - {1}) > 1 and sorted(zip(rec["primID"].tolist(), rec["segment"].tolist())) == want
    sc.release()
    dev.release()


# ---- scenes without a moving quad mesh are what they were -----------------------------------------------------------------------
def test_a_quad_mesh_with_one_time_step_lands_in_the_static_accel(rtc):
    dev = rtc.Device(CFG + "default")
    v, q = _grid_quads(5)
    out = []
    for one_step in (False, True):
        sc = rtc.Scene(dev)
        if one_step:
            sc.add_quads_mb([v], q)
        else:
            sc.add_quads(v, q)
        sc.commit()
        st = sc.stats()
        assert st["accelKind"] == ACCEL_QUAD_MOELLER and st["primBytes"] == 64 and st["primCount"] == len(q)
        out.append((sc.accel_data(0).tobytes(), sc.accel_data(2).tobytes(), sc.accel_root(), st["totalBytes"]))
        sc.release()
    assert out[0] == out[1]
    dev.release()


@pytest.mark.parametrize("other", ["tri", "trimb", "quad"])
def test_inspection_calls_describe_the_other_accel_when_there_is_one(rtc, other):
    dev = rtc.Device(CFG + "default")
    v, q = _grid_quads(7)
    t = np.concatenate([q[:, [0, 1, 3]], q[:, [2, 1, 3]]]).astype(np.uint32)
    mv, mq = _grid_quads(4)
    out = []
    for moving in (False, True):
        sc = rtc.Scene(dev)
        if other == "tri":
            assert sc.add_triangles(v, t) == 0
        elif other == "trimb":
            assert sc.add_triangles_mb(_steps(v, 2, (0, 1, 0)), t) == 0
        else:
            assert sc.add_quads(v, q) == 0
        if moving:
            assert sc.add_quads_mb(_steps(mv + 3, 3, (1, 0, 2)), mq) == 1
        sc.commit()
        st = sc.stats()
        assert st["accelKind"] == {"tri": ACCEL_TRI_MOELLER, "trimb": ACCEL_TRIMB_MOELLER, "quad": ACCEL_QUAD_MOELLER}[other]
        out.append((sc.accel_data(0).tobytes(), sc.accel_data(1).tobytes(), sc.accel_data(2).tobytes(), sc.accel_root(), st["primCount"],
                    st["primBytes"], st["leafCount"], st["totalBytes"]))
        sc.release()
    assert out[0][:7] == out[1][:7]
    assert out[1][7] > out[0][7]  # ... and the moving quad mesh's accel is counted
    dev.release()


def test_a_host_only_device_without_the_key_raises_as_before(rtc):
    dev = rtc.Device("gpu=none,quad_accel=default")
    sc = rtc.Scene(dev)
    v, q = _grid_quads(2)
    sc.add_quads_mb(_steps(v, 2, (0, 0, 1)), q)
    dev.lib.rtcCommitScene(sc.handle)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION
    sc.release()
    dev.release()
