"""CPU tests of single-level instancing (RTC_GEOMETRY_TYPE_INSTANCE) on a `gpu=none` device: API surface, the refusals of what is out
of scope, the contents of the instance accel (kinds 14 / 15), and the pinning of the inputs of the general-transform GPU test."""
import ctypes as C

import numpy as np
import pytest

import instance_helpers as ih
from helpers import random_soup
from instance_helpers import EMPTY, INST_DT, INVALID, LEAF, NODE_DT, TRI_DT

ROBUST = 4
FORMATS = ("RTC_FORMAT_FLOAT3X4_ROW_MAJOR", "RTC_FORMAT_FLOAT3X4_COLUMN_MAJOR", "RTC_FORMAT_FLOAT4X4_COLUMN_MAJOR")
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


def _soup_scene(rtc, dev, flags=0, n=64, seed=3):
    v, t = random_soup(n, seed)
    sc = rtc.Scene(dev, flags)
    sc.add_triangles(v, t)
    sc.commit()
    return sc, v, t


def _as_format(rtc, m34, name):
    m = np.asarray(m34, np.float32)
    if name.endswith("3X4_ROW_MAJOR"):
        return m.reshape(-1).copy()
    if name.endswith("3X4_COLUMN_MAJOR"):
        return m.T.reshape(-1).copy()
    full = np.eye(4, dtype=np.float32)
    full[:3] = m
    return full.T.reshape(-1).copy()


# ---- API surface ------------------------------------------------------------------------------------------------------------
def test_transform_round_trip_in_all_formats_and_identity_default(rtc):
    dev = rtc.Device("gpu=none")
    inner, _, _ = _soup_scene(rtc, dev)
    top = rtc.Scene(dev)
    gid = top.add_instance(inner)
    assert np.array_equal(top.get_instance_transform(gid), np.eye(4, dtype=np.float32)[:3])  # identity by default
    m = (np.arange(12, dtype=np.float32).reshape(3, 4) * 0.37 + 1.0)
    for fin in FORMATS:
        top.set_instance_transform(gid, _as_format(rtc, m, fin), getattr(rtc, fin))
        for fout in FORMATS:
            got = top.get_instance_transform(gid, getattr(rtc, fout))
            assert np.array_equal(got.reshape(-1), _as_format(rtc, m, fout)), (fin, fout)
        m = m + 1.0
    top.release()
    inner.release()
    dev.release()


def test_wrong_transform_format_is_an_invalid_argument(rtc):
    dev = rtc.Device("gpu=none")
    err = Errors(dev)
    g = dev.lib.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_INSTANCE)
    assert g and dev.error() == rtc.RTC_ERROR_NONE
    m = np.zeros(16, np.float32)
    for fmt in (rtc.RTC_FORMAT_FLOAT3, 0x9133, 0x9144, 0x9243):  # float3, 3x3 row-major, 4x4 row-major, 4x3 column-major
        dev.lib.rtcSetGeometryTransform(g, 0, fmt, m.ctypes.data)
        err.expect(rtc.RTC_ERROR_INVALID_ARGUMENT, "invalid matrix format")
        dev.lib.rtcGetGeometryTransform(g, 0.0, fmt, m.ctypes.data)
        err.expect(rtc.RTC_ERROR_INVALID_ARGUMENT, "invalid matrix format")
    dev.lib.rtcSetGeometryTransform(g, 1, rtc.RTC_FORMAT_FLOAT3X4_ROW_MAJOR, m.ctypes.data)  # time step 0 only
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "time step")
    dev.lib.rtcReleaseGeometry(g)
    dev.release()


def test_instanced_scene_must_be_on_the_same_device(rtc):
    dev, other = rtc.Device("gpu=none"), rtc.Device("gpu=none")
    err = Errors(dev)
    inner, _, _ = _soup_scene(rtc, other)
    g = dev.lib.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_INSTANCE)
    dev.lib.rtcSetGeometryInstancedScene(g, inner.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "different devices")
    dev.lib.rtcReleaseGeometry(g)
    inner.release()
    other.release()
    dev.release()


# ---- what is out of scope raises INVALID_OPERATION and says which ------------------------------------------------------------
def _commit_fails(rtc, top, err, text):
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, text)


@pytest.mark.parametrize("what", ["quads", "time steps", "subdivision", "instances"])
def test_instanced_scene_with_anything_but_static_triangles_is_refused(rtc, what):
    dev = rtc.Device("gpu=none,quad_accel=default")
    err = Errors(dev)
    v, t = random_soup(8, 1)
    inner = rtc.Scene(dev)
    inner.add_triangles(v, t)
    if what == "quads":
        inner.add_quads(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2, 3]], np.uint32))
    elif what == "time steps":
        inner.add_triangles_mb([v, v + 1], t)
    elif what == "subdivision":
        inner.add_subdiv(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), [4], [0, 1, 2, 3])
        inner.set_levels(2, 1)
    else:
        leaf, _, _ = _soup_scene(rtc, dev)
        inner.add_instance(leaf)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance(inner)
    _commit_fails(rtc, top, err, "static triangle meshes only")
    top.release()
    inner.release()
    dev.release()


def test_instanced_scenes_that_disagree_in_accel_kind_are_refused(rtc):
    dev = rtc.Device("gpu=none")
    err = Errors(dev)
    a, _, _ = _soup_scene(rtc, dev, ROBUST)
    b, _, _ = _soup_scene(rtc, dev, 0)
    top = rtc.Scene(dev)
    top.add_instance(a)
    top.add_instance(b, ih.affine((30, 0, 0)))
    _commit_fails(rtc, top, err, "disagree in triangle accel kind")
    dev.release()


def test_instance_time_steps_are_refused_at_commit(rtc):
    dev = rtc.Device("gpu=none")
    err = Errors(dev)
    inner, _, _ = _soup_scene(rtc, dev)
    top = rtc.Scene(dev)
    gid = top.add_instance(inner)
    dev.lib.rtcSetGeometryTimeStepCount(dev.lib.rtcGetGeometry(top.handle, gid), 2)
    assert dev.error() == rtc.RTC_ERROR_NONE
    _commit_fails(rtc, top, err, "more than one time step")
    dev.release()


def test_filter_function_inside_an_instanced_scene_is_refused(rtc):
    dev = rtc.Device("gpu=none")
    err = Errors(dev)
    inner, _, _ = _soup_scene(rtc, dev)
    fn = rtc.FILTER_FUNC(lambda args: None)
    inner.set_filters(0, intersect=fn)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance(inner)
    _commit_fails(rtc, top, err, "filter functions inside an instanced scene")
    dev.release()


def test_uncommitted_instanced_scene_is_refused_and_an_empty_one_left_out(rtc):
    dev = rtc.Device("gpu=none")
    err = Errors(dev)
    v, t = random_soup(8, 1)
    inner = rtc.Scene(dev)
    inner.add_triangles(v, t)  # not committed
    top = rtc.Scene(dev)
    top.add_instance(inner)
    _commit_fails(rtc, top, err, "instanced scene got not committed")
    inner.commit()
    top.commit()
    assert top.stats()["accelKind"] == ih.ACCEL_INST_TRI_MOELLER
    empty = rtc.Scene(dev)
    empty.commit()
    top.add_instance(empty)
    top.commit()
    assert len(top.accel_data(2).view(INST_DT)) == 1
    dev.release()


# ---- accel contents ---------------------------------------------------------------------------------------------------------
def _decode_child(node, i):
    lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for a in range(3):
        s = np.array([int(node["exp"][a]) << 23], np.uint32).view(np.float32)[0]
        o = node["origin"][a]
        lo[a] = np.float32(np.float64(node["q"][2 * a][i]) * np.float64(s) + np.float64(o))
        hi[a] = np.float32(np.float64(node["q"][2 * a + 1][i]) * np.float64(s) + np.float64(o))
    return lo, hi


def _top_leaves(nodes, root):
    """[(record, count, box or None, depth)] of the leaves reachable from root"""
    if root & LEAF:
        return [(root & 0x3FFFFFF, (root >> 26) & 31, None, 0)]
    out, todo = [], [(root, 1)]
    while todo:
        n, depth = todo.pop()
        for i, c in enumerate(nodes[n]["child"]):
            c = int(c)
            if c == EMPTY:
                continue
            if c & LEAF:
                out.append((c & 0x3FFFFFF, (c >> 26) & 31, _decode_child(nodes[n], i), depth))
            else:
                todo.append((c, depth + 1))
    return out


def _placements(n):
    """n transforms: a lattice of translations with a rotation and a non-uniform scale that differ per instance"""
    out = []
    for i in range(n):
        t = (25.0 * (i % 6), 25.0 * ((i // 6) % 6), 25.0 * (i // 36))
        out.append(ih.affine(t, (1.0 + 0.1 * (i % 4), 0.75, 1.25), ih.rotation((1, 1 + i % 3, 0.5), 13.0 * i)))
    return out


@pytest.mark.parametrize("flags,kind", [(ROBUST, ih.ACCEL_INST_TRI_PLUECKER), (0, ih.ACCEL_INST_TRI_MOELLER)])
@pytest.mark.parametrize("n", [1, 2, 9, 200])
def test_instance_accel_contents(rtc, n, flags, kind):
    dev = rtc.Device("gpu=none")
    inner, v, t = _soup_scene(rtc, dev, flags)
    inodes, iprims, iroot, istats = inner.accel_data(0).view(NODE_DT), inner.accel_data(1).view(TRI_DT), inner.accel_root(), inner.stats()
    assert len(iprims) == 64
    top = rtc.Scene(dev, flags)
    xf = _placements(n)
    gids = [top.add_instance(inner, m) for m in xf]
    top.commit()
    st = top.stats()
    assert st["accelKind"] == kind and st["primBytes"] == 64 and st["primCount"] == n and st["leafCount"] == n
    nodes, prims, recs, root = top.accel_data(0).view(NODE_DT), top.accel_data(1).view(TRI_DT), top.accel_data(2).view(INST_DT), top.accel_root()
    # one record per instance, the one instanced scene's records and nodes once, rebased behind the top-level tree
    assert len(recs) == n and sorted(recs["geomID"].tolist()) == gids
    assert prims.tobytes() == iprims.tobytes()
    ntop = len(nodes) - len(inodes)
    assert ntop >= 0
    tail = nodes[ntop:]
    for a, b in zip(tail, inodes):
        assert a["origin"].tobytes() == b["origin"].tobytes() and a["exp"].tobytes() == b["exp"].tobytes() and a["q"].tobytes() == b["q"].tobytes()
        for ca, cb in zip(a["child"].tolist(), b["child"].tolist()):
            assert ca == (cb if cb == EMPTY or cb & LEAF else cb + ntop)  # leaf offsets: the records start at 0
    want_root = iroot if iroot & LEAF else iroot + ntop
    assert (recs["root"] == want_root).all()
    # every top-level leaf holds exactly one instance, every instance has one, every child box holds its transformed corners
    leaves = _top_leaves(nodes[:ntop] if ntop else nodes, root)
    assert sorted(r for r, _, _, _ in leaves) == list(range(n)) and all(c == 1 for _, c, _, _ in leaves)
    lo, hi = v.min(0), v.max(0)
    corners = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)])
    all_lo, all_hi = np.full(3, np.inf), np.full(3, -np.inf)
    for rec_i, _, box, _ in leaves:
        m = xf[gids.index(int(recs["geomID"][rec_i]))]
        w = ih.xfm_points(m, corners)
        tol = 1e-5 * np.abs(w).max()
        all_lo, all_hi = np.minimum(all_lo, w.min(0)), np.maximum(all_hi, w.max(0))
        if box is not None:
            assert (box[0] <= w.min(0) + tol).all() and (box[1] >= w.max(0) - tol).all()
        # world2local is the inverse of local2world
        w2l = recs["world2local"][rec_i].reshape(4, 3).T  # columns vx, vy, vz, p -> [3,4]
        assert np.allclose(w2l, ih.world2local(m), rtol=1e-6, atol=1e-6)
    assert st["maxDepth"] == max(d for _, _, _, d in leaves) + 1 + istats["maxDepth"]
    blo, bhi = top.bounds()
    assert np.allclose(blo, all_lo, rtol=1e-5, atol=1e-4) and np.allclose(bhi, all_hi, rtol=1e-5, atol=1e-4)
    assert st["totalBytes"] == len(nodes) * 96 + len(prims) * 48 + len(recs) * 64
    top.release()
    inner.release()
    dev.release()


def test_two_distinct_instanced_scenes_are_stored_once_each(rtc):
    dev = rtc.Device("gpu=none")
    a, _, _ = _soup_scene(rtc, dev, seed=3)
    b, _, _ = _soup_scene(rtc, dev, n=40, seed=4)
    top = rtc.Scene(dev)
    for i in range(3):
        top.add_instance(a, ih.affine((30.0 * i, 0, 0)), geom_id=10 + i)
        top.add_instance(b, ih.affine((30.0 * i, 40, 0)), geom_id=20 + i)
    top.commit()
    prims, recs = top.accel_data(1).view(TRI_DT), top.accel_data(2).view(INST_DT)
    assert len(prims) == 64 + 40
    assert sorted(recs["geomID"].tolist()) == [10, 11, 12, 20, 21, 22]
    ra, rb = set(recs["root"][recs["geomID"] < 20].tolist()), set(recs["root"][recs["geomID"] >= 20].tolist())
    assert len(ra) == 1 and len(rb) == 1 and ra != rb
    dev.release()


def test_disabled_instance_is_absent_and_a_transform_change_shows_after_recommit(rtc):
    dev = rtc.Device("gpu=none")
    inner, _, _ = _soup_scene(rtc, dev)
    top = rtc.Scene(dev)
    g0 = top.add_instance(inner)
    g1 = top.add_instance(inner, ih.affine((50, 0, 0)))
    top.commit()
    assert len(top.accel_data(2).view(INST_DT)) == 2
    dev.lib.rtcDisableGeometry(dev.lib.rtcGetGeometry(top.handle, g0))
    top.commit()
    recs = top.accel_data(2).view(INST_DT)
    assert recs["geomID"].tolist() == [g1]
    assert np.allclose(recs["world2local"][0].reshape(4, 3).T, ih.world2local(ih.affine((50, 0, 0))))
    m = ih.affine((5, 6, 7), (2, 2, 2), ih.rotation((0, 1, 0), 30))
    top.set_instance_transform(g1, m)
    top.commit()
    recs = top.accel_data(2).view(INST_DT)
    assert np.allclose(recs["world2local"][0].reshape(4, 3).T, ih.world2local(m), rtol=1e-6, atol=1e-6)
    top.lib.rtcDetachGeometry(top.handle, g1)
    top.commit()
    assert top.stats()["accelKind"] == 0 and len(top.accel_data(2)) == 0
    dev.release()


def test_singular_transform_is_never_hit_and_no_error(rtc):
    dev = rtc.Device("gpu=none")
    inner, _, _ = _soup_scene(rtc, dev)
    top = rtc.Scene(dev)
    top.add_instance(inner, ih.affine((1, 2, 3), (1, 0, 1)))
    top.commit()
    recs = top.accel_data(2).view(INST_DT)
    assert len(recs) == 1 and not recs["world2local"].any()
    dev.release()


def test_tracing_instances_on_a_host_only_device_is_refused(rtc):
    dev = rtc.Device("gpu=none")
    inner, _, _ = _soup_scene(rtc, dev)
    top = rtc.Scene(dev)
    top.add_instance(inner)
    top.commit()
    rh = rtc.aligned_rayhits(1)
    top.intersect1M(rh, check=False)
    assert dev.error() != rtc.RTC_ERROR_NONE
    dev.release()


# ---- the inputs of the general-transform GPU test, pinned with the oracle alone ------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_general_transform_inputs_are_pinned(rtc, po, bomberman_tris, mode):
    v, tris = bomberman_tris
    meshes = {"m": (ih.snap(v * ih.SCALE), tris, 0)}
    inst = ih.general_instances()
    rays = ih.general_rays(rtc, po, meshes, inst)
    want, per = ih.oracle_instances(rtc, po, meshes, inst, rays, mode)
    hits = int((want["geomID"] != INVALID).sum())
    aside = int(ih.set_aside(want, per).sum())
    print(f"general transforms, mode {mode}: {hits} hits, {aside} rays may be set aside, {ih.equal_t_ties(per)} equal-t ties")
    assert hits > 2000
    assert ih.equal_t_ties(per) == 0
    assert aside <= 0.005 * hits
