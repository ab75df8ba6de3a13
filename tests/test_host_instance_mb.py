"""CPU tests of instance motion blur (instances with time steps, accel kinds 18..21) on a `gpu=none,quad_accel=default,inst_accel=default`
device: the one definition of world2local(time) (csrc/instance_xfm.h) against its numpy mirror and against float64, the time step API,
the accel's layout as accel.h documents it, what stays refused, and the pinning of the inputs of the general-transform GPU test."""
import ctypes as C

import numpy as np
import pytest

import instance_helpers as ih
import instance_mb_helpers as im
import instance_quads_helpers as iq
from helpers import random_soup
from instance_helpers import EMPTY, INST_DT, INVALID, LEAF, NODE_DT, TRI_DT
from instance_quads_helpers import QUAD_DT, ROBUST

CFG = "gpu=none,quad_accel=default,inst_accel=default"
ERRFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)
FORMATS = ("RTC_FORMAT_FLOAT3X4_ROW_MAJOR", "RTC_FORMAT_FLOAT3X4_COLUMN_MAJOR", "RTC_FORMAT_FLOAT4X4_COLUMN_MAJOR")
# rays the general-transform GPU test may set aside, per (quads, mode), and the hits they are a share of (test 6)
GENERAL_ASIDE = {(True, 0): (1, 10232), (True, 1): (1, 10232), (False, 0): (4, 10232), (False, 1): (4, 10232)}


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


# ---- the pinned cases of tests 1 and 2 ---------------------------------------------------------------------------------------------------
CASE_GEOMS, CASE_TIMES = 100, 20  # 2 000 (steps, time) cases


def _random_steps(rng):
    """2..5 steps: rotation x scales in [0.5, 2] x translation; the rotation between neighbouring steps is at most 60 degrees"""
    n = rng.randint(2, 6)
    rot = ih.rotation(rng.randn(3), rng.rand() * 360.0)
    steps = []
    for _ in range(n):
        steps.append(ih.affine(rng.rand(3) * 100.0 - 50.0, 0.5 + 1.5 * rng.rand(3), rot))
        rot = ih.rotation(rng.randn(3), rng.rand() * 60.0) @ rot
    return steps


def _case_times(rng, segments):
    """every k / S, some times outside [0, 1], the rest random in [0, 1]"""
    ks = [np.float32(k) / np.float32(segments) for k in range(segments + 1)]
    out = ks + [-0.25, 1.5, -1e-3, 1.0 + 1e-3]
    out += list(rng.rand(CASE_TIMES - len(out)))
    return np.asarray(out[:CASE_TIMES], np.float32)


@pytest.fixture(scope="module")
def cases(rtc):
    """[(steps, times, product's world2local [n,3,4], mirror's [n,3,4], mirror's ok)]"""
    rng = np.random.RandomState(20)
    dev = rtc.Device(CFG)
    out = []
    for _ in range(CASE_GEOMS):
        steps = _random_steps(rng)
        times = _case_times(rng, len(steps) - 1)
        g = dev.lib.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_INSTANCE)
        dev.lib.rtcSetGeometryTimeStepCount(g, len(steps))
        for i, m in enumerate(steps):
            dev.lib.rtcSetGeometryTransform(g, i, rtc.RTC_FORMAT_FLOAT3X4_ROW_MAJOR, np.ascontiguousarray(m).ctypes.data)
        got = np.zeros((len(times), 3, 4), np.float32)
        for k, t in enumerate(times):
            dev.lib.rtcamdGetGeometryWorld2Local(g, float(t), rtc.RTC_FORMAT_FLOAT3X4_ROW_MAJOR, got[k].ctypes.data)
        assert dev.error() == rtc.RTC_ERROR_NONE
        dev.lib.rtcReleaseGeometry(g)
        w, ok = im.world2local_at(steps, times)
        out.append((steps, times, got, w, ok))
    dev.release()
    return out


# ---- 1. the mirror equals the product, bit for bit -----------------------------------------------------------------------------------------
def test_world2local_export_equals_the_numpy_mirror_in_every_bit(cases):
    n = 0
    for steps, times, got, w, ok in cases:
        assert ok.all()
        assert got.tobytes() == w.tobytes(), (steps, times)
        n += len(times)
    assert n == 2000


# ---- 2. the same matrices against float64 --------------------------------------------------------------------------------------------------
def test_world2local_against_a_float64_inverse_of_the_float64_lerp(cases):
    """Bound: 1e-5 x the largest entry of the matrix (about 20 roundings of 2^-24 times the condition number <= 8 of these inputs).
    Measured maximum over the 2 000 cases: 3.685e-06 x the largest entry (printed by this test)."""
    worst = 0.0
    for steps, times, got, _, _ in cases:
        ref = im.world2local_f64(steps, times)
        err = np.abs(got.astype(np.float64) - ref).reshape(len(times), -1).max(1) / np.abs(ref).reshape(len(times), -1).max(1)
        worst = max(worst, float(err.max()))
    print(f"world2local vs float64: largest error {worst:.3e} x the largest entry")
    assert worst <= 1e-5


# ---- 3. rtcGetGeometryTransform(time) and the time step API -----------------------------------------------------------------------------------
def _as_format(m34, name):
    m = np.asarray(m34, np.float32)
    if name.endswith("3X4_ROW_MAJOR"):
        return m.reshape(-1).copy()
    if name.endswith("3X4_COLUMN_MAJOR"):
        return m.T.reshape(-1).copy()
    full = np.eye(4, dtype=np.float32)
    full[:3] = m
    return full.T.reshape(-1).copy()


def test_get_transform_returns_the_lerp_and_steps_round_trip(rtc):
    dev = rtc.Device(CFG)
    v, t = random_soup(8, 1)
    inner = rtc.Scene(dev)
    inner.add_triangles(v, t)
    inner.commit()
    rng = np.random.RandomState(4)
    steps = _random_steps(rng)
    while len(steps) < 3:
        steps = _random_steps(rng)
    top = rtc.Scene(dev)
    gid = top.add_instance_mb(inner, steps)
    # per step: 3x4 row-major in, 4x4 column-major out and back in, 3x4 row-major out - the step's time is k / S
    S = len(steps) - 1
    for k, m in enumerate(steps):
        tk = float(np.float32(k) / np.float32(S))
        full = top.get_instance_transform(gid, rtc.RTC_FORMAT_FLOAT4X4_COLUMN_MAJOR, time=tk)
        assert np.array_equal(full, _as_format(m, "RTC_FORMAT_FLOAT4X4_COLUMN_MAJOR"))
        top.set_instance_transform(gid, full, rtc.RTC_FORMAT_FLOAT4X4_COLUMN_MAJOR, time_step=k)
        assert np.array_equal(top.get_instance_transform(gid, time=tk), m)
    times = np.concatenate([np.random.RandomState(5).rand(50), [-0.5, 0.0, 1.0, 1.75]]).astype(np.float32)
    want = im.lerp_at(steps, times)
    for k, tm in enumerate(times):
        for f in FORMATS:
            got = top.get_instance_transform(gid, getattr(rtc, f), time=float(tm))
            assert np.array_equal(got.reshape(-1), _as_format(want[k], f)), (tm, f)
    # the lerp and its inverse belong together
    w = top.instance_world2local(gid, 0.3)
    m = np.eye(4)
    m[:3] = top.get_instance_transform(gid, time=0.3)
    assert np.allclose(np.linalg.inv(m)[:3], w, rtol=1e-5, atol=1e-4)
    top.release()
    inner.release()
    dev.release()


def test_time_step_count_keeps_old_steps_and_fills_new_ones_with_the_identity(rtc):
    dev = rtc.Device(CFG)
    err = Errors(dev)
    L = dev.lib
    g = L.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_INSTANCE)
    fmt = rtc.RTC_FORMAT_FLOAT3X4_ROW_MAJOR
    ident = np.eye(4, dtype=np.float32)[:3]
    a, b = ih.affine((1, 2, 3), (2, 2, 2)), ih.affine((-4, 5, 6), (1, 0.5, 3), ih.rotation((1, 2, 3), 40.0))

    def get(time):
        out = np.zeros((3, 4), np.float32)
        L.rtcGetGeometryTransform(g, time, fmt, out.ctypes.data)
        return out

    L.rtcSetGeometryTransform(g, 0, fmt, a.ctypes.data)
    L.rtcSetGeometryTransform(g, 1, fmt, a.ctypes.data)  # one step: only time step 0 exists
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "time step")
    L.rtcSetGeometryTimeStepCount(g, 3)
    assert dev.error() == rtc.RTC_ERROR_NONE
    assert np.array_equal(get(0.0), a) and np.array_equal(get(0.5), ident) and np.array_equal(get(1.0), ident)
    L.rtcSetGeometryTransform(g, 2, fmt, b.ctypes.data)
    L.rtcSetGeometryTransform(g, 3, fmt, b.ctypes.data)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "time step")
    assert np.array_equal(get(1.0), b)
    L.rtcSetGeometryTimeStepCount(g, 5)  # steps 0..2 kept, 3 and 4 the identity
    assert np.array_equal(get(0.0), a) and np.array_equal(get(0.25), ident) and np.array_equal(get(0.5), b)
    assert np.array_equal(get(0.75), ident) and np.array_equal(get(1.0), ident)
    L.rtcSetGeometryTimeStepCount(g, 1)  # back to one step: step 0, whatever the time
    assert np.array_equal(get(0.0), a) and np.array_equal(get(0.7), a)
    L.rtcSetGeometryTransform(g, 1, fmt, b.ctypes.data)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "time step")
    L.rtcSetGeometryTimeStepCount(g, 0)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "time steps out of range")
    L.rtcSetGeometryTimeStepCount(g, 130)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "time steps out of range")
    L.rtcReleaseGeometry(g)
    dev.release()


def test_world2local_export_checks_its_arguments_and_serves_one_step(rtc):
    dev = rtc.Device(CFG)
    err = Errors(dev)
    L = dev.lib
    out = np.zeros(16, np.float32)
    g = L.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_INSTANCE)
    assert dev.error() == rtc.RTC_ERROR_NONE
    L.rtcamdGetGeometryWorld2Local(g, 0.0, rtc.RTC_FORMAT_FLOAT3X4_ROW_MAJOR, None)
    err.expect(rtc.RTC_ERROR_INVALID_ARGUMENT, "is null")
    L.rtcamdGetGeometryWorld2Local(g, 0.0, rtc.RTC_FORMAT_FLOAT3, out.ctypes.data)
    err.expect(rtc.RTC_ERROR_INVALID_ARGUMENT, "invalid matrix format")
    tri = L.rtcNewGeometry(dev.handle, rtc.RTC_GEOMETRY_TYPE_TRIANGLE)
    L.rtcamdGetGeometryWorld2Local(tri, 0.0, rtc.RTC_FORMAT_FLOAT3X4_ROW_MAJOR, out.ctypes.data)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "not supported for this geometry")
    L.rtcReleaseGeometry(tri)
    # one step: the stored world2local of the static path (float64 inverse rounded once), in every format, for every time
    m = ih.affine((3, -2, 7), (1.5, 0.75, 2.0), ih.rotation((1, 2, 0.5), 33.0))
    L.rtcSetGeometryTransform(g, 0, rtc.RTC_FORMAT_FLOAT3X4_ROW_MAJOR, m.ctypes.data)
    for f in FORMATS:
        for time in (0.0, 0.6):
            out[:] = 0
            L.rtcamdGetGeometryWorld2Local(g, time, getattr(rtc, f), out.ctypes.data)
            want = _as_format(ih.world2local(m), f)
            assert np.array_equal(out[:len(want)], want), f
    sing = ih.affine((1, 2, 3), (1, 0, 1))  # singular: all zero
    L.rtcSetGeometryTransform(g, 0, rtc.RTC_FORMAT_FLOAT3X4_ROW_MAJOR, sing.ctypes.data)
    out[:] = 1
    L.rtcamdGetGeometryWorld2Local(g, 0.0, rtc.RTC_FORMAT_FLOAT3X4_ROW_MAJOR, out.ctypes.data)
    assert not out[:12].any() and dev.error() == rtc.RTC_ERROR_NONE
    L.rtcReleaseGeometry(g)
    dev.release()


# ---- 4. accel contents ---------------------------------------------------------------------------------------------------------------------------
def _random_quads(n, seed, extent=10.0, size=1.0):
    rng = np.random.RandomState(seed)
    c = rng.rand(n, 1, 3) * extent
    v = (c + (rng.rand(n, 4, 3) - 0.5) * size).astype(np.float32).reshape(-1, 3)
    return v, np.arange(4 * n, dtype=np.uint32).reshape(-1, 4)


def _inner(rtc, dev, flags, ntris, nquads, seed=3):
    sc = rtc.Scene(dev, flags)
    vs = []
    if ntris:
        v, t = random_soup(ntris, seed)
        sc.add_triangles(v, t, geom_id=0)
        vs.append(v)
    if nquads:
        v, q = _random_quads(nquads, seed + 1)
        sc.add_quads(v, q, geom_id=1)
        vs.append(v)
    sc.commit()
    return sc, np.concatenate(vs)


def _decode_child(node, i):
    lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for a in range(3):
        s = np.array([int(node["exp"][a]) << 23], np.uint32).view(np.float32)[0]
        o = node["origin"][a]
        lo[a] = np.float32(np.float64(node["q"][2 * a][i]) * np.float64(s) + np.float64(o))
        hi[a] = np.float32(np.float64(node["q"][2 * a + 1][i]) * np.float64(s) + np.float64(o))
    return lo, hi


def _top_leaves(nodes, root):
    """[(record, count, box or None)] of the top-level leaves (the top-level tree comes first: its leaves are reached before any
    instanced tree, whose nodes no top-level node refers to)"""
    if root & LEAF:
        return [(root & 0x3FFFFFF, (root >> 26) & 31, None)]
    out, todo = [], [root]
    while todo:
        n = todo.pop()
        for i, c in enumerate(nodes[n]["child"]):
            c = int(c)
            if c == EMPTY:
                continue
            if c & LEAF:
                out.append((c & 0x3FFFFFF, (c >> 26) & 31, _decode_child(nodes[n], i)))
            else:
                todo.append(c)
    return out


def _placements(n, moving_every=2):
    """n instances on a lattice; every `moving_every`-th has one step, the others 2..4 steps that rotate, scale and move"""
    out = []
    for i in range(n):
        t = np.array([25.0 * (i % 6), 25.0 * ((i // 6) % 6), 25.0 * (i // 36)])
        nsteps = 1 if i % moving_every == 0 else 2 + i % 3
        steps = [ih.affine(t + j * np.array([2.0, -1.0, 0.5 * i]), (1.0 + 0.1 * (i % 4) + 0.05 * j, 0.75, 1.25), ih.rotation((1, 1 + i % 3, 0.5), 13.0 * i + 25.0 * j))
                 for j in range(nsteps)]
        out.append(steps)
    return out


@pytest.mark.parametrize("flags", [0, ROBUST])
@pytest.mark.parametrize("nquads", [0, 30])
@pytest.mark.parametrize("n", [1, 2, 9, 60])
def test_accel_contents(rtc, n, nquads, flags):
    dev = rtc.Device(CFG)
    inner, verts = _inner(rtc, dev, flags, 64, nquads)
    placements = _placements(n, moving_every=3 if n > 1 else 2)
    if n == 1:
        placements = _placements(2)[1:]  # the only instance moves
    top = rtc.Scene(dev, flags)
    gids = [top.add_instance(inner, s[0]) if len(s) == 1 else top.add_instance_mb(inner, s) for s in placements]
    top.commit()
    st = top.stats()
    assert st["accelKind"] == im.kind(0 if flags else 1, nquads > 0)
    nodes, prims, blobs, root = top.accel_data(0).view(NODE_DT), top.accel_data(1).view(TRI_DT), top.accel_data(2), top.accel_root()
    nsteps = sum(len(s) for s in placements if len(s) > 1)
    assert st["leafCount"] == n and st["primBytes"] == 64 and len(blobs) == 64 * (n + nquads + nsteps)
    recs = blobs[:64 * n].view(INST_DT)
    quads = blobs[64 * n:64 * (n + nquads)].view(QUAD_DT)
    all_steps = blobs.view(im.STEP_DT)  # indexed in 64-byte units from the start of `blobs`
    assert sorted(recs["geomID"].tolist()) == gids
    own_quads = b""
    if nquads:  # the quad records as a scene of the quads alone exports them
        qs, _ = _inner(rtc, dev, flags, 0, nquads)
        own_quads = qs.accel_data(2).tobytes()
        qs.release()
    assert quads.tobytes() == own_quads and len(quads) == nquads
    assert prims.tobytes() == inner.accel_data(1).tobytes()
    lo, hi = verts.min(0), verts.max(0)
    corners = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)])
    leaves = _top_leaves(nodes, root)
    assert sorted(r for r, _, _ in leaves) == list(range(n)) and all(c == 1 for _, c, _ in leaves)
    used = []
    all_lo, all_hi = np.full(3, np.inf), np.full(3, -np.inf)
    for rec_i, _, box in leaves:
        r = recs[rec_i]
        steps = placements[gids.index(int(r["geomID"]))]
        # world2local: the inverse of step 0 as the static path computes it
        assert np.array_equal(r["world2local"].reshape(4, 3).T, ih.world2local(steps[0]))
        if len(steps) == 1:
            assert r["pad"][1] == 0
        else:
            S, first = int(r["pad"][1]) >> 24, int(r["pad"][1]) & 0xFFFFFF
            assert S == len(steps) - 1 and n + nquads <= first and first + len(steps) <= n + nquads + nsteps
            for j, m in enumerate(steps):
                assert np.array_equal(all_steps["local2world"][first + j].reshape(4, 3).T, m) and not all_steps["pad"][first + j].any()
            used += list(range(first, first + len(steps)))
        for m in steps:  # the leaf's box contains all eight corners of every step
            w = ih.xfm_points(m, corners)
            tol = 1e-5 * np.abs(w).max()
            all_lo, all_hi = np.minimum(all_lo, w.min(0)), np.maximum(all_hi, w.max(0))
            if box is not None:
                assert (box[0] <= w.min(0) + tol).all() and (box[1] >= w.max(0) - tol).all()
    assert sorted(used) == list(range(n + nquads, n + nquads + nsteps))  # every step once, behind the quads, without gaps
    blo, bhi = top.bounds()
    assert np.allclose(blo, all_lo, rtol=1e-5, atol=1e-4) and np.allclose(bhi, all_hi, rtol=1e-5, atol=1e-4)
    assert st["totalBytes"] == len(nodes) * 96 + len(prims) * 48 + len(blobs)
    top.release()
    inner.release()
    dev.release()


@pytest.mark.parametrize("flags", [0, ROBUST])
@pytest.mark.parametrize("nquads", [0, 30])
def test_one_step_instances_build_the_static_kinds_byte_for_byte(rtc, flags, nquads):
    """however the single step was set: directly, through rtcSetGeometryTimeStepCount(1), or after a count of 3 that went back to 1"""
    got = []
    for how in ("plain", "count1", "back"):
        dev = rtc.Device(CFG)
        inner, _ = _inner(rtc, dev, flags, 64, nquads)
        top = rtc.Scene(dev, flags)
        for i, steps in enumerate(_placements(9, moving_every=1)):
            if how == "plain":
                gid = top.add_instance(inner, steps[0])
            else:
                gid = top.add_instance_mb(inner, [steps[0]] if how == "count1" else [steps[0], steps[0] + 1, steps[0] * 2])
            if how == "back":
                top.lib.rtcSetGeometryTimeStepCount(top.lib.rtcGetGeometry(top.handle, gid), 1)
                top.lib.rtcCommitGeometry(top.lib.rtcGetGeometry(top.handle, gid))
        top.commit()
        st = top.stats()
        assert st["accelKind"] == im.static_kind(0 if flags else 1, nquads > 0)
        assert not top.accel_data(2)[:64 * 9].view(INST_DT)["pad"][:, 1].any()
        got.append(([top.accel_data(k).tobytes() for k in range(4)], st["accelKind"], top.accel_root(), st["maxDepth"]))
        top.release()
        inner.release()
        dev.release()
    assert got[0] == got[1] == got[2]


def test_moving_scene_keeps_the_static_layout_in_front_of_the_steps(rtc):
    """kinds 18..21 are the static layout plus steps: with the moving instances' steps all equal to step 0 the top-level tree, the trees,
    the records apart from pad[1] and the quads are the bytes of the static scene"""
    dev = rtc.Device(CFG)
    inner, _ = _inner(rtc, dev, 0, 64, 30)
    placements = _placements(9, moving_every=1)
    a, b = rtc.Scene(dev), rtc.Scene(dev)
    for i, steps in enumerate(placements):
        a.add_instance(inner, steps[0])
        if i % 2:
            b.add_instance_mb(inner, [steps[0]] * (2 + i % 3))
        else:
            b.add_instance(inner, steps[0])
    a.commit()
    b.commit()
    assert a.stats()["accelKind"] == iq.ACCEL_INST_MOELLER and b.stats()["accelKind"] == im.ACCEL_INSTMB_MOELLER
    assert a.accel_data(0).tobytes() == b.accel_data(0).tobytes() and a.accel_data(1).tobytes() == b.accel_data(1).tobytes()
    assert a.accel_root() == b.accel_root() and a.stats()["maxDepth"] == b.stats()["maxDepth"]
    sa, sb = a.accel_data(2), b.accel_data(2)
    rb = sb[:len(sa)].copy()
    moving = rb[:64 * 9].view(INST_DT)["pad"][:, 1] != 0
    assert int(moving.sum()) == 4
    rb[:64 * 9].view(INST_DT)["pad"][:, 1] = 0
    assert rb.tobytes() == sa.tobytes()
    a.release()
    b.release()
    inner.release()
    dev.release()


# ---- 5. what stays refused -------------------------------------------------------------------------------------------------------------------
def test_instance_with_steps_on_a_plain_host_only_device_is_refused(rtc):
    dev = rtc.Device("gpu=none")
    err = Errors(dev)
    v, t = random_soup(8, 1)
    inner = rtc.Scene(dev)
    inner.add_triangles(v, t)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance_mb(inner, [ih.affine(), ih.affine((0, 0, 2))])
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "instances with more than one time step are not supported")
    dev.release()


def test_instanced_scene_with_time_steps_stays_refused(rtc):
    dev = rtc.Device(CFG)
    err = Errors(dev)
    v, t = random_soup(8, 1)
    inner = rtc.Scene(dev)
    inner.add_triangles(v, t)
    inner.add_triangles_mb([v, v + 1], t)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance_mb(inner, [ih.affine(), ih.affine((0, 0, 2))])
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "static triangle and quad meshes only (no time steps, subdivision meshes or instances)")
    dev.release()


def test_step_with_bounds_that_are_not_finite_is_refused(rtc):
    dev = rtc.Device(CFG)
    err = Errors(dev)
    v, t = random_soup(8, 1)
    inner = rtc.Scene(dev)
    inner.add_triangles(v, t)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance_mb(inner, [ih.affine(), ih.affine((0, 0, 2)), ih.affine((0, np.inf, 0))])
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "bounds that are not finite")
    dev.release()


# ---- 6. the set-aside cap of the general-transform GPU test, with the oracle alone -------------------------------------------------------------
def general_scenes(bomberman, bomberman_tris, rtc, quads):
    if quads:
        return iq.quads_only(bomberman)
    v, t = bomberman_tris
    return {"m": {"tris": (ih.snap(v * ih.SCALE), t.astype(np.uint32), 0), "quads": None}}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("quads", [True, False])
def test_general_transform_inputs_are_pinned(rtc, po, bomberman, bomberman_tris, quads, mode):
    scenes = general_scenes(bomberman, bomberman_tris, rtc, quads)
    inst = im.general_instances()
    assert [len(s) for _, _, s in inst] == [3, 2, 3, 2, 3, 2, 3, 2, 3]
    rays = im.rays_with_times(rtc, po, scenes, inst, im.GENERAL_RAYS, im.GENERAL_SEED)
    want, per, isb, want_tri = im.oracle_instances(rtc, po, scenes, inst, rays, mode)
    hits = int((want["geomID"] != INVALID).sum())
    aside = int((iq.quad_set_aside(want, per, want_tri, [0]) if quads else ih.set_aside(want, per)).sum())
    print(f"general moving transforms over {'quads' if quads else 'triangles'}, mode {mode}: {hits} hits, {aside} rays may be set aside, {ih.equal_t_ties(per)} equal-t ties")
    assert hits > 1000
    assert aside <= 0.01 * hits
    assert (aside, hits) == GENERAL_ASIDE[(quads, mode)]
