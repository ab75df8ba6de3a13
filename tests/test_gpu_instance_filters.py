"""Filter functions on instanced meshes (device config inst_filters=1): geometry intersect / occluded filters inside instanced mesh
scenes and RTCIntersectContext::filter on scenes with mesh instances.  The device finds the closest candidate, the host runs the
callbacks, a rejected candidate goes on the ray's exclusion list - keyed by (instance, geomID, primID, bits of t) - and the ray is traced
again by the EXCL form of the two-level kernel (trace_instance_filter.hip).  Scenes and anchors: tests/inst_filter_helpers.py."""
import ctypes as C

import numpy as np
import pytest

import deep_stack_helpers as ds
import inst_filter_helpers as fh
import instance_helpers as ih
import instance_quads_helpers as iq
from helpers import fill_rays, random_rays_np

pytestmark = pytest.mark.gpu

INVALID = fh.INVALID
NQ = fh.NQ
TWO = [(0, (0.0, 0.0, 0.0)), (1, (2.0, 0.0, 0.0))]  # two instances side by side


@pytest.fixture(autouse=True)
def callback_errors():
    """asserts inside the callbacks count: ctypes would print and drop them"""
    fh.CALLBACK_ERRORS.clear()
    yield
    assert not fh.CALLBACK_ERRORS, fh.CALLBACK_ERRORS[:3]


RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]


def _alpha(rtc, calls=None, checks=None):
    """the alpha test of test 1: on instance 0 geometry g rejects x_local < 0.2 (g + 1), instance 1 rejects every even g"""
    def body(a):
        if calls is not None:
            calls.append((a.ray_id, a.inst, a.geom, a.prim, a.tfar))
        if checks is not None:
            checks(a)
        if a.inst == 0:
            if np.float32(a.x) < np.float32(0.2 * (a.geom + 1)):
                a.reject()
        elif a.geom % 2 == 0:
            a.reject()
    return fh.filter_func(rtc, body)


def _alpha_want(xl, which):
    """the accepted geometry: instance 0 - the first g with x >= 0.2 (g + 1), else the unfiltered last one; instance 1 - geometry 1"""
    g0 = np.array([next(g for g in range(NQ) if g == NQ - 1 or xi >= np.float32(0.2 * (g + 1))) for xi in xl])
    return np.where(which == 0, g0, 1)


# ---- 1. closed form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robust", [True, False])
def test_closed_form_alpha_test_per_instance(rtc, robust):
    calls = []
    flt = _alpha(rtc, calls)
    dev, top, inner = fh.stack_top(rtc, fh.cfg(robust), TWO, intersect=flt, filtered=range(NQ - 1))  # the last quad has no filter
    assert top.stats()["accelKind"] == (14 if robust else 15)
    n = 2000
    rh, xl, yl, which = fh.stack_rays(rtc, n, TWO)
    top.intersect1M(rh)
    want = _alpha_want(xl, which)
    assert np.array_equal(rh["geomID"], want.astype(np.uint32))
    assert np.array_equal(rh["instID"], which.astype(np.uint32))
    assert np.array_equal(rh["tfar"], (want + 1.0).astype(np.float32))  # exact: the local ray is exact, t = z_plane + 1
    assert np.array_equal(rh["primID"], (yl > xl).astype(np.uint32))
    # every candidate in front of the accepted one was offered exactly once, nearest first
    per_ray = {}
    for rid, inst, g, prim, t in calls:
        assert inst == which[rid] and prim == int(yl[rid] > xl[rid]) and t == np.float32(g + 1.0)
        per_ray.setdefault(rid, []).append(g)
    for i in range(n):
        assert per_ray[i] == list(range(min(want[i], NQ - 2) + 1)), (i, which[i], want[i], per_ray[i])
    fh.release(dev, top, inner)


# ---- 2. the instance is part of the key ----------------------------------------------------------------------------------------------------
def test_twin_instances_are_told_apart_by_the_instance_in_the_key(rtc):
    places = [(0, (0.0, 0.0, 0.0)), (1, (0.0, 0.0, 0.0)), (2, (0.0, 0.0, 0.5))]  # 0 and 1: the same transform, the same t bits and ids
    n = 600
    rays, xl, yl, which = fh.stack_rays(rtc, n, [places[0]])
    rejections = 0
    for twin, other in ((0, 1), (1, 0)):
        calls = []

        def body(a):
            calls.append((a.ray_id, a.inst, a.geom, a.prim))
            if a.inst == twin:
                a.reject()
        flt = fh.filter_func(rtc, body)
        dev, top, inner = fh.stack_top(rtc, fh.cfg(True), places, intersect=flt)
        got = fh.copy_of(rtc, rays)
        top.intersect1M(got)
        # the anchor: no filter anywhere, the rejected twin disabled
        dev2, top2, inner2 = fh.stack_top(rtc, fh.cfg(True), places)
        top2.set_enabled(twin, False)
        top2.commit()
        want = fh.copy_of(rtc, rays)
        top2.intersect1M(want)
        assert (want["instID"] == other).all() and (want["geomID"] == 0).all() and (want["tfar"] == 1.0).all()
        for f in ("instID", "geomID", "primID", "tfar"):
            assert got[f].tobytes() == want[f].tobytes(), (twin, f)
        assert got.tobytes() == want.tobytes()
        # each rejected candidate was offered exactly once, and it is the rejected twin's quad 0 (the other twin's lies at the same t and ends the ray)
        rejected = [c for c in calls if c[1] == twin]
        assert len(rejected) == len(set(rejected)) and all(c[2] == 0 for c in calls)
        assert len(calls) == len(set(calls)) == n + len(rejected)
        rejections += len(rejected)
        fh.release(dev2, top2, inner2)
        fh.release(dev, top, inner)
    # of two candidates at one t the kernel reports one: every ray had its first candidate rejected in exactly one of the two roles
    assert rejections == n


# ---- 3. what the callback sees --------------------------------------------------------------------------------------------------------------
class DerivedContext(C.Structure):
    """an application's context: RTCIntersectContext first, its own fields behind"""
    _fields_ = [("flags", C.c_int), ("filter", C.c_void_p), ("instID", C.c_uint * 1), ("pad", C.c_uint * 5), ("counter", C.c_ulonglong), ("magic", C.c_ulonglong)]


def test_what_the_callbacks_see(rtc):
    places = [(3, (0.0, 0.0, 0.0)), (9, (2.0, 0.0, 0.0))]
    tags = (C.c_uint * NQ)(*[1000 + g for g in range(NQ)])
    seen = {"geom": 0, "ctx": 0}
    d = DerivedContext()

    def geom_body(a):
        seen["geom"] += 1
        assert a.a.N == 1 and a.a.valid[0] == -1
        assert a.ctx.instID[0] == a.inst and a.inst in (3, 9)
        assert a.a.geometryUserPtr == C.addressof(tags) + 4 * a.geom  # the INSTANCED geometry's user data
        assert C.cast(a.a.geometryUserPtr, C.POINTER(C.c_uint))[0] == 1000 + a.geom
        assert a.tfar == np.float32(a.geom + 1.0)  # ray.tfar is the candidate's t while the callback runs
        assert a.a.context == C.addressof(d)       # the caller's own object, not a copy
        if a.geom < 2:
            a.reject()

    def ctx_body(a):
        seen["ctx"] += 1
        assert a.a.N == 1 and a.a.valid[0] == -1 and a.geom >= 2  # runs after the geometry's filter, only where that left the lane valid
        assert a.ctx.instID[0] == a.inst
        assert a.a.geometryUserPtr == C.addressof(tags) + 4 * a.geom
        mine = C.cast(a.a.context, C.POINTER(DerivedContext)).contents
        assert mine.magic == 0xC0FFEE1234
        mine.counter += 1
        if a.geom == 2:
            a.reject()

    gf, cf = fh.filter_func(rtc, geom_body), fh.filter_func(rtc, ctx_body)
    dev, top, inner = fh.stack_top(rtc, fh.cfg(True), places, intersect=gf)
    for g in range(NQ):
        inner.set_user_data(g, C.addressof(tags) + 4 * g)
    n = 128
    rh, xl, yl, which = fh.stack_rays(rtc, n, places)
    d.flags, d.filter, d.counter, d.magic = 0, C.cast(cf, C.c_void_p).value, 0, 0xC0FFEE1234
    d.instID[0] = 77
    top.lib.rtcIntersect1M(top.handle, C.cast(C.pointer(d), C.POINTER(rtc.RTCIntersectContext)), rh.ctypes.data, n, 80)
    dev.check("rtcIntersect1M")
    assert d.instID[0] == 77  # the value the caller's context had at the call
    assert (rh["geomID"] == 3).all() and (rh["tfar"] == 4.0).all()
    assert np.array_equal(rh["instID"], np.where(which == 0, 3, 9).astype(np.uint32))
    assert seen["geom"] == n * 4 and seen["ctx"] == n * 2 and d.counter == n * 2
    fh.release(dev, top, inner)


# ---- 4. reject-all -----------------------------------------------------------------------------------------------------------------------
def test_reject_all_leaves_the_records_untouched(rtc):
    seen = []

    def body(a):
        seen.append((a.ray_id, a.inst, a.geom, a.prim, a.tfar))
        a.reject()
    collect = fh.filter_func(rtc, body)
    places = TWO + [(2, (0.0, 0.0, 10.0))]  # the third instance lies behind the first: its quads are pierced by the same rays
    dev, top, inner = fh.stack_top(rtc, fh.cfg(True), places, intersect=collect, occluded=collect)
    n = 96
    rh, xl, yl, which = fh.stack_rays(rtc, n, TWO, seed=3)
    before = rh.copy()
    top.intersect1M(rh)
    assert rh.tobytes() == before.tobytes()
    pierced = int((which == 0).sum()) * 2 * NQ + int((which == 1).sum()) * NQ  # triangles over all instances
    assert len(seen) == len(set(seen)) == pierced
    occ = fh.occ_of(rtc, before)
    seen.clear()
    top.occluded1M(occ)
    assert occ.tobytes() == fh.occ_of(rtc, before).tobytes() and len(seen) == len(set(seen)) == pierced  # tfar stays unchanged
    fh.release(dev, top, inner)


# ---- 5. occlusion filter -----------------------------------------------------------------------------------------------------------------
def test_occlusion_filter_below_instances(rtc):
    def body(a):  # quads 0..2 are transparent for shadow rays
        if a.geom < 3:
            a.reject()
    only_far = fh.filter_func(rtc, body)
    dev, top, inner = fh.stack_top(rtc, fh.cfg(True), TWO, occluded=only_far)
    assert top.filter_flags() == rtc.RTCAMD_SCENE_FILTER_INSTANCED_OCCLUDED
    n = 512
    src, _, _, _ = fh.stack_rays(rtc, n, TWO, seed=5)
    occ = fh.occ_of(rtc, src)
    occ["tfar"][: n // 2] = 3.5  # these rays end between quad 2 (t = 3) and quad 3 (t = 4): nothing opaque in range
    top.occluded1M(occ)
    assert (occ["tfar"][: n // 2] == np.float32(3.5)).all()
    assert np.isneginf(occ["tfar"][n // 2:]).all()
    # closest-hit queries do not run the occlusion filter
    rh = fh.copy_of(rtc, src)
    top.intersect1M(rh)
    assert (rh["geomID"] == 0).all() and (rh["tfar"] == 1.0).all()
    fh.release(dev, top, inner)


# ---- 6. context filter on a scene with instances ---------------------------------------------------------------------------------------------
def test_context_filter_on_a_scene_with_instances(rtc):
    def body(a):
        if a.prim == 1:
            a.reject()
    no_prim1 = fh.filter_func(rtc, body)
    dev, top, inner = fh.stack_top(rtc, fh.cfg(True), TWO)
    assert top.filter_flags() == 0
    n = 512
    rh, xl, yl, which = fh.stack_rays(rtc, n, TWO, seed=6)
    before = rh.copy()
    top.intersect1M(rh, ctx=fh.context_with(rtc, no_prim1))
    upper = yl > xl  # triangle (0, 2, 3) = primID 1 covers y > x
    assert rh[upper].tobytes() == before[upper].tobytes()
    assert (rh["geomID"][~upper] == 0).all() and (rh["primID"][~upper] == 0).all() and (rh["tfar"][~upper] == 1.0).all()
    assert np.array_equal(rh["instID"][~upper], which[~upper].astype(np.uint32))
    occ = fh.occ_of(rtc, before)
    top.occluded1M(occ, ctx=fh.context_with(rtc, no_prim1))
    assert np.array_equal(occ["tfar"] == -np.inf, ~upper) and (occ["tfar"][upper] == np.inf).all()
    fh.release(dev, top, inner)


# ---- 7. the top scene's own filtered triangles beside filtered instances, in one batch ----------------------------------------------------------
def test_own_filtered_triangles_beside_filtered_instances(rtc):
    """Over instance 0 the top scene has a triangle pair of its own at z = 0.5 (between the instance's quads 0 and 1) and one at z = 1.5,
    geomIDs 20 and 21, with a filter of their own that rejects 20.  The instanced geometries reject g = 0 and g = 1: a ray over instance 0
    is offered quad 0 (rejected, INST list), then 20 (rejected, TRI list), then quad 1 (rejected, INST list) and ends on 21; over instance
    1 it ends on quad 2."""
    order = {}

    def inst_body(a):
        order.setdefault(a.ray_id, []).append(("i", a.inst, a.geom))
        assert a.ctx.instID[0] == a.inst
        if a.geom < 2:
            a.reject()

    def own_body(a):
        order.setdefault(a.ray_id, []).append(("o", a.inst, a.geom))
        assert a.ctx.instID[0] == 55 and a.inst == 55  # not on an instance: the context's value
        if a.geom == 20:
            a.reject()
    fi, fo = fh.filter_func(rtc, inst_body), fh.filter_func(rtc, own_body)

    def extra(top):
        for gid, z in ((20, 0.5), (21, 1.5)):
            assert top.add_triangles((fh.SQUARE + (0, 0, z)).astype(np.float32), fh.SQUARE_TRIS, geom_id=gid) == gid
            top.set_filters(gid, intersect=fo)
    dev, top, inner = fh.stack_top(rtc, fh.cfg(True), TWO, intersect=fi, extra=extra)
    assert top.filter_flags() == rtc.RTCAMD_SCENE_FILTER_INSTANCED_INTERSECT | rtc.RTCAMD_SCENE_FILTER_MESH_INTERSECT
    n = 400
    rh, xl, yl, which = fh.stack_rays(rtc, n, TWO, seed=7)
    top.intersect1M(rh, ctx=rtc.make_context(inst_id=55))
    first = which == 0
    assert np.array_equal(rh["geomID"], np.where(first, 21, 2).astype(np.uint32))
    assert np.array_equal(rh["tfar"], np.where(first, 2.5, 3.0).astype(np.float32))
    assert np.array_equal(rh["instID"], np.where(first, 55, 1).astype(np.uint32))
    for i in range(n):
        want = [("i", 0, 0), ("o", 55, 20), ("i", 0, 1), ("o", 55, 21)] if first[i] else [("i", 1, 0), ("i", 1, 1), ("i", 1, 2)]
        assert order[i] == want, (i, order[i])
    fh.release(dev, top, inner)


# ---- 8. equivalence with disabled geometry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("form", list(fh.EQ_KINDS))
def test_rejecting_geometries_equals_disabling_them(rtc, po, form, mode):
    case = "meshmb" if form == "meshmb_linear" else form
    pieces, instances, rays, rejected, aside = fh.equivalence_case(rtc, po, case, mode)
    ncalls = [0]

    def body(a):
        ncalls[0] += 1
        if a.geom in rejected:
            a.reject()
    flt = fh.filter_func(rtc, body)
    extra = fh.EQ_CFG.get(form, "")
    dev, top, inner = fh.eq_build(rtc, fh.cfg(False, True, extra), mode, pieces, instances, intersect=flt)
    assert top.stats()["accelKind"] == fh.EQ_KINDS[form][mode]
    got = fh.copy_of(rtc, rays)
    top.intersect1M(got)
    dev2, top2, inner2 = fh.eq_build(rtc, fh.cfg(False, False, extra), mode, pieces, instances, disabled=rejected)
    want = fh.copy_of(rtc, rays)
    top2.intersect1M(want)
    keep = ~aside
    g8, w8 = got.view(np.uint8).reshape(-1, 80), want.view(np.uint8).reshape(-1, 80)
    diff = (g8 != w8).any(1) & keep
    print(f"  {form}, mode {mode}: {int((want['geomID'] != INVALID).sum())} hits, {ncalls[0]} callbacks, {int(aside.sum())} rays set aside, {int(diff.sum())} records differ")
    assert not diff.any(), (form, mode, np.nonzero(diff)[0][:8], got[diff][:4], want[diff][:4])
    hit = want["geomID"] != INVALID
    assert hit.sum() > 100 and not np.isin(want["geomID"][hit], rejected).any()
    assert ncalls[0] >= hit.sum() + 50  # rejected layers in front of accepted ones were offered
    for d_, t_, i_ in ((dev2, top2, inner2), (dev, top, inner)):
        t_.release()
        i_.release()
        d_.release()


# ---- 9. a quad's diagonal --------------------------------------------------------------------------------------------------------------------
def test_a_ray_through_a_quads_diagonal_loses_both_triangles(rtc):
    """The documented limit of the t key: the two triangles of a quad share (geomID, primID) and a ray through v1-v3 hits both at one t,
    so rejecting one rejects both - the reference would offer the second one as well."""
    offered = []

    def body(a):
        offered.append((a.geom, a.tfar))
        if a.geom == 0:
            a.reject()
    flt = fh.filter_func(rtc, body)
    dev, top, inner = fh.stack_top(rtc, fh.cfg(), [(4, (1.0, 0.0, 0.0))], intersect=flt, filtered=range(2), quads=True, nq=2)
    assert top.stats()["accelKind"] in (16, 17)
    rh = rtc.aligned_rayhits(1)
    fill_rays(rh, np.array([[1.5, 0.5, -1.0]], np.float32), np.array([[0, 0, 1]], np.float32))  # local (0.5, 0.5): on the diagonal v1 = (1, 0) - v3 = (0, 1)
    top.intersect1M(rh)
    assert rh["geomID"][0] == 1 and rh["instID"][0] == 4 and rh["tfar"][0] == 2.0
    assert offered == [(0, 1.0), (1, 2.0)], offered  # quad 0 was offered ONCE
    fh.release(dev, top, inner)


# ---- 10. entry paths -------------------------------------------------------------------------------------------------------------------------
def _soa(aos, n, with_hit=True):
    fields = RAYF + (ih.HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


def test_every_entry_path_gives_the_same_records(rtc):
    import torch
    flt = _alpha(rtc)
    n = 512
    src, xl, yl, which = fh.stack_rays(rtc, n, TWO, seed=10)
    want_g = _alpha_want(xl, which)
    dev, top, inner = fh.stack_top(rtc, fh.cfg(True), TWO, intersect=flt, filtered=range(NQ - 1))
    L = top.lib
    want = fh.copy_of(rtc, src)
    top.intersect1M(want)
    assert np.array_equal(want["geomID"], want_g.astype(np.uint32)) and np.array_equal(want["instID"], which.astype(np.uint32))
    ctx = rtc.make_context()
    # rtcIntersect1
    one = fh.copy_of(rtc, src)
    for i in range(64):
        top.intersect1(one[i:i + 1])
    assert one[:64].tobytes() == want[:64].tobytes()
    # the packets
    for W in (4, 8, 16):
        fn = getattr(L, f"rtcIntersect{W}")
        fn.restype = None
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        valid = np.full(W, -1, np.int32)
        for a in range(64, 64 + 4 * W, W):
            pk = _soa(src[a:a + W], W)
            fn(valid.ctypes.data, top.handle, C.addressof(ctx), pk.ctypes.data)
            dev.check(f"rtcIntersect{W}")
            assert np.array_equal(pk, _soa(want[a:a + W], W)), (W, a)
    # rtcIntersectNM
    N, M = 4, 16
    buf = np.zeros((M, 20 * N), np.uint32)
    for m in range(M):
        buf[m] = _soa(src[256 + m * N: 256 + (m + 1) * N], N).ravel()
    L.rtcIntersectNM.restype = None
    L.rtcIntersectNM.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_size_t]
    L.rtcIntersectNM(top.handle, C.addressof(ctx), buf.ctypes.data, N, M, 20 * N * 4)
    dev.check("rtcIntersectNM")
    for m in range(M):
        assert np.array_equal(buf[m].reshape(20, N), _soa(want[256 + m * N: 256 + (m + 1) * N], N)), m
    # a device-resident ray buffer
    t = torch.from_numpy(src.view(np.uint8).reshape(-1, 80).copy()).cuda()
    top.intersect1M(t)
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == want.tobytes()
    # records with a stride that is no multiple of 16, host and device
    raw = np.zeros(n * 84 + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    strided = np.ndarray((n,), rtc.RAYHIT_DTYPE, raw, off, (84,))
    strided[:] = src
    top.intersect1M(strided)
    assert np.ascontiguousarray(strided).tobytes() == want.tobytes() and not raw[off:off + n * 84].reshape(n, 84)[:, 80:].any()
    traw = torch.zeros(n * 84 + 16, dtype=torch.uint8, device="cuda")
    tv = traw[4:4 + n * 84].view(n, 84)
    tv[:, :80] = torch.from_numpy(src.view(np.uint8).reshape(-1, 80).copy()).cuda()
    top.intersect1M(tv)
    torch.cuda.synchronize()
    assert tv[:, :80].cpu().numpy().tobytes() == want.tobytes()
    fh.release(dev, top, inner)
    # service=1: no service kernel for instances and none for filtered scenes - the calls reach the filter loop
    dev, top, inner = fh.stack_top(rtc, fh.cfg(True, True, "service=1"), TWO, intersect=flt, filtered=range(NQ - 1))
    g = fh.copy_of(rtc, src)
    for a in range(0, n, 32):
        top.intersect1M(g[a:a + 32])
    assert g.tobytes() == want.tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    fh.release(dev, top, inner)


# ---- 11. overflow area -----------------------------------------------------------------------------------------------------------------------
def test_filtered_rays_in_a_launch_that_uses_the_overflow_area(rtc):
    """The needle scene of tests/deep_stack_helpers.py below its three overlapping instances: more than half of the rays pop entries from
    the HBM stack columns (tests/test_host_deep_stack.py).  The stack depth is a build constant, so the anchor is not a second run with the
    stack in LDS but a property that holds at any depth: a context filter that rejects every candidate with t <= t0 must leave exactly
    the record a ray with tnear = t0 gets from the unfiltered kernel (the triangle tests' t does not depend on tnear; their range test
    is t > tnear) - t0 just behind the ray's first hit, so that the re-trace walks the deep tree again with its exclusion list."""
    scenes, inst = ds.instanced_scene("t"), ds.deep_instances()
    lo, hi = ds.instance_ray_box(scenes, inst)
    m = 2048
    org, dirs = random_rays_np(m, lo, hi, ds.GPU_RAY_SEED)
    rays = ds.rays_of(rtc, ds.snap(org), dirs, None)
    rays["id"] = np.arange(m)
    dev, top, inner = iq.build(rtc, 0, scenes, inst, "inst_filters=1")
    plain = ds.copy_of(rtc, rays)
    top.intersect1M(plain)
    hit = plain["geomID"] != INVALID
    assert hit.sum() > m // 2
    t0 = np.where(hit, plain["tfar"] * np.float32(1.0001), np.float32(0)).astype(np.float32)
    ncalls = [0]

    def body(a):
        ncalls[0] += 1
        if not a.tfar > t0[a.ray_id]:
            a.reject()
    flt = fh.filter_func(rtc, body)
    got = ds.copy_of(rtc, rays)
    top.intersect1M(got, ctx=fh.context_with(rtc, flt))
    want = ds.copy_of(rtc, rays)
    want["tnear"] = t0
    top.intersect1M(want)
    want["tnear"] = rays["tnear"]
    assert got.tobytes() == want.tobytes()
    second = want["geomID"] != INVALID
    assert (second & hit).sum() > 100 and ncalls[0] >= hit.sum() + (second & hit).sum()
    assert dev.error() == 0  # the overflow word stayed clear
    iq.release(dev, top, inner)


# ---- 12. invalid rays ------------------------------------------------------------------------------------------------------------------------
def test_invalid_rays_in_a_filtered_batch_are_untouched(rtc):
    ids = []

    def body(a):
        ids.append(a.ray_id)
        if a.geom == 0:
            a.reject()
    flt = fh.filter_func(rtc, body)
    dev, top, inner = fh.stack_top(rtc, fh.cfg(True), TWO, intersect=flt)
    n = 256
    rh, _, _, _ = fh.stack_rays(rtc, n, TWO, seed=12)
    rh["tfar"] = 100.0
    bad_range, bad_nan = np.arange(n) % 4 == 1, np.arange(n) % 4 == 3
    rh["tnear"][bad_range] = 200.0  # tnear > tfar
    rh["org_x"][bad_nan] = np.nan
    before = rh.copy()
    top.intersect1M(rh)
    bad = bad_range | bad_nan
    assert rh[bad].tobytes() == before[bad].tobytes()
    assert (rh["geomID"][~bad] == 1).all() and (rh["tfar"][~bad] == 2.0).all()
    assert not set(ids) & set(np.nonzero(bad)[0].tolist()) and len(ids) == 2 * int((~bad).sum())
    occ = fh.occ_of(rtc, before)
    top.occluded1M(occ)  # no occlusion filter set: the unfiltered any-hit kernel
    assert occ[bad].tobytes() == fh.occ_of(rtc, before)[bad].tobytes() and np.isneginf(occ["tfar"][~bad]).all()
    fh.release(dev, top, inner)


# ---- refusals that stay, with the key set -------------------------------------------------------------------------------------------------------
def test_counted_batches_stay_refused_and_without_the_key_nothing_changes(rtc):
    flt = fh.filter_func(rtc, lambda a: None)
    dev, top, inner = fh.stack_top(rtc, fh.cfg(True), TWO, intersect=flt)
    rh, _, _, _ = fh.stack_rays(rtc, 64, TWO)
    with pytest.raises(rtc.RTCError) as e:
        top.intersect1M_counted(rh.copy())
    assert e.value.code == rtc.RTC_ERROR_INVALID_OPERATION
    fh.release(dev, top, inner)
    dev, top, inner = fh.stack_top(rtc, fh.cfg(True, key=False), TWO)
    before = rh.copy()
    top.intersect1M(rh, ctx=fh.context_with(rtc, flt), check=False)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION and rh.tobytes() == before.tobytes()
    fh.release(dev, top, inner)


def test_context_filter_beside_subdivision_instances_stays_refused(rtc):
    """the two-level kernel of subdivision instances has no exclusion scan: with the key set, a context filter on a top scene that also
    places a subdivision scene is refused with the text it always had, and the records are untouched"""
    flt = fh.filter_func(rtc, lambda a: a.reject())
    dev = rtc.Device(fh.cfg())
    log = []
    errfn = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda u, c, msg: log.append((c, msg.decode())))
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(errfn, C.c_void_p), None)
    mesh = fh.stack_scene(rtc, dev)
    mesh.commit()
    patch = rtc.Scene(dev)
    # (pinned corners: the limit surface is the square)
    patch.add_subdiv(fh.SQUARE, np.array([4], np.uint32), np.arange(4, dtype=np.uint32), vertex_creases=(np.arange(4, dtype=np.uint32), np.full(4, np.inf, np.float32)))
    patch.set_levels(2, 1)
    patch.commit()
    top = rtc.Scene(dev)
    top.add_instance(mesh, ih.affine((0.0, 0.0, 0.0)))
    top.add_instance(patch, ih.affine((2.0, 0.0, 0.0)))
    top.commit()
    rh, _, _, _ = fh.stack_rays(rtc, 64, TWO)
    before = rh.copy()
    top.intersect1M(rh, ctx=fh.context_with(rtc, flt), check=False)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION and rh.tobytes() == before.tobytes()
    assert log and "RTCIntersectContext::filter is not supported on a scene with instances" in log[-1][1], log
    top.intersect1M(rh)  # unfiltered, both instance accels are traced
    assert (rh["geomID"] == 0).all() and np.array_equal(rh["instID"], (np.arange(64) % 2).astype(np.uint32))
    for s_ in (top, patch, mesh):
        s_.release()
    dev.release()

