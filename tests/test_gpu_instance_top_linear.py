"""Moving instances under time-dependent top-level boxes (device config inst_bounds=linear; accel kinds 32 / 33), traced by the TOPMB
form of the two-level kernel (trace_instance_top_linear.hip): a lane outside an instance reads QNodeMB8s.  Tree shape and box tests
cull, they never change a hit: the anchor of most cases is the same top scene on a device without the key, byte for byte.  Scenes,
instances and rays are those of tests/instance_top_linear_helpers.py; ray times lie on the grid k / 64 unless stated."""
import ctypes as C

import numpy as np
import pytest

import deep_stack_helpers as ds
import inst_filter_helpers as fh
import instance_helpers as ih
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import instance_mesh_mb_linear_helpers as iml
import instance_quads_helpers as iq
import instance_subdiv_helpers as isub
import instance_top_linear_helpers as itl
from helpers import INVALID, compare_hits, random_soup

pytestmark = pytest.mark.gpu

M = 4096
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]


def _trace(rtc, dev, top, rays):
    got, occ = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    top.intersect1M(got)
    top.occluded1M(occ)
    assert dev.error() == 0  # (the overflow word stayed clear)
    return got, occ


def _both(rtc, mode, scenes, inst, rays, base="", linear=itl.KEY, swept="inst_bounds=swept", swept_kinds=(18, 19, 20, 21)):
    """(got, occ) of the top scene on a device without the key and on one with it; asserts the kinds"""
    join = lambda a, b: a + ("," if a and b else "") + b  # noqa: E731
    out = []
    for cfg, kinds in ((join(base, swept), swept_kinds), (join(base, linear), (itl.kind(mode),))):
        dev, top, inner = imm.build(rtc, mode, scenes, inst, cfg)
        assert top.stats()["accelKind"] in kinds, (cfg, top.stats()["accelKind"])
        out.append(_trace(rtc, dev, top, rays))
        iq.release(dev, top, inner)
    return out


def _same(a, b, what):
    (g0, o0), (g1, o1) = a, b
    assert g0.tobytes() == g1.tobytes(), f"{what}: {int((g0.view(np.uint8).reshape(-1, 80) != g1.view(np.uint8).reshape(-1, 80)).any(1).sum())} hit records differ"
    assert o0.tobytes() == o1.tobytes(), f"{what}: occluded records differ"


def _per_instance(rtc, mode, scenes, inst, rays):
    """every instance alone in a top scene of its own on a device without the key: per[i] = its closest hits"""
    dev = rtc.Device("")
    inner = {k: imm.add_scene(rtc, dev, d, mode) for k, d in scenes.items()}
    per = []
    for gid, key, steps in inst:
        top = rtc.Scene(dev, iq.flags(mode))
        if len(steps) == 1:
            top.add_instance(inner[key], steps[0], geom_id=gid)
        else:
            top.add_instance_mb(inner[key], steps, geom_id=gid)
        top.commit()
        got = iq.copy(rtc, rays)
        top.intersect1M(got)
        per.append(got)
        top.release()
    for s in inner.values():
        s.release()
    dev.release()
    return per


# ---- 1. byte identity with the swept device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", itl.CASES)
def test_records_equal_the_swept_device_byte_for_byte(rtc, what, mode):
    """closest hit and occluded, robust and fast, the five containment scenes ((a): the fast mover beside a static instance).  Tree shape
    could change a winner only where two instances give a bit-identical t: asserted absent on the swept device, every instance traced
    alone there."""
    scenes = {"m": itl.soup_scene(200, 100, 3)}
    inst = itl.instances(what)
    rays = imm.aimed_rays(rtc, scenes, inst, M, 61, denom=64)
    swept, lin = _both(rtc, mode, scenes, inst, rays, swept_kinds=(20, 21))
    per = _per_instance(rtc, mode, scenes, inst, rays)
    assert ih.equal_t_ties(per) == 0
    merged, _ = iq.merge(rays, per, inst)
    assert merged.tobytes() == swept[0].tobytes()  # the swept output is the nearest of the instances' own hits
    _same(swept, lin, f"({what}) mode {mode}")
    got = lin[0]
    hit = got["geomID"] != INVALID
    moving = [g for g, _, s in inst if len(s) > 1]
    on_moving = np.isin(got["instID"][hit], moving)
    print(f"({what}) mode {mode}: {int(hit.sum())} hits, {int(on_moving.sum())} on moving instances, {len(np.unique(got['instID'][hit]))} instances hit, "
          f"{len(np.unique(rays['time'][hit]))} distinct times")
    assert int(hit.sum()) > M // 20 and on_moving.sum() > 50 and (~on_moving).sum() > 50
    assert len(np.unique(got["instID"][hit])) == len(inst) and len(np.unique(rays["time"][hit])) >= 33


# ---- 2. per-time oracle parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["c", "d"])
def test_grid_transforms_against_the_static_oracle_per_time(rtc, po, what, mode):
    """the three-step out-and-back instance and the five-step zig-zag: translations of whole numbers, ray origins on the 2^-10 grid and
    times k / 64 make world2local(time) and the local rays exact (asserted), so one static oracle scene per instance serves"""
    v, t = random_soup(300, 5)
    scenes = {"m": imm.desc(tris=(ih.snap(v), t, 0))}
    inst = itl.instances(what)
    rays = imm.aimed_rays(rtc, scenes, inst, M, 71, denom=64)
    want, per, _, _ = im.oracle_instances(rtc, po, scenes, inst, rays, mode, exact=True)
    dev, top, inner = imm.build(rtc, mode, scenes, inst, itl.KEY)
    assert top.stats()["accelKind"] == itl.kind(mode)
    got, occ = _trace(rtc, dev, top, rays)
    compare_hits(got, want, what=f"({what}) mode {mode}")
    hit = want["geomID"] != INVALID
    assert int(hit.sum()) > M // 20 and len(np.unique(rays["time"][hit])) >= 33 and set(np.unique(want["instID"][hit])) == {0, 1}
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    iq.release(dev, top, inner)


# ---- 3. a wave on both node types at once -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_one_wave_on_both_node_types(rtc, mode):
    """128 rays, alternating by lane: even rays are aimed at one static instance of a 512-triangle soup and spend their life deep inside
    its QNode8 tree; odd rays run along a row of the lattice of 40 instances, through many top-level boxes (depth 2 and more, QNodeMB8s)
    and mostly between the soups' triangles.  (The soup's triangles are 3 units wide, so that the aimed rays hit: 62 of the 64 by the
    oracle alone.)"""
    v, t = random_soup(512, 3, size=3.0)
    scenes = {"m": imm.desc(tris=(ih.snap(v), t, 0))}
    inst = itl.instances("e")
    n = 128
    rays = imm.aimed_rays(rtc, scenes, [inst[4]] * 2, n, 5, denom=64)  # instance 4: static
    assert len(inst[4][2]) == 1
    rng = np.random.RandomState(9)
    odd = np.arange(n) % 2 == 1
    k = int(odd.sum())
    org = ih.snap(np.stack([np.full(k, -20.0), 40.0 * rng.randint(0, 5, k) + rng.rand(k) * 10.0, rng.rand(k) * 10.0], 1))
    rays["org_x"][odd], rays["org_y"][odd], rays["org_z"][odd] = org[:, 0], org[:, 1], org[:, 2]
    rays["dir_x"][odd], rays["dir_y"][odd], rays["dir_z"][odd] = 1.0, ih.snap(rng.rand(k) * 0.05), ih.snap(rng.rand(k) * 0.05)
    dev, top, inner = imm.build(rtc, mode, scenes, inst, itl.KEY)
    _, leaves = itl.top_leaves(top)
    assert max(len(p) for p, _ in leaves) >= 2
    iq.release(dev, top, inner)
    swept, lin = _both(rtc, mode, scenes, inst, rays, swept_kinds=(18, 19))
    _same(swept, lin, f"one wave, mode {mode}")
    hit = lin[0]["geomID"] != INVALID
    print(f"mode {mode}: even rays {int(hit[~odd].sum())} hits of {int((~odd).sum())}, odd rays {int(hit[odd].sum())} of {k}")
    assert (lin[0]["instID"][~odd] == 4).sum() >= 32  # (a moving neighbour may cross in front of a few)


# ---- 4. all three keys -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_moving_meshes_below_a_moving_instance_under_all_three_keys(rtc, po, bomberman, mode):
    """scene (d) of instance_mesh_mb_helpers - "m": moving triangles and moving quads, "s": static triangles and quads - with "m" below a
    moving instance and "s" below a static one: kinds 32 / 33 with all four trees, the motion-blur trees as QNodeMB8s.  Byte identity
    with the device that has mb_bounds=linear,inst_mb_bounds=linear only (kinds 30 / 31), and per-time oracle parity (times k / 8)."""
    scenes = imm.scenes_d(bomberman)
    inst = [(0, "m", [ih.affine((0, 0, 0)), ih.affine((48, 8, -8))]), (1, "s", [ih.affine((0, 40, 0))])]
    rays = imm.aimed_rays(rtc, scenes, inst, M, 81, denom=8)
    only_mesh, lin = _both(rtc, mode, scenes, inst, rays, linear=itl.ALL_KEYS, swept=iml.LINEAR, swept_kinds=(30, 31))
    _same(only_mesh, lin, f"all three keys, mode {mode}")
    want, per, isb, _ = imm.oracle_instances(rtc, po, scenes, inst, rays, mode, exact=True)
    got = lin[0]
    ds.quad_allowances(got, want, isb, mode, quad_gids=imm.quad_gids(scenes))
    compare_hits(got, want, what=f"all three keys, mode {mode}")
    hit = want["geomID"] != INVALID
    per_kind = {int(g): int((got["geomID"][hit] == g).sum()) for g in np.unique(got["geomID"][hit])}
    print(f"mode {mode}: {int(hit.sum())} hits, per geomID {per_kind}")
    assert sorted(per_kind) == [3, 5, 7, 9] and min(per_kind.values()) >= 8, per_kind
    # without the two mesh keys the commit refuses, with the message that names all three
    dev = rtc.Device(itl.KEY)
    inner = {k: imm.add_scene(rtc, dev, d, mode) for k, d in scenes.items()}
    top = rtc.Scene(dev, iq.flags(mode))
    top.add_instance_mb(inner["m"], inst[0][2])
    log = []
    errfn = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda user, code, msg: log.append((code, (msg or b"").decode())))
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(errfn, C.c_void_p), None)
    top.lib.rtcCommitScene(top.handle)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION and all(k in log[-1][1] for k in ("mb_bounds=linear", "inst_mb_bounds=linear", "inst_bounds=linear")), log
    iq.release(dev, top, inner)


# ---- 5. times outside the shutter ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_times_outside_the_shutter_inf_and_nan(rtc, mode):
    """rays at -0.5, 1.5, +-inf and NaN mixed into valid ones.  The node step clamps the time (a NaN becomes 0) while the instance's
    transform extrapolates: such rays are no more conservative than under swept boxes, but every hit they report is a true one - the hit
    of that instance's scene traced directly with the local ray under the matrix the kernel uses (instance_mb_helpers.world2local_at; a
    matrix that is not finite: the instance is not entered).  The valid rays' records are those of a batch without the others."""
    scenes = {"m": itl.soup_scene(200, 100, 3)}
    inst = itl.instances("a") + [(2, "m", [ih.affine((12, 0, 14)), ih.affine((12, 6, 14)), ih.affine((12, 0, 14))])]
    rays = imm.aimed_rays(rtc, scenes, inst, M, 91, denom=64)
    oddt = np.array([-0.5, 1.5, np.inf, -np.inf, np.nan], np.float32)
    odd = np.arange(M) % 2 == 1
    rays["time"][odd] = oddt[(np.arange(M)[odd] // 2) % len(oddt)]
    dev, top, inner = imm.build(rtc, mode, scenes, inst, itl.KEY)
    assert top.stats()["accelKind"] == itl.kind(mode)
    got, occ = _trace(rtc, dev, top, rays)  # the run completes, the overflow flag is clear
    valid = rays[~odd].copy()
    alone = iq.copy(rtc, valid)
    top.intersect1M(alone)
    assert got[~odd].tobytes() == alone.tobytes()
    hit = got["geomID"] != INVALID
    assert got[~hit].tobytes() == rays[~hit].tobytes()  # misses are left untouched
    checked = 0
    finite = np.isfinite(rays["time"])
    for gid, key, steps in inst:
        # (a time that is not finite gives an interpolated matrix that is not finite: instance_xfm.h reports it, the instance is not entered)
        w, ok = im.world2local_at(steps, np.where(finite, rays["time"], np.float32(0)))
        if len(steps) > 1:
            ok = ok & finite
        sub = iq.copy(rtc, im.local_rays(rays, w, ok))
        inner[key].intersect1M(sub)
        mine = odd & hit & (got["instID"] == gid)
        assert ok[mine].all()  # no hit through a matrix that is not finite
        assert np.array_equal(got["geomID"][mine], sub["geomID"][mine]) and np.array_equal(got["primID"][mine], sub["primID"][mine])
        a, b = got["tfar"][mine].astype(np.float64), sub["tfar"][mine].astype(np.float64)
        assert np.all(np.abs(a - b) <= 1e-4 * np.abs(b))
        checked += int(mine.sum())
    per_time = {str(t): int((hit & odd & ((rays["time"] == t) | (np.isnan(t) & np.isnan(rays["time"])))).sum()) for t in oddt}
    print(f"mode {mode}: {int(hit[~odd].sum())} hits of valid rays, hits of odd-time rays {per_time}")
    assert checked == int((odd & hit).sum()) and checked > 50
    assert np.array_equal((occ["tfar"] == -np.inf)[~odd], hit[~odd])
    assert dev.error() == 0
    iq.release(dev, top, inner)


# ---- 6. entry paths ----------------------------------------------------------------------------------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (ih.HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_entry_paths_are_bit_identical(rtc, mode):
    """rtcIntersect1 / rtcOccluded1, 1M on host and device-resident records (aligned, and strided with a 4-byte aligned base: the VEC = false
    twins), packets 4 / 8 / 16, NM and Np, and small calls on a service=1 device: the records of the 1M path, on 256 rays"""
    import torch
    scenes = {"m": itl.soup_scene(200, 100, 3)}
    inst = itl.instances("d")
    m = 256
    rays = imm.aimed_rays(rtc, scenes, inst, m, 31, denom=64)
    dev, top, inner = imm.build(rtc, mode, scenes, inst, itl.KEY)
    assert top.stats()["accelKind"] == itl.kind(mode)
    L = top.lib
    want, wocc = _trace(rtc, dev, top, rays)
    hit = want["geomID"] != INVALID
    assert hit.sum() > 64 and set(np.unique(want["instID"][hit])) == {0, 1}
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()  # device-resident
    top.intersect1M(t)
    to = torch.from_numpy(iq.occ_of(rtc, rays).view(np.uint8).reshape(-1, 48).copy()).cuda()
    top.occluded1M(to)
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == want.tobytes() and to.cpu().numpy().tobytes() == wocc.tobytes()
    ctx = rtc.make_context()
    for recs, ref, occluded in ((rays, want, False), (iq.occ_of(rtc, rays), wocc, True)):  # pitch 96, base 4-byte aligned: load_ray<false>
        raw = torch.zeros(m * 96 + 16, dtype=torch.uint8, device="cuda")
        view = raw[4:4 + m * 96].view(m, 96)
        assert view.data_ptr() % 16 == 4
        sz = recs.dtype.itemsize
        view[:, :sz] = torch.from_numpy(recs.view(np.uint8).reshape(m, sz).copy()).cuda()
        (L.rtcOccluded1M if occluded else L.rtcIntersect1M)(top.handle, C.byref(ctx), view.data_ptr(), m, 96)
        dev.check("strided batch")
        torch.cuda.synchronize()
        assert view[:, :sz].contiguous().cpu().numpy().tobytes() == ref.tobytes()
    k = 64  # rtcIntersect1 / rtcOccluded1
    one, o1 = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    for i in range(k):
        top.intersect1(one[i:i + 1])
        top.occluded1(o1[i:i + 1])
    assert one[:k].tobytes() == want[:k].tobytes() and o1[:k].tobytes() == wocc[:k].tobytes()
    for width in (4, 8, 16):  # packets, per-lane times
        fn = getattr(L, f"rtcIntersect{width}")
        fn.restype = None
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        valid = np.full(width, -1, np.int32)
        for a in range(0, 64, width):
            pk = _soa(rays[a:a + width], width, True)
            fn(valid.ctypes.data, top.handle, C.addressof(ctx), pk.ctypes.data)
            dev.check(f"rtcIntersect{width}")
            assert np.array_equal(pk, _soa(want[a:a + width], width, True))
    nm = L.rtcIntersectNM
    nm.restype = None
    nm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_size_t]
    nfields = len(RAYF) + len(ih.HITF)
    packs = np.stack([_soa(rays[a:a + 4], 4, True) for a in range(0, 64, 4)])  # [16, fields, 4]
    nm(top.handle, C.addressof(ctx), packs.ctypes.data, 4, 16, nfields * 4 * 4)
    dev.check("rtcIntersectNM")
    assert np.array_equal(packs, np.stack([_soa(want[a:a + 4], 4, True) for a in range(0, 64, 4)]))
    comp = _soa(rays, 64, True)  # one array per component
    ptrs = (C.c_void_p * nfields)(*[comp[i].ctypes.data for i in range(nfields)])
    npf = L.rtcIntersectNp
    npf.restype = None
    npf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
    npf(top.handle, C.addressof(ctx), C.addressof(ptrs), 64)
    dev.check("rtcIntersectNp")
    assert np.array_equal(comp, _soa(want, 64, True))
    iq.release(dev, top, inner)
    # service=1: no service kernel for instances, the call combiner serves the small calls
    dev, top, inner = imm.build(rtc, mode, scenes, inst, itl.KEY + ",service=1")
    g = iq.copy(rtc, rays)
    for a in range(0, m, 32):
        top.intersect1M(g[a:a + 32])
    assert g.tobytes() == want.tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    iq.release(dev, top, inner)


# ---- 7. overflow area -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_the_chain_of_nested_instances_spills_to_hbm_and_equals_the_swept_device(rtc, mode):
    """itl.chain_case(): the host walk (test_host_instance_top_linear.py) pins that every ray writes stack slots beyond the 16 in LDS"""
    scenes, inst = itl.chain_case()
    rays = itl.chain_rays(rtc, 2048, ds.GPU_RAY_SEED)
    swept, lin = _both(rtc, mode, scenes, inst, rays, swept_kinds=(18, 19))
    _same(swept, lin, f"chain, mode {mode}")
    hit = lin[0]["geomID"] != INVALID
    print(f"mode {mode}: {int(hit.sum())} hits in {len(np.unique(lin[0]['instID'][hit]))} instances")
    assert hit.sum() > 1000 and len(np.unique(lin[0]["instID"][hit])) >= 10


def test_an_overflow_area_that_is_too_small_raises_the_documented_error(rtc, monkeypatch):
    """RTAMD_INST_SPILL_MAX=0 (read when the device is created): no overflow entries at all.  Pushes beyond the 16 slots in LDS are dropped
    behind their bounds check, the kernel raises the overflow word and the call RTC_ERROR_UNKNOWN - no silent wrong hits."""
    scenes, inst = itl.chain_case()
    rays = itl.chain_rays(rtc, 512, ds.GPU_RAY_SEED)
    monkeypatch.setenv("RTAMD_INST_SPILL_MAX", "0")
    dev, top, inner = imm.build(rtc, 1, scenes, inst, itl.KEY)
    monkeypatch.delenv("RTAMD_INST_SPILL_MAX")
    assert top.stats()["accelKind"] == 33
    log = []
    errfn = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda user, code, msg: log.append((code, (msg or b"").decode())))
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(errfn, C.c_void_p), None)
    got = iq.copy(rtc, rays)
    with pytest.raises(rtc.RTCError) as e:
        top.intersect1M(got)
    assert e.value.code == rtc.RTC_ERROR_UNKNOWN
    assert log and log[-1][0] == rtc.RTC_ERROR_UNKNOWN and "traversal stack overflow: a stack entry was dropped" in log[-1][1], log
    iq.release(dev, top, inner)


# ---- 8. filters ---------------------------------------------------------------------------------------------------------------------------------------------------
def _stack_top(rtc, cfg, intersect=None):
    """the quad stack of inst_filter_helpers (5 unit squares at z = 0..4, two triangles each) below a mover - instance 0, from x = 0 to
    x = 8 over two steps - and below a static instance 1 at (4, 0, 20), behind the mover's path as seen along +z"""
    dev = rtc.Device(cfg)
    inner = fh.stack_scene(rtc, dev)
    if intersect is not None:
        for g in range(3):  # the filter sits on the three front layers
            inner.set_filters(g, intersect=intersect)
    inner.commit()
    top = rtc.Scene(dev)
    assert top.add_instance_mb(inner, [ih.affine((0, 0, 0)), ih.affine((8, 0, 0))], geom_id=0) == 0
    assert top.add_instance(inner, ih.affine((4, 0, 20)), geom_id=1) == 1
    top.commit()
    return dev, top, inner


def _stack_rays(rtc, n, seed):
    """rays along +z from z = -1 through the mover where it is at the ray's time k / 64; x, y inside (0.05, 0.95), off the diagonals"""
    rh, xl, yl, _ = fh.stack_rays(rtc, n, [(0, (0.0, 0.0, 0.0))], seed)
    times = (np.random.RandomState(seed + 1).randint(0, 65, n) / 64.0).astype(np.float32)
    x = xl.astype(np.float64) + 8.0 * times.astype(np.float64)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    rh["org_x"], rh["time"] = x.astype(np.float32), times
    return rh, xl, yl, x


@pytest.mark.parametrize("kind", ["geometry", "context"])
def test_filters_below_a_moving_instance(rtc, kind):
    """1024 rays on an inst_filters=1,inst_bounds=linear device, against the closed form and against the same scene under inst_bounds=swept.
    geometry: an intersect filter on the three front layers rejects every second primitive (primID 1, y > x): such a ray's hit is layer 3
    at t = 4, the others hit layer 0 at t = 1.  context: RTCIntersectContext::filter rejects by instance - everything of the mover - so a
    ray hits the static instance behind (layer 0 at t = 21) where its x lies over it, and nothing elsewhere."""
    n = 1024
    rh, xl, yl, x = _stack_rays(rtc, n, 13)
    fh.CALLBACK_ERRORS.clear()
    if kind == "geometry":
        fn = fh.filter_func(rtc, lambda a: a.reject() if a.prim == 1 else None)
        geo, ctxfn = fn, None
    else:
        fn = fh.filter_func(rtc, lambda a: a.reject() if a.inst == 0 else None)
        geo, ctxfn = None, fn
    out = []
    for key in ("inst_bounds=linear", "inst_bounds=swept"):
        dev, top, inner = _stack_top(rtc, "inst_filters=1," + key, geo)
        assert top.stats()["accelKind"] == (33 if key.endswith("linear") else 19)
        got = fh.copy_of(rtc, rh)
        top.intersect1M(got, ctx=fh.context_with(rtc, ctxfn) if ctxfn else None)
        assert dev.error() == 0 and not fh.CALLBACK_ERRORS, fh.CALLBACK_ERRORS[:1]
        out.append(got)
        fh.release(dev, top, inner)
    got = out[0]
    assert got.tobytes() == out[1].tobytes()
    upper = yl > xl
    if kind == "geometry":
        assert (got["instID"] == 0).all()
        assert np.array_equal(got["geomID"], np.where(upper, 3, 0).astype(np.uint32)) and np.array_equal(got["primID"], upper.astype(np.uint32))
        assert np.array_equal(got["tfar"], np.where(upper, 4.0, 1.0).astype(np.float32))
        assert upper.sum() > 100 and (~upper).sum() > 100
    else:
        behind = (x > 4.0) & (x < 5.0)
        assert behind.sum() > 50 and (~behind).sum() > 50
        assert np.array_equal(got["geomID"] != INVALID, behind)
        assert (got["instID"][behind] == 1).all() and (got["geomID"][behind] == 0).all() and (got["tfar"][behind] == 21.0).all()
        xs = x - 4.0  # the ray in the static instance's space
        clear = behind & (np.abs(yl - xs) > 2.0 ** -9) & (np.abs(yl + xs - 1.0) > 2.0 ** -9)  # off its diagonals
        assert clear.sum() > 50 and np.array_equal(got["primID"][clear], (yl > xs)[clear].astype(np.uint32))
        assert got[~behind].tobytes() == rh[~behind].tobytes()


# ---- 9. a top scene of both classes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isub.FAMILIES)
def test_mesh_instances_beside_subdivision_instances(rtc, bomberman, accel):
    """mesh instances under kind 32 / 33 beside subdivision instances, which stay kinds 24 / 25 over a swept QNode8 top level: the records
    of the swept device"""
    v, fs, fi = isub.bomberman_faces(bomberman, 32)
    meshes = {"sub": (v, fs, fi, 3, 2)}
    lo, hi = isub.mesh_box(meshes["sub"])
    sub_inst = [(10, "sub", [ih.affine((0, 0, 30)), ih.affine((6, 0, 30))]), (11, "sub", [ih.affine((0, 30, 30))])]
    scenes = {"m": itl.soup_scene(200, 100, 3)}
    mesh_inst = itl.instances("c")
    rays_mesh = imm.aimed_rays(rtc, scenes, mesh_inst, 2048, 41, denom=64)
    rays_sub = imm.aimed_rays(rtc, {"sub": imm.desc(tris=(v, None, 0))}, sub_inst, 2048, 43, denom=64)
    rays = iq.copy(rtc, np.concatenate([rays_mesh, rays_sub]))
    out = []
    for key in ("inst_bounds=swept", itl.KEY):
        def extra(top, dev):
            m = imm.add_scene(rtc, dev, scenes["m"], 1)
            for gid, _, steps in mesh_inst:
                if len(steps) > 1:
                    assert top.add_instance_mb(m, steps, geom_id=gid) == gid
                else:
                    assert top.add_instance(m, steps[0], geom_id=gid) == gid
            return [m]

        dev, top, inner = isub.build(rtc, accel, meshes, sub_inst, key, extra)
        assert top.stats()["accelKind"] == (33 if key == itl.KEY else 21)  # the mesh instance accel
        sub_nodes = top.accel_data(0 + rtc.ACCEL_DATA_INSTSUBDIV)  # the second instance accel: QNode8s only, top level included
        assert len(sub_nodes) > 0 and len(sub_nodes) % 96 == 0
        got, occ = _trace(rtc, dev, top, rays)
        out.append((got, occ))
        isub.release(dev, top, inner)
    _same(out[0], out[1], f"both classes, {accel}")
    got = out[1][0]
    hit = got["geomID"] != INVALID
    on_sub = np.isin(got["instID"][hit], [10, 11])
    print(f"{accel}: {int(hit.sum())} hits, {int(on_sub.sum())} below subdivision instances")
    assert on_sub.sum() > 100 and (~on_sub).sum() > 100
