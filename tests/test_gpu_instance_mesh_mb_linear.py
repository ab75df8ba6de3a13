"""Motion-blur meshes below an instance over time-dependent node boxes (device config mb_bounds=linear,inst_mb_bounds=linear; accel kinds
30 / 31), traced by the NODEMB form of the two-level kernel (trace_instance_mesh_mb_linear.hip): the lanes of a wave pick their node
step by the tree they are in.  Scenes, instances and legs are those of tests/instance_mesh_mb_helpers.py, at most 4096 rays per case.
The direct leg traces the instanced scenes themselves on the same device (kinds 26..29, pinned to the oracle by
test_gpu_mb_linear_bounds.py): the trees below the instances are the same nodes, so the records are equal byte for byte, ties included."""
import ctypes as C

import numpy as np
import pytest

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import instance_mesh_mb_linear_helpers as iml
import instance_quads_helpers as iq
import mb_linear_helpers as mb
from helpers import INVALID, compare_hits, fill_rays

pytestmark = pytest.mark.gpu

CFG = iml.LINEAR
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
UP = np.array([0, 0, 1], np.float32)
M = 4096


def _scenes(what, bomberman):
    return {"a": imm.scenes_a, "b": imm.scenes_b, "c": imm.scenes_c, "d": imm.scenes_d}[what](bomberman)


def _direct_leg(rtc, dev, top, inner, inst, rays, what, ties=True):
    want, per = im.direct_instances(rtc, inner, inst, rays)
    if ties:
        assert ih.equal_t_ties(per) == 0, what
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    assert dev.error() == 0
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got.view(np.uint8).reshape(-1, 80) != want.view(np.uint8).reshape(-1, 80)).any(1).sum())} records differ"
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    assert dev.error() == 0
    hit = want["geomID"] != INVALID
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and occ["tfar"][~hit].tobytes() == rays["tfar"][~hit].tobytes()
    return got


# ---- 1. the direct leg: byte for byte -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["a", "b", "c", "d"])
def test_exact_transforms_equal_the_instanced_scenes_traced_directly(rtc, bomberman, what, mode):
    """scenes (a)-(d) under grid-exact transforms, static and moving instances mixed; ray times k / 8, 0 and 1 included"""
    scenes = _scenes(what, bomberman)
    inst = im.exact_instances(9, tuple(scenes))
    inst = [(g, k, s if g % 2 else s[:1]) for g, k, s in inst]  # moving and static instances mixed
    assert any(len(s) > 1 for _, _, s in inst) and any(len(s) == 1 for _, _, s in inst)
    rays = imm.aimed_rays(rtc, scenes, inst, M, 61, denom=8)
    assert {0.0, 1.0} <= set(rays["time"].tolist()) and len(np.unique(rays["time"])) == 9
    dev, top, inner = imm.build(rtc, mode, scenes, inst, CFG)
    assert top.stats()["accelKind"] == iml.kind(mode)
    assert all(s.stats()["accelKind"] in (26, 27, 28, 29) for k, s in inner.items() if scenes[k]["tris"] is None and scenes[k]["quads"] is None)
    got = _direct_leg(rtc, dev, top, inner, inst, rays, f"exact instances of scenes ({what}), mode {mode}")
    hit = got["geomID"] != INVALID
    per_kind = {int(g): int((got["geomID"][hit] == g).sum()) for g in np.unique(got["geomID"][hit])}
    print(f"({what}) mode {mode}: {int(hit.sum())} hits, per geomID {per_kind}, {len(np.unique(got['instID'][hit]))} instances")
    assert int(hit.sum()) > M // 20 and len(np.unique(rays["time"][hit])) >= 5
    assert len(np.unique(got["instID"][hit])) == 9 and (got["instID"][~hit] == INVALID).all()
    if what in "cd":
        assert sorted(per_kind) == [3, 5, 7, 9], per_kind
    iq.release(dev, top, inner)


# ---- 2. the oracle leg ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["a", "b"])
def test_grid_transforms_against_the_static_oracle_per_time(rtc, po, bomberman, what, mode):
    scenes = _scenes(what, bomberman)
    inst = [(g, k, [m]) for g, k, m in iq.grid_instances(9)]
    rays = imm.aimed_rays(rtc, scenes, inst, M, 71, denom=4)  # on the 2^-10 grid, times k / 4
    want, per, isb, _ = imm.oracle_instances(rtc, po, scenes, inst, rays, mode, exact=True)
    dev, top, inner = imm.build(rtc, mode, scenes, inst, CFG)
    assert top.stats()["accelKind"] == iml.kind(mode)
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    if what == "b":
        ds.quad_allowances(got, want, isb, mode)
    compare_hits(got, want, what=f"grid instances of scenes ({what}), mode {mode}")
    hit = want["geomID"] != INVALID
    assert int(hit.sum()) > M // 20 and len(np.unique(rays["time"][hit])) == 5 and len(np.unique(want["instID"][hit])) == 9
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    iq.release(dev, top, inner)


# ---- 3. general transforms ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_general_transforms(rtc, po, bomberman, mode):
    """instance_mesh_mb_helpers.general_case (the inputs test_host_instance_mesh_mb.py pins), its first 4096 rays, at the project's 1e-4
    relative tolerance; rays set aside as there"""
    scenes, inst, rays, want, per, isb, aside = imm.general_case(rtc, po, bomberman, mode, imm.GENERAL_SEED)
    rays, want, isb, aside, per = rays[:M], want[:M], isb[:M], aside[:M], [p[:M] for p in per]
    hits = int((want["geomID"] != INVALID).sum())
    assert hits > M // 20 and aside.sum() <= 0.02 * len(rays)
    dev, top, inner = imm.build(rtc, mode, scenes, inst, CFG)
    assert top.stats()["accelKind"] == iml.kind(mode)
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    keep = ~aside
    if mode == 1:  # Moeller B-lane u / v: the oracle maps after the division, the kernel before (deep_stack_helpers.quad_allowances)
        b = isb & keep
        for f in ("u", "v"):
            assert np.all(np.abs(got[f][b].astype(np.float64) - want[f][b]) <= 4e-7 + 1e-4 * np.abs(want[f][b]))
            want[f][b] = got[f][b]
    compare_hits(got[keep], want[keep], what=f"general transforms over scene (c), mode {mode}")
    for k in np.nonzero(aside)[0]:  # a ray set aside is still a miss, or a hit within 1e-4 in t of SOME instance's oracle hit
        if got["geomID"][k] == INVALID:
            assert got["tfar"][k] == rays["tfar"][k]
            continue
        ts = [float(p["tfar"][k]) for p in per if p["geomID"][k] != INVALID]
        assert any(abs(float(got["tfar"][k]) - t) <= 1e-4 * abs(t) for t in ts), (k, got[k], ts)
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    assert np.array_equal((occ["tfar"] == -np.inf)[keep], (want["geomID"] != INVALID)[keep])
    iq.release(dev, top, inner)


# ---- 4. fast mover below an instance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("quads", [False, True], ids=["triangles", "quads"])
def test_fast_mover_below_a_static_and_a_moving_instance(rtc, quads, mode):
    """test_gpu_mb_linear_bounds.py's closed form below instances: a flat 8 x 8 grid in z = 0 that moves by 16 x its extent along x and
    by 2 along z between its two steps; instance 5 is static at z + 1, instance 9 moves from z + 1 to z + 3 at x + 1024.  A ray down -z
    from z = 10 above where the grid is at the ray's time meets it at t = 9 - 2 time (instance 5) or 9 - 4 time (instance 9); above where
    the grid is at 1 - time there is nothing.  The records are those of the same top scene on a mb_bounds=swept device."""
    v, idx = mb.grid_quads(iml.FAST_N) if quads else mb.grid_tris(iml.FAST_N)
    v = v.copy()
    v[:, 2] = 0
    shift = np.array([iml.FAST_SHIFT, 0.0, 2.0])
    steps = [v, (v + shift).astype(np.float32)]
    scenes = {"m": imm.desc(quads_mb=(steps, idx, 4)) if quads else imm.desc(tris_mb=(steps, idx, 4))}
    inst = [(5, "m", [ih.affine((0, 0, 1))]), (9, "m", [ih.affine((1024, 0, 1)), ih.affine((1024, 0, 3))])]
    n = 512
    rng = np.random.RandomState(11)
    times = rng.rand(2 * n) * 0.999 + 0.0005  # random, not dyadic
    times[n:] = np.where(np.abs(times[n:] - 0.5) > 0.1, times[n:], times[n:] * 0.3)
    assert (np.abs(times[n:] - 0.5) > 0.1).all()
    second = np.arange(2 * n) % 2 == 1
    p = np.stack([rng.rand(2 * n) * 7 + 0.5 + np.where(second, 1024.0, 0.0), rng.rand(2 * n) * 7 + 0.5, np.full(2 * n, 10.0)], 1)
    at = times.copy()
    at[n:] = 1.0 - times[n:]  # the second half aims at where the grid is at the mirrored time
    org = (p + at[:, None] * shift * np.array([1, 1, 0])).astype(np.float32)
    rays = ds.rays_of(rtc, org, np.tile(np.array([0, 0, -1], np.float32), (2 * n, 1)))
    rays["time"] = times.astype(np.float32)
    out = {}
    for cfg in (CFG, "mb_bounds=swept"):
        dev, top, inner = imm.build(rtc, mode, scenes, inst, cfg)
        assert top.stats()["accelKind"] == (iml.kind(mode) if cfg == CFG else imm.kind(mode))
        got, occ = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
        top.intersect1M(got)
        top.occluded1M(occ)
        assert dev.error() == 0
        out[cfg] = (got, occ)
        iq.release(dev, top, inner)
    got, occ = out[CFG]
    assert (got["geomID"][:n] == 4).all() and (got["geomID"][n:] == INVALID).all()
    assert np.array_equal(got["instID"][:n], np.where(second[:n], 9, 5).astype(np.uint32))
    t64 = rays["time"][:n].astype(np.float64)
    closed = np.where(second[:n], 9.0 - 4.0 * t64, 9.0 - 2.0 * t64)
    err = np.abs(got["tfar"][:n].astype(np.float64) - closed)
    print(f"fast mover below instances, mode {mode}: {n} hits, largest |t - closed form| {err.max():.2e}")
    assert (err <= 1e-5).all()
    assert (occ["tfar"][:n] == -np.inf).all() and np.array_equal(occ["tfar"][n:], rays["tfar"][n:])
    assert got.tobytes() == out["mb_bounds=swept"][0].tobytes() and occ.tobytes() == out["mb_bounds=swept"][1].tobytes()


# ---- 5. lanes of one wave in different trees -------------------------------------------------------------------------------------------------------------
WAVE_RAYS, WAVE_SEED = 256, 5


def wave_case(rtc, bomberman):
    """scene (d) - "s": static triangles and quads, "m": motion-blur triangles and quads - under 4 exact instances that alternate between
    the two scenes; ray i is aimed at instance i % 4 (imm.aimed_rays), every 8th ray is turned round and most of those meet nothing:
    a wave of 64 consecutive rays holds lanes at top level, in static trees and in motion-blur trees at once.  The seed is chosen with
    the oracle (imm.oracle_instances): each tree kind wins 32 rays or more, every 64 consecutive rays have all four and misses"""
    scenes = imm.scenes_d(bomberman)
    inst = im.exact_instances(4, ("s", "m"))
    rays = imm.aimed_rays(rtc, scenes, inst, WAVE_RAYS, WAVE_SEED, denom=8)
    away = np.arange(WAVE_RAYS) % 8 == 7
    for f in ("dir_x", "dir_y", "dir_z"):
        rays[f][away] = -rays[f][away]
    return scenes, inst, rays, away


@pytest.mark.parametrize("mode", [0, 1])
def test_lanes_of_one_wave_in_different_trees(rtc, bomberman, mode):
    scenes, inst, rays, away = wave_case(rtc, bomberman)
    dev, top, inner = imm.build(rtc, mode, scenes, inst, CFG)
    assert top.stats()["accelKind"] == iml.kind(mode)
    got = _direct_leg(rtc, dev, top, inner, inst, rays, f"one wave in four trees, mode {mode}")
    wins = {g: int((got["geomID"] == g).sum()) for g in (3, 5, 7, 9)}
    print(f"mode {mode}: {wins}, {int((got['geomID'] == INVALID).sum())} misses")
    assert min(wins.values()) >= 8, wins
    for w in range(0, WAVE_RAYS, 64):  # every group of 64 consecutive rays: all four trees and rays that stay outside
        g = got["geomID"][w:w + 64]
        assert all((g == k).any() for k in (3, 5, 7, 9, INVALID)), (w, np.unique(g))
    iq.release(dev, top, inner)


# ---- 6. times outside the shutter, and NaN ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_times_outside_the_shutter_and_nan_equal_the_direct_leg(rtc, bomberman, mode):
    """ray.time in {-0.5, 1.5, NaN} (and 0.5 for comparison): the node step clamps the time (a NaN becomes 0) while the records extrapolate,
    at top level and below an instance alike"""
    scenes = imm.scenes_c(bomberman)
    inst = im.exact_instances(6, moving=False)
    rays = imm.aimed_rays(rtc, scenes, inst, 2048, 83, denom=8)
    rays["time"] = np.array([-0.5, 1.5, np.nan, 0.5], np.float32)[np.arange(len(rays)) % 4]
    dev, top, inner = imm.build(rtc, mode, scenes, inst, CFG)
    assert top.stats()["accelKind"] == iml.kind(mode)
    got = _direct_leg(rtc, dev, top, inner, inst, rays, f"times outside [0, 1], mode {mode}", ties=False)
    hit = got["geomID"] != INVALID
    for k in range(4):
        assert hit[k::4].sum() > 50, (k, int(hit[k::4].sum()))
    assert got[~hit].tobytes() == rays[~hit].tobytes()  # misses are left untouched
    assert dev.error() == 0
    iq.release(dev, top, inner)


# ---- 7. every entry path gives the bytes of one device-resident rtcIntersect1M -----------------------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (ih.HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


def _strided_device_copy(torch, rays):
    """the records in a device-resident array with a pitch of 96 bytes whose base is 4-byte aligned only: the kernels' VEC = false twins"""
    m = len(rays)
    raw = torch.zeros(m * 96 + 16, dtype=torch.uint8, device="cuda")
    view = raw[4:4 + m * 96].view(m, 96)
    assert view.data_ptr() % 16 == 4
    sz = rays.dtype.itemsize
    view[:, :sz] = torch.from_numpy(rays.view(np.uint8).reshape(m, sz).copy()).cuda()
    return view


@pytest.mark.parametrize("mode", [0, 1])
def test_entry_paths_are_bit_identical(rtc, po, bomberman, mode):
    import torch
    scenes = imm.scenes_c(bomberman)
    inst = im.general_instances()
    m = M
    rays = imm.rays_with_times(rtc, po, scenes, inst, m, 31, denom=None)
    dev, top, inner = imm.build(rtc, mode, scenes, inst, CFG)
    assert top.stats()["accelKind"] == iml.kind(mode)
    L = top.lib
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    top.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    hit = want["geomID"] != INVALID
    assert all(int((want["geomID"] == g).sum()) >= 8 for g in (3, 5, 7, 9)), [int((want["geomID"] == g).sum()) for g in (3, 5, 7, 9)]
    to = torch.from_numpy(iq.occ_of(rtc, rays).view(np.uint8).reshape(-1, 48).copy()).cuda()
    top.occluded1M(to)
    torch.cuda.synchronize()
    wocc = to.cpu().numpy().reshape(-1).view(rtc.RAY_DTYPE)
    assert np.array_equal(wocc["tfar"] == -np.inf, hit)
    ctx = rtc.make_context()
    for recs, ref, occluded in ((rays, want, False), (iq.occ_of(rtc, rays), wocc, True)):  # pitch 96, base 4-byte aligned: load_ray<false>
        view = _strided_device_copy(torch, recs)
        (L.rtcOccluded1M if occluded else L.rtcIntersect1M)(top.handle, C.byref(ctx), view.data_ptr(), m, 96)
        dev.check("strided batch")
        torch.cuda.synchronize()
        sz = recs.dtype.itemsize
        assert view[:, :sz].contiguous().cpu().numpy().tobytes() == ref.tobytes()
    h = iq.copy(rtc, rays)  # a host batch
    top.intersect1M(h)
    assert h.tobytes() == want.tobytes()
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
    # rtcIntersectNM (N = 4 packets) and rtcIntersectNp (pointers per component)
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
    dev, top, inner = imm.build(rtc, mode, scenes, inst, CFG + ",service=1")
    g = iq.copy(rtc, rays)
    for a in range(0, 512, 32):
        top.intersect1M(g[a:a + 32])
    assert g[:512].tobytes() == want[:512].tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    iq.release(dev, top, inner)


# ---- 8. the stack's overflow area ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_needle_soups_spill_to_hbm_and_agree_with_the_direct_leg(rtc, mode):
    """imm.deep_scene() under deep_instances(): the host walk over both node types (test_host_instance_mesh_mb_linear.py) pins that rays
    write stack slots beyond the 16 in LDS while a tree marker is stacked"""
    scenes = imm.deep_scene()
    inst = [(g, k, [m]) for g, k, m in ds.deep_instances()]
    lo, hi = ds.instance_ray_box({"m": {"tris": scenes["m"]["tris"], "quads": scenes["m"]["quads"]}}, ds.deep_instances())
    rays = rtc.aligned_rayhits(M)
    rng = np.random.RandomState(ds.GPU_RAY_SEED)
    org = ds.snap(lo + rng.rand(M, 3) * (hi - lo))
    fill_rays(rays, org, rng.randn(M, 3).astype(np.float32))
    rays["time"] = np.asarray(ds.TIMES, np.float32)[np.arange(M) % len(ds.TIMES)]
    dev, top, inner = imm.build(rtc, mode, scenes, inst, CFG)
    assert top.stats()["accelKind"] == iml.kind(mode)
    got = _direct_leg(rtc, dev, top, inner, inst, rays, f"needle soups, mode {mode}")
    hit = got["geomID"] != INVALID
    print(f"mode {mode}: {int(hit.sum())} hits, per geomID {[int((got['geomID'] == g).sum()) for g in (3, 5, 7, 9)]}")
    assert int(hit.sum()) > M // 20 and all((got["geomID"] == g).any() for g in (3, 5, 7, 9))
    assert dev.error() == 0
    iq.release(dev, top, inner)


@pytest.mark.parametrize("mode", [0, 1])
def test_tree_markers_in_the_overflow_area_agree_with_the_direct_leg(rtc, mode):
    """imm.marker_spill_case(): 128 instances with nearly coinciding bounds put the tree markers themselves beyond the 16 slots in LDS (the
    host walk pins it)"""
    scenes, inst = imm.marker_spill_case()
    rays = imm.marker_spill_rays(rtc, 2000, ds.GPU_RAY_SEED)
    dev, top, inner = imm.build(rtc, mode, scenes, inst, CFG)
    assert top.stats()["accelKind"] == iml.kind(mode)
    got = _direct_leg(rtc, dev, top, inner, inst, rays, f"markers in the overflow area, mode {mode}")
    hit = got["geomID"] != INVALID
    print(f"mode {mode}: {int(hit.sum())} hits in {len(np.unique(got['instID'][hit]))} instances")
    assert int(hit.sum()) > 100
    assert dev.error() == 0
    iq.release(dev, top, inner)


# ---- 9. unchanged ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_context_filter_and_counted_batches_stay_refused(rtc, bomberman, mode):
    scenes = imm.scenes_a(bomberman)
    dev, top, inner = imm.build(rtc, mode, scenes, [(0, "m", [ih.affine()])], CFG)
    assert top.stats()["accelKind"] == iml.kind(mode)
    log = []
    errfn = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda user, code, msg: log.append((code, (msg or b"").decode())))
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(errfn, C.c_void_p), None)
    rh = rtc.aligned_rayhits(64)
    fill_rays(rh, np.zeros((64, 3), np.float32), np.tile(UP, (64, 1)))
    src = rh.copy()
    fn = rtc.FILTER_FUNC(lambda args: None)
    ctx = rtc.make_context()
    ctx.filter = C.cast(fn, C.c_void_p)
    occ = iq.occ_of(rtc, rh)
    osrc = occ.copy()
    for call in (lambda: top.intersect1M(rh, ctx=ctx, check=False), lambda: top.occluded1M(occ, ctx=ctx, check=False)):
        call()
        assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION
        assert log and log[-1][0] == rtc.RTC_ERROR_INVALID_OPERATION and "filter is not supported on a scene with instances" in log[-1][1], log
    for counted, recs in ((top.intersect1M_counted, rh), (top.occluded1M_counted, occ)):
        with pytest.raises(rtc.RTCError) as e:
            counted(recs)
        assert e.value.code == rtc.RTC_ERROR_INVALID_OPERATION
        assert "counted batches are not supported on a scene with instances" in log[-1][1], log
    assert rh.tobytes() == src.tobytes() and occ.tobytes() == osrc.tobytes()  # records untouched
    iq.release(dev, top, inner)
