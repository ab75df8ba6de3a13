"""Instanced scenes that hold triangle and quad meshes with time steps (accel kinds 22 / 23), traced by the MESHMB form of the two-level
kernel (trace_instance_mesh_mb.hip): inside an instance the local ray traverses the scene's static triangles, motion-blur triangles,
static quads and motion-blur quads one after the other; ray.time passes through unchanged.  Scenes, instances and the legs are those of
tests/instance_mesh_mb_helpers.py; meshes are bomberman scaled by instance_helpers.SCALE and snapped to the 2^-10 grid."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
from helpers import INVALID, compare_hits, fill_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
SQ = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
Q1 = np.array([[0, 1, 2, 3]], np.uint32)
T2 = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
UP = np.array([0, 0, 1], np.float32)
# the knobs of tests/test_gpu_deep_stack.py: shares of 32 rays, refills of single lanes, leaf passes only when every lane waits
KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL")
SMALL_SHARES = {"RTAMD_CHUNK": "32", "RTAMD_REFILL_BATCH": "1", "RTAMD_LEAF_BATCH": "64"}


# ---- 1. closed form ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", ["quad", "tris"])
def test_closed_form_moving_square_below_a_static_and_a_moving_instance(rtc, shape, mode):
    steps = [SQ, SQ + np.array([0, 0, 2], np.float32)]  # the unit square moves from z = 0 to z = 2 inside the instanced scene
    scenes = {"m": imm.desc(quads_mb=(steps, Q1, 4)) if shape == "quad" else imm.desc(tris_mb=(steps, T2, 4))}
    # instance 5: static at z + 1; instance 9: moving from z + 1 to z + 3, shifted by x = 100
    inst = [(5, "m", [ih.affine((0, 0, 1))]), (9, "m", [ih.affine((100, 0, 1)), ih.affine((100, 0, 3))])]
    dev, top, inner = imm.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == imm.kind(mode)
    n = 128
    rng = np.random.RandomState(3)
    if shape == "quad":  # local points on the 2^-10 grid, half of them on either side of the v1-v3 diagonal x + y = 1
        loc = ih.snap(rng.rand(n, 2) * 0.45 + 0.03)
        side = np.arange(n) % 4 >= 2
        loc[side] = 1.0 - loc[side]
    else:  # half of them on either side of the v0-v2 diagonal x = y
        x = rng.rand(n) * 0.5 + 0.2
        d = rng.rand(n) * 0.1 + 0.04
        side = np.arange(n) % 4 >= 2
        loc = ih.snap(np.stack([x, np.where(side, x + d, x - d)], 1))
    second = np.arange(n) % 2 == 1
    time = ((np.arange(n) // 2) % 9 / 8.0).astype(np.float32)
    org = np.stack([np.where(second, loc[:, 0] + 100.0, loc[:, 0]), loc[:, 1], np.full(n, -1.0)], 1).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(UP, (n, 1)))
    rh["time"] = time
    ref = rtc.aligned_rayhits(2)  # the local normal, from the instanced scene itself: one ray on either side of the diagonal
    fill_rays(ref, np.array([[0.5, 0.25, -1.0], [0.5, 0.75, -1.0]], np.float32), np.tile(UP, (2, 1)))
    inner["m"].intersect1M(ref)
    assert (ref["geomID"] == 4).all() and (ref["Ng_x"] == 0).all() and (ref["Ng_y"] == 0).all() and ref["Ng_z"][0] != 0 and ref["Ng_z"][0] == ref["Ng_z"][1]
    top.intersect1M(rh, ctx=rtc.make_context(inst_id=77))  # the context's instID is replaced by the instance's
    assert (rh["geomID"] == 4).all()
    assert np.array_equal(rh["instID"], np.where(second, 9, 5).astype(np.uint32))
    # exact: the square is at z = 2 time locally; instance 5 adds 1, instance 9 adds 1 + 2 time; the rays start at z = -1
    assert np.array_equal(rh["tfar"], np.where(second, 2.0 + 4.0 * time, 2.0 + 2.0 * time).astype(np.float32))
    assert (rh["Ng_x"] == 0).all() and (rh["Ng_y"] == 0).all() and (rh["Ng_z"] == ref["Ng_z"][0]).all()  # Ng stays local
    if shape == "quad":
        assert (rh["primID"] == 0).all() and ((rh["u"] + rh["v"] > 1) == side).all()
    else:
        assert np.array_equal(rh["primID"], side.astype(np.uint32))
    occ = iq.occ_of(rtc, rh)
    short = np.arange(n) % 8 >= 4
    occ["tfar"] = np.where(short, 0.5, np.inf).astype(np.float32)  # the short ones end in front of the squares
    top.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, ~short) and (occ["tfar"][short] == 0.5).all()
    iq.release(dev, top, inner)


# ---- 2. the direct leg: byte for byte, no oracle arithmetic -------------------------------------------------------------------------------------
def _scenes(what, bomberman):
    return {"a": imm.scenes_a, "b": imm.scenes_b, "c": imm.scenes_c, "d": imm.scenes_d}[what](bomberman)


def _direct_leg(rtc, top, inner, inst, rays, what):
    want, per = im.direct_instances(rtc, inner, inst, rays)
    assert ih.equal_t_ties(per) == 0, what
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got.view(np.uint8).reshape(-1, 80) != want.view(np.uint8).reshape(-1, 80)).any(1).sum())} records differ"
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    hit = want["geomID"] != INVALID
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    return got


def _later_tree_wins_nearer(rtc, dev, scenes, inst, rays, got, mode):
    """rays whose hit lies in a later tree of the winning instance's scene at a smaller t than a candidate of an earlier tree: every
    part of scene "m" as a scene of its own, traced with the winning instance's exact local rays"""
    d = scenes["m"]
    parts = [p for p in imm.PARTS if d[p] is not None]
    alone = [imm.add_scene(rtc, dev, imm.desc(**{p: d[p]}), mode) for p in parts]
    t = np.full((len(inst), len(parts), len(rays)), np.inf)
    for i, (gid, _, steps) in enumerate(inst):
        w, ok = im.world2local_at(steps, rays["time"])
        for k, sc in enumerate(alone):
            sub = rtc.aligned_rayhits(len(rays))
            sub[:] = im.local_rays(rays, w, ok, exact=True)
            sc.intersect1M(sub)
            t[i, k] = np.where(sub["geomID"] != INVALID, sub["tfar"], np.inf)
    for sc in alone:
        sc.release()
    hit = np.nonzero(got["geomID"] != INVALID)[0]
    win = {g: i for i, (g, _, _) in enumerate(inst)}
    count = 0
    for r in hit:
        tt = t[win[int(got["instID"][r])], :, r]
        k = int(np.argmin(tt))
        assert tt[k] == got["tfar"][r] and d[parts[k]][2] == got["geomID"][r]
        count += bool(np.isfinite(tt[:k]).any())
    return count


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["a", "b", "c", "d"])
def test_exact_transforms_equal_the_instanced_scenes_traced_directly(rtc, po, bomberman, what, mode):
    scenes = _scenes(what, bomberman)
    keys = tuple(scenes)
    inst = im.exact_instances(9, keys)
    assert any(len(s) > 1 for _, _, s in inst)
    if what == "d":  # moving and static instances mixed
        inst = [(g, k, s if g % 2 else s[:1]) for g, k, s in inst]
    rays = imm.aimed_rays(rtc, scenes, inst, 20000, 61, denom=8)  # on the 2^-10 grid, times k / 8
    dev, top, inner = imm.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == imm.kind(mode)
    got = _direct_leg(rtc, top, inner, inst, rays, f"exact instances of scenes ({what}), mode {mode}")
    hit = got["geomID"] != INVALID
    per_kind = {int(g): int((got["geomID"][hit] == g).sum()) for g in np.unique(got["geomID"][hit])}
    times = len(np.unique(rays["time"][hit]))
    print(f"({what}) mode {mode}: {int(hit.sum())} hits, per geomID {per_kind}, {times} distinct times, {len(np.unique(got['instID'][hit]))} instances")
    assert int(hit.sum()) > 1000 and times >= 5
    assert len(np.unique(got["instID"][hit])) == 9 and (got["instID"][~hit] == INVALID).all()
    if what == "c":
        assert sorted(per_kind) == [3, 5, 7, 9] and min(per_kind.values()) >= 2000, per_kind
        later = _later_tree_wins_nearer(rtc, dev, scenes, inst, rays, got, mode)
        print(f"(c) mode {mode}: {later} rays end in a later tree at a smaller t than an earlier tree's candidate")
        assert later >= 1
    iq.release(dev, top, inner)


# ---- 3. the oracle leg: independent of the product's kernels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["a", "b"])
def test_grid_transforms_against_the_static_oracle_per_time(rtc, po, bomberman, what, mode):
    scenes = _scenes(what, bomberman)
    inst = [(g, k, [m]) for g, k, m in iq.grid_instances(9)]
    rays = imm.aimed_rays(rtc, scenes, inst, 20000, 71, denom=4)  # on the 2^-10 grid, times k / 4
    want, per, isb, _ = imm.oracle_instances(rtc, po, scenes, inst, rays, mode, exact=True)
    dev, top, inner = imm.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == imm.kind(mode)
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    if what == "b":
        ds.quad_allowances(got, want, isb, mode)
    compare_hits(got, want, what=f"grid instances of scenes ({what}), mode {mode}")
    hit = want["geomID"] != INVALID
    assert int(hit.sum()) > 1000 and len(np.unique(rays["time"][hit])) == 5 and len(np.unique(want["instID"][hit])) == 9
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    iq.release(dev, top, inner)


# ---- 4. general transforms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_general_transforms(rtc, po, bomberman, mode):
    """moving and static instances with rotations and non-uniform scales over scene (c), times random on the k/8 grid (where the lerped
    vertices are exact in fp32, so that a static oracle scene per time holds the mesh the kernel sees); rays within 1e-4 of an edge or
    of a quad's diagonal, or with a second instance within 1e-4 in t, are set aside: at most 2 % (pinned on the CPU,
    test_host_instance_mesh_mb.py)."""
    scenes, inst, rays, want, per, isb, aside = imm.general_case(rtc, po, bomberman, mode, imm.GENERAL_SEED)
    hits = int((want["geomID"] != INVALID).sum())
    print(f"mode {mode}: {hits} hits, {int(aside.sum())} rays set aside")
    assert hits > 1000 and aside.sum() <= 0.02 * len(rays)
    dev, top, inner = imm.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == imm.kind(mode)
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


# ---- 5. every entry path gives the bytes of one device-resident rtcIntersect1M ----------------------------------------------------------------------
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
    m = 20000
    rays = imm.rays_with_times(rtc, po, scenes, inst, m, 31, denom=None)
    dev, top, inner = imm.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == imm.kind(mode)
    L = top.lib
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    top.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    hit = want["geomID"] != INVALID
    assert int(hit.sum()) > 3000 and all(int((want["geomID"] == g).sum()) > 300 for g in (3, 5, 7, 9))
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
    # four batches in flight on four streams
    src = [np.roll(rays, 5000 * b).view(np.uint8).reshape(m, 80) for b in range(4)]
    streams = [torch.cuda.Stream() for _ in range(4)]
    piped = [torch.from_numpy(s.copy()).cuda() for s in src]
    torch.cuda.synchronize()
    for i, b in enumerate(piped):
        dev.set_stream(streams[i].cuda_stream)
        top.intersect1M(b, check=False)
    torch.cuda.synchronize()
    dev.check("batches in flight")
    for b, p in enumerate(piped):
        assert p.cpu().numpy().tobytes() == np.roll(want, 5000 * b).tobytes()
    iq.release(dev, top, inner)
    # service=1: no service kernel for instances, the call combiner serves the small calls
    dev, top, inner = imm.build(rtc, mode, scenes, inst, "service=1")
    g = iq.copy(rtc, rays)
    for a in range(0, 1024, 32):
        top.intersect1M(g[a:a + 32])
    assert g[:1024].tobytes() == want[:1024].tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    iq.release(dev, top, inner)


# ---- 6. the stack's overflow area ---------------------------------------------------------------------------------------------------------------
def _knobs(monkeypatch, knobs):
    """the tuning knobs are read when a device is created"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("mode", [0, 1])
def test_needle_soups_of_all_four_kinds_spill_to_hbm_and_agree_with_the_direct_leg(rtc, monkeypatch, mode):
    """imm.deep_scene(): needle soups as motion-blur triangles and quads beside a static needle mesh of each kind, under
    deep_instances().  The host walk (test_host_instance_mesh_mb.py) pins that at least 10 % of its rays write stack slots beyond the 16
    in LDS while a tree marker is stacked."""
    _knobs(monkeypatch, {})
    scenes = imm.deep_scene()
    inst = [(g, k, [m]) for g, k, m in ds.deep_instances()]
    lo, hi = ds.instance_ray_box({"m": {"tris": scenes["m"]["tris"], "quads": scenes["m"]["quads"]}}, ds.deep_instances())
    rays = rtc.aligned_rayhits(ds.GPU_RAYS)
    rng = np.random.RandomState(ds.GPU_RAY_SEED)
    org = ds.snap(lo + rng.rand(ds.GPU_RAYS, 3) * (hi - lo))
    fill_rays(rays, org, rng.randn(ds.GPU_RAYS, 3).astype(np.float32))
    rays["time"] = np.asarray(ds.TIMES, np.float32)[np.arange(ds.GPU_RAYS) % len(ds.TIMES)]
    dev, top, inner = imm.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == imm.kind(mode)
    want, per = im.direct_instances(rtc, inner, inst, rays)
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    assert dev.error() == 0
    ties = ih.equal_t_ties(per)
    hit = want["geomID"] != INVALID
    print(f"mode {mode}: {int(hit.sum())} hits, per geomID {[int((want['geomID'] == g).sum()) for g in (3, 5, 7, 9)]}, {ties} ties between instances")
    assert ties == 0 and int(hit.sum()) > 1000
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(occ["tfar"] == -np.inf, hit)
    iq.release(dev, top, inner)
    _knobs(monkeypatch, SMALL_SHARES)
    dev, top, inner = imm.build(rtc, mode, scenes, inst)
    g2, o2 = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    top.intersect1M(g2)
    top.occluded1M(o2)
    assert g2.tobytes() == got.tobytes() and o2.tobytes() == occ.tobytes(), "small shares differ"
    assert dev.error() == 0
    iq.release(dev, top, inner)


@pytest.mark.parametrize("mode", [0, 1])
def test_tree_markers_in_the_overflow_area_agree_with_the_direct_leg(rtc, mode):
    """imm.marker_spill_case(): 128 instances with nearly coinciding bounds put the exit marker and the tree markers themselves beyond
    the 16 slots in LDS (the host walk pins it), so a marker is pushed to the overflow column and popped from it with the tree's root in
    the distance word."""
    scenes, inst = imm.marker_spill_case()
    rays = imm.marker_spill_rays(rtc, 2000, ds.GPU_RAY_SEED)
    dev, top, inner = imm.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == imm.kind(mode)
    want, per = im.direct_instances(rtc, inner, inst, rays)
    got, occ = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    top.intersect1M(got)
    top.occluded1M(occ)
    assert dev.error() == 0
    hit = want["geomID"] != INVALID
    ties = ih.equal_t_ties(per)
    print(f"mode {mode}: {int(hit.sum())} hits in {len(np.unique(want['instID'][hit]))} instances, {ties} ties between instances")
    assert ties == 0 and int(hit.sum()) > 500
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    iq.release(dev, top, inner)


# ---- 7. unchanged --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_context_filter_and_counted_batches_stay_refused(rtc, bomberman, mode):
    scenes = imm.scenes_a(bomberman)
    dev, top, inner = imm.build(rtc, mode, scenes, [(0, "m", [ih.affine()])])
    assert top.stats()["accelKind"] == imm.kind(mode)
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


def test_instance_mesh_motion_blur_example_runs(tmp_path):
    exe = str(tmp_path / "instance_mesh_motion_blur_min")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "instance_mesh_motion_blur_min.c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instance_mesh_motion_blur_min: ok" in out.stdout
