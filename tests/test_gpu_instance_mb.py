"""Instance motion blur: instances with time steps (accel kinds 18..21), traced by the XFMB form of the two-level kernel of
trace_instance.hip.  A ray at ray.time enters a moving instance through world2local(time) = inverse(lerp(step[itime], step[itime + 1],
ftime)) (csrc/instance_xfm.h), whose numpy mirror (tests/instance_mb_helpers.py, pinned to the product bit for bit by
tests/test_host_instance_mb.py) gives the per-ray matrices of both legs: the local-frame oracle, and - for transforms under which
world2local(time) is exact - the instanced scene traced directly with the exact local rays."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import instance_helpers as ih
import instance_mb_helpers as im
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


def tri_scenes(bomberman_tris):
    v, t = bomberman_tris
    s = ih.snap(v * ih.SCALE)
    assert np.abs(s).max() < 16
    return {"m": {"tris": (s, t.astype(np.uint32), 0), "quads": None}}


def _scenes(what, bomberman, bomberman_tris):
    if what == "quads":
        return iq.quads_only(bomberman), ("m",)
    if what == "tris":
        return tri_scenes(bomberman_tris), ("m",)
    return iq.mixed_scenes(bomberman), ("a", "b")


# ---- 1. closed form --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", ["quad", "tris"])
def test_closed_form_moving_plane(rtc, shape, mode):
    scenes = {"m": {"tris": None, "quads": (SQ, Q1, 0)}} if shape == "quad" else {"m": {"tris": (SQ, T2, 0), "quads": None}}
    # instance 5 moves from z = 1 to z = 3; instance 9 is static: scaled by 2 about the origin and moved by x = 100 (its plane stays z = 0)
    inst = [(5, "m", [ih.affine((0, 0, 1)), ih.affine((0, 0, 3))]), (9, "m", [ih.affine((100, 0, 0), (2, 2, 2))])]
    dev, top, inner = im.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == im.kind(mode, shape == "quad")
    n = 128
    rng = np.random.RandomState(3)
    if shape == "quad":  # local points on the 2^-10 grid, half of them on either side of the v1-v3 diagonal x + y = 1 (none within 1/64 of it)
        loc = ih.snap(rng.rand(n, 2) * 0.45 + 0.03)
        side = np.arange(n) % 4 >= 2
        loc[side] = 1.0 - loc[side]
    else:  # half of them on either side of the v0-v2 diagonal x = y (none within 1/32 of it)
        x = rng.rand(n) * 0.5 + 0.2
        d = rng.rand(n) * 0.1 + 0.04
        side = np.arange(n) % 4 >= 2  # y > x: the second triangle (v0, v2, v3)
        loc = ih.snap(np.stack([x, np.where(side, x + d, x - d)], 1))
    second = np.arange(n) % 2 == 1
    time = ((np.arange(n) // 2) % 9 / 8.0).astype(np.float32)
    org = np.stack([np.where(second, 2.0 * loc[:, 0] + 100.0, loc[:, 0]), np.where(second, 2.0 * loc[:, 1], loc[:, 1]), np.full(n, -1.0)], 1).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(UP, (n, 1)))
    rh["time"] = time
    ref = rtc.aligned_rayhits(2)  # the local normal, from the instanced scene itself: one ray on either side of the diagonal
    fill_rays(ref, np.array([[0.5, 0.25, -1.0], [0.5, 0.75, -1.0]], np.float32), np.tile(UP, (2, 1)))
    inner["m"].intersect1M(ref)
    assert (ref["geomID"] == 0).all() and (ref["Ng_x"] == 0).all() and (ref["Ng_y"] == 0).all() and ref["Ng_z"][0] != 0 and ref["Ng_z"][0] == ref["Ng_z"][1]
    top.intersect1M(rh, ctx=rtc.make_context(inst_id=77))  # the context's instID is replaced by the instance's
    assert (rh["geomID"] == 0).all()
    assert np.array_equal(rh["instID"], np.where(second, 9, 5).astype(np.uint32))
    # exact: the moving plane is at z = 1 + 2 * time (time = k / 8), the static one at z = 0; t = z_plane + 1
    assert np.array_equal(rh["tfar"], np.where(second, 1.0, 2.0 + 2.0 * time).astype(np.float32))
    assert (rh["Ng_x"] == 0).all() and (rh["Ng_y"] == 0).all() and (rh["Ng_z"] == ref["Ng_z"][0]).all()  # Ng stays local
    # three roundings of at most 2^-24 each on values up to 1: 1.8e-7, taken twice (test_closed_form_translation_and_scale)
    tol = 4e-7
    if shape == "quad":  # u = x, v = y of the local point on both sides of the diagonal
        assert (rh["primID"] == 0).all()
        want_u, want_v = loc[:, 0], loc[:, 1]
        assert ((rh["u"] + rh["v"] > 1) == side).all()
    else:  # (v0, v1, v2): p = v0 + u (1, 0) + v (1, 1); (v0, v2, v3): p = v0 + u (1, 1) + v (0, 1)
        assert np.array_equal(rh["primID"], side.astype(np.uint32))
        want_u = np.where(side, loc[:, 0], loc[:, 0] - loc[:, 1])
        want_v = np.where(side, loc[:, 1] - loc[:, 0], loc[:, 1])
    assert np.all(np.abs(rh["u"] - want_u) <= tol) and np.all(np.abs(rh["v"] - want_v) <= tol) and side.sum() == n // 2
    occ = iq.occ_of(rtc, rh)
    short = np.arange(n) % 8 >= 4
    occ["tfar"] = np.where(short, 0.5, np.inf).astype(np.float32)  # the short ones end in front of the planes
    top.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, ~short) and (occ["tfar"][short] == 0.5).all()
    # the export gives the matrix of a ray's time: the world-space normal is its transposed linear part applied to Ng
    w = top.instance_world2local(5, 0.25)
    assert np.array_equal(w, ih.affine((0, 0, -1.5)))
    iq.release(dev, top, inner)


# ---- 2. the exact direct leg: no oracle arithmetic ----------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["quads", "tris", "mixed"])
def test_exact_transforms_equal_the_instanced_scene_traced_directly(rtc, po, bomberman, bomberman_tris, what, mode):
    scenes, keys = _scenes(what, bomberman, bomberman_tris)
    inst = im.exact_instances(9, keys)
    assert sorted({len(s) for _, _, s in inst}) == [2, 3, 5]
    rays = im.rays_with_times(rtc, po, scenes, inst, 20000, 61, snapped=True, eighths=True)
    dev, top, inner = im.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == im.kind(mode, what != "tris")
    got = _direct_leg(rtc, top, inner, inst, rays, f"exact moving instances of {what}, mode {mode}")
    hit = got["geomID"] != INVALID
    assert int(hit.sum()) > 1000, int(hit.sum())
    assert len(np.unique(got["instID"][hit])) == 9 and (got["instID"][~hit] == INVALID).all()
    assert len(np.unique(rays["time"][hit])) == 9  # hits at every k / 8
    iq.release(dev, top, inner)


# ---- 3. identical steps equal the static scene ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_identical_steps_give_the_bytes_of_the_static_scene(rtc, po, bomberman, mode):
    scenes, keys = iq.mixed_scenes(bomberman), ("a", "b")
    one = im.exact_instances(9, keys, moving=False)
    same = [(g, k, [s[0]] * (2 + g % 4)) for g, k, s in one]
    # times k / 8: madd(1 - f, a, f * a) == a holds in fp32 only while 1 - f, f * a and the sum are exact - signed powers of two and
    # translations on the 2^-10 grid below 256 times a multiple of 1/8 are; at a random time the lerp of two equal steps is a rounded a
    rays = im.rays_with_times(rtc, po, scenes, one, 20000, 62, snapped=True, eighths=True)
    for _, _, steps in same:
        w, ok = im.world2local_at(steps, rays["time"])
        assert ok.all() and (w == ih.world2local(steps[0])).all()
    dev, top, inner = im.build(rtc, mode, scenes, same)
    dev2, stat, inner2 = im.build(rtc, mode, scenes, one)
    assert top.stats()["accelKind"] == im.kind(mode, True) and stat.stats()["accelKind"] == im.static_kind(mode, True)
    got, want = iq.copy(rtc, rays), iq.copy(rtc, rays)
    top.intersect1M(got)
    stat.intersect1M(want)
    assert got.tobytes() == want.tobytes() and int((want["geomID"] != INVALID).sum()) > 1000
    og, ow = iq.occ_of(rtc, rays), iq.occ_of(rtc, rays)
    top.occluded1M(og)
    stat.occluded1M(ow)
    assert og.tobytes() == ow.tobytes()
    iq.release(dev2, stat, inner2)
    iq.release(dev, top, inner)


# ---- 4. static beside moving ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_one_step_instances_beside_moving_ones_return_the_static_bytes(rtc, po, bomberman, mode):
    scenes, keys = iq.mixed_scenes(bomberman), ("a", "b")
    static = [(g, k, [m]) for g, k, m in iq.general_instances(keys)]
    # three moving instances above the static ones' rays (the statics stay below y = 60)
    moving = [(20 + i, keys[i % 2], [ih.affine((60.0 * i - 60.0, 400.0 + 30.0 * j, 5.0 * j), (1.2, 0.9, 1.0), ih.rotation((1, i, 2), 25.0 * j + 10.0 * i)) for j in range(2 + i)])
              for i in range(3)]
    rays = im.rays_with_times(rtc, po, scenes, static, 20000, 63)
    dev, top, inner = im.build(rtc, mode, scenes, static + moving)
    dev2, stat, inner2 = im.build(rtc, mode, scenes, static)
    assert top.stats()["accelKind"] == im.kind(mode, True) and stat.stats()["accelKind"] == im.static_kind(mode, True)
    got, want = iq.copy(rtc, rays), iq.copy(rtc, rays)
    top.intersect1M(got)
    stat.intersect1M(want)
    ends_static = got["instID"] < 20  # a hit in a one-step instance
    assert int(ends_static.sum()) > 1000
    assert got[ends_static].tobytes() == want[ends_static].tobytes()
    away = (got["geomID"] == INVALID) | ends_static  # the moving instances are out of these rays' way
    assert int((~away).sum()) <= len(rays) // 100
    assert got[away].tobytes() == want[away].tobytes()
    iq.release(dev2, stat, inner2)
    iq.release(dev, top, inner)


# ---- 5. company across accels --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_moving_instance_beside_top_level_meshes_nearest_hit_wins(rtc, mode):
    scenes = {"m": {"tris": None, "quads": (SQ, Q1, 0)}}
    # the unit quad stretched over x in [0, 4), moving from z = 2 to z = 4 (geomID 10)
    inst = [(10, "m", [ih.affine((0, 0, 2), (4, 1, 1)), ih.affine((0, 0, 4), (4, 1, 1))])]

    def extra(top):
        # a motion-blur triangle mesh (geomID 1) over x in [0, 2) moving from z = 1 to z = 5; a static quad mesh (geomID 2) over x in [2, 4) at z = 3
        v = np.concatenate([SQ, SQ + (1, 0, 0)]).astype(np.float32)
        tris = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.uint32)
        top.add_triangles_mb([v + (0, 0, 1), v + (0, 0, 5)], tris, geom_id=1)
        q = np.concatenate([SQ + (2, 0, 3), SQ + (3, 0, 3)]).astype(np.float32)
        top.add_quads(q, np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.uint32), geom_id=2)

    dev, top, inner = im.build(rtc, mode, scenes, inst, extra=extra)
    n = 256
    rng = np.random.RandomState(5)
    x = (np.arange(n) % 4 + 0.1 + 0.8 * rng.rand(n)).astype(np.float32)  # away from the seams
    org = np.stack([x, (rng.rand(n) * 0.9 + 0.05), np.full(n, -1.0)], 1).astype(np.float32)
    k8 = np.array([0, 1, 2, 3, 5, 6, 7, 8])[(np.arange(n) // 4) % 8]  # times k / 8 without 1/2, where the planes meet
    time = (k8 / 8.0).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(UP, (n, 1)))
    rh["time"] = time
    cell = np.floor(x).astype(int)
    z_inst, z_tri, z_quad = 2.0 + 2.0 * time, 1.0 + 4.0 * time, np.full(n, 3.0)
    z_other = np.where(cell < 2, z_tri, z_quad)
    inst_wins = z_inst < z_other
    assert inst_wins.sum() > 50 and (~inst_wins).sum() > 50 and (inst_wins[cell < 2].sum() > 20) and (inst_wins[cell >= 2].sum() > 20)
    for ctx_inst in (INVALID, 77):
        got = iq.copy(rtc, rh)
        top.intersect1M(got, ctx=rtc.make_context(inst_id=ctx_inst))
        assert np.array_equal(got["geomID"], np.where(inst_wins, 0, np.where(cell < 2, 1, 2)).astype(np.uint32))
        assert np.array_equal(got["instID"], np.where(inst_wins, 10, ctx_inst).astype(np.uint32))  # instID only for instance hits
        # planes at eighths seen along +z from z = -1: every operand and the result are exact
        assert np.array_equal(got["tfar"], (np.where(inst_wins, z_inst, z_other) + 1.0).astype(np.float32))
    iq.release(dev, top, inner)


# ---- 6. general transforms ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["quads", "tris"])
def test_general_transforms(rtc, po, bomberman, bomberman_tris, what, mode):
    scenes, _ = _scenes(what, bomberman, bomberman_tris)
    inst = im.general_instances()
    rays = im.rays_with_times(rtc, po, scenes, inst, im.GENERAL_RAYS, im.GENERAL_SEED)
    want, per, isb, want_tri = im.oracle_instances(rtc, po, scenes, inst, rays, mode)
    aside = iq.quad_set_aside(want, per, want_tri, [0]) if what == "quads" else ih.set_aside(want, per)
    hits = int((want["geomID"] != INVALID).sum())
    assert hits > 1000 and aside.sum() <= 0.01 * hits  # the cap, pinned on the CPU (test_host_instance_mb.py)
    dev, top, inner = im.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == im.kind(mode, what == "quads")
    for g, _, steps in inst:  # the export is the mirror's matrix, bit for bit: the oracle's local rays are the kernel's
        tm = rays["time"][g::500]
        w, ok = im.world2local_at(steps, tm)
        assert ok.all() and all(np.array_equal(top.instance_world2local(g, float(t)), w[i]) for i, t in enumerate(tm))
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    keep = ~aside
    if mode == 1 and what == "quads":
        b = isb & keep
        for f in ("u", "v"):
            assert np.all(np.abs(got[f][b].astype(np.float64) - want[f][b]) <= 4e-7 + 1e-4 * np.abs(want[f][b]))
            want[f][b] = got[f][b]
    compare_hits(got[keep], want[keep], what=f"general moving transforms over {what}, mode {mode}")
    # a ray set aside is still a miss, or a hit within 1e-4 in t of SOME instance's oracle hit
    for k in np.nonzero(aside)[0]:
        if got["geomID"][k] == INVALID:
            assert got["tfar"][k] == rays["tfar"][k]
            continue
        ts = [float(p["tfar"][k]) for p in per if p["geomID"][k] != INVALID]
        assert any(abs(float(got["tfar"][k]) - t) <= 1e-4 * abs(t) for t in ts), (k, got[k], ts)
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    assert np.array_equal((occ["tfar"] == -np.inf)[keep], (want["geomID"] != INVALID)[keep])
    iq.release(dev, top, inner)


# ---- 7. singular interpolation ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", ["quad", "tris"])
def test_singular_interpolated_transform_is_not_entered(rtc, shape, mode):
    scenes = {"m": {"tris": None, "quads": (SQ, Q1, 0)}} if shape == "quad" else {"m": {"tris": (SQ, T2, 0), "quads": None}}
    # diag(1, 1, 1) -> diag(-1, 1, 1) at z = 2: at time 1/2 the x column is zero; at time 1 the quad lies over x in (-1, 0]
    inst = [(3, "m", [ih.affine((0, 0, 2)), ih.affine((0, 0, 2), (-1, 1, 1))])]
    dev, top, inner = im.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == im.kind(mode, shape == "quad")
    assert not top.instance_world2local(3, 0.5).any()  # the export says so: all zero
    n = 96
    rng = np.random.RandomState(9)
    time = np.array([0.0, 0.5, 1.0], np.float32)[np.arange(n) % 3]
    x = (rng.rand(n) * 0.8 + 0.1) * np.where(time == 1.0, -1.0, np.where(np.arange(n) % 2 == 0, 1.0, -1.0))
    org = np.stack([x, rng.rand(n) * 0.8 + 0.1, np.full(n, -1.0)], 1).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(UP, (n, 1)))
    rh["time"] = time
    src = rh.copy()
    top.intersect1M(rh)
    assert dev.error() == rtc.RTC_ERROR_NONE
    mid = time == 0.5
    assert rh[mid].tobytes() == src[mid].tobytes()  # untouched
    hits = (time == 1.0) | ((time == 0.0) & (x > 0))
    assert np.array_equal(rh["geomID"] != INVALID, hits) and hits.sum() > 40
    assert (rh["tfar"][hits] == 3.0).all() and (rh["instID"][hits] == 3).all()
    assert not any(np.isnan(rh[f]).any() for f in ("org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "Ng_x", "Ng_y", "Ng_z", "u", "v"))
    occ = iq.occ_of(rtc, src)
    top.occluded1M(occ)
    assert dev.error() == rtc.RTC_ERROR_NONE
    assert np.array_equal(occ["tfar"] == -np.inf, hits) and np.array_equal(occ["tfar"][~hits], src["tfar"][~hits])
    iq.release(dev, top, inner)


# ---- 8. every entry path gives the bytes of one device-resident rtcIntersect1M --------------------------------------------------------------------------------
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
    scenes = iq.mixed_scenes(bomberman)
    inst = im.general_instances(keys=("a", "b"))
    m = 20000
    rays = im.rays_with_times(rtc, po, scenes, inst, m, 31)
    dev, top, inner = im.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == im.kind(mode, True)
    L = top.lib
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    top.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    hit = want["geomID"] != INVALID
    assert int(hit.sum()) > 3000 and int((want["geomID"] == 3).sum()) > 500 and int((want["geomID"] == 7).sum()) > 500
    to = torch.from_numpy(iq.occ_of(rtc, rays).view(np.uint8).reshape(-1, 48).copy()).cuda()
    top.occluded1M(to)
    torch.cuda.synchronize()
    wocc = to.cpu().numpy().reshape(-1).view(rtc.RAY_DTYPE)
    assert np.array_equal(wocc["tfar"] == -np.inf, hit)
    # a record array with a pitch of 96 bytes and a base that is only 4-byte aligned: the VEC = false twins (the time is read at byte 28)
    ctx = rtc.make_context()
    for recs, ref, occluded in ((rays, want, False), (iq.occ_of(rtc, rays), wocc, True)):
        view = _strided_device_copy(torch, recs)
        (L.rtcOccluded1M if occluded else L.rtcIntersect1M)(top.handle, C.byref(ctx), view.data_ptr(), m, 96)
        dev.check("strided batch")
        torch.cuda.synchronize()
        sz = recs.dtype.itemsize
        assert view[:, :sz].contiguous().cpu().numpy().tobytes() == ref.tobytes()
    # host batch above tunePipeMinRays (pipelined) and below it (staged; <= 512 rays: traced in place)
    h = iq.copy(rtc, rays)
    top.intersect1M(h)
    assert h.tobytes() == want.tobytes()
    s = iq.copy(rtc, rays)
    top.intersect1M(s[:9000])
    for a in range(9000, 10000, 500):
        top.intersect1M(s[a:a + 500])
    assert s[:10000].tobytes() == want[:10000].tobytes()
    ho = iq.occ_of(rtc, rays)
    top.occluded1M(ho)
    assert ho.tobytes() == wocc.tobytes()
    # rtcIntersect1 / rtcOccluded1
    k = 64
    one = iq.copy(rtc, rays)
    o1 = iq.occ_of(rtc, rays)
    for i in range(k):
        top.intersect1(one[i:i + 1])
        top.occluded1(o1[i:i + 1])
    assert one[:k].tobytes() == want[:k].tobytes() and o1[:k].tobytes() == wocc[:k].tobytes()
    # rtcIntersect1Mp
    p = iq.copy(rtc, rays)
    arr = (C.c_void_p * 256)(*[p[i:i + 1].ctypes.data for i in range(256)])
    L.rtcIntersect1Mp(top.handle, C.byref(ctx), arr, 256)
    dev.check("rtcIntersect1Mp")
    assert p[:256].tobytes() == want[:256].tobytes()
    # a packet call, per-lane times
    fn = L.rtcIntersect8
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    valid = np.full(8, -1, np.int32)
    for a in range(0, 64, 8):
        assert len(np.unique(rays["time"][a:a + 8])) == 8
        pk = _soa(rays[a:a + 8], 8, True)
        fn(valid.ctypes.data, top.handle, C.addressof(ctx), pk.ctypes.data)
        dev.check("rtcIntersect8")
        assert np.array_equal(pk, _soa(want[a:a + 8], 8, True))
    iq.release(dev, top, inner)
    # two shards on one GPU, and service=1 (no service kernel for instances: the call combiner serves the small calls)
    for cfg, small in (("gpus=0:0", False), ("service=1", True)):
        dev, top, inner = im.build(rtc, mode, scenes, inst, cfg)
        g = iq.copy(rtc, rays)
        if small:
            for a in range(0, 2048, 32):
                top.intersect1M(g[a:a + 32])
            assert g[:2048].tobytes() == want[:2048].tobytes()
            assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
        else:
            top.intersect1M(g)
            assert g.tobytes() == want.tobytes()
        iq.release(dev, top, inner)


# ---- 9. updates --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_transform_update_matches_a_fresh_scene(rtc, po, bomberman, mode):
    scenes = iq.mixed_scenes(bomberman)
    inst = im.general_instances(keys=("a", "b"))
    moved = []
    for g, k, steps in inst:
        m = np.asarray(steps[1], np.float64)
        new = steps[:1] + [ih.affine((m[0, 3] + 3.0, m[1, 3] - 2.0, m[2, 3]), (1.1, 0.9, 1.0), ih.rotation((0, 1, 0.3), 20.0 * g))] + steps[2:]
        moved.append((g, k, new))
    rays = im.rays_with_times(rtc, po, scenes, inst, 8192, 5)
    dev, top, inner = im.build(rtc, mode, scenes, inst)
    before = iq.copy(rtc, rays)
    top.intersect1M(before)
    for g, _, steps in moved:
        top.set_instance_transform(g, steps[1], time_step=1)  # rtcSetGeometryTransform + rtcCommitGeometry
    top.commit()
    after = iq.copy(rtc, rays)
    top.intersect1M(after)
    dev2, fresh, inner2 = im.build(rtc, mode, scenes, moved)
    want = iq.copy(rtc, rays)
    fresh.intersect1M(want)
    assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()
    assert int((want["geomID"] != INVALID).sum()) > 500
    iq.release(dev2, fresh, inner2)
    iq.release(dev, top, inner)


@pytest.mark.parametrize("mode", [0, 1])
def test_time_step_count_back_to_one_returns_to_the_static_kind(rtc, po, bomberman, mode):
    scenes = iq.mixed_scenes(bomberman)
    static = iq.general_instances(keys=("a", "b"))
    inst = [(g, k, [m]) for g, k, m in static]
    g4, k4, m4 = static[4]
    inst[4] = (g4, k4, [m4, ih.affine((m4[0, 3] + 5.0, m4[1, 3], m4[2, 3] - 4.0), (1.0, 1.2, 0.8), ih.rotation((1, 1, 0), 35.0))])  # the only moving one
    rays = im.rays_with_times(rtc, po, scenes, inst, 8192, 6)
    dev, top, inner = im.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == im.kind(mode, True)
    before = iq.copy(rtc, rays)
    top.intersect1M(before)
    g = top.lib.rtcGetGeometry(top.handle, g4)
    top.lib.rtcSetGeometryTimeStepCount(g, 1)
    top.lib.rtcCommitGeometry(g)
    top.commit()
    assert top.stats()["accelKind"] == im.static_kind(mode, True)
    after = iq.copy(rtc, rays)
    top.intersect1M(after)
    dev2, fresh, inner2 = iq.build(rtc, mode, scenes, static)
    want = iq.copy(rtc, rays)
    fresh.intersect1M(want)
    assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()
    assert top.accel_data(2).tobytes() == fresh.accel_data(2).tobytes() and top.accel_data(0).tobytes() == fresh.accel_data(0).tobytes()
    iq.release(dev2, fresh, inner2)
    iq.release(dev, top, inner)


# ---- 10. four batches in flight ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_four_batches_on_four_streams_match_serial(rtc, po, bomberman, mode):
    import torch
    scenes = iq.mixed_scenes(bomberman)
    inst = im.general_instances(keys=("a", "b"))
    dev, top, inner = im.build(rtc, mode, scenes, inst)
    n = 20000
    src = [im.rays_with_times(rtc, po, scenes, inst, n, 40 + b).view(np.uint8).reshape(n, 80) for b in range(4)]
    serial = [torch.from_numpy(s.copy()).cuda() for s in src]
    for b in serial:
        top.intersect1M(b)
    dev.synchronize()
    streams = [torch.cuda.Stream() for _ in range(4)]
    piped = [torch.from_numpy(s.copy()).cuda() for s in src]
    torch.cuda.synchronize()
    for i, b in enumerate(piped):
        dev.set_stream(streams[i].cuda_stream)
        top.intersect1M(b, check=False)
    torch.cuda.synchronize()
    dev.check("pipelined batches")
    nh = 0
    for a, b in zip(serial, piped):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        nh += int((a.view(torch.int32)[:, 18] != -1).sum().item())
    assert nh > 4000
    iq.release(dev, top, inner)


# ---- 11. the C example -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_instance_motion_blur_example_runs(tmp_path):
    exe = str(tmp_path / "instance_motion_blur_min")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "instance_motion_blur_min.c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instance_motion_blur_min: ok" in out.stdout
