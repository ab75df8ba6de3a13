"""Motion-blur triangle meshes (time steps, ray.time) traced by the TriMB leaves of trace_tri_mb.hip.

The oracle has no motion blur, so the parity tests make it exact by construction: every vertex coordinate of every time step is
snapped to a multiple of 2^-10 below 64 and the ray times are multiples of 1 / (4 S), so ftime is 0, 1/4, 1/2 or 3/4 and every
interpolated coordinate is a multiple of 2^-12 below 2^7 - exactly representable in fp32 whatever form the lerp takes.  One static
po.TriangleScene per distinct time, built from those exact vertices (float64, cast), traces the rays of that time."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from helpers import INVALID, compare_hits, fill_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")
ROBUST = 4  # RTC_SCENE_FLAG_ROBUST
MODES = {0: "pluecker", 1: "moeller"}
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
SCALE = 0.0625  # bomberman spans +-246: scaled so that every coordinate of every (moved) step stays below 64 before it is snapped
HITF = ["Ng_x", "Ng_y", "Ng_z", "u", "v", "primID", "geomID", "instID"]


def _device(rtc, mode, extra=""):
    # tri_accel_mb=default: mode 0 = robust scene (Pluecker, accel kind 10), mode 1 = non-robust scene (Moeller, kind 11)
    return rtc.Device(extra), (ROBUST if mode == 0 else 0)


def _snap(v):
    s = (np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0)
    assert np.abs(s).max() < 64
    return s.astype(np.float32)


def _rot_y(v, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    m = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    ctr = (v.min(0) + v.max(0)) / 2
    return (np.asarray(v, np.float64) - ctr) @ m.T + ctr


def _at_time(steps, time):
    """the mesh at `time` (getTimeSegment + lerp in float64; exact in fp32 for snapped steps and times k / (4 S))"""
    S = len(steps) - 1
    ts = np.float64(time) * S
    it = int(min(max(np.floor(ts), 0), S - 1))
    f = ts - it
    v = (1.0 - f) * steps[it].astype(np.float64) + f * steps[it + 1].astype(np.float64)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v.astype(np.float32)


@pytest.fixture(scope="module")
def two_steps(bomberman_tris):
    v, tris = bomberman_tris
    assert len(tris) == 1454
    s0 = _snap(v * SCALE)
    ext = s0.max(0) - s0.min(0)
    # step 1: rotated about y by 20 degrees and moved by 0.3 x extent along x (the mesh is flat in y: a move along y as well would
    # make the box the rays are drawn from 30 % taller and leave fewer than 5 000 hits per time)
    s1 = _snap(_rot_y(s0, 20.0) + np.array([0.3 * ext[0], 0.0, 0.0]))
    return [s0, s1], tris


@pytest.fixture(scope="module")
def five_steps(bomberman_tris):
    v, tris = bomberman_tris
    s0 = _snap(v * SCALE)
    ext = s0.max(0) - s0.min(0)
    # a curved path: rotation and a parabola, so that the four segments differ
    return [_snap(_rot_y(s0, 12.0 * k) + ext * np.array([0.1 * k, 0.03 * k * k, -0.05 * k])) for k in range(5)], tris


def _bounds(steps):
    a = np.concatenate(steps)
    return a.min(0), a.max(0)


def _timed_rays(rtc, po, m, steps, times, seed):
    lo, hi = _bounds(steps)
    src = po.make_random_rays(m, lo, hi, seed=seed)
    rays = rtc.aligned_rayhits(m)
    rays[:] = src
    rays["time"] = np.asarray(times, np.float32)[np.arange(m) % len(times)]
    return rays


def _oracle_per_time(rtc, po, steps, tris, rays, mode, geom_id=0):
    """the rays traced by one static oracle scene per distinct time"""
    want = rays.copy()
    for t in np.unique(rays["time"]):
        sel = np.nonzero(rays["time"] == t)[0]
        sub = rtc.aligned_rayhits(len(sel))
        sub[:] = rays[sel]
        orc = po.TriangleScene(_at_time(steps, t), tris, mode, np.full(len(tris), geom_id, np.uint32))
        orc.intersect1M(sub, nthreads=16)
        orc.free()
        want[sel] = sub
    return want


def _occ_of(rtc, rays):
    occ = rtc.aligned_rays(len(rays))
    for f in occ.dtype.names:
        occ[f] = rays[f]
    return occ


def _mb_scene(rtc, mode, steps, tris, extra=""):
    dev, flags = _device(rtc, mode, extra)
    sc = rtc.Scene(dev, flags)
    sc.add_triangles_mb(steps, tris)
    sc.commit()
    assert sc.stats()["accelKind"] == (10 if mode == 0 else 11)
    return dev, sc


# ---- 4. closed form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_translating_triangle_closed_form(rtc, mode):
    tri = np.array([[-1, -1, 0], [3, -1, 0], [-1, 3, 0]], np.float32)
    idx = np.array([[0, 1, 2]], np.uint32)
    dev, sc = _mb_scene(rtc, mode, [tri, tri + np.array([0, 0, 1], np.float32)], idx)
    n = 256
    rng = np.random.RandomState(7)
    org = np.stack([rng.rand(n) * 0.9 + 0.05, rng.rand(n) * 0.9 + 0.05, -np.ones(n)], 1).astype(np.float32)
    d = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    times = rng.rand(n).astype(np.float32)  # random, not dyadic
    times[0], times[1] = -0.25, 1.5         # outside [0, 1]: the segment is extrapolated
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, d)
    rh["time"] = times
    sc.intersect1M(rh)
    assert (rh["geomID"] == 0).all() and (rh["primID"] == 0).all()
    assert np.all(np.abs(rh["tfar"].astype(np.float64) - (1.0 + times.astype(np.float64))) <= 1e-5)
    # u, v do not depend on z for these rays: the static triangle's answer
    dev0, flags = _device(rtc, mode)
    st = rtc.Scene(dev0, flags)
    st.add_triangles(tri, idx)
    st.commit()
    ref = rtc.aligned_rayhits(n)
    fill_rays(ref, org, d)
    st.intersect1M(ref)
    assert (ref["geomID"] == 0).all()
    assert np.all(np.abs(rh["u"] - ref["u"]) <= 2e-6) and np.all(np.abs(rh["v"] - ref["v"]) <= 2e-6)
    st.release()
    dev0.release()
    occ = _occ_of(rtc, rh)
    occ["tfar"] = np.inf
    occ["tfar"][5], occ["time"][5] = 0.5, 0.9  # the triangle is at distance 1.9 at that time
    sc.occluded1M(occ)
    keep = np.arange(n) == 5
    assert (occ["tfar"][~keep] == -np.inf).all() and occ["tfar"][5] == np.float32(0.5)
    # tnear > tfar is skipped, a miss leaves the record untouched
    one = rtc.aligned_rayhits(2)
    fill_rays(one, np.array([[0.2, 0.2, -1], [5, 5, -1]], np.float32), d[:2])
    one["time"] = 0.5
    one["tnear"][0], one["tfar"][0] = 3.0, 2.0
    before = one.copy()
    sc.intersect1M(one)
    assert one.tobytes() == before.tobytes()
    sc.release()
    dev.release()


# ---- 5. block and tie rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_coincident_triangles_follow_the_static_block_rule(rtc, mode):
    tri = np.array([[-1, -1, 0], [3, -1, 0.5], [-1, 3, 0.25]], np.float32)
    v0 = np.tile(tri, (9, 1))
    idx = np.arange(27, dtype=np.uint32).reshape(9, 3)
    steps = [v0, (v0 + np.array([0.5, 0.25, 1.0], np.float32)).astype(np.float32)]
    dev, sc = _mb_scene(rtc, mode, steps, idx)
    assert sc.accel_root() & 0x80000000 and sc.stats()["primCount"] == 9  # one leaf, three blocks
    n = 64
    rng = np.random.RandomState(3)
    org = np.stack([rng.rand(n) * 0.9 + 0.05, rng.rand(n) * 0.9 + 0.05, -np.ones(n)], 1).astype(np.float32)
    d = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    for time in (0.0, 0.25, 0.5, 1.0):
        rh = rtc.aligned_rayhits(n)
        fill_rays(rh, org, d)
        rh["time"] = time
        sc.intersect1M(rh)
        dev0, flags = _device(rtc, mode)
        st = rtc.Scene(dev0, flags)
        st.add_triangles(_at_time(steps, time), idx)
        st.commit()
        ref = rtc.aligned_rayhits(n)
        fill_rays(ref, org, d)
        ref["time"] = time
        st.intersect1M(ref)
        assert (ref["geomID"] == 0).all()
        assert np.array_equal(rh["primID"], ref["primID"]) and np.array_equal(rh["geomID"], ref["geomID"])
        assert np.allclose(rh["tfar"], ref["tfar"], rtol=1e-6)
        st.release()
        dev0.release()
    sc.release()
    dev.release()


# ---- 6. / 7. parity against the per-time oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_two_step_parity(rtc, po, two_steps, mode):
    steps, tris = two_steps
    dev, sc = _mb_scene(rtc, mode, steps, tris)
    times = [0.0, 0.25, 0.5, 0.75, 1.0]
    rays = _timed_rays(rtc, po, 200000, steps, times, seed=31)
    want = _oracle_per_time(rtc, po, steps, tris, rays, mode)
    got = rays.copy()
    sc.intersect1M(got)
    for t in times:
        hits = int(((want["geomID"] != INVALID) & (rays["time"] == np.float32(t))).sum())
        print(f"two steps ({MODES[mode]}), time {t}: {hits} hits")
        assert hits >= 5000, (t, hits)
    compare_hits(got, want, 1e-4, f"two-step bomberman {MODES[mode]}")
    occ = _occ_of(rtc, rays)
    sc.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, want["geomID"] != INVALID)
    assert np.array_equal(occ["tfar"][occ["tfar"] != -np.inf], rays["tfar"][occ["tfar"] != -np.inf])
    sc.release()
    dev.release()


@pytest.mark.parametrize("mode", [0, 1])
def test_five_step_parity(rtc, po, five_steps, mode):
    steps, tris = five_steps
    dev, sc = _mb_scene(rtc, mode, steps, tris)
    assert sc.stats()["primCount"] == 4 * len(tris)
    times = [k / 16.0 for k in range(17)]  # k = 4, 8, 12: a step time, floor() puts it into the segment that STARTS there
    rays = _timed_rays(rtc, po, 100000, steps, times, seed=32)
    want = _oracle_per_time(rtc, po, steps, tris, rays, mode)
    got = rays.copy()
    sc.intersect1M(got)
    hits = compare_hits(got, want, 1e-4, f"five-step bomberman {MODES[mode]}")
    per_time = [int(((want["geomID"] != INVALID) & (rays["time"] == np.float32(t))).sum()) for t in times]
    print(f"five steps ({MODES[mode]}): {hits} hits, per time {per_time}")
    assert min(per_time) >= 100, per_time  # every time, the step times 4/16, 8/16, 12/16 among them, is exercised
    occ = _occ_of(rtc, rays)
    sc.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, want["geomID"] != INVALID)
    sc.release()
    dev.release()


# ---- 8. mixed scene ---------------------------------------------------------------------------------------------------------
def _random_quads(n, seed, lo, hi):
    rng = np.random.RandomState(seed)
    c = (lo + rng.rand(n, 1, 3) * (hi - lo)).astype(np.float32)
    size = 0.1 * float(np.max(hi - lo))
    v = (c + (rng.rand(n, 4, 3).astype(np.float32) - 0.5) * size).astype(np.float32).reshape(-1, 3)
    return v, np.arange(4 * n, dtype=np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("mode", [0, 1])
def test_mixed_scene_equals_the_accels_traced_in_reference_order(rtc, po, bomberman, mode):
    verts, fs, fi = bomberman
    lo, hi = verts.min(0), verts.max(0)
    tv, tt = _random_quads(300, 5, lo, hi)
    tris = tt[:, :3].copy()
    mv, mt = _random_quads(300, 7, lo, hi)
    mtris = mt[:, :3].copy()
    msteps = [mv, (mv + 0.2 * (hi - lo)).astype(np.float32), (mv + np.array([0.2, 0.5, 0.1], np.float32) * (hi - lo)).astype(np.float32)]
    qv, qq = _random_quads(400, 6, lo, hi)

    def scene(parts):
        dev, flags = _device(rtc, mode)
        sc = rtc.Scene(dev, flags)
        if "t" in parts:
            sc.add_triangles(tv, tris, geom_id=0)
        if "m" in parts:
            sc.add_triangles_mb(msteps, mtris, geom_id=1)
        if "q" in parts:
            sc.add_quads(qv, qq, geom_id=2)
        if "s" in parts:
            sc.add_subdiv(verts, fs, fi, geom_id=3)
        sc.commit()
        return dev, sc

    m = 100000
    rays = po.make_random_rays(m, lo, hi + 0.3 * (hi - lo), seed=9)
    rays["time"] = np.random.RandomState(4).rand(m).astype(np.float32)
    dev, sc = scene("tmqs")
    got = rtc.aligned_rayhits(m)
    got[:] = rays
    sc.intersect1M(got)
    want = rtc.aligned_rayhits(m)
    want[:] = rays
    for p in "tmqs":  # Scene::commit order (scene.cpp:650-654), AccelN traces them one after another
        d1, s1 = scene(p)
        s1.intersect1M(want)
        s1.release()
        d1.release()
    assert got.tobytes() == want.tobytes()
    counts = [int((got["geomID"] == g).sum()) for g in range(4)]
    print(f"mixed scene ({MODES[mode]}): hits per geometry {counts}")
    assert min(counts) > 100, counts
    sc.release()
    dev.release()


@pytest.mark.parametrize("mode", [0, 1])
def test_coincident_static_and_resting_moving_triangle_return_the_moving_mesh(rtc, mode):
    dev, flags = _device(rtc, mode)
    sc = rtc.Scene(dev, flags)
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    idx = np.array([[0, 1, 2]], np.uint32)
    assert sc.add_triangles(v, idx) == 0
    assert sc.add_triangles_mb([v, v], idx) == 1
    sc.commit()
    n = 64
    rng = np.random.RandomState(2)
    org = np.stack([rng.rand(n) * 0.4 + 0.05, rng.rand(n) * 0.4 + 0.05, -np.ones(n)], 1).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(np.array([0, 0, 1], np.float32), (n, 1)))
    rh["time"] = rng.rand(n).astype(np.float32)
    sc.intersect1M(rh)
    assert (rh["geomID"] == 1).all()  # traced after the static triangles, the depth test T <= absDen * tfar accepts the equal t
    assert np.allclose(rh["tfar"], 1.0)
    sc.release()
    dev.release()


# ---- 9. filters ---------------------------------------------------------------------------------------------------------------
NT = 5


def _ray_fields(args):
    ray = C.cast(args.contents.ray, C.POINTER(C.c_float * 12)).contents
    hit = C.cast(args.contents.hit, C.POINTER(C.c_uint * 8)).contents
    return ray, hit


def _stack(rtc, mode):
    """triangle g moves from z = g to z = g + 1: a ray along +z from z = -1 at `time` meets it at g + 1 + time"""
    dev, flags = _device(rtc, mode)
    sc = rtc.Scene(dev, flags)
    for z in range(NT):
        v = np.array([[-1, -1, z], [3, -1, z], [-1, 3, z]], np.float32)
        assert sc.add_triangles_mb([v, v + np.array([0, 0, 1], np.float32)], np.array([[0, 1, 2]], np.uint32)) == z
    return dev, sc


def _stack_rays(rtc, n, seed=1):
    rng = np.random.RandomState(seed)
    rh = rtc.aligned_rayhits(n)
    org = np.stack([rng.rand(n) * 0.9 + 0.05, rng.rand(n) * 0.9 + 0.05, -np.ones(n)], 1).astype(np.float32)
    fill_rays(rh, org, np.tile(np.array([0, 0, 1], np.float32), (n, 1)))
    rh["time"] = (rng.randint(0, 8, n) / 8.0).astype(np.float32)
    return rh


@pytest.mark.parametrize("mode", [0, 1])
def test_motion_blur_intersection_filter(rtc, mode):
    dev, sc = _stack(rtc, mode)
    calls = []

    @rtc.FILTER_FUNC
    def flt(args):  # triangle g rejects rays whose x < 0.2 * (g + 1)
        ray, hit = _ray_fields(args)
        g = hit[6]
        calls.append((ray[0], g))
        assert hit[5] == 0 and abs(ray[8] - (g + 1.0 + ray[7])) < 1e-5  # ray.tfar = candidate distance = g + 1 + time
        if ray[0] < 0.2 * (g + 1):
            args.contents.valid[0] = 0

    for g in range(NT - 1):
        sc.set_filters(g, intersect=flt)
    sc.commit()
    n = 3000
    rh = _stack_rays(rtc, n)
    x, times = rh["org_x"].copy(), rh["time"].copy()
    sc.intersect1M(rh)
    want = np.array([next(g for g in range(NT) if g == NT - 1 or xi >= np.float32(0.2 * (g + 1))) for xi in x])
    assert np.array_equal(rh["geomID"], want.astype(np.uint32))
    assert np.allclose(rh["tfar"], want + 1.0 + times, atol=1e-5)
    assert (rh["primID"] == 0).all()
    per_ray = {}
    for xo, g in calls:
        per_ray.setdefault(xo, []).append(g)
    for xi, w in zip(x, want):
        assert per_ray[xi] == list(range(min(w, NT - 2) + 1))
    sc.release()
    dev.release()


@pytest.mark.parametrize("mode", [0, 1])
def test_motion_blur_occlusion_and_context_filters(rtc, mode):
    dev, sc = _stack(rtc, mode)

    @rtc.FILTER_FUNC
    def occ_flt(args):  # triangles 0..3 never occlude
        ray, hit = _ray_fields(args)
        assert abs(ray[8] - (hit[6] + 1.0 + ray[7])) < 1e-5
        if hit[6] < NT - 1:
            args.contents.valid[0] = 0

    for g in range(NT):
        sc.set_filters(g, occluded=occ_flt)
    sc.commit()
    n = 500
    rh = _stack_rays(rtc, n)
    occ = _occ_of(rtc, rh)
    occ2 = occ.copy()
    sc.occluded1M(occ)
    assert (occ["tfar"] == -np.inf).all()  # the last triangle occludes
    occ2["tfar"] = np.float32(NT - 0.5)    # ... but it is at NT + time, beyond tfar: nothing occludes
    sc.occluded1M(occ2)
    assert (occ2["tfar"] == np.float32(NT - 0.5)).all()

    # context filter: rejects every candidate with x < 0.5 on triangles 0, 1 -> those rays hit triangle 2
    @rtc.FILTER_FUNC
    def ctx_flt(args):
        ray, hit = _ray_fields(args)
        if hit[6] < 2 and ray[0] < 0.5:
            args.contents.valid[0] = 0

    ctx = rtc.make_context()
    ctx.filter = C.cast(ctx_flt, C.c_void_p)
    rh2 = _stack_rays(rtc, n, seed=4)
    x, times = rh2["org_x"].copy(), rh2["time"].copy()
    sc.intersect1M(rh2, ctx=ctx)
    g = np.where(x < 0.5, 2, 0)
    assert np.array_equal(rh2["geomID"], g.astype(np.uint32))
    assert np.allclose(rh2["tfar"], g + 1.0 + times, atol=1e-5)
    sc.release()
    dev.release()


# ---- 10. every entry path gives bit-identical hits --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_entry_paths_are_bit_identical(rtc, po, two_steps, mode):
    import torch
    steps, tris = two_steps
    m = 40000
    rays = _timed_rays(rtc, po, m, steps, [0.0], seed=21)
    rays["time"] = np.random.RandomState(8).rand(m).astype(np.float32) * 1.2 - 0.1  # mixed times, some outside [0, 1]
    dev, sc = _mb_scene(rtc, mode, steps, tris)
    # device-resident batch = the reference answer
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    sc.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    nhits = int((want["geomID"] != INVALID).sum())
    assert nhits > 1000
    # host, pipelined (>= 16 k rays)
    h = rtc.aligned_rayhits(m)
    h[:] = rays
    sc.intersect1M(h)
    assert h.tobytes() == want.tobytes()
    # host, small batches (<= 512 rays: zero-copy)
    s = rtc.aligned_rayhits(m)
    s[:] = rays
    for a in range(0, 4096, 500):
        sc.intersect1M(s[a:a + 500])
    assert s[:4096].tobytes() == want[:4096].tobytes()
    # instrumented twin
    c = rtc.aligned_rayhits(m)
    c[:] = rays
    cnt = sc.intersect1M_counted(c)
    assert c.tobytes() == want.tobytes()
    assert cnt["rays"] == m and cnt["hits"] == nhits and cnt["primTests"] > 0
    # multi-threaded rtcIntersect1 (call combiner)
    k = 2048
    g = rtc.aligned_rayhits(k)
    g[:] = rays[:k]
    errors = []

    def worker(i0):
        try:
            for i in range(i0, k, 16):
                sc.intersect1(g[i:i + 1])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(16)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[0]
    assert g.tobytes() == want[:k].tobytes()
    sc.release()
    dev.release()
    # service=1: there is no resident service kernel for the motion-blur accel, its small calls go through the combiner
    dev, sc = _mb_scene(rtc, mode, steps, tris, "service=1")
    sv = rtc.aligned_rayhits(k)
    sv[:] = rays[:k]
    for i in range(0, k, 32):
        sc.intersect1M(sv[i:i + 32])
    assert sv.tobytes() == want[:k].tobytes()
    sc.release()
    dev.release()


# ---- 11. packets ------------------------------------------------------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_packets_carry_a_time_per_lane(rtc, po, two_steps, mode):
    steps, tris = two_steps
    dev, sc = _mb_scene(rtc, mode, steps, tris)
    L = sc.lib
    n = 2048
    src = _timed_rays(rtc, po, n, steps, [0.0], seed=5)
    src["time"] = np.random.RandomState(6).rand(n).astype(np.float32)
    want = src.copy()
    sc.intersect1M(want)
    assert int((want["geomID"] != INVALID).sum()) > 100
    wocc = _occ_of(rtc, src)
    sc.occluded1M(wocc)
    ctx = rtc.make_context()
    words = slice(0, 20)
    for W in (4, 8, 16):
        fn_i, fn_o = getattr(L, f"rtcIntersect{W}"), getattr(L, f"rtcOccluded{W}")
        for fn in (fn_i, fn_o):
            fn.restype = None
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        valid = np.full(W, -1, np.int32)
        for p in range(0, 256, W):
            pk = _soa(src[p:p + W], W, True)
            fn_i(valid.ctypes.data, sc.handle, C.addressof(ctx), pk.ctypes.data)
            dev.check("packet")
            assert np.array_equal(pk[words], _soa(want[p:p + W], W, True)[words])
            po_ = _soa(src[p:p + W], W, False)
            fn_o(valid.ctypes.data, sc.handle, C.addressof(ctx), po_.ctypes.data)
            dev.check("packet occluded")
            assert np.array_equal(po_[8], wocc["tfar"][p:p + W].view(np.uint32))
    # stream of packets, and the SoA pointer stream
    N, M = 8, 16
    buf = np.zeros((M, 20 * N), np.uint32)
    for m in range(M):
        buf[m] = _soa(src[1024 + m * N: 1024 + (m + 1) * N], N, True).ravel()
    L.rtcIntersectNM.restype = None
    L.rtcIntersectNM.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_size_t]
    L.rtcIntersectNM(sc.handle, C.addressof(ctx), buf.ctypes.data, N, M, 20 * N * 4)
    dev.check("rtcIntersectNM")
    for m in range(M):
        assert np.array_equal(buf[m].reshape(20, N), _soa(want[1024 + m * N: 1024 + (m + 1) * N], N, True))
    k = 300
    cols = {f: np.ascontiguousarray(src[f][1500:1500 + k]) for f in RAYF + HITF[:-1]}
    inst = np.full(k, INVALID, np.uint32)

    class Np(C.Structure):
        _fields_ = [(f, C.c_void_p) for f in RAYF + HITF]

    a = Np(*[cols[f].ctypes.data for f in RAYF + HITF[:-1]], inst.ctypes.data)
    L.rtcIntersectNp.restype = None
    L.rtcIntersectNp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
    L.rtcIntersectNp(sc.handle, C.addressof(ctx), C.addressof(a), k)
    dev.check("rtcIntersectNp")
    w = want[1500:1500 + k]
    for f in ("tfar", "geomID", "primID", "u", "v", "Ng_x", "Ng_y", "Ng_z"):
        assert np.array_equal(cols[f].view(np.uint32), w[f].view(np.uint32)), f
    sc.release()
    dev.release()


# ---- 12. the C example ----------------------------------------------------------------------------------------------------------
def test_motion_blur_example_runs(tmp_path):
    exe = str(tmp_path / "motion_blur_min")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "motion_blur_min.c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "motion_blur_min: ok" in out.stdout
