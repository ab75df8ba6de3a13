"""Motion-blur quad meshes (time steps, ray.time) traced by the QuadMB leaves of trace_quad_mb.hip.

The oracle has no motion blur, so the parity tests make it exact by construction (as tests/test_gpu_motion_blur.py does for
triangles): every vertex coordinate of every time step is snapped to a multiple of 2^-10 below 64 and the ray times are multiples of
1 / (4 S), so ftime is 0, 1/4, 1/2 or 3/4 and every interpolated coordinate is a multiple of 2^-12 below 2^7 - exactly representable
in fp32 whatever form the lerp takes.  One static oracle scene per distinct time traces the rays of that time; for quads that scene is
the split oracle of tests/test_gpu_quads.py: po.TriangleScene on the A triangles (v0, v1, v3) of every quad, then the B triangles
(v2, v1, v3), with the B mapping (u = 1 - v_tri, v = 1 - u_tri, Ng negated) applied to its answers."""
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
HITF = ["Ng_x", "Ng_y", "Ng_z", "u", "v", "primID", "geomID", "instID"]
SCALE = 0.0625  # bomberman spans +-246: scaled so that every coordinate of every (moved) step stays below 64 before it is snapped
UNIT = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
Q1 = np.array([[0, 1, 2, 3]], np.uint32)
UP = np.array([0, 0, 1], np.float32)


def _device(rtc, mode, extra=""):
    # quad_accel_mb=default: mode 0 = robust scene (Pluecker, accel kind 12), mode 1 = non-robust scene (Moeller, kind 13)
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


def _at_time(steps, time, exact=True):
    """the mesh at `time` (getTimeSegment + lerp in float64; exact in fp32 for snapped steps and times k / (4 S))"""
    S = len(steps) - 1
    ts = np.float64(time) * S
    it = int(min(max(np.floor(ts), 0), S - 1))
    f = ts - it
    v = (1.0 - f) * steps[it].astype(np.float64) + f * steps[it + 1].astype(np.float64)
    assert not exact or np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v.astype(np.float32)


def _bomberman_quads(bomberman):
    v, fs, fi = bomberman
    assert (fs == 4).all()
    return v, fi.reshape(-1, 4).astype(np.uint32)


@pytest.fixture(scope="module")
def two_steps(bomberman):
    v, quads = _bomberman_quads(bomberman)
    assert len(quads) == 727
    s0 = _snap(v * SCALE)
    ext = s0.max(0) - s0.min(0)
    # step 1: rotated about y by 20 degrees and moved by 0.3 x extent along x
    s1 = _snap(_rot_y(s0, 20.0) + np.array([0.3 * ext[0], 0.0, 0.0]))
    return [s0, s1], quads


@pytest.fixture(scope="module")
def five_steps(bomberman):
    v, quads = _bomberman_quads(bomberman)
    s0 = _snap(v * SCALE)
    ext = s0.max(0) - s0.min(0)
    # a curved path: rotation and a parabola, so that the four segments differ
    return [_snap(_rot_y(s0, 12.0 * k) + ext * np.array([0.1 * k, 0.03 * k * k, -0.05 * k])) for k in range(5)], quads


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


def _split_oracle(po, verts, quads, mode):
    """TriangleScene on the split triangles: A of every quad, then B; geomID 0 = A, 1 = B; primID = quad index"""
    tris = np.concatenate([quads[:, [0, 1, 3]], quads[:, [2, 1, 3]]]).astype(np.uint32)
    gids = np.concatenate([np.zeros(len(quads)), np.ones(len(quads))]).astype(np.uint32)
    pids = np.concatenate([np.arange(len(quads)), np.arange(len(quads))]).astype(np.uint32)
    return po.TriangleScene(verts, tris, mode, gids, pids)


def _map_b(want, geom_id=0):
    """apply the B mapping to oracle records whose hit came from a B triangle (geomID 1); returns the B mask"""
    isb = want["geomID"] == 1
    u, v = want["u"][isb].copy(), want["v"][isb].copy()
    want["u"][isb] = np.float32(1) - v
    want["v"][isb] = np.float32(1) - u
    for f in ("Ng_x", "Ng_y", "Ng_z"):
        want[f][isb] = -want[f][isb]
    hit = want["geomID"] != INVALID
    want["geomID"][hit] = geom_id
    return isb


def _oracle_per_time(rtc, po, steps, quads, rays, mode):
    """the rays traced by one static split oracle scene per distinct time, B mapping applied; returns (records, B mask)"""
    want = rays.copy()
    isb = np.zeros(len(rays), bool)
    for t in np.unique(rays["time"]):
        sel = np.nonzero(rays["time"] == t)[0]
        sub = rtc.aligned_rayhits(len(sel))
        sub[:] = rays[sel]
        orc = _split_oracle(po, _at_time(steps, t), quads, mode)
        orc.intersect1M(sub, nthreads=16)
        orc.free()
        isb[sel] = _map_b(sub)
        want[sel] = sub
    return want, isb


def _parity(got, want, isb, rays, times, mode, what):
    """compare_hits(..., 1e-4) with the two allowances of test_bomberman_quads_1m_parity; returns hits per time"""
    hit = want["geomID"] != INVALID
    if mode == 1:
        # Moeller B lanes: the oracle's u_tri / v_tri come after the division; 1 - v_tri vs (absDen - V) / absDen differ by ulps of 1
        b = isb & (got["geomID"] != INVALID)
        for f in ("u", "v"):
            assert np.all(np.abs(got[f][b].astype(np.float64) - want[f][b]) <= 4e-7 + 1e-4 * np.abs(want[f][b]))
            want[f][b] = got[f][b]
    # rays within 1e-4 of the v1-v3 diagonal hit A and B within ulps and the oracle's rcp may rank them the other way; on a non-planar
    # quad the two normals differ: the normal the kernel reports is taken (ids, t, u, v are still compared)
    diag = hit & (np.abs(want["u"].astype(np.float64) + want["v"] - 1.0) < 1e-4)
    for f in ("Ng_x", "Ng_y", "Ng_z"):
        want[f][diag] = got[f][diag]
    per_time = [int((hit & (rays["time"] == np.float32(t))).sum()) for t in times]
    ndiag = [int((diag & (rays["time"] == np.float32(t))).sum()) for t in times]
    print(f"{what}: hits per time {per_time}, diagonal rays per time {ndiag}, {int((isb & hit).sum())} hits on B triangles")
    assert int(diag.sum()) < int(hit.sum()) // 100, int(diag.sum())
    compare_hits(got, want, 1e-4, what)
    return per_time


def _occ_of(rtc, rays):
    occ = rtc.aligned_rays(len(rays))
    for f in occ.dtype.names:
        occ[f] = rays[f]
    return occ


def _mb_scene(rtc, mode, steps, quads, extra=""):
    dev, flags = _device(rtc, mode, extra)
    sc = rtc.Scene(dev, flags)
    sc.add_quads_mb(steps, quads)
    sc.commit()
    assert sc.stats()["accelKind"] == (12 if mode == 0 else 13)
    return dev, sc


def _static_quads(rtc, mode, verts, quads):
    dev, flags = _device(rtc, mode)
    sc = rtc.Scene(dev, flags)
    sc.add_quads(verts, quads)
    sc.commit()
    return dev, sc


# ---- 1. closed form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_translating_quad_closed_form(rtc, mode):
    dev, sc = _mb_scene(rtc, mode, [UNIT, UNIT + UP], Q1)
    n = 256
    rng = np.random.RandomState(7)
    org = np.stack([rng.rand(n) * 0.9 + 0.05, rng.rand(n) * 0.9 + 0.05, -np.ones(n)], 1).astype(np.float32)
    d = np.tile(UP, (n, 1))
    times = rng.rand(n).astype(np.float32)  # random, not dyadic
    times[0], times[1] = -0.25, 1.5         # outside [0, 1]: the segment is extrapolated
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, d)
    rh["time"] = times
    sc.intersect1M(rh)
    assert (rh["geomID"] == 0).all() and (rh["primID"] == 0).all()
    assert np.all(np.abs(rh["tfar"].astype(np.float64) - (1.0 + times.astype(np.float64))) <= 1e-5)
    # u, v do not depend on z for these rays: the static quad's answer
    dev0, st = _static_quads(rtc, mode, UNIT, Q1)
    ref = rtc.aligned_rayhits(n)
    fill_rays(ref, org, d)
    st.intersect1M(ref)
    assert (ref["geomID"] == 0).all()
    assert np.all(np.abs(rh["u"] - ref["u"]) <= 2e-6) and np.all(np.abs(rh["v"] - ref["v"]) <= 2e-6)
    st.release()
    dev0.release()
    # both halves are hit: A reports u + v <= 1 (the x + y < 1 side of the unit quad), B the mapped u + v >= 1
    side_b = rh["u"].astype(np.float64) + rh["v"] > 1.0
    assert np.array_equal(side_b, org[:, 0].astype(np.float64) + org[:, 1] > 1.0)
    assert 32 < int(side_b.sum()) < n - 32
    occ = _occ_of(rtc, rh)
    occ["tfar"] = np.inf
    occ["tfar"][5], occ["time"][5] = 0.5, 0.9  # the quad is at distance 1.9 at that time
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


# ---- 2. block and tie rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_coincident_quads_follow_the_static_block_rule(rtc, mode):
    quad = np.array([[0, 0, 0], [1, 0, 0.5], [1, 1, 0.125], [0, 1, 0.25]], np.float32)  # non-planar
    v0 = np.tile(quad, (9, 1))
    idx = np.arange(36, dtype=np.uint32).reshape(9, 4)
    steps = [v0, (v0 + np.array([0.5, 0.25, 1.0], np.float32)).astype(np.float32)]
    dev, sc = _mb_scene(rtc, mode, steps, idx)
    assert sc.accel_root() & 0x80000000 and sc.stats()["primCount"] == 9  # one leaf, blocks of 4 + 4 + 1
    n = 64
    rng = np.random.RandomState(3)
    d = np.tile(UP, (n, 1))
    for time in (0.0, 0.25, 0.5, 1.0):
        shift = np.float32(time) * np.array([0.5, 0.25, 0.0], np.float32)
        org = (np.stack([rng.rand(n) * 0.9 + 0.05, rng.rand(n) * 0.9 + 0.05, -np.ones(n)], 1) + shift).astype(np.float32)
        rh = rtc.aligned_rayhits(n)
        fill_rays(rh, org, d)
        rh["time"] = time
        sc.intersect1M(rh)
        dev0, st = _static_quads(rtc, mode, _at_time(steps, time), idx)
        ref = rtc.aligned_rayhits(n)
        fill_rays(ref, org, d)
        ref["time"] = time
        st.intersect1M(ref)
        assert (ref["geomID"] == 0).all()
        assert np.array_equal(rh["primID"], ref["primID"]) and np.array_equal(rh["geomID"], ref["geomID"])
        assert np.allclose(rh["tfar"], ref["tfar"], rtol=1e-6)
        st.release()
        dev0.release()
        # the same rays as eight 8-ray calls (sparsely filled waves: child-parallel form) give the same bytes
        small = rtc.aligned_rayhits(n)
        fill_rays(small, org, d)
        small["time"] = time
        for a in range(0, n, 8):
            sc.intersect1M(small[a:a + 8])
        assert small.tobytes() == rh.tobytes()
    sc.release()
    dev.release()


# ---- 3. / 4. parity against the per-time split oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_two_step_parity(rtc, po, two_steps, mode):
    steps, quads = two_steps
    dev, sc = _mb_scene(rtc, mode, steps, quads)
    assert sc.stats()["primCount"] == len(quads)
    times = [0.0, 0.25, 0.5, 0.75, 1.0]
    rays = _timed_rays(rtc, po, 200000, steps, times, seed=31)
    want, isb = _oracle_per_time(rtc, po, steps, quads, rays, mode)
    got = rays.copy()
    sc.intersect1M(got)
    per_time = _parity(got, want, isb, rays, times, mode, f"two-step bomberman quads {MODES[mode]}")
    assert min(per_time) >= 5000, per_time
    occ = _occ_of(rtc, rays)
    sc.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, want["geomID"] != INVALID)
    assert np.array_equal(occ["tfar"][occ["tfar"] != -np.inf], rays["tfar"][occ["tfar"] != -np.inf])
    sc.release()
    dev.release()


@pytest.mark.parametrize("mode", [0, 1])
def test_five_step_parity(rtc, po, five_steps, mode):
    steps, quads = five_steps
    dev, sc = _mb_scene(rtc, mode, steps, quads)
    assert sc.stats()["primCount"] == 4 * len(quads)
    times = [k / 16.0 for k in range(17)]  # k = 4, 8, 12: a step time, floor() puts it into the segment that STARTS there
    # seed 31 as in the two-step test: the inputs for which the oracle alone gives 475 hits at the least populated time.  (With seed
    # 32, the seed of the triangle test, ray 72434 passes within 5e-5 of the edge that quads 139 and 143 share; both report the
    # bit-identical t = 11.920346 and the hit is whichever the traversal meets last - the BVH over the segment records and the
    # oracle's BVH over the static triangles at that time order them differently.  Such a tie has no reference answer.)
    rays = _timed_rays(rtc, po, 100000, steps, times, seed=31)
    want, isb = _oracle_per_time(rtc, po, steps, quads, rays, mode)
    got = rays.copy()
    sc.intersect1M(got)
    per_time = _parity(got, want, isb, rays, times, mode, f"five-step bomberman quads {MODES[mode]}")
    assert min(per_time) >= 100, per_time  # every time, the step times 4/16, 8/16, 12/16 among them, is exercised (oracle: 475)
    occ = _occ_of(rtc, rays)
    sc.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, want["geomID"] != INVALID)
    sc.release()
    dev.release()


# ---- 5. mixed scene ---------------------------------------------------------------------------------------------------------
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
    ext = hi - lo
    tv, tt = _random_quads(300, 5, lo, hi)
    tris = tt[:, :3].copy()
    mv, mt = _random_quads(300, 7, lo, hi)
    mtris = mt[:, :3].copy()
    msteps = [mv, (mv + 0.2 * ext).astype(np.float32), (mv + np.array([0.2, 0.5, 0.1], np.float32) * ext).astype(np.float32)]
    qv, qq = _random_quads(400, 6, lo, hi)
    # two moving quad meshes over the same space, one segment and four: records of different S share leaves
    av, aq = _random_quads(300, 8, lo, hi)
    asteps = [av, (av + np.array([0.1, 0.2, -0.1], np.float32) * ext).astype(np.float32)]
    bv, bq = _random_quads(300, 9, lo, hi)
    bsteps = [(bv + np.float32(k) * np.array([0.05, 0.1, 0.02], np.float32) * ext + np.float32(0.01 * k * k) * ext).astype(np.float32) for k in range(5)]

    def scene(parts):
        dev, flags = _device(rtc, mode)
        sc = rtc.Scene(dev, flags)
        if "t" in parts:
            sc.add_triangles(tv, tris, geom_id=0)
        if "m" in parts:
            sc.add_triangles_mb(msteps, mtris, geom_id=1)
        if "q" in parts:
            sc.add_quads(qv, qq, geom_id=2)
        if "Q" in parts:
            sc.add_quads_mb(asteps, aq, geom_id=3)
            sc.add_quads_mb(bsteps, bq, geom_id=4)
        if "s" in parts:
            sc.add_subdiv(verts, fs, fi, geom_id=5)
        sc.commit()
        return dev, sc

    m = 100000
    rays = po.make_random_rays(m, lo, hi + 0.3 * ext, seed=9)
    rays["time"] = np.random.RandomState(4).rand(m).astype(np.float32)
    dev, sc = scene("tmqQs")
    got = rtc.aligned_rayhits(m)
    got[:] = rays
    sc.intersect1M(got)
    want = rtc.aligned_rayhits(m)
    want[:] = rays
    for p in "tmqQs":  # Scene::commit order (scene.cpp:650-654), AccelN traces them one after another
        d1, s1 = scene(p)
        if p == "Q":
            assert s1.stats()["accelKind"] == (12 if mode == 0 else 13) and s1.stats()["primCount"] == len(aq) + 4 * len(bq)
        s1.intersect1M(want)
        s1.release()
        d1.release()
    assert got.tobytes() == want.tobytes()
    counts = [int((got["geomID"] == g).sum()) for g in range(6)]
    print(f"mixed scene ({MODES[mode]}): hits per geometry {counts}")
    assert min(counts) > 100, counts
    sc.release()
    dev.release()


# ---- 6. coincidence -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_coincident_static_and_resting_moving_quad_return_the_moving_mesh(rtc, mode):
    dev, flags = _device(rtc, mode)
    sc = rtc.Scene(dev, flags)
    assert sc.add_quads(UNIT, Q1) == 0
    assert sc.add_quads_mb([UNIT, UNIT], Q1) == 1
    sc.commit()
    n = 64
    rng = np.random.RandomState(2)
    org = np.stack([rng.rand(n) * 0.9 + 0.05, rng.rand(n) * 0.9 + 0.05, -np.ones(n)], 1).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(UP, (n, 1)))
    rh["time"] = rng.rand(n).astype(np.float32)
    sc.intersect1M(rh)
    assert (rh["geomID"] == 1).all()  # traced after the static quads, the depth test T <= absDen * tfar accepts the equal t
    assert np.allclose(rh["tfar"], 1.0)
    sc.release()
    dev.release()


# ---- 7. filters ---------------------------------------------------------------------------------------------------------------
NQ = 5


def _ray_fields(args):
    ray = C.cast(args.contents.ray, C.POINTER(C.c_float * 12)).contents
    hit = C.cast(args.contents.hit, C.POINTER(C.c_uint * 8)).contents
    return ray, hit


def _stack(rtc, mode):
    """quad g moves from z = g to z = g + 1: a ray along +z from z = -1 at `time` meets it at g + 1 + time"""
    dev, flags = _device(rtc, mode)
    sc = rtc.Scene(dev, flags)
    for z in range(NQ):
        v = (UNIT + np.float32(z) * UP).astype(np.float32)
        assert sc.add_quads_mb([v, v + UP], Q1) == z
    return dev, sc


def _stack_rays(rtc, n, seed=1):
    rng = np.random.RandomState(seed)
    rh = rtc.aligned_rayhits(n)
    org = np.stack([rng.rand(n) * 0.9 + 0.05, rng.rand(n) * 0.9 + 0.05, -np.ones(n)], 1).astype(np.float32)
    fill_rays(rh, org, np.tile(UP, (n, 1)))
    rh["time"] = (rng.randint(0, 8, n) / 8.0).astype(np.float32)
    return rh


@pytest.mark.parametrize("mode", [0, 1])
def test_motion_blur_quad_intersection_filter(rtc, mode):
    dev, sc = _stack(rtc, mode)
    calls = []

    @rtc.FILTER_FUNC
    def flt(args):  # quad g rejects rays whose x < 0.2 * (g + 1)
        ray, hit = _ray_fields(args)
        g = hit[6]
        calls.append((ray[0], ray[1], g))
        assert hit[5] == 0 and abs(ray[8] - (g + 1.0 + ray[7])) < 1e-5  # ray.tfar = candidate distance = g + 1 + time
        if ray[0] < 0.2 * (g + 1):
            args.contents.valid[0] = 0

    for g in range(NQ - 1):
        sc.set_filters(g, intersect=flt)
    sc.commit()
    n = 3000
    rh = _stack_rays(rtc, n)
    x, y, times = rh["org_x"].copy(), rh["org_y"].copy(), rh["time"].copy()
    sc.intersect1M(rh)
    want = np.array([next(g for g in range(NQ) if g == NQ - 1 or xi >= np.float32(0.2 * (g + 1))) for xi in x])
    assert np.array_equal(rh["geomID"], want.astype(np.uint32))
    assert np.allclose(rh["tfar"], want + 1.0 + times, atol=1e-5)
    assert (rh["primID"] == 0).all()
    # every quad in front of the accepted one is offered once, front to back, then the accepted one (the last quad has no filter)
    per_ray = {}
    for xo, yo, g in calls:
        per_ray.setdefault((xo, yo), []).append(g)
    for xi, yi, w in zip(x, y, want):
        assert per_ray[(xi, yi)] == list(range(min(w, NQ - 2) + 1))
    sc.release()
    dev.release()


@pytest.mark.parametrize("mode", [0, 1])
def test_motion_blur_quad_occlusion_and_context_filters(rtc, mode):
    dev, sc = _stack(rtc, mode)

    @rtc.FILTER_FUNC
    def occ_flt(args):  # quads 0..3 never occlude
        ray, hit = _ray_fields(args)
        assert abs(ray[8] - (hit[6] + 1.0 + ray[7])) < 1e-5
        if hit[6] < NQ - 1:
            args.contents.valid[0] = 0

    for g in range(NQ):
        sc.set_filters(g, occluded=occ_flt)
    sc.commit()
    n = 500
    rh = _stack_rays(rtc, n)
    occ = _occ_of(rtc, rh)
    occ2 = occ.copy()
    sc.occluded1M(occ)
    assert (occ["tfar"] == -np.inf).all()  # the last quad occludes
    occ2["tfar"] = np.float32(NQ - 0.5)    # ... but it is at NQ + time, beyond tfar: nothing occludes
    sc.occluded1M(occ2)
    assert (occ2["tfar"] == np.float32(NQ - 0.5)).all()

    # context filter: rejects every candidate with x < 0.5 on quads 0, 1 -> those rays hit quad 2
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


# ---- 8. every entry path gives bit-identical hits -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_entry_paths_are_bit_identical(rtc, po, two_steps, mode):
    import torch
    steps, quads = two_steps
    m = 40000
    rays = _timed_rays(rtc, po, m, steps, [0.0], seed=21)
    rays["time"] = np.random.RandomState(8).rand(m).astype(np.float32) * 1.2 - 0.1  # mixed times, some outside [0, 1]
    dev, sc = _mb_scene(rtc, mode, steps, quads)
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
    # service=1: there is no resident service kernel for the motion-blur accels, their small calls go through the combiner
    dev, sc = _mb_scene(rtc, mode, steps, quads, "service=1")
    sv = rtc.aligned_rayhits(k)
    sv[:] = rays[:k]
    for i in range(0, k, 32):
        sc.intersect1M(sv[i:i + 32])
    assert sv.tobytes() == want[:k].tobytes()
    sc.release()
    dev.release()


# ---- 9. packets ---------------------------------------------------------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_packets_carry_a_time_per_lane(rtc, po, two_steps, mode):
    steps, quads = two_steps
    dev, sc = _mb_scene(rtc, mode, steps, quads)
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


# ---- 10. the C example ----------------------------------------------------------------------------------------------------------
def test_quad_motion_blur_example_runs(tmp_path):
    exe = str(tmp_path / "quad_motion_blur_min")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "quad_motion_blur_min.c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "quad_motion_blur_min: ok" in out.stdout
