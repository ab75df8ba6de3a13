"""Quad meshes (RTC_GEOMETRY_TYPE_QUAD) traced by the Quad4v leaves of trace_quad.hip.  The reference tests 4 quads as one 8-wide block of
triangles (AVX form): A = (v0, v1, v3) in lanes 0-3, B = (v2, v1, v3) in lanes 4-7, one select_min (lowest lane wins ties); hits on B
report Ng negated and u / v mapped (Pluecker: u = 1 - v_tri, v = 1 - u_tri; Moeller: U' = absDen - V, V' = absDen - U before the division).
Expected answers come from the oracle's triangle entry points (orc_*_block, TriangleScene) plus that mapping."""
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
QUAD_DT = np.dtype([("v0", "<f4", 3), ("geomID", "<u4"), ("v1", "<f4", 3), ("primID", "<u4"), ("v2", "<f4", 3), ("pad0", "<u4"),
                    ("v3", "<f4", 3), ("pad1", "<u4")])
MODES = {0: "pluecker", 1: "moeller"}
ROBUST = 4  # RTC_SCENE_FLAG_ROBUST


def _device(rtc, mode, extra=""):
    # mode 0: quad_accel=default on a robust scene (Pluecker), mode 1: the explicit quad4v accel (Moeller)
    cfg = "" if mode == 0 else "quad_accel=bvh8.quad4v"
    if extra:
        cfg = (cfg + "," + extra) if cfg else extra
    return rtc.Device(cfg), (ROBUST if mode == 0 else 0)


def _bomberman_quads(bomberman):
    v, fs, fi = bomberman
    assert (fs == 4).all()
    return v, fi.reshape(-1, 4).astype(np.uint32)


def _split_oracle(po, verts, quads, mode):
    """TriangleScene on the split triangles: A of every quad, then B; geomID 0 = A, 1 = B; primID = quad index"""
    a = quads[:, [0, 1, 3]]
    b = quads[:, [2, 1, 3]]
    tris = np.concatenate([a, b]).astype(np.uint32)
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


# ---- 1. known answers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_unit_quad_known_answers(rtc, mode):
    dev, flags = _device(rtc, mode)
    sc = rtc.Scene(dev, flags)
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    assert sc.add_quads(v, np.array([[0, 1, 2, 3]], np.uint32)) == 0
    sc.commit()
    rng = np.random.RandomState(3)
    n = 512
    px = (rng.rand(n) * 0.96 + 0.02).astype(np.float32)
    py = (rng.rand(n) * 0.96 + 0.02).astype(np.float32)
    org = np.stack([px, py, -np.ones(n, np.float32)], 1).astype(np.float32)
    d = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, d)
    sc.intersect1M(rh)
    assert (rh["geomID"] == 0).all() and (rh["primID"] == 0).all()
    assert np.allclose(rh["tfar"], 1.0, atol=1e-6)
    # quad parametrisation: A (u+v <= 1 side, x+y < 1 here) has u = x, v = y; B maps back to the same (x, y)
    assert np.allclose(rh["u"], px, atol=2e-6) and np.allclose(rh["v"], py, atol=2e-6)
    # Ng of A = cross(v1-v0, v3-v0) direction: -z for (e1 = v0-v1, e2 = v3-v0) -> cross(e2, e1) = +z * ... ; B negated = same direction
    ng = np.stack([rh["Ng_x"], rh["Ng_y"], rh["Ng_z"]], 1)
    assert np.allclose(ng[:, :2], 0, atol=1e-6)
    assert (np.sign(ng[:, 2]) == np.sign(ng[0, 2])).all() and ng[0, 2] != 0
    # single-ray call gives the same record
    one = rtc.aligned_rayhits(1)
    fill_rays(one, org[:1], d[:1])
    sc.intersect1(one)
    assert one.tobytes() == rh[:1].tobytes()
    # occluded: tfar = -inf for every hit, untouched for misses
    occ = rtc.aligned_rays(n + 1)
    org2 = np.concatenate([org, np.array([[2, 2, -1]], np.float32)])
    fill_rays(occ, org2, np.concatenate([d, d[:1]]))
    sc.occluded1M(occ)
    assert (occ["tfar"][:n] == -np.inf).all() and occ["tfar"][n] == np.inf
    o1 = rtc.aligned_rays(1)
    fill_rays(o1, org[:1], d[:1])
    sc.occluded1(o1)
    assert o1["tfar"][0] == -np.inf
    sc.release()
    dev.release()


# ---- 2. block semantics -----------------------------------------------------------------------------------------------
def _soa(pts):
    return np.ascontiguousarray(np.asarray(pts, np.float32).T.reshape(-1))  # x[4], y[4], z[4]


@pytest.mark.parametrize("mode", [0, 1])
def test_block_semantics_against_the_oracle_blocks(rtc, po, mode):
    L = po.lib()
    blockfn = L.orc_pluecker_block if mode == 0 else L.orc_moeller_block
    rng = np.random.RandomState(11 + mode)
    checked = bsides = ties = 0
    for trial in range(6):
        c = (rng.rand(4, 1, 3) * 0.6).astype(np.float32)
        v = (c + (rng.rand(4, 4, 3).astype(np.float32) - 0.5)).astype(np.float32).reshape(-1, 3)
        q = np.arange(16, dtype=np.uint32).reshape(4, 4)
        dev, flags = _device(rtc, mode)
        sc = rtc.Scene(dev, flags)
        sc.add_quads(v, q)
        sc.commit()
        rec = sc.accel_data(2).view(QUAD_DT)
        assert len(rec) == 4 and sc.accel_root() & 0x80000000  # one leaf = one block of 4 quads, in record order
        v0, v1, v2, v3 = (_soa(rec[f"v{k}"]) for k in range(4))
        # targets: random points of random quads, and points on each quad's v1-v3 diagonal (A must win the tie)
        tg = []
        for k in range(4):
            p = [rec[f"v{j}"][k] for j in range(4)]
            for s in np.linspace(0.1, 0.9, 9, dtype=np.float32):
                tg.append(p[1] + s * (p[3] - p[1]))
            for _ in range(40):
                a, b = rng.rand(2)
                tg.append((1 - a) * ((1 - b) * p[0] + b * p[1]) + a * ((1 - b) * p[3] + b * p[2]))
        tg = np.asarray(tg, np.float32)
        org = (tg + rng.randn(len(tg), 3).astype(np.float32) * 2).astype(np.float32)
        d = (tg - org).astype(np.float32)
        rh = rtc.aligned_rayhits(len(tg))
        fill_rays(rh, org, d)
        sc.intersect1M(rh)
        out = np.zeros(6, np.float32)
        for i in range(len(tg)):
            o, dd = np.ascontiguousarray(org[i]), np.ascontiguousarray(d[i])
            la = blockfn(v0.ctypes.data, v1.ctypes.data, v3.ctypes.data, o.ctypes.data, dd.ctypes.data, 0.0, np.inf, out.ctypes.data)
            ra = out.copy()
            lb = blockfn(v2.ctypes.data, v1.ctypes.data, v3.ctypes.data, o.ctypes.data, dd.ctypes.data, 0.0, np.inf, out.ctypes.data)
            rb = out.copy()
            if la < 0 and lb < 0:
                assert rh["geomID"][i] == INVALID
                continue
            useb = la < 0 or (lb >= 0 and rb[0] < ra[0])  # 8-lane select_min: lanes 0-3 (A) win ties against lanes 4-7 (B)
            # the oracle's rcp is rcpps + Newton (ulps off a division): where A and B are hit within a few ulps (rays through the
            # v1-v3 diagonal of a non-planar quad) the two may rank them differently - then either candidate is accepted
            near = la >= 0 and lb >= 0 and abs(float(ra[0]) - float(rb[0])) <= 1e-6 * abs(float(ra[0]))
            got_ng = np.array([rh["Ng_x"][i], rh["Ng_y"][i], rh["Ng_z"][i]], np.float64)
            t, u, vv = float(rh["tfar"][i]), float(rh["u"][i]), float(rh["v"][i])

            def matches(b):
                lane = (lb + 4) if b else la
                r = rb if b else ra
                if not (rh["geomID"][i] == 0 and rh["primID"][i] == rec["primID"][lane & 3]):
                    return False
                if abs(t - r[0]) > 1e-4 * abs(r[0]) + 1e-30:
                    return False
                if b:
                    eu, ev = np.float32(1) - r[2], np.float32(1) - r[1]
                    tol = 4e-7 if mode == 1 else 0.0  # Moeller maps before the division: a few ulps of 1 apart
                    ng = -r[3:6]
                else:
                    eu, ev, tol, ng = r[1], r[2], 0.0, r[3:6]
                if abs(u - eu) > max(tol, 1e-4 * max(abs(eu), 1e-3)) or abs(vv - ev) > max(tol, 1e-4 * max(abs(ev), 1e-3)):
                    return False
                return bool(np.all(np.abs(got_ng - ng) <= 1e-4 * (np.linalg.norm(ng) + 1e-30)))

            if near:
                assert matches(False) or matches(True), (trial, i)
                ties += 1
            else:
                assert matches(useb), (trial, i, useb, la, lb)
                bsides += int(useb)
            checked += 1
        sc.release()
        dev.release()
    assert checked > 500 and bsides > 50, (checked, bsides, ties)


# ---- 3. bomberman as 727 quads ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_bomberman_quads_1m_parity(rtc, po, bomberman, mode):
    verts, quads = _bomberman_quads(bomberman)
    assert len(quads) == 727
    dev, flags = _device(rtc, mode)
    sc = rtc.Scene(dev, flags)
    sc.add_quads(verts, quads)
    sc.commit()
    assert sc.stats()["accelKind"] == (8 if mode == 0 else 9)
    lo, hi = verts.min(0), verts.max(0)
    m = 1 << 20
    rays = po.make_random_rays(m, lo, hi, seed=0)
    got = rtc.aligned_rayhits(m)
    got[:] = rays
    want = got.copy()
    orc = _split_oracle(po, verts, quads, mode)
    orc.intersect1M(want, nthreads=16)
    isb = _map_b(want)
    sc.intersect1M(got)
    hits = int((want["geomID"] != INVALID).sum())
    print(f"bomberman quads ({MODES[mode]}): {hits} hits of {m} rays, {int(isb.sum())} on B triangles")
    if mode == 1:
        # Moeller B lanes: the oracle's u_tri / v_tri come after the division; 1 - v_tri vs (absDen - V) / absDen differ by ulps of 1
        for f in ("u", "v"):
            assert np.all(np.abs(got[f][isb].astype(np.float64) - want[f][isb]) <= 4e-7 + 1e-4 * np.abs(want[f][isb]))
            want[f][isb] = got[f][isb]
    # rays through a quad's v1-v3 diagonal hit A and B within ulps; the oracle's rcp (rcpps + Newton) may rank them the other way, and
    # on a non-planar quad the two normals differ: there the normal the kernel reports is taken (ids, t, u, v are still compared)
    hit = want["geomID"] != INVALID
    diag = hit & (np.abs(want["u"].astype(np.float64) + want["v"] - 1.0) < 1e-4)
    for f in ("Ng_x", "Ng_y", "Ng_z"):
        want[f][diag] = got[f][diag]
    assert int(diag.sum()) < hits // 100, int(diag.sum())
    compare_hits(got, want, 1e-4, f"bomberman quads {MODES[mode]}")
    occ = rtc.aligned_rays(m)
    for f in occ.dtype.names:
        occ[f] = rays[f]
    sc.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, want["geomID"] != INVALID)
    orc.free()
    sc.release()
    dev.release()


# ---- 4. mixed scenes ----------------------------------------------------------------------------------------------------
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
    qv, qq = _random_quads(400, 6, lo, hi)
    cfg = ("tri_accel=bvh8.triangle4v" if mode == 0 else "tri_accel=bvh8.triangle4,quad_accel=bvh8.quad4v")

    def scene(parts):
        dev = rtc.Device(cfg)
        sc = rtc.Scene(dev, ROBUST if mode == 0 else 0)
        if "t" in parts:
            sc.add_triangles(tv, tris, geom_id=0)
        if "q" in parts:
            sc.add_quads(qv, qq, geom_id=1)
        if "s" in parts:
            sc.add_subdiv(verts, fs, fi, geom_id=2)
        sc.commit()
        return dev, sc

    m = 200000
    rays = po.make_random_rays(m, lo, hi, seed=9)
    dev, sc = scene("tqs")
    got = rtc.aligned_rayhits(m)
    got[:] = rays
    sc.intersect1M(got)
    want = rtc.aligned_rayhits(m)
    want[:] = rays
    for p in "tqs":  # Scene::commit order (scene.cpp:650-654), AccelN traces them one after another
        d1, s1 = scene(p)
        s1.intersect1M(want)
        s1.release()
        d1.release()
    assert got.tobytes() == want.tobytes()
    counts = [int((got["geomID"] == g).sum()) for g in range(3)]
    assert min(counts) > 100, counts
    sc.release()
    dev.release()


@pytest.mark.parametrize("mode", [0, 1])
def test_coincident_triangle_and_quad_return_the_quad(rtc, mode):
    dev, flags = _device(rtc, mode, "tri_accel=bvh8.triangle4v" if mode == 0 else "tri_accel=bvh8.triangle4")
    sc = rtc.Scene(dev, flags)
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    sc.add_triangles(v, np.array([[0, 1, 3]], np.uint32))  # = triangle A of the quad
    sc.add_quads(v, np.array([[0, 1, 2, 3]], np.uint32))
    sc.commit()
    n = 64
    rng = np.random.RandomState(2)
    org = np.stack([rng.rand(n) * 0.4 + 0.05, rng.rand(n) * 0.4 + 0.05, -np.ones(n)], 1).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(np.array([0, 0, 1], np.float32), (n, 1)))
    sc.intersect1M(rh)
    assert (rh["geomID"] == 1).all()  # traced after the triangles, depth test T <= absDen * tfar accepts the equal t
    assert np.allclose(rh["tfar"], 1.0)
    sc.release()
    dev.release()


# ---- 5. filters ---------------------------------------------------------------------------------------------------------
NQ = 5


def _ray_fields(args):
    ray = C.cast(args.contents.ray, C.POINTER(C.c_float * 12)).contents
    hit = C.cast(args.contents.hit, C.POINTER(C.c_uint * 8)).contents
    return ray, hit


def _stack(rtc, mode):
    dev, flags = _device(rtc, mode)
    sc = rtc.Scene(dev, flags)
    for z in range(NQ):
        v = np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]], np.float32)
        assert sc.add_quads(v, np.array([[0, 1, 2, 3]], np.uint32)) == z
    return dev, sc


def _rays(rtc, n, seed=1):
    rng = np.random.RandomState(seed)
    rh = rtc.aligned_rayhits(n)
    org = np.stack([rng.rand(n) * 0.9 + 0.05, rng.rand(n) * 0.9 + 0.05, -np.ones(n)], 1).astype(np.float32)
    fill_rays(rh, org, np.tile(np.array([0, 0, 1], np.float32), (n, 1)))
    return rh


@pytest.mark.parametrize("mode", [0, 1])
def test_quad_intersection_filter(rtc, mode):
    dev, sc = _stack(rtc, mode)
    calls = []

    @rtc.FILTER_FUNC
    def flt(args):  # quad g rejects rays whose x < 0.2 * (g + 1)
        ray, hit = _ray_fields(args)
        g = hit[6]
        calls.append((ray[0], g))
        assert hit[5] == 0 and abs(ray[8] - (g + 1.0)) < 1e-5
        if ray[0] < 0.2 * (g + 1):
            args.contents.valid[0] = 0

    for g in range(NQ - 1):
        sc.set_filters(g, intersect=flt)
    sc.commit()
    n = 3000
    rh = _rays(rtc, n)
    x = rh["org_x"].copy()
    sc.intersect1M(rh)
    want = np.array([next(g for g in range(NQ) if g == NQ - 1 or xi >= np.float32(0.2 * (g + 1))) for xi in x])
    assert np.array_equal(rh["geomID"], want.astype(np.uint32))
    assert np.allclose(rh["tfar"], want + 1.0, atol=1e-5)
    assert (rh["primID"] == 0).all()
    per_ray = {}
    for xo, g in calls:
        per_ray.setdefault(xo, []).append(g)
    for xi, w in zip(x, want):
        assert per_ray[xi] == list(range(min(w, NQ - 2) + 1))
    sc.release()
    dev.release()


@pytest.mark.parametrize("mode", [0, 1])
def test_quad_occlusion_and_context_filters(rtc, mode):
    dev, sc = _stack(rtc, mode)

    @rtc.FILTER_FUNC
    def occ_flt(args):  # quads 0..3 never occlude
        ray, hit = _ray_fields(args)
        if hit[6] < NQ - 1:
            args.contents.valid[0] = 0

    for g in range(NQ):
        sc.set_filters(g, occluded=occ_flt)
    sc.commit()
    n = 500
    rh = _rays(rtc, n)
    occ = rtc.aligned_rays(n)
    for f in occ.dtype.names:
        occ[f] = rh[f]
    occ2 = occ.copy()
    sc.occluded1M(occ)
    assert (occ["tfar"] == -np.inf).all()  # the last quad occludes
    occ2["tfar"] = np.float32(NQ - 0.5)    # ... but it is beyond tfar: nothing occludes
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
    rh2 = _rays(rtc, n, seed=4)
    x = rh2["org_x"].copy()
    sc.intersect1M(rh2, ctx=ctx)
    assert np.array_equal(rh2["geomID"], np.where(x < 0.5, 2, 0).astype(np.uint32))
    sc.release()
    dev.release()


# ---- 6. every entry path gives bit-identical hits --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_entry_paths_are_bit_identical(rtc, po, bomberman, mode):
    import torch
    verts, quads = _bomberman_quads(bomberman)
    lo, hi = verts.min(0), verts.max(0)

    def scene(extra=""):
        dev, flags = _device(rtc, mode, extra)
        sc = rtc.Scene(dev, flags)
        sc.add_quads(verts, quads)
        sc.commit()
        return dev, sc

    m = 40000
    rays = po.make_random_rays(m, lo, hi, seed=21)
    dev, sc = scene()
    # device-resident batch = the reference answer
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    sc.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    assert int((want["geomID"] != INVALID).sum()) > 1000
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
    assert cnt["rays"] == m and cnt["hits"] == int((want["geomID"] != INVALID).sum())
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
    # persistent service (service=1): a quad-only scene is served by the quad service kernel
    dev, sc = scene("service=1")
    sv = rtc.aligned_rayhits(k)
    sv[:] = rays[:k]
    for i in range(0, k, 32):
        sc.intersect1M(sv[i:i + 32])
    assert sv.tobytes() == want[:k].tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) >= 1
    sc.release()
    dev.release()


# ---- 7. the C example -----------------------------------------------------------------------------------------------------
def test_quad_geometry_example_runs(tmp_path):
    exe = str(tmp_path / "quad_geometry_min")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "quad_geometry_min.c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "quad_geometry_min: ok" in out.stdout
