"""The linear-bounds motion-blur accels (device config mb_bounds=linear: accel kinds 26..29, time-dependent nodes, the NODE_MB node step
of trace_loop.hip.h in its lane-per-ray and its octet form) against the oracle.

The oracle has no motion blur; as in test_gpu_motion_blur.py / test_gpu_quad_motion_blur.py the parity tests make it exact by construction:
every vertex of every time step is a multiple of 2^-10 below 64, the ray times are multiples of 1 / (4 S), and one static oracle scene per
distinct time traces the rays of that time."""
import ctypes as C

import numpy as np
import pytest

import deep_stack_helpers as ds
import mb_linear_helpers as mb
from helpers import INVALID, compare_hits, fill_rays, random_rays_np

pytestmark = pytest.mark.gpu

MODES = {0: "pluecker", 1: "moeller"}
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
HITF = ["Ng_x", "Ng_y", "Ng_z", "u", "v", "primID", "geomID", "instID"]
N_PARITY = 16384


def _scene(rtc, mode, steps, idx, extra="", bounds="linear"):
    """mode 0: robust scene (Pluecker), mode 1: Moeller; the kinds are 26..29 under mb_bounds=linear and 10..13 under swept"""
    quads = idx.shape[1] == 4
    dev = rtc.Device(("mb_bounds=" + bounds) + ("," + extra if extra else ""))
    sc = rtc.Scene(dev, ds.ROBUST if mode == 0 else 0)
    (sc.add_quads_mb if quads else sc.add_triangles_mb)(steps, idx)
    sc.commit()
    st = sc.stats()
    assert st["accelKind"] == ((28 if quads else 26) if bounds == "linear" else (12 if quads else 10)) + mode
    assert st["nodeBytes"] == (144 if bounds == "linear" else 96)
    return dev, sc


def _timed_rays(rtc, po, m, steps, times, seed):
    lo, hi = ds.bounds(*steps)
    rays = rtc.aligned_rayhits(m)
    rays[:] = po.make_random_rays(m, lo, hi, seed=seed)
    rays["time"] = np.asarray(times, np.float32)[np.arange(m) % len(times)]
    rays["id"] = np.arange(m, dtype=np.uint32)
    return rays


@pytest.fixture(scope="module")
def meshes(bomberman, bomberman_tris):
    v, tris = bomberman_tris
    assert len(tris) == 1454
    quads = bomberman[2].reshape(-1, 4).astype(np.uint32)
    return {("two", False): (mb.bomberman_two_steps(v), tris), ("five", False): (mb.bomberman_five_steps(v), tris),
            ("two", True): (mb.bomberman_two_steps(v), quads), ("five", True): (mb.bomberman_five_steps(v), quads)}


_oracle_cache = {}


def _parity_case(rtc, po, meshes, which, quads, mode):
    """rays and oracle records of one parity case, computed once per module: (steps, idx, rays, want, isb, times)"""
    key = (which, quads, mode)
    if key not in _oracle_cache:
        steps, idx = meshes[(which, quads)]
        S = len(steps) - 1
        times = [k / (4.0 * S) for k in range(4 * S + 1)]  # 0 and 1 among them; k = 4, 8, 12 of five steps: a step time
        rays = _timed_rays(rtc, po, N_PARITY, steps, times, seed=31)
        want, isb = ds.oracle_per_time(rtc, po, steps, idx, rays, mode, nthreads=16)
        _oracle_cache[key] = (steps, idx, rays, want, isb, times)
    return _oracle_cache[key]


def _check(rtc, got, occ, rays, want, isb, quads, mode, what):
    want = want.copy()
    if quads:
        ds.quad_allowances(got, want, isb, mode)
    nh = compare_hits(got, want, 1e-4, what)
    hit = want["geomID"] != INVALID
    assert np.array_equal(occ["tfar"] == -np.inf, hit), what
    assert np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit]), what
    return nh


# ---- 7. exact parity per ray time, both node-step forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("oct_max", [None, "0"], ids=["octet steps in the drain", "lane steps only"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("quads", [False, True], ids=["triangles", "quads"])
@pytest.mark.parametrize("which", ["two", "five"])
def test_parity_per_ray_time(rtc, po, monkeypatch, meshes, which, quads, mode, oct_max):
    steps, idx, rays, want, isb, times = _parity_case(rtc, po, meshes, which, quads, mode)
    monkeypatch.delenv("RTAMD_OCT_MAX", raising=False)
    if oct_max is not None:
        monkeypatch.setenv("RTAMD_OCT_MAX", oct_max)  # read when the device is created
    dev, sc = _scene(rtc, mode, steps, idx)
    got = ds.copy_of(rtc, rays)
    sc.intersect1M(got)
    occ = ds.occ_of(rtc, rays)
    sc.occluded1M(occ)
    what = f"{which}-step bomberman {'quads' if quads else 'triangles'}, {MODES[mode]}, linear bounds"
    nh = _check(rtc, got, occ, rays, want, isb, quads, mode, what)
    hit = want["geomID"] != INVALID
    per_time = [int((hit & (rays["time"] == np.float32(t))).sum()) for t in times]
    print(f"{what}: {nh} hits, per time {per_time}")
    assert min(per_time) >= 16, per_time  # every time, 0, 1 and the step times among them, is exercised
    sc.release()
    dev.release()


# ---- 8. fast mover ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_fast_mover_is_hit_where_it_is_at_the_rays_time(rtc, mode):
    """a flat 8 x 8 grid in z = 0 that moves by 16 x its extent along x (and by 2 along z) between its two steps: a ray down -z from
    z = 5 above where the grid is at the ray's time meets it at t = 5 - 2 time; above where it is at 1 - time there is nothing"""
    v, tris = mb.grid_tris(8)
    v = v.copy()
    v[:, 2] = 0
    shift = np.array([16 * 8.0, 0.0, 2.0])
    steps = [v, (v + shift).astype(np.float32)]
    n = 512
    rng = np.random.RandomState(11)
    times = rng.rand(2 * n) * 0.999 + 0.0005  # random, not dyadic
    times[n:] = np.where(np.abs(times[n:] - 0.5) > 0.1, times[n:], times[n:] * 0.3)
    assert (np.abs(times[n:] - 0.5) > 0.1).all()
    p = np.stack([rng.rand(2 * n) * 7 + 0.5, rng.rand(2 * n) * 7 + 0.5, np.full(2 * n, 5.0)], 1)
    at = times.copy()
    at[n:] = 1.0 - times[n:]  # the second half aims at where the grid is at the mirrored time
    org = (p + at[:, None] * shift * np.array([1, 1, 0])).astype(np.float32)
    rays = ds.rays_of(rtc, org, np.tile(np.array([0, 0, -1], np.float32), (2 * n, 1)))
    rays["time"] = times.astype(np.float32)
    out = {}
    for bounds in ("linear", "swept"):
        dev, sc = _scene(rtc, mode, steps, tris, bounds=bounds)
        got = ds.copy_of(rtc, rays)
        sc.intersect1M(got)
        occ = ds.occ_of(rtc, rays)
        sc.occluded1M(occ)
        out[bounds] = (got, occ)
        sc.release()
        dev.release()
    got, occ = out["linear"]
    assert (got["geomID"][:n] == 0).all() and (got["geomID"][n:] == INVALID).all()
    closed = 5.0 - 2.0 * rays["time"][:n].astype(np.float64)
    err = np.abs(got["tfar"][:n].astype(np.float64) - closed)
    print(f"fast mover ({MODES[mode]}): {n} hits, largest |t - closed form| {err.max():.2e}")
    assert (err <= 1e-5).all()
    assert (occ["tfar"][:n] == -np.inf).all() and np.array_equal(occ["tfar"][n:], rays["tfar"][n:])
    assert got.tobytes() == out["swept"][0].tobytes() and occ.tobytes() == out["swept"][1].tobytes()


# ---- 9. work counters ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quads", [False, True], ids=["triangles", "quads"])
def test_linear_bounds_visit_fewer_leaves_and_test_fewer_primitives(rtc, po, meshes, quads):
    steps, idx = meshes[("two", quads)]
    m = 65536
    rays = _timed_rays(rtc, po, m, steps, [0.0], seed=41)
    rays["time"] = np.random.RandomState(42).rand(m).astype(np.float32)
    cnt = {}
    for bounds in ("swept", "linear"):
        dev, sc = _scene(rtc, 0, steps, idx, bounds=bounds)
        got = ds.copy_of(rtc, rays)
        cnt[bounds] = sc.intersect1M_counted(got)
        assert cnt[bounds]["rays"] == m
        sc.release()
        dev.release()
    s, l = cnt["swept"], cnt["linear"]
    print(f"scene (a), {'quads' if quads else 'triangles'}, {m} rays, swept -> linear: nodeVisits {s['nodeVisits']} -> {l['nodeVisits']} "
          f"({l['nodeVisits'] / s['nodeVisits']:.3f}), leafVisits {s['leafVisits']} -> {l['leafVisits']} ({l['leafVisits'] / s['leafVisits']:.3f}), "
          f"primTests {s['primTests']} -> {l['primTests']} ({l['primTests'] / s['primTests']:.3f}), hits {s['hits']} / {l['hits']}")
    assert l["hits"] == s["hits"] and s["hits"] > m // 20
    assert l["primTests"] < s["primTests"] and l["leafVisits"] < s["leafVisits"]


# ---- 10. entry paths ----------------------------------------------------------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


def _aos(rtc, soa):
    out = rtc.aligned_rayhits(soa.shape[1])
    for k, f in enumerate(RAYF + HITF):
        out[f] = soa[k].view(out.dtype[f])
    return out


@pytest.fixture(scope="module")
def entry_case(rtc, po, meshes):
    steps, idx = meshes[("two", False)]
    rays = _timed_rays(rtc, po, 256, steps, [0.0, 0.25, 0.5, 0.75, 1.0], seed=51)
    out = {}
    for mode in (0, 1):
        want, _ = ds.oracle_per_time(rtc, po, steps, idx, rays, mode)
        # the second-nearest hit: the oracle again, from just beyond the first one
        again = ds.copy_of(rtc, rays)
        hit = want["geomID"] != INVALID
        again["tnear"][hit] = np.nextafter(want["tfar"][hit], np.float32(np.inf))
        second, _ = ds.oracle_per_time(rtc, po, steps, idx, again, mode)
        second["tnear"] = rays["tnear"]
        assert int(hit.sum()) >= 16 and int((second["geomID"] != INVALID).sum()) >= 4  # (one ray in eight hits the flat mesh at all)
        out[mode] = (want, second)
    return steps, idx, rays, out


@pytest.mark.parametrize("mode", [0, 1])
def test_entry_paths_agree_with_the_oracle(rtc, entry_case, mode):
    import torch
    steps, idx, rays, wants = entry_case
    want, second = wants[mode]
    hit = want["geomID"] != INVALID
    n = len(rays)
    dev, sc = _scene(rtc, mode, steps, idx)
    L = sc.lib
    # rtcIntersect1 / rtcOccluded1
    one = ds.copy_of(rtc, rays)
    occ = ds.occ_of(rtc, rays)
    for i in range(n):
        sc.intersect1(one[i:i + 1])
        sc.occluded1(occ[i:i + 1])
    compare_hits(one, want, 1e-4, "rtcIntersect1")
    assert np.array_equal(occ["tfar"] == -np.inf, hit)
    # packets of 4 / 8 / 16
    ctx = rtc.make_context()
    for W in (4, 8, 16):
        fn_i, fn_o = getattr(L, f"rtcIntersect{W}"), getattr(L, f"rtcOccluded{W}")
        for fn in (fn_i, fn_o):
            fn.restype = None
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        valid = np.full(W, -1, np.int32)
        got, gocc = [], []
        for p in range(0, n, W):
            pk = _soa(rays[p:p + W], W, True)
            fn_i(valid.ctypes.data, sc.handle, C.addressof(ctx), pk.ctypes.data)
            dev.check("packet")
            got.append(_aos(rtc, pk))
            po_ = _soa(rays[p:p + W], W, False)
            fn_o(valid.ctypes.data, sc.handle, C.addressof(ctx), po_.ctypes.data)
            dev.check("packet occluded")
            gocc.append(po_[8].view(np.float32).copy())
        compare_hits(np.concatenate(got), want, 1e-4, f"rtcIntersect{W}")
        assert np.array_equal(np.concatenate(gocc) == -np.inf, hit), W
    # a device-resident batch
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    sc.intersect1M(t)
    torch.cuda.synchronize()
    compare_hits(t.cpu().numpy().reshape(-1).view(rays.dtype), want, 1e-4, "device-resident batch")
    # instrumented twins: the plain kernels' bytes
    plain, c = ds.copy_of(rtc, rays), ds.copy_of(rtc, rays)
    sc.intersect1M(plain)
    cnt = sc.intersect1M_counted(c)
    assert c.tobytes() == plain.tobytes() and cnt["rays"] == n and cnt["hits"] == int(hit.sum())
    pocc, cocc = ds.occ_of(rtc, rays), ds.occ_of(rtc, rays)
    sc.occluded1M(pocc)
    sc.occluded1M_counted(cocc)
    assert cocc.tobytes() == pocc.tobytes()
    sc.release()
    dev.release()

    # a geometry filter that rejects every ray's first candidate: the second-nearest hit
    dev, sc = _scene(rtc, mode, steps, idx)
    seen = set()

    @rtc.FILTER_FUNC
    def flt(args):
        ray = C.cast(args.contents.ray, C.POINTER(C.c_uint * 12)).contents
        if ray[10] not in seen:
            seen.add(ray[10])
            args.contents.valid[0] = 0

    sc.set_filters(0, intersect=flt)
    sc.commit()
    f = ds.copy_of(rtc, rays)
    sc.intersect1M(f)
    assert len(seen) == int(hit.sum())
    compare_hits(f, second, 1e-4, "filter that rejects the first candidate")
    sc.release()
    dev.release()

    # service=1: no resident service kernel for these kinds, small calls fall back to the combiner
    dev, sc = _scene(rtc, mode, steps, idx, extra="service=1")
    sv = ds.copy_of(rtc, rays)
    for i in range(0, n, 32):
        sc.intersect1M(sv[i:i + 32])
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    compare_hits(sv, want, 1e-4, "service=1")
    sc.release()
    dev.release()


def _random_quads(n, seed, lo, hi):
    rng = np.random.RandomState(seed)
    c = (lo + rng.rand(n, 1, 3) * (hi - lo)).astype(np.float32)
    size = 0.1 * float(np.max(hi - lo))
    v = (c + (rng.rand(n, 4, 3).astype(np.float32) - 0.5) * size).astype(np.float32).reshape(-1, 3)
    return v, np.arange(4 * n, dtype=np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("mode", [0, 1])
def test_mixed_scene_equals_the_swept_device_record_for_record(rtc, mode):
    """a static mesh, a moving triangle mesh (three steps) and a moving quad mesh (two steps) in one scene: the trees differ, the
    records must not - on rays that hit no two primitives at a bit-identical t (checked on the swept device: with every ray's first hit
    rejected by a filter, the second hit has another t)"""
    lo, hi = np.zeros(3, np.float32), np.full(3, 8.0, np.float32)
    tv, tt = _random_quads(300, 5, lo, hi)
    mv, mt = _random_quads(300, 7, lo, hi)
    msteps = [mv, (mv + 0.2 * (hi - lo)).astype(np.float32), (mv + np.array([0.2, 0.5, 0.1], np.float32) * (hi - lo)).astype(np.float32)]
    qv, qq = _random_quads(300, 6, lo, hi)
    qsteps = [qv, (qv + np.array([-0.3, 0.1, 0.4], np.float32) * (hi - lo)).astype(np.float32)]
    m = 4096
    org, dirs = random_rays_np(m, lo, hi + 0.3 * (hi - lo), 9)
    rays = ds.rays_of(rtc, org, dirs)
    rays["time"] = np.random.RandomState(4).rand(m).astype(np.float32)
    rays["id"] = np.arange(m, dtype=np.uint32)
    seen = set()

    @rtc.FILTER_FUNC
    def flt(args):
        ray = C.cast(args.contents.ray, C.POINTER(C.c_uint * 12)).contents
        if ray[10] not in seen:
            seen.add(ray[10])
            args.contents.valid[0] = 0

    def scene(bounds, filtered=False):
        dev = rtc.Device("mb_bounds=" + bounds)
        sc = rtc.Scene(dev, ds.ROBUST if mode == 0 else 0)
        sc.add_triangles(tv, tt[:, :3].copy(), geom_id=0)
        sc.add_triangles_mb(msteps, mt[:, :3].copy(), geom_id=1)
        sc.add_quads_mb(qsteps, qq, geom_id=2)
        if filtered:
            for g in range(3):
                sc.set_filters(g, intersect=flt)
        sc.commit()
        return dev, sc

    out = {}
    for bounds in ("swept", "linear"):
        dev, sc = scene(bounds)
        got = ds.copy_of(rtc, rays)
        sc.intersect1M(got)
        occ = ds.occ_of(rtc, rays)
        sc.occluded1M(occ)
        out[bounds] = (got, occ)
        sc.release()
        dev.release()
    first = out["swept"][0]
    hit = first["geomID"] != INVALID
    counts = [int((first["geomID"] == g).sum()) for g in range(3)]
    print(f"mixed scene ({MODES[mode]}): hits per geometry {counts}")
    assert min(counts) > 50, counts
    dev, sc = scene("swept", filtered=True)
    again = ds.copy_of(rtc, rays)
    sc.intersect1M(again)
    sc.release()
    dev.release()
    assert len(seen) == int(hit.sum())
    assert (again["tfar"][hit] != first["tfar"][hit]).all(), "two primitives at a bit-identical t: such a ray has no reference answer"
    assert out["linear"][0].tobytes() == first.tobytes()
    assert out["linear"][1].tobytes() == out["swept"][1].tobytes()


# ---- 11. stack overflow path --------------------------------------------------------------------------------------------------------
DEEP_RAYS, DEEP_SEED = 160, 23


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("quads", [False, True], ids=["triangles", "quads"])
def test_rays_beyond_the_lds_stack(rtc, po, monkeypatch, quads, mode):
    """the needle soup of test_gpu_deep_stack.py at the size it uses for the swept motion-blur kernels: rays whose traversal stack, walked
    on the host over the new tree (boxes decoded at the ray's time), passes the 16 entries the kernel keeps in LDS"""
    steps, idx = ds.sliver_soup_mb(ds.N_SLIVERS, ds.SOUP_SEED, quads=quads)
    org, dirs = random_rays_np(DEEP_RAYS, *ds.bounds(*steps), DEEP_SEED)
    rays = ds.rays_of(rtc, org, dirs, ds.TIMES)
    want, isb = ds.oracle_per_time(rtc, po, steps, idx, rays, mode)
    first = None
    for name, knobs in (("lane form", {"RTAMD_OCT_MAX": "0", "RTAMD_OCT_LEAF": "0"}), ("octet form", {"RTAMD_OCT_MAX": "32", "RTAMD_OCT_LEAF": "1"})):
        for k in ("RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_KERNEL", "RTAMD_CULL"):
            monkeypatch.delenv(k, raising=False)
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        dev, sc = _scene(rtc, mode, steps, idx)
        if first is None:
            nodes = sc.accel_data(0).view(mb.NODEMB_DT)
            recs = sc.accel_data(2)
            leaves = ds.quad_mb_leaves(recs.view(ds.QUADMB_DT)) if quads else ds.tri_mb_leaves(recs.view(ds.TRIMB_DT))
            deepest = mb.simulate_stack_mb(nodes, sc.accel_root(), leaves, org, dirs, rays["time"], threshold=ds.LDS_STACK)
            nspill = int((deepest >= ds.LDS_STACK).sum())
            print(f"needle {'quads' if quads else 'triangles'} ({MODES[mode]}): depth {sc.stats()['maxDepth']}, {nspill} of {DEEP_RAYS} rays pass slot "
                  f"{ds.LDS_STACK} on the host, deepest slot {int(deepest.max())}")
            assert nspill >= 1
        got = ds.copy_of(rtc, rays)
        cnt = sc.intersect1M_counted(got)
        occ = ds.occ_of(rtc, rays)
        sc.occluded1M(occ)
        assert cnt["stackSpills"] >= nspill, (name, cnt["stackSpills"], nspill)
        assert dev.error() == 0
        _check(rtc, got, occ, rays, want, isb, quads, mode, f"needle soup, {name}")
        if first is None:
            first = got
        else:
            assert got.tobytes() == first.tobytes()
        sc.release()
        dev.release()
