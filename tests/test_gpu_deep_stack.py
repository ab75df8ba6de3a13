"""The HBM overflow part of the traversal stack, in every kernel that has one.

A ray's stack lives in LDS up to slot 16 (lane kernels: trace_loop.hip.h, trace_instance.hip) or slot 8 (ray-pool kernel: trace_pool.hip.h)
and in a per-lane column of an HBM overflow area beyond that; the host sizes the column from 7 * (maxDepth + 1) + 2 and every launch
context owns an area.  Ordinary meshes never get there (bomberman: slot 7 at most), so the scenes here are the needle soups of
tests/deep_stack_helpers.py, for which tests/test_host_deep_stack.py shows on the CPU that 55-77 % of the rays pass slot 16 and over 90 %
slot 8.  Every case compares with the oracle (IDs exact, 1e-4) and demands identical bytes from the forms of the kernels that treat the
boundary differently: the lane-per-ray and the octet node step (an octet hands a ray back when its next push could leave LDS), the
ray-pool kernel, and the instrumented twins, whose stackSpills counter must show that the overflow area really was written."""
import numpy as np
import pytest

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_quads_helpers as iq
from helpers import INVALID, compare_hits, random_rays_np

pytestmark = pytest.mark.gpu

KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL")
LANE_FORM = {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "0", "RTAMD_OCT_LEAF": "0"}    # every node and leaf step one ray per lane
OCTET_FORM = {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "32", "RTAMD_OCT_LEAF": "1"}  # 8 lanes per ray wherever the kernel allows it
POOL = {"RTAMD_KERNEL": "pool"}
SMALL_SHARES = {"RTAMD_CHUNK": "32", "RTAMD_REFILL_BATCH": "1", "RTAMD_LEAF_BATCH": "64"}
MIN_SPILLS = 0.05 * ds.GPU_RAYS  # every ray above slot 16 pushes at least one entry to HBM, and the host test guarantees >= 10 % of the rays


def _knobs(monkeypatch, knobs):
    """the tuning knobs are read when a device is created"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def _rays(rtc, lo, hi, times=None, snapped=False):
    org, dirs = random_rays_np(ds.GPU_RAYS, lo, hi, ds.GPU_RAY_SEED)
    return ds.rays_of(rtc, ds.snap(org) if snapped else org, dirs, times)


def _trace(rtc, sc, rays, counted=True):
    """closest hit and any hit, plain and (counted) through the instrumented twins, which must give the same bytes; returns
    (rayhits, rays, stackSpills of the closest-hit twin)"""
    got = ds.copy_of(rtc, rays)
    sc.intersect1M(got)
    occ = ds.occ_of(rtc, rays)
    sc.occluded1M(occ)
    spills = None
    if counted:
        c = ds.copy_of(rtc, rays)
        cnt = sc.intersect1M_counted(c)
        assert c.tobytes() == got.tobytes(), "the instrumented closest-hit twin differs from the plain kernel"
        assert cnt["rays"] == len(rays)
        co = ds.occ_of(rtc, rays)
        ocnt = sc.occluded1M_counted(co)
        assert co.tobytes() == occ.tobytes(), "the instrumented any-hit twin differs from the plain kernel"
        spills = cnt["stackSpills"]
        print(f"    stackSpills: closest hit {spills}, any hit {ocnt['stackSpills']} ({len(rays)} rays)")
    return got, occ, spills


def _sweep(rtc, monkeypatch, forms, make_scene, rays, check_first, what):
    """the same scene traced under every knob set of `forms`: the first is checked against the oracle by check_first(got, occ), the others
    must repeat its bytes; every counted form must have written the overflow area"""
    first = None
    for name, knobs in forms.items():
        _knobs(monkeypatch, knobs)
        dev, sc = make_scene()
        print(f"  {what}, {name}:")
        got, occ, spills = _trace(rtc, sc, rays)
        assert spills >= MIN_SPILLS, (what, name, spills)
        if first is None:
            check_first(got, occ)
            first = (name, got, occ)
        else:
            assert got.tobytes() == first[1].tobytes(), f"{what}: closest hit, {name} differs from {first[0]}"
            assert occ.tobytes() == first[2].tobytes(), f"{what}: any hit, {name} differs from {first[0]}"
        assert dev.error() == 0  # the `overflow` word stayed clear: no entry was dropped
        sc.release()
        dev.release()
    return first[1]


def _scene(rtc, cfg, flags, add):
    dev = rtc.Device(cfg)
    sc = rtc.Scene(dev, flags)
    add(sc)
    sc.commit()
    return dev, sc


# ---- triangles ----------------------------------------------------------------------------------------------------------------------------
TRI_CFG = {0: "tri_accel=bvh8.triangle4v", 1: "tri_accel=bvh8.triangle4"}


@pytest.fixture(scope="module")
def tri_soup():
    return ds.sliver_soup(ds.N_SLIVERS, ds.SOUP_SEED)


@pytest.mark.parametrize("mode", [0, 1])
def test_triangles_lane_octet_and_pool_kernels_agree_beyond_the_lds_stack(rtc, po, monkeypatch, tri_soup, mode):
    v, t = tri_soup
    rays = _rays(rtc, *ds.bounds(v))
    orc = po.TriangleScene(v, t, mode)
    want = ds.copy_of(rtc, rays)
    orc.intersect1M(want, nthreads=8)
    wocc = ds.occ_of(rtc, rays)
    orc.occluded1M(wocc, nthreads=8)
    orc.free()

    def check(got, occ):
        nh = compare_hits(got, want, 1e-4, f"needle triangles, mode {mode}")
        assert nh > ds.GPU_RAYS // 2, nh
        assert np.array_equal(occ["tfar"], wocc["tfar"])

    _sweep(rtc, monkeypatch, {"lane form": LANE_FORM, "octet form": OCTET_FORM, "ray-pool kernel": POOL},
           lambda: _scene(rtc, TRI_CFG[mode], 0, lambda s: s.add_triangles(v, t)), rays, check, f"needle triangles, mode {mode}")


# ---- quads --------------------------------------------------------------------------------------------------------------------------------
def _quad_device(mode):
    # mode 0: quad_accel=default on a robust scene (Pluecker), mode 1: the explicit quad4v accel (Moeller) - tests/test_gpu_quads.py
    return ("" if mode == 0 else "quad_accel=bvh8.quad4v"), (ds.ROBUST if mode == 0 else 0)


@pytest.mark.parametrize("mode", [0, 1])
def test_quads_lane_and_octet_forms_agree_beyond_the_lds_stack(rtc, po, monkeypatch, mode):
    v, q = ds.sliver_soup(ds.N_SLIVERS, ds.SOUP_SEED, quads=True)
    rays = _rays(rtc, *ds.bounds(v))
    orc = iq.split_oracle(po, v, q, mode)
    want = ds.copy_of(rtc, rays)
    orc.intersect1M(want, nthreads=8)
    orc.free()
    isb = iq.map_b(want)

    def check(got, occ):
        nd = ds.quad_allowances(got, want, isb, mode)
        nh = compare_hits(got, want, 1e-4, f"needle quads, mode {mode}")
        print(f"    {nh} hits, {int(isb.sum())} on B triangles, {nd} on a diagonal")
        assert nh > ds.GPU_RAYS // 2, nh
        hit = want["geomID"] != INVALID
        assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])

    cfg, flags = _quad_device(mode)
    _sweep(rtc, monkeypatch, {"lane form": LANE_FORM, "octet form": OCTET_FORM}, lambda: _scene(rtc, cfg, flags, lambda s: s.add_quads(v, q)),
           rays, check, f"needle quads, mode {mode}")


# ---- motion blur --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("quads", [False, True], ids=["triangles", "quads"])
def test_motion_blur_lane_and_octet_forms_agree_beyond_the_lds_stack(rtc, po, monkeypatch, quads, mode):
    steps, idx = ds.sliver_soup_mb(ds.N_SLIVERS, ds.SOUP_SEED, quads=quads)
    rays = _rays(rtc, *ds.bounds(*steps), times=ds.TIMES)
    want, isb = ds.oracle_per_time(rtc, po, steps, idx, rays, mode)
    what = f"motion-blur needle {'quads' if quads else 'triangles'}, mode {mode}"

    def check(got, occ):
        if quads:
            ds.quad_allowances(got, want, isb, mode)
        compare_hits(got, want, 1e-4, what)
        hit = want["geomID"] != INVALID
        per_time = [int((hit & (rays["time"] == np.float32(t))).sum()) for t in ds.TIMES]
        print(f"    hits per time {per_time}")
        assert min(per_time) > ds.GPU_RAYS // (4 * len(ds.TIMES)), per_time
        assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])

    def make():
        dev, sc = _scene(rtc, "", ds.ROBUST if mode == 0 else 0, lambda s: s.add_quads_mb(steps, idx) if quads else s.add_triangles_mb(steps, idx))
        assert sc.stats()["accelKind"] == (12 if quads else 10) + mode
        return dev, sc

    _sweep(rtc, monkeypatch, {"lane form": LANE_FORM, "octet form": OCTET_FORM}, make, rays, check, what)


# ---- instances ----------------------------------------------------------------------------------------------------------------------------
def _strided_device_copy(torch, rays):
    """the records in a device-resident array with a pitch of 96 bytes whose base is 4-byte aligned only: the kernels' load_ray<false> /
    store_hit<false>"""
    m = len(rays)
    raw = torch.zeros(m * 96 + 16, dtype=torch.uint8, device="cuda")
    view = raw[4:4 + m * 96].view(m, 96)
    assert view.data_ptr() % 16 == 4
    sz = rays.dtype.itemsize  # 80 (RTCRayHit) or 48 (RTCRay)
    view[:, :sz] = torch.from_numpy(rays.view(np.uint8).reshape(m, sz).copy()).cuda()
    return view


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["t", "q", "tq"])
def test_instances_markers_survive_the_overflow_area(rtc, po, monkeypatch, kind, mode):
    """Three overlapping instances of a needle scene: the exit marker, the marker of the pending quad tree ('tq') and the top-level entries
    below them are popped from HBM columns for more than half of the rays (tests/test_host_deep_stack.py).  There is no instrumented twin of
    this kernel; the precondition is the host test's simulation."""
    import torch
    scenes, inst = ds.instanced_scene(kind), ds.deep_instances()
    rays = _rays(rtc, *ds.instance_ray_box(scenes, inst), snapped=True)
    what = f"instances of '{kind}', mode {mode}"
    _knobs(monkeypatch, {})
    dev, top, inner = iq.build(rtc, mode, scenes, inst)
    quad_kind = iq.ACCEL_INST_PLUECKER if mode == 0 else iq.ACCEL_INST_MOELLER
    tri_kind = ih.ACCEL_INST_TRI_PLUECKER if mode == 0 else ih.ACCEL_INST_TRI_MOELLER
    assert top.stats()["accelKind"] == (quad_kind if "q" in kind else tri_kind)
    got = ds.copy_of(rtc, rays)
    top.intersect1M(got)
    occ = ds.occ_of(rtc, rays)
    top.occluded1M(occ)
    # leg 2: the merged direct traces of the instanced scene with the exact local rays, byte for byte
    direct, per = iq.direct_instances(rtc, inner, inst, rays)
    assert ih.equal_t_ties(per) == 0
    ndiff = int((got.view(np.uint8).reshape(-1, 80) != direct.view(np.uint8).reshape(-1, 80)).any(1).sum())
    assert got.tobytes() == direct.tobytes(), f"{what}: {ndiff} records differ from the merged direct traces"
    hit = direct["geomID"] != INVALID
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    # leg 1: the oracle
    want, _, isb, _ = iq.oracle_instances(rtc, po, scenes, inst, rays, mode, exact=True)
    nd = ds.quad_allowances(got, want, isb, mode, quad_gids=[7])
    nh = compare_hits(got, want, 1e-4, what)
    per_inst = [int((got["instID"][hit] == g).sum()) for g, _, _ in inst]
    print(f"  {what}: {nh} hits, per instance {per_inst}, {int(isb.sum())} on B triangles, {nd} on a diagonal")
    assert nh > ds.GPU_RAYS // 2 and min(per_inst) > 100, (nh, per_inst)
    if kind == "tq":
        assert int((got["geomID"] == 3).sum()) > 1000 and int((got["geomID"] == 7).sum()) > 1000
    # the same bytes from a 96-byte strided, 4-byte aligned record array: the exit marker re-reads the ray through load_ray<VEC>
    for sz, ref, call in ((80, got, top.intersect1M), (48, occ, top.occluded1M)):
        view = _strided_device_copy(torch, ds.copy_of(rtc, rays) if sz == 80 else ds.occ_of(rtc, rays))
        call(view)
        torch.cuda.synchronize()
        assert view[:, :sz].cpu().numpy().tobytes() == ref.tobytes(), f"{what}: strided records differ ({sz}-byte payload)"
    assert dev.error() == 0
    iq.release(dev, top, inner)
    # ... and with small queue shares, lanes refilled one at a time and leaves that wait for a full wave
    _knobs(monkeypatch, SMALL_SHARES)
    dev, top, inner = iq.build(rtc, mode, scenes, inst)
    g2 = ds.copy_of(rtc, rays)
    top.intersect1M(g2)
    o2 = ds.occ_of(rtc, rays)
    top.occluded1M(o2)
    assert g2.tobytes() == got.tobytes() and o2.tobytes() == occ.tobytes(), f"{what}: small shares differ"
    assert dev.error() == 0
    iq.release(dev, top, inner)


# ---- overflow areas belong to launch contexts -----------------------------------------------------------------------------------------------
def test_four_batches_in_flight_keep_their_overflow_areas_apart(rtc, monkeypatch, tri_soup):
    import torch
    v, t = tri_soup
    rays = _rays(rtc, *ds.bounds(v))
    _knobs(monkeypatch, LANE_FORM)
    dev, sc = _scene(rtc, TRI_CFG[0], 0, lambda s: s.add_triangles(v, t))
    src = rays.view(np.uint8).reshape(-1, 80)
    serial = torch.from_numpy(src.copy()).cuda()
    sc.intersect1M(serial)
    dev.synchronize()
    assert int((serial.view(torch.int32)[:, 18] != -1).sum().item()) > ds.GPU_RAYS // 2
    streams = [torch.cuda.Stream() for _ in range(4)]
    piped = [torch.from_numpy(src.copy()).cuda() for _ in range(4)]
    torch.cuda.synchronize()
    for b, s in zip(piped, streams):
        dev.set_stream(s.cuda_stream)
        sc.intersect1M(b, check=False)
    torch.cuda.synchronize()
    dev.check("four batches in flight")
    for i, b in enumerate(piped):
        assert torch.equal(b, serial), f"batch {i} in flight differs from the serial trace"
    assert dev.error() == 0
    sc.release()
    dev.release()


# ---- service ------------------------------------------------------------------------------------------------------------------------------
def test_service_calls_equal_the_batch_trace(rtc, monkeypatch, tri_soup):
    """2048 rays in calls of 32 on a service=1 device.  Whether the resident kernel takes them (per-job spillDepth) or the call falls back to
    the combiner (need > SPILL_DEPTH) is the service's business; the records are the batch's."""
    v, t = tri_soup
    k = 2048
    rays = _rays(rtc, *ds.bounds(v))[:k]
    _knobs(monkeypatch, {})
    dev, sc = _scene(rtc, "service=1," + TRI_CFG[0], 0, lambda s: s.add_triangles(v, t))
    want = ds.copy_of(rtc, rays)
    sc.intersect1M(want)
    wocc = ds.occ_of(rtc, rays)
    sc.occluded1M(wocc)
    assert int((want["geomID"] != INVALID).sum()) > k // 2
    got, occ = ds.copy_of(rtc, rays), ds.occ_of(rtc, rays)
    for a in range(0, k, 32):
        sc.intersect1M(got[a:a + 32])
        sc.occluded1M(occ[a:a + 32])
    print(f"  service calls: {dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS)} of {2 * k // 32}")
    assert got.tobytes() == want.tobytes() and occ.tobytes() == wocc.tobytes()
    assert dev.error() == 0
    sc.release()
    dev.release()
