"""Every form of the cBVH kernels against the oracle (tests/cbvh_forms_helpers.py has the inputs, tests/test_host_cbvh_forms.py the expected side).

launch_cbvh (csrc/trace_cbvh.hip.h) picks, per fork mode and compression level C, one of three kernel forms: the quad form (four lanes per ray;
the default), the one-ray-per-lane form in the lane skeleton (RTAMD_CBVH_FORM=lane, RTAMD_KERNEL=lane) and the one-ray-per-lane form in the
ray-pool skeleton (RTAMD_KERNEL=pool, csrc/trace_pool.hip.h - the library's own choice for compressed.grid and for triangles from 2.5 M rays per
launch on).  Each exists as closest hit / any hit, plain / counted twin and for 16-byte aligned / other records.  Per (mode, L, C):

  a. the quad form is held against the oracle: byte for byte against the oracle in product arithmetic and classified against the oracle in reference
     arithmetic (helpers.check_fork_parity; the order-dependent modes walk the product's BVH8), any hit against the oracle on its own tree;
  b. every form, on a device of its own, gives the bytes of (a) from rtcIntersect1M, rtcOccluded1M and their counted twins, twice (the ray-to-wave
     assignment is dynamic), and the twins count 20 000 rays and as many hits as there are hit records (any hit: occluded rays);
  c. every form gives the same records from an array with a pitch of 96 bytes (any hit: 48-byte records, pitch 64) whose base is only 4-byte aligned,
     and leaves the padding alone: a DEVICE-RESIDENT array reaches the kernels' load_ray<false> / store_hit<false> twins, a host array of that shape
     (tests/test_gpu_triangles.py test_stream_semantics) is repacked by the staging code on its way there and back;
  d. the rays of the matrix all start with tfar = inf, so a blob is entered with a finite ray.tfar only after a first hit.  The traced records of (a) -
     tfar = the hit distance - are therefore traced AGAIN: the quad form must give the bytes of the oracle in product arithmetic on that input (one
     record in 250 000 within 1e-5, the allowance of helpers.check_fork_parity's regression leg), the other forms the bytes of the quad form.

The counted twin also tells the skeletons apart: the pool skeleton reports RTCAMDTraceCounters::maxRaySteps == 0 (it keeps no per-lane step count,
trace_pool.hip.h), the lane skeleton the step count of its deepest ray (> 0 whenever a ray was traced).  Every leg asserts on it, so a knob that no
longer selects the form it names fails here instead of comparing a kernel with itself.

The last four tests cover the library's automatic switch to the pool skeleton (Device::tunePoolMinRays = 2.5 M rays in one launch; only a
device-resident batch is launched whole, the host pipeline cuts a host batch into chunks below the threshold)."""
import importlib

import numpy as np
import pytest

import cbvh_forms_helpers as cf
from helpers import INVALID, check_fork_parity, compare_hits

pytestmark = pytest.mark.gpu

PAD = 0xA5


@pytest.fixture(scope="module")
def inputs(po, bomberman):
    m = cf.mesh(bomberman)
    return m, cf.make_rays(po, m[0])


def _strided_device_copy(torch, recs, pitch):
    """the records in a device-resident array with a pitch of `pitch` bytes whose base is 4-byte aligned only; padding bytes = PAD"""
    n, sz = len(recs), recs.dtype.itemsize
    raw = torch.full((n * pitch + 16,), PAD, dtype=torch.uint8, device="cuda")
    view = raw[4:4 + n * pitch].view(n, pitch)
    assert view.data_ptr() % 16 == 4 and pitch > sz
    view[:, :sz] = torch.from_numpy(recs.view(np.uint8).reshape(n, sz).copy()).cuda()
    torch.cuda.synchronize()
    return view


def _strided_host_copy(rtc, recs, pitch):
    """(raw bytes, record view) of a host array with a pitch of `pitch` bytes whose base is 4-byte aligned only; padding bytes = PAD"""
    n = len(recs)
    raw = np.full(n * pitch + 64, PAD, dtype=np.uint8)
    off = ((-raw.ctypes.data) % 16) + 4
    view = np.ndarray(shape=(n,), dtype=recs.dtype, buffer=raw.data, offset=off, strides=(pitch,))
    view[:] = recs
    assert view.ctypes.data % 16 == 4
    return raw[off:off + n * pitch].reshape(n, pitch), view


def _skeleton_matches(cnt, form):
    """maxRaySteps: 0 from the pool skeleton, the deepest ray's step count from the lane skeleton (module docstring)"""
    return (cnt["maxRaySteps"] == 0) == (form == "pool")


@pytest.mark.parametrize("L,C", cf.PAIRS)
@pytest.mark.parametrize("accel", cf.MODES)
def test_form_matrix(rtc, po, monkeypatch, inputs, accel, L, C):
    import torch
    m, src = inputs
    n = len(src)
    osrc = cf.occ_of(rtc, src)
    what = f"{accel} L{L} C{C}"
    want = wocc = want2 = None
    for form in cf.FORMS:
        dev, sc = cf.build(rtc, monkeypatch, accel, L, C, form, m)
        assert sc.stats()["primCount"] == cf.blob_count(L, C)
        dev.set_stream(torch.cuda.current_stream().cuda_stream)  # torch's copies and the traces of device-resident records are then stream-ordered
        if form == "quad":
            # ---- a. the reference leg: default knobs against the oracle
            orc = cf.oracle(po, sc, accel, C)

            def trace_oracle():
                w = src.copy()
                orc.intersect1M(w, nthreads=8)
                return w

            want = rtc.aligned_rayhits(n)
            want[:] = src
            sc.intersect1M(want)
            check_fork_parity(po, want, trace_oracle, accel, what=what, cell=2.0 ** -L)
            orc.free()
            hit = want["geomID"] != INVALID
            nh = int(hit.sum())
            print(f"[cbvh forms] {what}: {nh} hits")
            assert nh >= cf.HITS_FLOOR
            wocc = osrc.copy()
            sc.occluded1M(wocc)
            own = cf.oracle(po, sc, accel, C, same_tree=False)  # the any-hit stub reports every blob whose bounds the ray meets: order free
            oocc = osrc.copy()
            own.occluded1M(oocc, nthreads=8)
            own.free()
            occluded = wocc["tfar"] == -np.inf
            diff = int((occluded != (oocc["tfar"] == -np.inf)).sum())
            print(f"[cbvh forms] {what}: {int(occluded.sum())} occluded, {diff} differ from the oracle on its own tree")
            assert diff <= max(2, n // 20000), diff
            assert np.all(occluded[hit])
            assert wocc[~occluded].tobytes() == osrc[~occluded].tobytes()
            nocc = int(occluded.sum())
            # ---- d. the expected side of the second visit (finite tfar at blob entry)
            orc = cf.oracle(po, sc, accel, C)
            o2 = want.copy()
            with po.fork_arith(1):
                orc.intersect1M(o2, nthreads=8)
            orc.free()
            want2 = rtc.aligned_rayhits(n)
            want2[:] = want
            sc.intersect1M(want2)
            nd2, moved = cf.differing(want2, o2), cf.differing(want2, want)
            print(f"[cbvh forms] {what}: second visit, {nd2} records differ from the oracle in product arithmetic, {moved} records changed")
            assert nd2 <= max(1, n // 250000), nd2
            if nd2:
                bad = (want2.view(np.uint8).reshape(n, 80) != o2.view(np.uint8).reshape(n, 80)).any(1)
                compare_hits(want2[bad], o2[bad], rtol=1e-5, what=what + " (second visit, product arithmetic)")
            assert np.array_equal(want2["geomID"] != INVALID, hit)  # a hit stays a hit (found again at t <= tfar or replaced), a miss a miss
        # ---- b. this form, plain and counted, closest hit and any hit, twice
        for rep in range(2):
            tag = f"{what}, {form} form, run {rep}"
            got = rtc.aligned_rayhits(n)
            got[:] = src
            sc.intersect1M(got)
            assert got.tobytes() == want.tobytes(), f"{tag}: rtcIntersect1M, {cf.differing(got, want)} records differ"
            got[:] = src
            cnt = sc.intersect1M_counted(got)
            assert got.tobytes() == want.tobytes(), f"{tag}: counted twin, {cf.differing(got, want)} records differ"
            assert cnt["rays"] == n and cnt["hits"] == nh, (tag, cnt["rays"], cnt["hits"], nh)
            assert _skeleton_matches(cnt, form), (tag, cnt["maxRaySteps"])
            occ = osrc.copy()
            sc.occluded1M(occ)
            assert occ.tobytes() == wocc.tobytes(), f"{tag}: rtcOccluded1M, {cf.differing(occ, wocc)} records differ"
            occ = osrc.copy()
            cnt = sc.occluded1M_counted(occ)
            assert occ.tobytes() == wocc.tobytes(), f"{tag}: counted any-hit twin, {cf.differing(occ, wocc)} records differ"
            assert cnt["rays"] == n and cnt["hits"] == nocc, (tag, cnt["rays"], cnt["hits"], nocc)
            assert _skeleton_matches(cnt, form), (tag, cnt["maxRaySteps"])
        # ---- c. records that are not 16-byte aligned, device resident
        for recs, ref, pitch, call in ((src, want, 96, sc.intersect1M), (osrc, wocc, 64, sc.occluded1M)):
            sz = recs.dtype.itemsize
            view = _strided_device_copy(torch, recs, pitch)
            call(view)
            dev.synchronize()
            out = view.cpu().numpy()
            assert out[:, :sz].tobytes() == ref.tobytes(), f"{what}, {form} form: device records of pitch {pitch} differ ({sz}-byte payload)"
            assert (out[:, sz:] == PAD).all(), f"{what}, {form} form: padding of the {pitch}-byte device records was written"
            out, hview = _strided_host_copy(rtc, recs, pitch)
            call(hview)
            assert out[:, :sz].tobytes() == ref.tobytes(), f"{what}, {form} form: host records of pitch {pitch} differ ({sz}-byte payload)"
            assert (out[:, sz:] == PAD).all(), f"{what}, {form} form: padding of the {pitch}-byte host records was written"
        # ---- d. second visit: the traced records again
        got = rtc.aligned_rayhits(n)
        got[:] = want
        sc.intersect1M(got)
        assert got.tobytes() == want2.tobytes(), f"{what}, {form} form: second visit, {cf.differing(got, want2)} records differ from the quad form"
        assert dev.error() == rtc.RTC_ERROR_NONE
        sc.release()
        dev.release()


# ---- the automatic switch to the pool skeleton ------------------------------------------------------------------------------------------
M_SWITCH = 2_600_000  # above Device::tunePoolMinRays (2 500 000)


@pytest.fixture(scope="module")
def switch_rays(bomberman):
    rg = importlib.import_module("embree-compressed_amd.raygen")
    verts = bomberman[0]
    return rg.make_random_rays(M_SWITCH, verts.min(0), verts.max(0), seed=2025)  # uint8 [M, 80]


def _switch_scene(rtc, bomberman, kind):
    verts, fs, fi = bomberman
    if kind == "tri":
        dev = rtc.Device("tri_accel=bvh8.triangle4v")
        sc = rtc.Scene(dev)
        sc.add_triangles(verts, rtc.fan_triangulate(fs, fi))
    else:
        dev = rtc.Device("subdiv_accel=bvh4.compressed.grid")
        sc = rtc.Scene(dev)
        sc.add_subdiv(verts, fs, fi)
        sc.set_levels(3, 2)
    sc.commit()
    return dev, sc


@pytest.mark.parametrize("occluded", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("kind", ["tri", "grid"])
def test_large_batches_switch_to_the_pool_skeleton(rtc, bomberman, monkeypatch, switch_rays, kind, occluded):
    """2.6 M device-resident rays in one launch on a default device (the library picks the pool skeleton for triangles and compressed.grid from
    2.5 M rays on) and on an RTAMD_KERNEL=lane device: identical bytes.  RTCAMDTraceCounters::maxRaySteps of the counted twin separates the two
    skeletons (0 from the pool skeleton, > 0 from the lane skeleton), so the leg also asserts that the switch happened - and that it does not
    happen for a batch below the threshold."""
    import torch
    rec = 48 if occluded else 80
    rays = torch.from_numpy(switch_rays).cuda()[:, :rec].contiguous()
    out, steps, small = {}, {}, {}
    for name in ("default", "lane"):
        cf.set_form(monkeypatch, "quad")
        if name == "lane":
            monkeypatch.setenv("RTAMD_KERNEL", "lane")
        dev, sc = _switch_scene(rtc, bomberman, kind)
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        trace, counted = (sc.occluded1M, sc.occluded1M_counted) if occluded else (sc.intersect1M, sc.intersect1M_counted)
        got, again, few = rays.clone(), rays.clone(), rays[:100_000].clone()
        torch.cuda.synchronize()
        trace(got)
        dev.synchronize()
        out[name] = got
        cnt = counted(again)
        dev.synchronize()
        assert torch.equal(again, got), f"{kind}, {name} device: the counted twin differs from the plain kernel"
        found = int(torch.isneginf(got.view(torch.float32)[:, 8]).sum().item()) if occluded else int((got.view(torch.int32)[:, 18] != -1).sum().item())
        assert cnt["rays"] == M_SWITCH and cnt["hits"] == found and 0.05 * M_SWITCH < found < 0.6 * M_SWITCH, (cnt["rays"], cnt["hits"], found)
        steps[name] = cnt["maxRaySteps"]
        small[name] = counted(few)["maxRaySteps"]
        dev.synchronize()
        assert torch.equal(few, got[:100_000]), f"{kind}, {name} device: a batch below the threshold differs"
        assert dev.error() == rtc.RTC_ERROR_NONE
        sc.release()
        dev.release()
    assert torch.equal(out["default"], out["lane"]), f"{kind}: pool and lane skeleton differ on {M_SWITCH} rays"
    assert steps["default"] == 0 and steps["lane"] > 0, steps       # the default device switched, the lane device did not
    assert small["default"] > 0 and small["lane"] > 0, small        # below the threshold both run the lane skeleton
