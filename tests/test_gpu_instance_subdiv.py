"""Instanced scenes that hold subdivision meshes (accel kinds 24 / 25), traced by trace_instance_subdiv.hip: a ray enters an instance as
in the mesh kernels and meets, below it, the one-ray-per-lane leaves of the subdivision kernels - the eager grid cell or the cBVH blob
walk of bvh4.compressed.leaf - on its LOCAL ray.  Scenes, rays and expected records are those of tests/instance_subdiv_helpers.py:
the expected side of every byte-for-byte leg is the instanced scene traced directly, with the instance's exact local rays (lattice
translations, power-of-two scales) and the instance's geomID as instID.

compressed.leaf is order dependent (far = min(frustum exit, ray.tfar) at blob entry): where rays may meet several instances only the
two classes of instance_subdiv_helpers.order_free_classes are compared."""
import ctypes as C

import numpy as np
import pytest

import instance_helpers as ih
import instance_mb_helpers as im
import instance_quads_helpers as iq
import instance_subdiv_helpers as isd
from helpers import INVALID, compare_hits, random_soup

pytestmark = pytest.mark.gpu

RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
CASES = [("faces", L, Cl) for L, Cl in isd.LEVELS] + [("cube", 3, 2), ("full", 3, 2)]


def _mesh(bomberman, shape, L, Cl):
    m = {"faces": lambda: isd.bomberman_faces(bomberman), "cube": isd.cube, "full": lambda: isd.bomberman_faces(bomberman, None)}[shape]()
    return {"m": m + (L, Cl)}


def _check(got, want, what):
    assert got.tobytes() == want.tobytes(), f"{what}: {isd.differing(got, want)} of {len(got)} records differ"


# ---- 1. short rays: byte for byte ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
@pytest.mark.parametrize("shape,L,Cl", CASES)
def test_short_rays_equal_the_instanced_scene_traced_directly(rtc, bomberman, monkeypatch, accel, shape, L, Cl):
    """rays that cannot reach any other instance: the record is the instanced scene's own, traced directly in the default form of its
    kernel, with the coherent flag, and (compressed.leaf) in the one-ray-per-lane form, whose blob walk is the function the instance
    kernel calls; rays that hit nothing keep their records"""
    monkeypatch.delenv("RTAMD_CBVH_FORM", raising=False)
    meshes = _mesh(bomberman, shape, L, Cl)
    inst = isd.lattice_instances(9)
    rays, owner = isd.short_rays(rtc, meshes, inst, 1200, 5)
    isd.assert_cannot_reach_others(meshes, inst, rays, owner)
    dev, top, inner = isd.build(rtc, accel, meshes, inst)
    assert top.stats()["accelKind"] == isd.KIND[accel]
    got = iq.copy(rtc, rays)
    top.intersect1M(got, ctx=rtc.make_context(inst_id=77))  # the context's instID is replaced by the instance's
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    what = f"{accel} {shape} L{L} C{Cl}"
    for coherent in (False, True):
        _check(got, isd.direct_owned(rtc, inner, inst, rays, owner, coherent=coherent), f"{what}, coherent {coherent}")
    _check(occ, isd.direct_owned(rtc, inner, inst, rays, owner, occluded=True), f"{what}, any hit")
    hit = got["geomID"] != INVALID
    per_inst = np.bincount(owner[hit], minlength=len(inst))
    print(f"{what}: {int(hit.sum())} hits of {len(rays)} rays, per instance {per_inst.tolist()}, {int((occ['tfar'] == -np.inf).sum())} occluded")
    assert per_inst.min() >= 50 and (~hit).sum() >= 50
    assert np.array_equal(got["instID"][hit], np.array([g for g, _, _ in inst], np.uint32)[owner[hit]]) and (got["instID"][~hit] == INVALID).all()
    assert np.all((occ["tfar"] == -np.inf)[hit])
    if accel == isd.LEAF:
        assert (got["Ng_x"][hit] == 1).all() and (got["Ng_y"][hit] == 0).all() and (got["Ng_z"][hit] == 0).all()  # the fork's dummy normal
    else:
        assert np.array_equal(occ["tfar"] == -np.inf, hit)
    isd.release(dev, top, inner)
    if accel == isd.LEAF and shape != "full":
        monkeypatch.setenv("RTAMD_CBVH_FORM", "lane")  # read when a device is created
        dev = rtc.Device("subdiv_accel=" + accel)
        lane = {"m": isd.add_inner(rtc, dev, meshes["m"])}
        _check(got, isd.direct_owned(rtc, lane, inst, rays, owner), f"{what}, one ray per lane")
        lane["m"].release()
        dev.release()


# ---- 2. crossing rays ----------------------------------------------------------------------------------------------------------------------
CROSS_SPACING, CROSS_RAYS = 64.0, 20000  # cubes on a 4 x 5 lattice: about 2 % of the rays hit two of them (measured with the CPU oracle)


def test_crossing_rays_eager_equal_the_merged_direct_traces(rtc):
    meshes = {"m": isd.cube() + (4, 2)}
    inst = isd.lattice_instances(20, spacing=CROSS_SPACING)
    rays = isd.crossing_rays(rtc, meshes, inst, CROSS_RAYS, 7)
    dev, top, inner = isd.build(rtc, isd.EAGER, meshes, inst)
    per = isd.direct_all(rtc, inner, inst, rays)
    assert ih.equal_t_ties(per) == 0  # the two smallest t of every ray differ
    want = isd.merge(rays, per, inst)
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    _check(got, want, "eager, crossing rays")
    hit = want["geomID"] != INVALID
    two = int((np.stack([p["geomID"] != INVALID for p in per]).sum(0) >= 2).sum())
    print(f"eager crossing rays: {int(hit.sum())} hits in {len(np.unique(want['instID'][hit]))} instances, {two} rays hit two or more")
    assert int(hit.sum()) > 5000 and len(np.unique(want["instID"][hit])) == 20 and two >= 100
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    isd.release(dev, top, inner)


def test_crossing_rays_compressed_leaf_order_free_classes(rtc):
    meshes = {"m": isd.cube() + (4, 2)}
    inst = isd.lattice_instances(20, spacing=CROSS_SPACING)
    rays = isd.crossing_rays(rtc, meshes, inst, CROSS_RAYS, 7)
    dev, top, inner = isd.build(rtc, isd.LEAF, meshes, inst)
    none, single, want = isd.order_free_classes(rtc, inner, inst, rays)
    print(f"compressed.leaf crossing rays: {int(none.sum())} hit nothing, {int(single.sum())} hit one instance only, {len(rays) - int((none | single).sum())} others")
    # condition on the inputs, from the direct traces alone
    assert (none | single).sum() >= 0.95 * len(rays) and single.sum() >= 1000
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    _check(got[none], rays[none], "compressed.leaf, rays that hit nothing")
    _check(got[single], want[single], "compressed.leaf, rays that hit one instance")
    rest = ~(none | single)
    assert (got["geomID"][rest] != INVALID).all()  # some instance is hit whatever the order
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    _check(occ, isd.occluded_any(rtc, inner, inst, rays), "compressed.leaf, any hit")
    assert np.all((occ["tfar"] == -np.inf)[got["geomID"] != INVALID])
    isd.release(dev, top, inner)


# ---- 3. general transforms, eager -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,L", [("cube", 4), ("faces", 3)])
def test_general_transforms_against_the_subdivision_oracle(rtc, po, bomberman, shape, L):
    """rotations and non-uniform scales: the oracle's eager traversal (po.SubdivScene on the instanced scene's own cells) per instance on
    instance_helpers.local_rays, merged by smallest t; IDs exact, t / u / v within 1e-4 relative"""
    meshes = _mesh(bomberman, shape, L, 1)
    inst = isd.static(iq.general_instances())
    rays = isd.crossing_rays(rtc, meshes, inst, 20000, 11)
    dev, top, inner = isd.build(rtc, isd.EAGER, meshes, inst)
    sc = inner["m"]
    orc = po.SubdivScene(sc.accel_data(2), sc.stats()["primBytes"], 2, 1)
    per = []
    for gid, _, steps in inst:
        sub = rtc.aligned_rayhits(len(rays))
        sub[:] = ih.local_rays(rays, ih.world2local(steps[0]))
        orc.intersect1M(sub, nthreads=16)
        for f in ("org_x", "org_y", "org_z", "dir_x", "dir_y", "dir_z"):
            sub[f] = rays[f]
        per.append(sub)
    orc.free()
    want = isd.merge(rays, per, inst)
    t = np.sort(np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf).astype(np.float64) for p in per]), axis=0)
    both = np.isfinite(t[1])
    assert np.all(t[1][both] - t[0][both] > 1e-4 * np.abs(t[0][both]))  # input condition: no second instance within the tolerance
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    nh = compare_hits(got, want, 1e-4, f"general transforms, eager, {shape}")
    hit = want["geomID"] != INVALID
    print(f"general transforms, {shape}: {nh} hits in {len(np.unique(want['instID'][hit]))} instances")
    assert int(hit.sum()) > 3000 and len(np.unique(want["instID"][hit])) == 9
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    isd.release(dev, top, inner)


# ---- 4. moving instances ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_moving_instances_equal_the_static_instance_at_the_rays_time(rtc, bomberman, accel):
    """instances with 2 and 3 transform steps (signed axis permutations, power-of-two scales, translations on the grid), ray times k / 8:
    short rays against the instanced scene traced directly under world2local(time)"""
    meshes = _mesh(bomberman, "faces", 3, 2)
    inst = [(g, k, s[:3]) for g, k, s in im.exact_instances(6)]
    assert sorted({len(s) for _, _, s in inst}) == [2, 3]
    rays, owner = isd.short_rays(rtc, meshes, inst, 2000, 9, times=[k / 8.0 for k in (0, 3, 8, 1, 4, 6, 2, 7, 5)])
    isd.assert_cannot_reach_others(meshes, inst, rays, owner)
    dev, top, inner = isd.build(rtc, accel, meshes, inst)
    assert top.stats()["accelKind"] == isd.KIND[accel]
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    _check(got, isd.direct_owned(rtc, inner, inst, rays, owner), f"{accel}, moving instances")
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    _check(occ, isd.direct_owned(rtc, inner, inst, rays, owner, occluded=True), f"{accel}, moving instances, any hit")
    hit = got["geomID"] != INVALID
    per_inst = np.bincount(owner[hit], minlength=len(inst))
    print(f"{accel}, moving instances: {int(hit.sum())} hits of {len(rays)} rays, per instance {per_inst.tolist()}, {len(np.unique(rays['time'][hit]))} times")
    assert per_inst.min() >= 50 and len(np.unique(rays["time"][hit])) == 9
    isd.release(dev, top, inner)


# ---- 5. a top scene of both classes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_mixed_top_scene_equals_the_scene_without_the_subdivision_instance_merged(rtc, bomberman, accel):
    """one instance of a triangle scene, one of a quad scene, one of a subdivision scene and a triangle mesh of the top scene's own, with
    disjoint boxes.  The subdivision instance is traced last, against the tfar the other accels left: expected = the same top scene
    without it, then the subdivision instance's direct trace on those records."""
    qv, qq = iq.bomberman_quads(bomberman)
    tt = np.concatenate([qq[:, [0, 1, 2]], qq[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.uint32)
    sv, st = random_soup(512, 5, extent=4.0, size=2.0)
    sv = ih.snap(sv * 8.0) + np.array([0.0, -60.0, 0.0], np.float32)  # spans y = -68 .. -20, below the three instances
    sub_mesh = isd.bomberman_faces(bomberman) + (4, 2)
    places = {"tri": ih.affine((0.0, 0.0, 0.0)), "quad": ih.affine((0.0, 40.0, 0.0), (0.5,) * 3), "sub": ih.affine((0.0, 80.0, 0.0), (2.0,) * 3)}

    def make(with_subdiv):
        dev = rtc.Device("subdiv_accel=" + accel)
        tri, quad = rtc.Scene(dev), rtc.Scene(dev)
        tri.add_triangles(qv, tt)
        tri.commit()
        quad.add_quads(qv, qq)
        quad.commit()
        sub = isd.add_inner(rtc, dev, sub_mesh)
        top = rtc.Scene(dev)
        assert top.add_triangles(sv, st, geom_id=0) == 0
        assert top.add_instance(tri, places["tri"], geom_id=1) == 1
        assert top.add_instance(quad, places["quad"], geom_id=2) == 2
        if with_subdiv:
            assert top.add_instance(sub, places["sub"], geom_id=3) == 3
        top.commit()
        return dev, top, [tri, quad, sub]

    boxes_of = {"m": sub_mesh, "q": (qv,), "s": (sv,)}
    inst = [(1, "q", [places["tri"]]), (2, "q", [places["quad"]]), (3, "m", [places["sub"]]), (0, "s", [ih.affine()])]
    rays = isd.crossing_rays(rtc, boxes_of, inst, 20000, 13)
    dev0, top0, keep0 = make(False)
    base = iq.copy(rtc, rays)
    top0.intersect1M(base)
    occ0 = iq.occ_of(rtc, rays)
    top0.occluded1M(occ0)
    dev, top, keep = make(True)
    assert len(top.accel_data(rtc.ACCEL_DATA_INSTSUBDIV + 0)) > 0 and top.stats() == {**top0.stats(), "totalBytes": top.stats()["totalBytes"]}
    sub = isd.direct(rtc, keep[2], 3, [places["sub"]], base, tfar=base["tfar"])  # against the tfar the other accels left
    want = base.copy()
    sel = sub["geomID"] != INVALID
    want[sel] = sub[sel]
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    _check(got, want, f"{accel}, mixed top scene")
    counts = [int((want["instID"] == g).sum()) for g in (1, 2, 3)] + [int(((want["geomID"] == 0) & (want["instID"] == INVALID)).sum())]
    behind = int(((base["geomID"] != INVALID) & sel).sum())
    print(f"{accel}, mixed top scene: hits per instance 1, 2, 3 and on the top scene's mesh {counts}; {behind} rays hit the subdivision instance in front of another hit")
    assert min(counts) >= 300 and behind >= 20
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    osub = isd.direct(rtc, keep[2], 3, [places["sub"]], rays, occluded=True)
    wocc = occ0.copy()
    wocc["tfar"][osub["tfar"] == -np.inf] = -np.inf
    _check(occ, wocc, f"{accel}, mixed top scene, any hit")
    for d, tp, ks in ((dev, top, keep), (dev0, top0, keep0)):
        tp.release()
        for s in ks:
            s.release()
        d.release()


# ---- 6. / 7. every entry path (1 / 1M / 1Mp / packets; device-resident, host, sharded) gives the bytes of one device-resident rtcIntersect1M; service=1 ---------------------------------------------------
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


@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_entry_paths_are_bit_identical(rtc, bomberman, accel):
    import torch
    meshes = _mesh(bomberman, "faces", 3, 2)
    inst = isd.lattice_instances(8)
    g, k, s = inst[5]
    inst[5] = (g, k, [s[0], ih.affine((48.0, 41.0, 3.0), (2.0,) * 3)])  # one of them moves
    m = 20000
    rays = isd.crossing_rays(rtc, meshes, inst, m, 31)
    rays["time"] = (np.arange(m) % 5 / 4.0).astype(np.float32)
    dev, top, inner = isd.build(rtc, accel, meshes, inst)
    assert top.stats()["accelKind"] == isd.KIND[accel]
    L = top.lib
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    top.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    hit = want["geomID"] != INVALID
    assert int(hit.sum()) > 3000 and len(np.unique(want["instID"][hit])) == 8
    to = torch.from_numpy(iq.occ_of(rtc, rays).view(np.uint8).reshape(-1, 48).copy()).cuda()
    top.occluded1M(to)
    torch.cuda.synchronize()
    wocc = to.cpu().numpy().reshape(-1).view(rtc.RAY_DTYPE)
    assert np.all((wocc["tfar"] == -np.inf)[hit])
    ctx = rtc.make_context()
    for recs, ref, occluded in ((rays, want, False), (iq.occ_of(rtc, rays), wocc, True)):  # pitch 96, base 4-byte aligned: load_ray<false>
        view = _strided_device_copy(torch, recs)
        (L.rtcOccluded1M if occluded else L.rtcIntersect1M)(top.handle, C.byref(ctx), view.data_ptr(), m, 96)
        dev.check("strided batch")
        torch.cuda.synchronize()
        sz = recs.dtype.itemsize
        assert view[:, :sz].contiguous().cpu().numpy().tobytes() == ref.tobytes()
    # host batches: above tunePipeMinRays (pipelined) and below it (staged; <= 512 rays: traced in place)
    h = iq.copy(rtc, rays)
    top.intersect1M(h)
    assert h.tobytes() == want.tobytes()
    s, so = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    top.intersect1M(s[:9000])
    top.occluded1M(so[:9000])
    for a in range(9000, 10000, 500):
        top.intersect1M(s[a:a + 500])
        top.occluded1M(so[a:a + 500])
    assert s[:10000].tobytes() == want[:10000].tobytes() and so[:10000].tobytes() == wocc[:10000].tobytes()
    ho = iq.occ_of(rtc, rays)
    top.occluded1M(ho)
    assert ho.tobytes() == wocc.tobytes()
    k = 64  # rtcIntersect1 / rtcOccluded1
    one, o1 = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    for i in range(k):
        top.intersect1(one[i:i + 1])
        top.occluded1(o1[i:i + 1])
    assert one[:k].tobytes() == want[:k].tobytes() and o1[:k].tobytes() == wocc[:k].tobytes()
    # rtcIntersect1Mp / rtcOccluded1Mp: an array of pointers to records
    p, po_ = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    arr = (C.c_void_p * 256)(*[p[i:i + 1].ctypes.data for i in range(256)])
    L.rtcIntersect1Mp(top.handle, C.byref(ctx), arr, 256)
    dev.check("rtcIntersect1Mp")
    arr = (C.c_void_p * 256)(*[po_[i:i + 1].ctypes.data for i in range(256)])
    L.rtcOccluded1Mp(top.handle, C.byref(ctx), arr, 256)
    dev.check("rtcOccluded1Mp")
    assert p[:256].tobytes() == want[:256].tobytes() and po_[:256].tobytes() == wocc[:256].tobytes()
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
    isd.release(dev, top, inner)
    # two shards on one GPU: the accel is uploaded once per shard, a host batch is split between them
    dev, top, inner = isd.build(rtc, accel, meshes, inst, "gpus=0:0")
    g2, o2 = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    top.intersect1M(g2)
    top.occluded1M(o2)
    assert g2.tobytes() == want.tobytes() and o2.tobytes() == wocc.tobytes()
    isd.release(dev, top, inner)
    # service=1: no service kernel for instances, the call combiner serves the small calls; the answers are those of service=0
    dev, top, inner = isd.build(rtc, accel, meshes, inst, "service=1")
    g1, o1 = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    for a in range(0, 1024, 32):
        top.intersect1M(g1[a:a + 32])
        top.occluded1M(o1[a:a + 32])
    assert g1[:1024].tobytes() == want[:1024].tobytes() and o1[:1024].tobytes() == wocc[:1024].tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    isd.release(dev, top, inner)


# ---- 8. the rules across instanced scenes, on a device with a GPU --------------------------------------------------------------------------------
def test_mixed_compression_levels_are_refused_at_commit(rtc):
    dev = rtc.Device("subdiv_accel=" + isd.LEAF)
    log = []
    errfn = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda user, code, msg: log.append((code, (msg or b"").decode())))
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(errfn, C.c_void_p), None)
    a, b = isd.add_inner(rtc, dev, isd.cube() + (4, 2)), isd.add_inner(rtc, dev, isd.cube() + (4, 3))
    top = rtc.Scene(dev)
    top.add_instance(a, geom_id=3)
    top.add_instance(b, ih.affine((10, 0, 0)), geom_id=7)
    top.lib.rtcCommitScene(top.handle)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION
    assert log and "the scene of instance 7 has bvh4.compressed.leaf at compression level 3, the scene of instance 3 bvh4.compressed.leaf at compression level 2" in log[-1][1], log
    top.release(); a.release(); b.release(); dev.release()


def test_context_filter_and_counted_batches_stay_refused(rtc):
    dev, top, inner = isd.build(rtc, isd.EAGER, {"m": isd.cube() + (3, 1)}, isd.lattice_instances(2))
    log = []
    errfn = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda user, code, msg: log.append((code, (msg or b"").decode())))
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(errfn, C.c_void_p), None)
    rh = isd.crossing_rays(rtc, {"m": isd.cube() + (3, 1)}, isd.lattice_instances(2), 64, 3)
    src = rh.copy()
    fn = rtc.FILTER_FUNC(lambda args: None)
    ctx = rtc.make_context()
    ctx.filter = C.cast(fn, C.c_void_p)
    top.intersect1M(rh, ctx=ctx, check=False)
    assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION and "filter is not supported on a scene with instances" in log[-1][1], log
    with pytest.raises(rtc.RTCError):
        top.intersect1M_counted(rh)
    assert "counted batches are not supported on a scene with instances" in log[-1][1], log
    assert rh.tobytes() == src.tobytes()
    isd.release(dev, top, inner)
