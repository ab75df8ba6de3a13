"""Moving instances of subdivision scenes under time-dependent top-level boxes (inst_subdiv_bounds=linear, accel kinds 34 / 35), traced by
the TOPMB form of the subdivision two-level kernel (trace_instance_subdiv_top_linear.hip): a lane outside an instance reads QNodeMB8s.
Tree shape and box tests differ from the swept device's; a conservative box can only remove entries that find nothing, so the records
must be the swept device's byte for byte - except bvh4.compressed.leaf closest hits on rays that can meet several instances, which
depend on the visiting order (instance_subdiv_helpers.order_free_classes).  Scenes, instances and the host-side layout checks are those
of tests/instance_subdiv_top_linear_helpers.py and tests/test_host_instance_subdiv_top_linear.py."""
import ctypes as C

import numpy as np
import pytest

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
import instance_subdiv_helpers as isd
import instance_subdiv_top_linear_helpers as stl
import instance_top_linear_helpers as itl
from helpers import INVALID, fill_rays, random_rays_np

pytestmark = pytest.mark.gpu

RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL", "RTAMD_CBVH_FORM")
SMALL_SHARES = {"RTAMD_CHUNK": "32", "RTAMD_REFILL_BATCH": "1", "RTAMD_LEAF_BATCH": "64"}
TIMES8 = [k / 8.0 for k in (0, 3, 8, 1, 4, 6, 2, 7, 5)]


def _trace(rtc, dev, top, rays):
    got, occ = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    top.intersect1M(got)
    top.occluded1M(occ)
    assert dev.error() == 0  # (the overflow word stayed clear)
    return got, occ


def _pair(rtc, accel, meshes, inst):
    """the scene on a device without the key and on one with it; asserts the kinds"""
    swept, lin = stl.build_pair(rtc, accel, meshes, inst)
    assert swept[1].stats()["accelKind"] == isd.KIND[accel] and lin[1].stats()["accelKind"] == stl.KIND[accel]
    return swept, lin


def _same(a, b, what):
    (g0, o0), (g1, o1) = a, b
    assert g0.tobytes() == g1.tobytes(), f"{what}: {isd.differing(g0, g1)} hit records differ from the swept device's"
    assert o0.tobytes() == o1.tobytes(), f"{what}: {isd.differing(o0, o1)} occluded records differ from the swept device's"


# ---- 1. short rays under each motion pattern -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
@pytest.mark.parametrize("what", ["a", "b", "c", "d"])
def test_short_rays_equal_the_swept_device_and_the_direct_traces(rtc, accel, what):
    """fast translation, 90 degree rotation, out-and-back over 3 steps, 5-step zig-zag, each beside a static instance; ray times k / 8
    cycled.  Every record equals the swept device's.  The direct traces need world2local(time) and the local rays exact in fp32
    (instance_subdiv_helpers.direct asserts it): that holds at every k / 8 for the translations; the lerp of the rotation (b) has an
    exact inverse at the times 0, 1/2 and 1 only (its determinant is (1 - f)^2 + f^2), so there the direct leg takes the rays of these
    three times and the other six are held to the swept device alone."""
    meshes = {"m": stl.big_cube()}
    inst = itl.instances(what)
    rays, owner = isd.short_rays(rtc, meshes, inst, 3000, 9, times=TIMES8)
    isd.assert_cannot_reach_others(meshes, inst, rays, owner)
    swept, lin = _pair(rtc, accel, meshes, inst)
    rs, rl = _trace(rtc, swept[0], swept[1], rays), _trace(rtc, lin[0], lin[1], rays)
    hit = rl[0]["geomID"] != INVALID
    per_inst = np.bincount(owner[hit], minlength=len(inst))
    print(f"({what}) {accel}: {int(hit.sum())} hits of {len(rays)} rays, per instance {per_inst.tolist()}, {len(np.unique(rays['time'][hit]))} times")
    _same(rs, rl, f"({what}) {accel}")
    exact = np.isin(rays["time"], [0.0, 0.5, 1.0]) if what == "b" else np.ones(len(rays), bool)
    sub = iq.copy(rtc, rays[exact])
    inner = lin[2]
    want = isd.direct_owned(rtc, inner, inst, sub, owner[exact])
    wocc = isd.direct_owned(rtc, inner, inst, sub, owner[exact], occluded=True)
    assert rl[0][exact].tobytes() == want.tobytes(), f"{isd.differing(rl[0][exact], want)} records differ from the direct traces"
    assert rl[1][exact].tobytes() == wocc.tobytes(), f"{isd.differing(rl[1][exact], wocc)} occluded records differ from the direct traces"
    dhit = want["geomID"] != INVALID
    per_direct = np.bincount(owner[exact][dhit], minlength=len(inst))
    print(f"({what}) {accel}: direct leg on {int(exact.sum())} rays, hits per instance {per_direct.tolist()}, {int((~dhit).sum())} misses")
    assert per_direct.min() >= 50 and (~dhit).sum() >= 50 and per_inst.min() >= 50
    assert np.array_equal(want["instID"][dhit], np.array([g for g, _, _ in inst], np.uint32)[owner[exact][dhit]])
    assert len(np.unique(rays["time"][hit])) == 9
    for b in (swept, lin):
        isd.release(*b)


# ---- 2. crossing rays over a 4 x 5 lattice of moving cubes ---------------------------------------------------------------------------------------------
CROSS_SPACING, CROSS_RAYS = 64.0, 20000


def _moving_lattice():
    """instance_subdiv_helpers.lattice_instances(20) with a second step each: the same linear part, the translation moved by (2, -1, 1/2)
    times 1 + i % 3 - world2local(time) stays exact at the times k / 4"""
    out = []
    for g, k, (m,) in isd.lattice_instances(20, spacing=CROSS_SPACING):
        m1 = np.array(m, np.float32)
        m1[:, 3] += np.array([2.0, -1.0, 0.5], np.float32) * np.float32(1 + g % 3)
        out.append((g, k, [m, m1]))
    return out


def _crossing(rtc, meshes, inst):
    rays = isd.crossing_rays(rtc, meshes, inst, CROSS_RAYS, 7)
    rays["time"] = (np.arange(CROSS_RAYS) % 5 / 4.0).astype(np.float32)
    return rays


def test_crossing_rays_eager_equal_the_swept_device_and_the_merged_direct_traces(rtc):
    meshes = {"m": isd.cube() + (4, 2)}
    inst = _moving_lattice()
    rays = _crossing(rtc, meshes, inst)
    swept, lin = _pair(rtc, isd.EAGER, meshes, inst)
    per = isd.direct_all(rtc, lin[2], inst, rays)
    assert ih.equal_t_ties(per) == 0  # the two smallest t of every ray differ: no winner depends on the tree's shape
    want = isd.merge(rays, per, inst)
    rs, rl = _trace(rtc, swept[0], swept[1], rays), _trace(rtc, lin[0], lin[1], rays)
    hit = want["geomID"] != INVALID
    two = int((np.stack([p["geomID"] != INVALID for p in per]).sum(0) >= 2).sum())
    print(f"eager crossing rays: {int(hit.sum())} hits in {len(np.unique(want['instID'][hit]))} instances, {two} rays hit two or more")
    _same(rs, rl, "eager, crossing rays")
    assert rl[0].tobytes() == want.tobytes(), f"{isd.differing(rl[0], want)} records differ from the merged direct traces"
    assert np.array_equal(rl[1]["tfar"] == -np.inf, hit) and np.array_equal(rl[1]["tfar"][~hit], rays["tfar"][~hit])
    assert int(hit.sum()) > 1000 and len(np.unique(want["instID"][hit])) == 20
    for b in (swept, lin):
        isd.release(*b)


def test_crossing_rays_compressed_leaf_order_free_classes(rtc):
    meshes = {"m": isd.cube() + (4, 2)}
    inst = _moving_lattice()
    rays = _crossing(rtc, meshes, inst)
    swept, lin = _pair(rtc, isd.LEAF, meshes, inst)
    none, single, want = isd.order_free_classes(rtc, lin[2], inst, rays)
    print(f"compressed.leaf crossing rays: {int(none.sum())} hit nothing, {int(single.sum())} hit one instance only, {len(rays) - int((none | single).sum())} others")
    assert (none | single).sum() >= 0.95 * len(rays) and single.sum() >= 1000  # condition on the inputs, from the direct traces alone
    rs, rl = _trace(rtc, swept[0], swept[1], rays), _trace(rtc, lin[0], lin[1], rays)
    got, occ = rl
    assert got[none].tobytes() == rays[none].tobytes(), "compressed.leaf, rays that hit nothing"
    assert got[single].tobytes() == want[single].tobytes(), f"compressed.leaf, rays that hit one instance: {isd.differing(got[single], want[single])} differ"
    assert rs[0][none | single].tobytes() == got[none | single].tobytes()
    rest = ~(none | single)
    assert (got["geomID"][rest] != INVALID).all()  # some instance is hit whatever the order
    assert occ.tobytes() == isd.occluded_any(rtc, lin[2], inst, rays).tobytes(), "compressed.leaf, any hit"
    assert occ.tobytes() == rs[1].tobytes()
    assert np.all((occ["tfar"] == -np.inf)[got["geomID"] != INVALID])
    for b in (swept, lin):
        isd.release(*b)


# ---- 3. a fast mover -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_a_fast_mover_is_met_at_its_time_only(rtc, accel):
    """the cube moves by 40 along x over the shutter, beside a static one; 2048 rays from a sphere of radius 4 through the middle of where
    the mover is at time 0, ending before they reach any other place: at ray.time = 1 the records stay untouched, at time 0 every ray hits with the mover's instID"""
    meshes = {"m": isd.cube() + (4, 2)}
    inst = [(5, "m", [ih.affine((0, 0, 0)), ih.affine((40, 0, 0))]), (2, "m", [ih.affine((0, 20, 0))])]
    m = 2048
    rng = np.random.RandomState(5)
    u = rng.randn(m, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    org = ih.snap(4.0 * u)
    tgt = ih.snap((rng.rand(m, 3) - 0.5) * 0.5)
    rays = rtc.aligned_rayhits(m)
    fill_rays(rays, org, (tgt - org).astype(np.float32), tfar=2.0)  # t = 1 at the target: the rays end near the sphere, far from the other places
    swept, lin = _pair(rtc, accel, meshes, inst)
    for time, hits in ((1.0, False), (0.0, True)):
        rays["time"] = np.float32(time)
        rs, rl = _trace(rtc, swept[0], swept[1], rays), _trace(rtc, lin[0], lin[1], rays)
        _same(rs, rl, f"fast mover, {accel}, time {time}")
        got, occ = rl
        if hits:
            assert (got["geomID"] == 0).all() and (got["instID"] == 5).all() and (got["tfar"] < 1.0).all() and (occ["tfar"] == -np.inf).all()
        else:
            assert got.tobytes() == rays.tobytes() and occ.tobytes() == iq.occ_of(rtc, rays).tobytes()
    for b in (swept, lin):
        isd.release(*b)


# ---- 4. times outside the shutter ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_times_outside_the_shutter_equal_the_swept_device(rtc, accel):
    """ray.time = -0.5, 1.5 and NaN beside a valid 0.25: the node step clamps to the nearer end (NaN: 0), the instance entry is what it
    always was - it EXTRAPOLATES the transform (itime is clamped, ftime is not; a NaN gives a matrix that is not finite and the instance
    is not entered).  A ray at such a time therefore meets the instance, if at all, where no box of either device was made for: under
    swept boxes it enters wherever it crosses the union of the steps, under the key where it crosses the box of the nearer end, and what
    it then finds is decided by the extrapolated place alone.  The two devices give the same bytes exactly where no ray can reach that
    place, which is how the inputs are made: pattern (a) carries the cube from x in [1, 9] to [25, 33]; at time -0.5 it is at
    [-11, -3], at 1.5 at [37, 45]; every ray starts inside its instance's world box (x in [1, 33] for the mover) and ends 2.5 units
    further at most (directions have the largest component +-1), so it stays within x in [-1.5, 35.5].  What remains tested: the clamp
    (an unclamped NaN plane would lose the static instance's hits, an unclamped time would move no box of a static instance but the
    mover's), the valid rays among the others, and that nothing else is disturbed."""
    meshes = {"m": stl.big_cube()}
    inst = itl.instances("a")
    rng = np.random.RandomState(17)
    per = 2400
    recs = []
    for lo, hi in isd.world_boxes(meshes, inst):
        o = ih.snap(lo + rng.rand(per, 3) * (hi - lo))
        d = rng.randn(per, 3)
        d = (np.round(d / np.abs(d).max(1, keepdims=True) * 256.0) / 256.0).astype(np.float32)
        r = rtc.aligned_rayhits(per)
        fill_rays(r, o, d, tfar=2.5)
        recs.append(r)
    rays = iq.copy(rtc, np.concatenate(recs))
    times = np.array([-0.5, 1.5, np.nan, 0.25], np.float32)
    rays["time"] = times[np.arange(len(rays)) % 4]
    x_end = rays["org_x"] + rays["tfar"] * rays["dir_x"]
    assert min(rays["org_x"].min(), x_end.min()) > -3.0 and max(rays["org_x"].max(), x_end.max()) < 37.0  # nobody reaches the extrapolated places
    swept, lin = _pair(rtc, accel, meshes, inst)
    rs, rl = _trace(rtc, swept[0], swept[1], rays), _trace(rtc, lin[0], lin[1], rays)
    hit = rl[0]["geomID"] != INVALID
    per_time = [int(hit[k::4].sum()) for k in range(4)]
    on_mover = [int((hit & (rl[0]["instID"] == 0))[k::4].sum()) for k in range(4)]
    print(f"{accel}: hits at times -0.5, 1.5, NaN, 0.25: {per_time}, of them on the mover {on_mover}")
    _same(rs, rl, f"times outside the shutter, {accel}")
    assert min(per_time) >= 50 and on_mover[:3] == [0, 0, 0] and on_mover[3] >= 10
    for b in (swept, lin):
        isd.release(*b)


# ---- 5. both keys together ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_mesh_instances_under_inst_bounds_linear_beside_subdivision_instances_under_the_key(rtc, bomberman, accel):
    """mesh instances under kind 32 / 33 beside subdivision instances under kind 34 / 35 in one top scene: the records of the device
    with neither key"""
    v, fs, fi = isd.bomberman_faces(bomberman, 32)
    meshes = {"sub": (v, fs, fi, 3, 2)}
    sub_inst = [(10, "sub", [ih.affine((0, 0, 30)), ih.affine((6, 0, 30))]), (11, "sub", [ih.affine((0, 30, 30))])]
    scenes = {"m": itl.soup_scene(200, 100, 3)}
    mesh_inst = itl.instances("c")
    rays_mesh = imm.aimed_rays(rtc, scenes, mesh_inst, 2048, 41, denom=64)
    rays_sub = imm.aimed_rays(rtc, {"sub": imm.desc(tris=(v, None, 0))}, sub_inst, 2048, 43, denom=64)
    rays = iq.copy(rtc, np.concatenate([rays_mesh, rays_sub]))
    out = []
    for cfg in ("", itl.KEY + "," + stl.KEY):
        def extra(top, dev):
            m = imm.add_scene(rtc, dev, scenes["m"], 1)
            for gid, _, steps in mesh_inst:
                if len(steps) > 1:
                    assert top.add_instance_mb(m, steps, geom_id=gid) == gid
                else:
                    assert top.add_instance(m, steps[0], geom_id=gid) == gid
            return [m]

        dev, top, inner = isd.build(rtc, accel, meshes, sub_inst, cfg, extra)
        assert top.stats()["accelKind"] == (33 if cfg else 21)  # the mesh instance accel
        words = top.accel_data(3 + rtc.ACCEL_DATA_INSTSUBDIV).view(np.uint32)  # the second instance accel
        sub_nodes = top.accel_data(0 + rtc.ACCEL_DATA_INSTSUBDIV)
        if cfg:  # kind 34 / 35: four words, two sections
            assert len(words) == 4 and len(sub_nodes) == (int(words[3]) + int(words[2])) * 144 and words[2] >= 1
        else:
            assert len(words) == 2 and len(sub_nodes) > 0 and len(sub_nodes) % 96 == 0
        out.append(_trace(rtc, dev, top, rays))
        isd.release(dev, top, inner)
    _same(out[0], out[1], f"both keys, {accel}")
    got = out[1][0]
    hit = got["geomID"] != INVALID
    on_sub = np.isin(got["instID"][hit], [10, 11])
    print(f"{accel}: {int(hit.sum())} hits, {int(on_sub.sum())} below subdivision instances")
    assert on_sub.sum() > 100 and (~on_sub).sum() > 100


# ---- 6. every entry path ---------------------------------------------------------------------------------------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (ih.HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_entry_paths_are_bit_identical(rtc, bomberman, accel):
    """rtcIntersect1 / 4 / 8 / 16, 1M on host and device-resident records (aligned, and strided with a 4-byte aligned base: the VEC = false
    twins), 1Mp, NM, Np, small calls on a service=1 device, and the occluded twins: the records of rtcIntersect1M / rtcOccluded1M"""
    import torch
    meshes = {"m": isd.bomberman_faces(bomberman) + (3, 2)}
    inst = isd.lattice_instances(8)
    for i, to in ((5, (48.0, 41.0, 3.0)), (2, (70.0, 6.0, 2.0))):  # two of them move
        g, k, s = inst[i]
        inst[i] = (g, k, [s[0], ih.affine(to, (float(s[0][0, 0]),) * 3)])
    m = 4096
    rays = isd.crossing_rays(rtc, meshes, inst, m, 31)
    rays["time"] = (np.arange(m) % 5 / 4.0).astype(np.float32)
    dev, top, inner = isd.build(rtc, accel, meshes, inst, stl.KEY)
    assert top.stats()["accelKind"] == stl.KIND[accel]
    L = top.lib
    want, wocc = _trace(rtc, dev, top, rays)
    hit = want["geomID"] != INVALID
    print(f"{accel}: {int(hit.sum())} hits in {len(np.unique(want['instID'][hit]))} instances")
    assert int(hit.sum()) > 300 and len(np.unique(want["instID"][hit])) >= 6 and len(np.unique(rays["time"][hit])) == 5
    assert np.all((wocc["tfar"] == -np.inf)[hit])
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()  # device-resident
    top.intersect1M(t)
    to = torch.from_numpy(iq.occ_of(rtc, rays).view(np.uint8).reshape(-1, 48).copy()).cuda()
    top.occluded1M(to)
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == want.tobytes() and to.cpu().numpy().tobytes() == wocc.tobytes()
    ctx = rtc.make_context()
    for recs, ref, occluded in ((rays, want, False), (iq.occ_of(rtc, rays), wocc, True)):  # pitch 96, base 4-byte aligned: load_ray<false>
        raw = torch.zeros(m * 96 + 16, dtype=torch.uint8, device="cuda")
        view = raw[4:4 + m * 96].view(m, 96)
        assert view.data_ptr() % 16 == 4
        sz = recs.dtype.itemsize
        view[:, :sz] = torch.from_numpy(recs.view(np.uint8).reshape(m, sz).copy()).cuda()
        (L.rtcOccluded1M if occluded else L.rtcIntersect1M)(top.handle, C.byref(ctx), view.data_ptr(), m, 96)
        dev.check("strided batch")
        torch.cuda.synchronize()
        assert view[:, :sz].contiguous().cpu().numpy().tobytes() == ref.tobytes()
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
        fi, fo = getattr(L, f"rtcIntersect{width}"), getattr(L, f"rtcOccluded{width}")
        for fn in (fi, fo):
            fn.restype = None
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        valid = np.full(width, -1, np.int32)
        for a in range(0, 64, width):
            pk = _soa(rays[a:a + width], width, True)
            fi(valid.ctypes.data, top.handle, C.addressof(ctx), pk.ctypes.data)
            dev.check(f"rtcIntersect{width}")
            assert np.array_equal(pk, _soa(want[a:a + width], width, True))
            pk = _soa(rays[a:a + width], width, False)
            fo(valid.ctypes.data, top.handle, C.addressof(ctx), pk.ctypes.data)
            dev.check(f"rtcOccluded{width}")
            assert np.array_equal(pk, _soa(wocc[a:a + width], width, False))
    nfields = len(RAYF) + len(ih.HITF)
    for name, with_hit, ref in (("rtcIntersect", True, want), ("rtcOccluded", False, wocc)):
        nf = nfields if with_hit else len(RAYF)
        nm = getattr(L, name + "NM")
        nm.restype = None
        nm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_size_t]
        packs = np.stack([_soa(rays[a:a + 4], 4, with_hit) for a in range(0, 64, 4)])  # [16, fields, 4]
        nm(top.handle, C.addressof(ctx), packs.ctypes.data, 4, 16, nf * 4 * 4)
        dev.check(name + "NM")
        assert np.array_equal(packs, np.stack([_soa(ref[a:a + 4], 4, with_hit) for a in range(0, 64, 4)]))
        comp = _soa(rays, 64, with_hit)  # one array per component
        ptrs = (C.c_void_p * nf)(*[comp[i].ctypes.data for i in range(nf)])
        npf = getattr(L, name + "Np")
        npf.restype = None
        npf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
        npf(top.handle, C.addressof(ctx), C.addressof(ptrs), 64)
        dev.check(name + "Np")
        assert np.array_equal(comp, _soa(ref, 64, with_hit))
    isd.release(dev, top, inner)
    # service=1: no service kernel for instances, the call combiner serves the small calls; the answers are those of service=0
    dev, top, inner = isd.build(rtc, accel, meshes, inst, stl.KEY + ",service=1")
    assert top.stats()["accelKind"] == stl.KIND[accel]
    g1, o1 = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    for a in range(0, 1024, 32):
        top.intersect1M(g1[a:a + 32])
        top.occluded1M(o1[a:a + 32])
    assert g1[:1024].tobytes() == want[:1024].tobytes() and o1[:1024].tobytes() == wocc[:1024].tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    isd.release(dev, top, inner)


# ---- 7. overflow area ------------------------------------------------------------------------------------------------------------------------------------------------
def _knobs(monkeypatch, knobs):
    """the tuning knobs are read when a device is created"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_needle_patches_under_moving_deep_instances_spill_to_hbm(rtc, monkeypatch, accel):
    """the scene of test_gpu_instance_subdiv_deep_stack.py with a second step for each of the three overlapping instances.  The host walk
    (no primitive tests: the walk of a ray that hits nothing) shows that misses among the sampled rays write slots beyond the 16 in
    LDS and none beyond what the host reserved; `overflow` stays clear; eager bytes equal the swept device and the merged direct
    traces, compressed.leaf is checked on the order-free classes; small queue shares repeat the bytes."""
    _knobs(monkeypatch, {})
    meshes, inst = stl.needle_meshes(), stl.deep_moving_instances()
    lo, hi = isd.world_boxes(meshes, [(g, k, s[:1]) for g, k, s in inst])[0]
    n, sample = 8000, 100
    org, dirs = random_rays_np(n, lo.astype(np.float32), hi.astype(np.float32), ds.GPU_RAY_SEED)
    rays = ds.rays_of(rtc, ds.snap(org), ih.snap(dirs * 4.0))  # origins and directions on the 2^-10 grid: the local rays are exact
    rays["time"] = np.asarray(ds.TIMES, np.float32)[np.arange(n) % len(ds.TIMES)]
    swept, lin = _pair(rtc, accel, meshes, inst)
    dev, top, inner = lin
    st = top.stats()
    assert ds.stack_capacity(st["maxDepth"]) > ds.LDS_STACK
    rs, rl = _trace(rtc, swept[0], swept[1], rays), _trace(rtc, dev, top, rays)
    got, occ = rl
    assert dev.error() == 0
    o = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1)[:sample]
    d = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1)[:sample]
    deepest = stl.simulate_stack(top, rtc, len(inst), o, d, rays["time"][:sample])
    miss = got["geomID"][:sample] == INVALID
    deep = int((miss & (deepest >= ds.LDS_STACK)).sum())
    print(f"{accel}: maxDepth {st['maxDepth']}, {int(miss.sum())} of {sample} sampled rays miss, {deep} of them pass slot {ds.LDS_STACK}, deepest slot {int(deepest.max())}")
    assert deep >= sample // 10 and deepest.max() < ds.stack_capacity(st["maxDepth"])
    hit = got["geomID"] != INVALID
    if accel == isd.EAGER:
        _same(rs, rl, "needle patches, eager")
        per = isd.direct_all(rtc, inner, inst, rays)
        assert ih.equal_t_ties(per) == 0
        want = isd.merge(rays, per, inst)
        assert got.tobytes() == want.tobytes(), f"{isd.differing(got, want)} records differ from the merged direct traces"
        assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    else:
        none, single, want = isd.order_free_classes(rtc, inner, inst, rays)
        print(f"{accel}: {int(none.sum())} rays hit nothing, {int(single.sum())} one instance only")
        assert got[none].tobytes() == rays[none].tobytes() and got[single].tobytes() == want[single].tobytes()
        assert rs[0][none | single].tobytes() == got[none | single].tobytes()
        assert none.sum() >= 100 and single.sum() >= 100
        assert occ.tobytes() == isd.occluded_any(rtc, inner, inst, rays).tobytes() and occ.tobytes() == rs[1].tobytes()
    per_inst = [int((got["instID"][hit] == g).sum()) for g, _, _ in inst]
    print(f"{accel}: {int(hit.sum())} hits, per instance {per_inst}")
    assert int(hit.sum()) > 400 and min(per_inst) > 20
    for b in (swept, lin):
        isd.release(*b)
    # ... and with small queue shares, lanes refilled one at a time and leaves that wait for a full wave
    _knobs(monkeypatch, SMALL_SHARES)
    dev, top, inner = isd.build(rtc, accel, meshes, inst, stl.KEY)
    g2, o2 = _trace(rtc, dev, top, rays)
    assert g2.tobytes() == got.tobytes() and o2.tobytes() == occ.tobytes(), "small shares differ"
    isd.release(dev, top, inner)


# ---- 8. invalid rays ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_invalid_rays_leave_the_others_alone(rtc, bomberman, accel):
    """after test_gpu_instance_subdiv_edge_rays.py, where the argument why no poisoned field forms an out-of-range index is written down;
    what the TOPMB form adds: ray.time reaches the node step only through fminf(fmaxf(time, 0), 1) - a NaN becomes 0, an infinity an
    end - and picks no address; a lane outside an instance indexes QNodeMB8s by references of the top-level tree alone."""
    import edge_rays_helpers as er
    meshes = {"m": isd.bomberman_faces(bomberman) + (3, 2)}
    inst = isd.lattice_instances(9)
    g, k, s = inst[4]
    inst[4] = (g, k, [s[0], ih.affine((45.0, 38.0, 2.0), (1.0,) * 3), ih.affine((50.0, 44.0, -1.0), (1.0,) * 3)])
    dev, top, inner = isd.build(rtc, accel, meshes, inst, stl.KEY)
    assert top.stats()["accelKind"] == stl.KIND[accel]
    n = 10_000
    clean = er.with_times(isd.crossing_rays(rtc, meshes, inst, n, 91))
    want = iq.copy(rtc, clean)
    top.intersect1M(want)
    nh = int((want["geomID"] != INVALID).sum())
    print(f"invalid rays, {accel}: {nh} hits of the clean batch in {len(np.unique(want['instID'][want['geomID'] != INVALID]))} instances")
    assert nh > 250
    bad = np.arange(100, n, 1001)  # ten rays
    assert len(bad) == 10
    fields = ["org_x", "dir_y", "tnear", "tfar", "dir_z", "org_z", "time", "time", "time", "time"]
    values = [np.nan, np.nan, np.nan, np.nan, np.inf, -np.inf, np.nan, np.inf, -3.0, 7.0]

    def poison(recs):
        for j, i in enumerate(bad):
            recs[fields[j]][i] = values[j]
        recs["dir_x"][bad[-1]] = recs["dir_y"][bad[-1]] = recs["dir_z"][bad[-1]] = 0.0  # null direction
        recs["tnear"][bad[-2]], recs["tfar"][bad[-2]] = 5.0, 1.0  # inverted range

    dirty = iq.copy(rtc, clean)
    poison(dirty)
    top.intersect1M(dirty)
    keep = np.ones(n, bool)
    keep[bad] = False
    assert dirty[keep].tobytes() == want[keep].tobytes()
    assert dirty["geomID"][bad[-2]] == INVALID and dirty["tfar"][bad[-2]] == 1.0  # skipped
    wocc = iq.occ_of(rtc, clean)
    top.occluded1M(wocc)
    occ = iq.occ_of(rtc, clean)
    poison(occ)
    top.occluded1M(occ)
    assert occ[keep].tobytes() == wocc[keep].tobytes()
    assert occ["tfar"][bad[-2]] == 1.0
    assert np.all((wocc["tfar"] == -np.inf)[want["geomID"] != INVALID])
    assert dev.error() == 0
    isd.release(dev, top, inner)
