"""Single-level instancing (RTC_GEOMETRY_TYPE_INSTANCE) traced by the two-level kernel of trace_instance.hip.

The oracle has no instancing: the expected records come from po.TriangleScene on the local mesh, once per instance, with that
instance's local rays, merged by smallest t (tests/instance_helpers.py).  The exact-parity tests make the local rays exact by
construction: vertices and ray origins on the 2^-10 grid, translations on that grid, uniform power-of-two scales, no rotations - the
local origin (o - t) / s and direction d / s are then exactly representable in fp32 whatever the operation order (asserted in float64)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import instance_helpers as ih
from helpers import INVALID, compare_hits, fill_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")
ROBUST = 4
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]


def _flags(mode):
    return ROBUST if mode == 0 else 0  # mode 0: Pluecker / robust (kind 14), mode 1: Moeller / fast (kind 15)


@pytest.fixture(scope="module")
def mesh(bomberman_tris):
    v, tris = bomberman_tris
    assert len(tris) == 1454
    s = ih.snap(v * ih.SCALE)
    assert np.abs(s).max() < 16
    return s, tris


def _build(rtc, mode, meshes, instances, cfg="", extra=None):
    """top scene of `instances` [(geomID, mesh key, l2w)] over one instanced scene per mesh key; extra(top) adds other geometry"""
    dev = rtc.Device(cfg)
    inner = {}
    for key, (v, t, gid) in meshes.items():
        sc = rtc.Scene(dev, _flags(mode))
        sc.add_triangles(v, t, geom_id=gid)
        sc.commit()
        inner[key] = sc
    top = rtc.Scene(dev, _flags(mode))
    for gid, key, l2w in instances:
        assert top.add_instance(inner[key], l2w, geom_id=gid) == gid
    if extra:
        extra(top)
    top.commit()
    return dev, top, inner


def _release(dev, top, inner):
    top.release()
    for s in inner.values():
        s.release()
    dev.release()


def _copy(rtc, rays):
    out = rtc.aligned_rayhits(len(rays))  # 16-byte aligned (rtcIntersect1 contract)
    out[:] = rays
    return out


def _occ_of(rtc, rays):
    occ = rtc.aligned_rays(len(rays))
    for f in occ.dtype.names:
        occ[f] = rays[f]
    return occ


def _grid_instances(n):
    """n instances on the 2^-10 grid: translations on a lattice with spacing 40 (a scaled-by-two copy spans < 62), scales 1/2, 1, 2"""
    out = []
    for i in range(n):
        s = (0.5, 1.0, 2.0)[i % 3]
        # (every component differs from instance to instance: the mesh has large axis-aligned faces, and two overlapping copies with
        # a common coordinate would share a plane - and rays that hit both at the same t)
        t = (40.0 * (i % 4) + 0.125 * i, 40.0 * ((i // 4) % 5) + 5.0 / 1024.0 * i, 40.0 * (i // 20) + 1.0 / 1024.0 * i)
        out.append((i, "m", ih.affine(t, (s, s, s))))
    return out


# ---- closed form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_closed_form_translation_and_scale(rtc, mode):
    tri = np.array([[-1, -1, 0], [3, -1, 0], [-1, 3, 0]], np.float32)
    meshes = {"m": (tri, np.array([[0, 1, 2]], np.uint32), 0)}
    # instance 5: moved to z = 2; instance 9: scaled by 2 about the origin and moved by x = 100 (its plane stays z = 0)
    inst = [(5, "m", ih.affine((0, 0, 2))), (9, "m", ih.affine((100, 0, 0), (2, 2, 2)))]
    dev, top, inner = _build(rtc, mode, meshes, inst)
    assert top.stats()["accelKind"] == (14 if mode == 0 else 15)
    n = 128
    rng = np.random.RandomState(3)
    xy = ih.snap(rng.rand(n, 2) * 0.9 + 0.05)  # on the 2^-10 grid: the ray-relative vertices of the Pluecker test are then exact, Ng the same for every ray
    second = np.arange(n) % 2 == 1
    org = np.stack([xy[:, 0] + np.where(second, 100.0, 0.0), xy[:, 1], np.full(n, -1.0)], 1).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(np.array([0, 0, 1], np.float32), (n, 1)))
    # the local normal: mode 0 stable_triangle_normal of (v2 - v0, v0 - v1, v1 - v2), mode 1 cross(v2 - v0, v0 - v1): both (0, 0, -16)
    sc1 = rtc.Scene(dev, _flags(mode))
    sc1.add_triangles(tri, np.array([[0, 1, 2]], np.uint32))
    sc1.commit()
    loc = rtc.aligned_rayhits(1)
    fill_rays(loc, np.array([[0.5, 0.5, -1.0]], np.float32), np.array([[0, 0, 1]], np.float32))
    sc1.intersect1M(loc)
    ng = (loc["Ng_x"][0], loc["Ng_y"][0], loc["Ng_z"][0])
    assert loc["geomID"][0] == 0 and ng[0] == 0 and ng[1] == 0 and ng[2] != 0
    top.intersect1M(rh, ctx=rtc.make_context(inst_id=77))  # the context's instID is replaced by the instance's
    assert (rh["geomID"] == 0).all() and (rh["primID"] == 0).all()
    assert np.array_equal(rh["instID"], np.where(second, 9, 5).astype(np.uint32))
    assert np.array_equal(rh["tfar"], np.where(second, 1.0, 3.0).astype(np.float32))  # exact: t = (z_plane + 1) / 1
    assert (rh["Ng_x"] == ng[0]).all() and (rh["Ng_y"] == ng[1]).all() and (rh["Ng_z"] == ng[2]).all()  # Ng stays local (scale 2 would make it 4x)
    occ = _occ_of(rtc, rh)
    occ["tfar"] = np.where(np.arange(n) % 4 < 2, np.inf, 0.5).astype(np.float32)  # the short ones end in front of the planes
    top.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, np.arange(n) % 4 < 2) and (occ["tfar"][np.arange(n) % 4 >= 2] == 0.5).all()
    sc1.release()
    _release(dev, top, inner)


# ---- exact parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 9, 200])
def test_exact_parity_on_the_grid(rtc, po, mesh, n, mode):
    meshes = {"m": (mesh[0], mesh[1], 0)}
    inst = _grid_instances(n)
    rays = ih.general_rays(rtc, po, meshes, inst, snapped=True, m=8192, seed=100 + n)
    want, per = ih.oracle_instances(rtc, po, meshes, inst, rays, mode, exact=True)
    assert ih.equal_t_ties(per) == 0
    dev, top, inner = _build(rtc, mode, meshes, inst)
    got = rtc.aligned_rayhits(len(rays))
    got[:] = rays
    top.intersect1M(got)
    nh = compare_hits(got, want, what=f"{n} instances, mode {mode}")
    assert nh > (200 if n > 2 else 1000), nh
    hit = want["geomID"] != INVALID
    assert set(np.unique(want["instID"][hit]).tolist()) <= set(range(n)) and (got["instID"][~hit] == INVALID).all()
    occ = _occ_of(rtc, rays)
    top.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, hit)
    assert np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    _release(dev, top, inner)


# ---- general transforms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_general_transforms(rtc, po, mesh, mode):
    meshes = {"m": (mesh[0], mesh[1], 0)}
    inst = ih.general_instances()
    rays = ih.general_rays(rtc, po, meshes, inst)
    want, per = ih.oracle_instances(rtc, po, meshes, inst, rays, mode)
    aside = ih.set_aside(want, per)
    hits = int((want["geomID"] != INVALID).sum())
    assert aside.sum() <= 0.005 * hits  # the cap pinned on the CPU (test_host_instances.py)
    dev, top, inner = _build(rtc, mode, meshes, inst)
    # the library's world-to-local is the documented one (inverse in double precision, rounded once), bit for bit: the oracle's local
    # rays are then the kernel's
    for r in top.accel_data(2).view(ih.INST_DT):
        assert np.array_equal(r["world2local"].reshape(4, 3).T, ih.world2local(inst[int(r["geomID"])][2]))
    got = rtc.aligned_rayhits(len(rays))
    got[:] = rays
    top.intersect1M(got)
    keep = ~aside
    compare_hits(got[keep], want[keep], what=f"general transforms, mode {mode}")
    # a ray set aside is still a miss, or a hit within 1e-4 in t of SOME instance's oracle hit
    for k in np.nonzero(aside)[0]:
        if got["geomID"][k] == INVALID:
            assert got["tfar"][k] == rays["tfar"][k]
            continue
        ts = [float(p["tfar"][k]) for p in per if p["geomID"][k] != INVALID]
        assert any(abs(float(got["tfar"][k]) - t) <= 1e-4 * abs(t) for t in ts), (k, got[k], ts)
    occ = _occ_of(rtc, rays)
    top.occluded1M(occ)
    assert np.array_equal((occ["tfar"] == -np.inf)[keep], (want["geomID"] != INVALID)[keep])
    _release(dev, top, inner)


# ---- mixed scene: instances next to a triangle mesh and a quad mesh ---------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_mixed_scene_closest_hit_wins_across_accels(rtc, mode):
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    meshes = {"m": (sq, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), 0)}
    # the instanced unit square at z = 2 over x in [0, 4) (four instances, geomIDs 10..13)
    inst = [(10 + i, "m", ih.affine((float(i), 0, 2))) for i in range(4)]

    def extra(top):
        # a top-level triangle mesh (geomID 1) at z = 1 over x in [0, 1) and at z = 3 over x in [1, 2); a quad (geomID 2) at z = 1 over [2, 3) and z = 3 over [3, 4)
        v = np.concatenate([sq + (0, 0, 1), sq + (1, 0, 3)]).astype(np.float32)
        top.add_triangles(v, np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.uint32), geom_id=1)
        q = np.concatenate([sq + (2, 0, 1), sq + (3, 0, 3)]).astype(np.float32)
        top.add_quads(q, np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.uint32), geom_id=2)

    dev, top, inner = _build(rtc, mode, meshes, inst, extra=extra)
    n = 256
    rng = np.random.RandomState(5)
    x = (np.arange(n) % 4 + 0.1 + 0.8 * rng.rand(n)).astype(np.float32)  # away from the seams
    org = np.stack([x, (rng.rand(n) * 0.9 + 0.05), np.full(n, -1.0)], 1).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(np.array([0, 0, 1], np.float32), (n, 1)))
    for ctx_inst in (INVALID, 77):
        got = _copy(rtc, rh)
        top.intersect1M(got, ctx=rtc.make_context(inst_id=ctx_inst))
        cell = np.floor(x).astype(int)
        # cells 0 and 2: the top-level geometry at z = 1 is nearer; cells 1 and 3: the instance at z = 2 is
        assert np.array_equal(got["geomID"], np.array([1, 0, 2, 0], np.uint32)[cell])
        assert np.array_equal(got["instID"], np.where(cell % 2 == 1, 10 + cell, ctx_inst).astype(np.uint32))
        assert np.array_equal(got["tfar"], np.where(cell % 2 == 1, 3.0, 2.0).astype(np.float32))
    _release(dev, top, inner)


# ---- two instanced scenes, three instances each, geomIDs from rtcAttachGeometryByID ------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_shared_and_distinct_instanced_scenes(rtc, po, mesh, mode):
    v, tris = mesh
    meshes = {"a": (v, tris[0::2], 3), "b": (ih.snap(v * 0.5), tris[1::2], 7)}  # every other triangle; b at half size, instanced at scale 2
    inst = []
    for i in range(3):
        inst.append((20 + 2 * i, "a", ih.affine((40.0 * i, 0.5, 0), (1, 1, 1))))
        inst.append((41 - 3 * i, "b", ih.affine((40.0 * i + 0.25, 4.0, 1.0), (2, 2, 2))))
    rays = ih.general_rays(rtc, po, meshes, inst, snapped=True, m=8192, seed=77)
    want, per = ih.oracle_instances(rtc, po, meshes, inst, rays, mode, exact=True)
    assert ih.equal_t_ties(per) == 0
    dev, top, inner = _build(rtc, mode, meshes, inst)
    got = rtc.aligned_rayhits(len(rays))
    got[:] = rays
    top.intersect1M(got)
    assert compare_hits(got, want, what="two instanced scenes") > 500
    hit = got["geomID"] != INVALID
    assert set(np.unique(got["geomID"][hit]).tolist()) == {3, 7}
    assert set(np.unique(got["instID"][hit]).tolist()) == {g for g, _, _ in inst}
    assert ((got["instID"][hit] >= 35) == (got["geomID"][hit] == 7)).all()  # scene b's instances are 41, 38, 35
    _release(dev, top, inner)


# ---- a row of 64 instances, rays along the row ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_row_of_instances_rays_along_the_row(rtc, po, mesh, mode):
    meshes = {"m": (mesh[0], mesh[1], 0)}
    # spacing 3 along x: the boxes (about 30 wide) overlap their ten neighbours on either side
    # (y and z differ from copy to copy, or the copies' axis-aligned faces would share planes: equal-t hits on two instances)
    inst = [(i, "m", ih.affine((3.0 * i, i / 64.0, ((i * 7) % 64) / 128.0))) for i in range(64)]
    lo, hi = ih.instances_bounds(meshes, inst)
    m = 8192
    rng = np.random.RandomState(9)
    org = np.stack([np.full(m, lo[0] - 1.0), lo[1] + rng.rand(m) * (hi[1] - lo[1]), lo[2] + rng.rand(m) * (hi[2] - lo[2])], 1)
    org = ih.snap(org)
    d = np.stack([np.ones(m), (rng.rand(m) - 0.5) * 0.05, (rng.rand(m) - 0.5) * 0.05], 1).astype(np.float32)
    rays = rtc.aligned_rayhits(m)
    fill_rays(rays, org, d)
    want, per = ih.oracle_instances(rtc, po, meshes, inst, rays, mode, exact=True)
    assert ih.equal_t_ties(per) == 0
    dev, top, inner = _build(rtc, mode, meshes, inst)
    got = _copy(rtc, rays)
    top.intersect1M(got)   # a dropped stack entry would raise RTC_ERROR_UNKNOWN here
    dev.synchronize()
    assert compare_hits(got, want, what="row of 64") > 1000
    occ = _occ_of(rtc, rays)
    top.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, want["geomID"] != INVALID)
    _release(dev, top, inner)


# ---- every entry path gives the bytes of one device-resident rtcIntersect1M ------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (ih.HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_entry_paths_are_bit_identical(rtc, po, mesh, mode):
    import torch
    meshes = {"m": (mesh[0], mesh[1], 0)}
    inst = ih.general_instances()
    m = 40000
    rays = ih.general_rays(rtc, po, meshes, inst, m=m, seed=31)
    dev, top, inner = _build(rtc, mode, meshes, inst)
    L = top.lib
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    top.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    assert int((want["geomID"] != INVALID).sum()) > 5000
    to = torch.from_numpy(_occ_of(rtc, rays).view(np.uint8).reshape(-1, 48).copy()).cuda()
    top.occluded1M(to)
    torch.cuda.synchronize()
    wocc = to.cpu().numpy().reshape(-1).view(rtc.RAY_DTYPE)
    assert np.array_equal(wocc["tfar"] == -np.inf, want["geomID"] != INVALID)
    # host batch above tunePipeMinRays (pipelined) and below it (staged; <= 512 rays: traced in place)
    h = _copy(rtc, rays)
    top.intersect1M(h)
    assert h.tobytes() == want.tobytes()
    s = _copy(rtc, rays)
    top.intersect1M(s[:9000])
    for a in range(9000, 10000, 500):
        top.intersect1M(s[a:a + 500])
    assert s[:10000].tobytes() == want[:10000].tobytes()
    ho = _occ_of(rtc, rays)
    top.occluded1M(ho)
    assert ho.tobytes() == wocc.tobytes()
    # rtcIntersect1 / rtcOccluded1
    k = 64
    one = _copy(rtc, rays)
    o1 = _occ_of(rtc, rays)
    for i in range(k):
        top.intersect1(one[i:i + 1])
        top.occluded1(o1[i:i + 1])
    assert one[:k].tobytes() == want[:k].tobytes() and o1[:k].tobytes() == wocc[:k].tobytes()
    # rtcIntersect1Mp
    p = _copy(rtc, rays)
    arr = (C.c_void_p * 256)(*[p[i:i + 1].ctypes.data for i in range(256)])
    ctx = rtc.make_context()
    L.rtcIntersect1Mp(top.handle, C.byref(ctx), arr, 256)
    dev.check("rtcIntersect1Mp")
    assert p[:256].tobytes() == want[:256].tobytes()
    # a packet call
    fn = L.rtcIntersect8
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    valid = np.full(8, -1, np.int32)
    for a in range(0, 64, 8):
        pk = _soa(rays[a:a + 8], 8, True)
        fn(valid.ctypes.data, top.handle, C.addressof(ctx), pk.ctypes.data)
        dev.check("rtcIntersect8")
        assert np.array_equal(pk, _soa(want[a:a + 8], 8, True))
    _release(dev, top, inner)
    # two shards on one GPU, and service=1 (no service kernel for instances: the call combiner serves the small calls)
    for cfg, small in (("gpus=0:0", False), ("service=1", True)):
        dev, top, inner = _build(rtc, mode, meshes, inst, cfg)
        g = _copy(rtc, rays)
        if small:
            for a in range(0, 2048, 32):
                top.intersect1M(g[a:a + 32])
            assert g[:2048].tobytes() == want[:2048].tobytes()
            assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
        else:
            top.intersect1M(g)
            assert g.tobytes() == want.tobytes()
        _release(dev, top, inner)


# ---- updates ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_transform_update_matches_a_fresh_scene(rtc, po, mesh, mode):
    meshes = {"m": (mesh[0], mesh[1], 0)}
    inst = ih.general_instances()
    moved = [(g, k, ih.affine((m[0, 3] + 3.0, m[1, 3] - 2.0, m[2, 3]), (1.1, 0.9, 1.0), ih.rotation((0, 1, 0.3), 20.0 * g))) for g, k, m in inst]
    rays = ih.general_rays(rtc, po, meshes, inst, m=8192, seed=5)
    dev, top, inner = _build(rtc, mode, meshes, inst)
    before = _copy(rtc, rays)
    top.intersect1M(before)
    for g, _, m in moved:
        top.set_instance_transform(g, m)  # rtcSetGeometryTransform + rtcCommitGeometry
    top.commit()
    after = _copy(rtc, rays)
    top.intersect1M(after)
    dev2, fresh, inner2 = _build(rtc, mode, meshes, moved)
    want = _copy(rtc, rays)
    fresh.intersect1M(want)
    assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()
    assert int((want["geomID"] != INVALID).sum()) > 500
    _release(dev2, fresh, inner2)
    _release(dev, top, inner)


# ---- refused at the call --------------------------------------------------------------------------------------------------------------
def test_context_filter_and_counted_batches_are_refused(rtc, mesh):
    meshes = {"m": (mesh[0], mesh[1], 0)}
    dev, top, inner = _build(rtc, 1, meshes, [(0, "m", ih.affine())])
    log = []
    errfn = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda u, c, msg: log.append((c, msg.decode())))
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(errfn, C.c_void_p), None)
    rh = rtc.aligned_rayhits(64)
    fill_rays(rh, np.zeros((64, 3), np.float32), np.tile(np.array([0, 0, 1], np.float32), (64, 1)))
    src = rh.copy()
    fn = rtc.FILTER_FUNC(lambda args: None)
    ctx = rtc.make_context()
    ctx.filter = C.cast(fn, C.c_void_p)
    for call in (lambda: top.intersect1M(rh, ctx=ctx, check=False), lambda: top.occluded1M(_occ_of(rtc, rh), ctx=ctx, check=False)):
        call()
        assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION
        assert log and log[-1][0] == rtc.RTC_ERROR_INVALID_OPERATION and "filter is not supported on a scene with instances" in log[-1][1], log
    assert rh.tobytes() == src.tobytes()
    for counted in (top.intersect1M_counted, top.occluded1M_counted):
        with pytest.raises(rtc.RTCError) as e:
            counted(rh.copy() if counted == top.intersect1M_counted else _occ_of(rtc, rh))
        assert e.value.code == rtc.RTC_ERROR_INVALID_OPERATION
        assert "counted batches are not supported on a scene with instances" in log[-1][1], log
    _release(dev, top, inner)


# ---- the C example -------------------------------------------------------------------------------------------------------------------
def test_instance_example_runs(tmp_path):
    exe = str(tmp_path / "instance_min")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "instance_min.c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instance_min: ok" in out.stdout
