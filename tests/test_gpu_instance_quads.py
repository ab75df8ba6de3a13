"""Instanced scenes that hold quad meshes, alone or beside triangles (accel kinds 16 / 17), traced by the QUADS form of the two-level
kernel of trace_instance.hip.

Two legs (tests/instance_quads_helpers.py).  Leg 1, the oracle: per instance the local rays through po.TriangleScene for the scene's
triangles and then, on the same records, through the split-triangle scene of its quads, the B mapping applied, merged by smallest t.
Leg 2, no oracle arithmetic: for exact transforms (vertices, origins and translations on the 2^-10 grid, uniform power-of-two scales) the
instanced scene traced directly with the exact local rays - a plain scene, traced by the static triangle and quad kernels - is the
expected record of that instance, byte for byte apart from instID."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import instance_helpers as ih
import instance_quads_helpers as iq
from helpers import INVALID, compare_hits, fill_rays
from instance_helpers import LEAF, NODE_DT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
SQ = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
Q1 = np.array([[0, 1, 2, 3]], np.uint32)


def _kind(mode):
    return iq.ACCEL_INST_PLUECKER if mode == 0 else iq.ACCEL_INST_MOELLER


def _direct_leg(rtc, top, inner, inst, rays, what):
    """leg 2: the trace of `top` equals the merged direct traces byte for byte (instID: the instance's geomID); returns the records"""
    want, per = iq.direct_instances(rtc, inner, inst, rays)
    assert ih.equal_t_ties(per) == 0, what
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got.view(np.uint8).reshape(-1, 80) != want.view(np.uint8).reshape(-1, 80)).any(1).sum())} records differ"
    occ = iq.occ_of(rtc, rays)
    top.occluded1M(occ)
    hit = want["geomID"] != INVALID
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    return got


# ---- 1. closed form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_closed_form_translation_and_scale(rtc, mode):
    scenes = {"m": {"tris": None, "quads": (SQ, Q1, 0)}}
    # instance 5: moved to z = 2; instance 9: scaled by 2 about the origin and moved by x = 100 (its plane stays z = 0)
    inst = [(5, "m", ih.affine((0, 0, 2))), (9, "m", ih.affine((100, 0, 0), (2, 2, 2)))]
    dev, top, inner = iq.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == _kind(mode)
    n = 128
    rng = np.random.RandomState(3)
    # local points on the 2^-10 grid, half of them on either side of the v1-v3 diagonal x + y = 1 (and none within 1/64 of it)
    loc = ih.snap(rng.rand(n, 2) * 0.45 + 0.03)
    bside = np.arange(n) % 4 >= 2
    loc[bside] = 1.0 - loc[bside]
    second = np.arange(n) % 2 == 1
    org = np.stack([np.where(second, 2.0 * loc[:, 0] + 100.0, loc[:, 0]), np.where(second, 2.0 * loc[:, 1], loc[:, 1]), np.full(n, -1.0)], 1).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(np.array([0, 0, 1], np.float32), (n, 1)))
    # the local normal, from the instanced scene itself: one ray on A, one on B
    ref = rtc.aligned_rayhits(2)
    fill_rays(ref, np.array([[0.25, 0.25, -1.0], [0.75, 0.75, -1.0]], np.float32), np.array([[0, 0, 1], [0, 0, 1]], np.float32))
    inner["m"].intersect1M(ref)
    assert (ref["geomID"] == 0).all() and (ref["Ng_x"] == 0).all() and (ref["Ng_y"] == 0).all() and ref["Ng_z"][0] != 0
    assert ref["Ng_z"][0] == ref["Ng_z"][1]  # B's normal is negated: the quad has one orientation
    top.intersect1M(rh, ctx=rtc.make_context(inst_id=77))  # the context's instID is replaced by the instance's
    assert (rh["geomID"] == 0).all() and (rh["primID"] == 0).all()
    assert np.array_equal(rh["instID"], np.where(second, 9, 5).astype(np.uint32))
    assert np.array_equal(rh["tfar"], np.where(second, 1.0, 3.0).astype(np.float32))  # exact: t = (z_plane + 1) / 1
    assert (rh["Ng_x"] == 0).all() and (rh["Ng_y"] == 0).all() and (rh["Ng_z"] == ref["Ng_z"][0]).all()  # Ng stays local (scale 2 would make it 4x)
    # the quad's parametrisation on both sides of the diagonal: u = x, v = y of the local point (A: as computed; B: mapped back)
    # three roundings of at most 2^-24 each on values up to 1 (the division, and for B the subtraction from 1 or from absDen and the
    # product with the reciprocal): 1.8e-7, taken twice
    tol = 4e-7
    assert np.all(np.abs(rh["u"] - loc[:, 0]) <= tol) and np.all(np.abs(rh["v"] - loc[:, 1]) <= tol)
    assert ((rh["u"] + rh["v"] > 1) == bside).all() and bside.sum() == n // 2
    occ = iq.occ_of(rtc, rh)
    occ["tfar"] = np.where(np.arange(n) % 8 < 4, np.inf, 0.5).astype(np.float32)  # the short ones end in front of the planes
    top.occluded1M(occ)
    assert np.array_equal(occ["tfar"] == -np.inf, np.arange(n) % 8 < 4) and (occ["tfar"][np.arange(n) % 8 >= 4] == 0.5).all()
    iq.release(dev, top, inner)


# ---- 2. a triangle and a quad coincident inside the instanced scene -----------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_coincident_triangle_and_quad_inside_the_instance_return_the_quad(rtc, mode):
    scenes = {"m": {"tris": (SQ, np.array([[0, 1, 3]], np.uint32), 4), "quads": (SQ, Q1, 6)}}  # the triangle = triangle A of the quad
    inst = [(2, "m", ih.affine((8, 0, 1), (2, 2, 2)))]
    dev, top, inner = iq.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == _kind(mode)
    n = 64
    rng = np.random.RandomState(2)
    loc = ih.snap(rng.rand(n, 2) * 0.4 + 0.05)
    org = np.stack([2.0 * loc[:, 0] + 8.0, 2.0 * loc[:, 1], np.full(n, -1.0)], 1).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(np.array([0, 0, 1], np.float32), (n, 1)))
    tri_only = {"m": {"tris": scenes["m"]["tris"], "quads": None}}
    dev2, top2, inner2 = iq.build(rtc, mode, tri_only, inst)
    alone = iq.copy(rtc, rh)
    top2.intersect1M(alone)
    assert (alone["geomID"] == 4).all() and (alone["tfar"] == 2.0).all()
    top.intersect1M(rh)
    # traced after the triangles against the tfar they left: the depth test accepts the equal t, the quad's ids replace the triangle's
    assert (rh["geomID"] == 6).all() and (rh["primID"] == 0).all() and (rh["instID"] == 2).all()
    assert np.array_equal(rh["tfar"], alone["tfar"])
    iq.release(dev2, top2, inner2)
    iq.release(dev, top, inner)


# ---- 3. exact parity on the grid: bomberman's 727 quads --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 9])
def test_exact_parity_on_the_grid(rtc, po, bomberman, n, mode):
    scenes = iq.quads_only(bomberman)
    inst = iq.grid_instances(n)
    rays = ih.general_rays(rtc, po, iq.bounds_meshes(scenes), inst, snapped=True, m=iq.PARITY_RAYS, seed=iq.PARITY_SEED[n])
    want, per, isb, _ = iq.oracle_instances(rtc, po, scenes, inst, rays, mode, exact=True)
    assert ih.equal_t_ties(per) == 0
    dev, top, inner = iq.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == _kind(mode)
    got = _direct_leg(rtc, top, inner, inst, rays, f"{n} instances of quads, mode {mode}")  # leg 2, and occluded == hit mask
    # leg 1, with the allowances and caps of test_bomberman_quads_1m_parity
    hits = int((want["geomID"] != INVALID).sum())
    if mode == 1:  # Moeller B lanes: 1 - v_tri against (absDen - V) / absDen, ulps of 1 apart
        for f in ("u", "v"):
            assert np.all(np.abs(got[f][isb].astype(np.float64) - want[f][isb]) <= 4e-7 + 1e-4 * np.abs(want[f][isb]))
            want[f][isb] = got[f][isb]
    diag = iq.diagonal(want)
    assert int(diag.sum()) < hits // 100, int(diag.sum())
    for f in ("Ng_x", "Ng_y", "Ng_z"):
        want[f][diag] = got[f][diag]
    nh = compare_hits(got, want, what=f"{n} instances of quads, mode {mode}")
    assert nh > (200 if n > 2 else 1000), nh
    hit = want["geomID"] != INVALID
    assert set(np.unique(want["instID"][hit]).tolist()) <= set(range(n)) and (got["instID"][~hit] == INVALID).all()
    iq.release(dev, top, inner)


# ---- 4. triangles and quads in one instanced scene, two scenes that split the faces differently ------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_mixed_instanced_scenes(rtc, po, bomberman, mode):
    scenes = iq.mixed_scenes(bomberman)
    # (scales 1, 2, 2: at 8192 rays the half-size copies of the lattice would collect some 30 hits each, below the floor asserted here)
    inst = iq.grid_instances(6, keys=("a", "b"), scales=(1.0, 2.0, 2.0))
    rays = ih.general_rays(rtc, po, iq.bounds_meshes(scenes), inst, snapped=True, m=8192, seed=77)
    dev, top, inner = iq.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == _kind(mode)
    got = _direct_leg(rtc, top, inner, inst, rays, f"mixed scenes, mode {mode}")
    hit = got["geomID"] != INVALID
    for g in (3, 7):
        assert int((got["geomID"][hit] == g).sum()) > 100
    for i in range(6):
        assert int((got["instID"][hit] == i).sum()) > 100, i
    iq.release(dev, top, inner)


# ---- 5. quad leaves longer than one block ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_leaves_longer_than_one_block(rtc, po, mode):
    v, q = iq.overlapping_quads()
    scenes = {"m": {"tris": None, "quads": (v, q, 0)}}
    inst = [(i, "m", ih.affine((4.0 * i + 0.125 * i, 3.0 / 1024.0 * i, 0.5 * i), ((0.5, 1.0, 2.0)[i % 3],) * 3)) for i in range(3)]
    rays = ih.general_rays(rtc, po, iq.bounds_meshes(scenes), inst, snapped=True, m=4096, seed=13)
    dev, top, inner = iq.build(rtc, mode, scenes, inst)
    nodes, root = inner["m"].accel_data(0).view(NODE_DT), inner["m"].accel_root()
    refs = [root] if root & LEAF else [int(c) for nd in nodes for c in nd["child"] if c != 0xFFFFFFFF and c & LEAF]
    assert max((r >> 26) & 31 for r in refs) > 4
    got = _direct_leg(rtc, top, inner, inst, rays, f"long leaves, mode {mode}")
    assert int((got["geomID"] != INVALID).sum()) > 500
    iq.release(dev, top, inner)


# ---- 6. instances of a quad scene next to a top-level triangle mesh and a top-level quad mesh --------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_top_level_company_closest_hit_wins_across_accels(rtc, mode):
    scenes = {"m": {"tris": None, "quads": (SQ, Q1, 0)}}
    # the instanced unit quad at z = 2 over x in [0, 4) (four instances, geomIDs 10..13)
    inst = [(10 + i, "m", ih.affine((float(i), 0, 2))) for i in range(4)]

    def extra(top):
        # a top-level triangle mesh (geomID 1) at z = 1 over x in [0, 1) and at z = 3 over x in [1, 2); a quad mesh (geomID 2) at z = 1 over [2, 3) and z = 3 over [3, 4)
        v = np.concatenate([SQ + (0, 0, 1), SQ + (1, 0, 3)]).astype(np.float32)
        top.add_triangles(v, np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.uint32), geom_id=1)
        q = np.concatenate([SQ + (2, 0, 1), SQ + (3, 0, 3)]).astype(np.float32)
        top.add_quads(q, np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.uint32), geom_id=2)

    dev, top, inner = iq.build(rtc, mode, scenes, inst, extra=extra)
    n = 256
    rng = np.random.RandomState(5)
    x = (np.arange(n) % 4 + 0.1 + 0.8 * rng.rand(n)).astype(np.float32)  # away from the seams
    org = np.stack([x, (rng.rand(n) * 0.9 + 0.05), np.full(n, -1.0)], 1).astype(np.float32)
    rh = rtc.aligned_rayhits(n)
    fill_rays(rh, org, np.tile(np.array([0, 0, 1], np.float32), (n, 1)))
    for ctx_inst in (INVALID, 77):
        got = iq.copy(rtc, rh)
        top.intersect1M(got, ctx=rtc.make_context(inst_id=ctx_inst))
        cell = np.floor(x).astype(int)
        # cells 0 and 2: the top-level geometry at z = 1 is nearer; cells 1 and 3: the instance at z = 2 is
        assert np.array_equal(got["geomID"], np.array([1, 0, 2, 0], np.uint32)[cell])
        assert np.array_equal(got["instID"], np.where(cell % 2 == 1, 10 + cell, ctx_inst).astype(np.uint32))
        assert np.array_equal(got["tfar"], np.where(cell % 2 == 1, 3.0, 2.0).astype(np.float32))
    iq.release(dev, top, inner)


# ---- 7. general transforms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_general_transforms(rtc, po, bomberman, mode):
    scenes = iq.quads_only(bomberman)
    inst = iq.general_instances()
    rays = ih.general_rays(rtc, po, iq.bounds_meshes(scenes), inst, m=iq.GENERAL_RAYS, seed=iq.GENERAL_SEED)
    want, per, isb, want_tri = iq.oracle_instances(rtc, po, scenes, inst, rays, mode)
    aside = iq.quad_set_aside(want, per, want_tri, [0])
    hits = int((want["geomID"] != INVALID).sum())
    assert aside.sum() <= 0.01 * hits  # the cap, pinned on the CPU (test_host_instance_quads.py)
    dev, top, inner = iq.build(rtc, mode, scenes, inst)
    for r in top.accel_data(2)[:64 * len(inst)].view(ih.INST_DT):  # the documented world-to-local, bit for bit: the oracle's local rays are the kernel's
        assert np.array_equal(r["world2local"].reshape(4, 3).T, ih.world2local(inst[int(r["geomID"])][2]))
    got = iq.copy(rtc, rays)
    top.intersect1M(got)
    keep = ~aside
    if mode == 1:
        b = isb & keep
        for f in ("u", "v"):
            assert np.all(np.abs(got[f][b].astype(np.float64) - want[f][b]) <= 4e-7 + 1e-4 * np.abs(want[f][b]))
            want[f][b] = got[f][b]
    compare_hits(got[keep], want[keep], what=f"general transforms over quads, mode {mode}")
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


# ---- 8. every entry path gives the bytes of one device-resident rtcIntersect1M -----------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (ih.HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_entry_paths_are_bit_identical(rtc, po, bomberman, mode):
    import torch
    scenes = iq.mixed_scenes(bomberman)
    inst = iq.general_instances(keys=("a", "b"))
    m = 40000
    rays = ih.general_rays(rtc, po, iq.bounds_meshes(scenes), inst, m=m, seed=31)
    dev, top, inner = iq.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == _kind(mode)
    L = top.lib
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    top.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    hit = want["geomID"] != INVALID
    assert int(hit.sum()) > 5000 and int((want["geomID"] == 3).sum()) > 1000 and int((want["geomID"] == 7).sum()) > 1000
    to = torch.from_numpy(iq.occ_of(rtc, rays).view(np.uint8).reshape(-1, 48).copy()).cuda()
    top.occluded1M(to)
    torch.cuda.synchronize()
    wocc = to.cpu().numpy().reshape(-1).view(rtc.RAY_DTYPE)
    assert np.array_equal(wocc["tfar"] == -np.inf, hit)
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
    iq.release(dev, top, inner)
    # two shards on one GPU, and service=1 (no service kernel for instances: the call combiner serves the small calls)
    for cfg, small in (("gpus=0:0", False), ("service=1", True)):
        dev, top, inner = iq.build(rtc, mode, scenes, inst, cfg)
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


# ---- 9. refused at the call ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_context_filter_and_counted_batches_are_refused(rtc, bomberman, mode):
    scenes = iq.quads_only(bomberman)
    dev, top, inner = iq.build(rtc, mode, scenes, [(0, "m", ih.affine())])
    assert top.stats()["accelKind"] == _kind(mode)
    log = []
    errfn = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda u, c, msg: log.append((c, msg.decode())))
    dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(errfn, C.c_void_p), None)
    rh = rtc.aligned_rayhits(64)
    fill_rays(rh, np.zeros((64, 3), np.float32), np.tile(np.array([0, 0, 1], np.float32), (64, 1)))
    src = rh.copy()
    fn = rtc.FILTER_FUNC(lambda args: None)
    ctx = rtc.make_context()
    ctx.filter = C.cast(fn, C.c_void_p)
    occ = iq.occ_of(rtc, rh)
    osrc = occ.copy()
    for call in (lambda: top.intersect1M(rh, ctx=ctx, check=False), lambda: top.occluded1M(occ, ctx=ctx, check=False)):
        call()
        assert dev.error() == rtc.RTC_ERROR_INVALID_OPERATION
        assert log and log[-1][0] == rtc.RTC_ERROR_INVALID_OPERATION and "filter is not supported on a scene with instances" in log[-1][1], log
    for counted, recs, orig in ((top.intersect1M_counted, rh, src), (top.occluded1M_counted, occ, osrc)):
        with pytest.raises(rtc.RTCError) as e:
            counted(recs)
        assert e.value.code == rtc.RTC_ERROR_INVALID_OPERATION
        assert "counted batches are not supported on a scene with instances" in log[-1][1], log
    assert rh.tobytes() == src.tobytes() and occ.tobytes() == osrc.tobytes()  # records untouched
    iq.release(dev, top, inner)


# ---- 10. updates ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_transform_update_matches_a_fresh_scene(rtc, po, bomberman, mode):
    scenes = iq.mixed_scenes(bomberman)
    inst = iq.general_instances(keys=("a", "b"))
    moved = [(g, k, ih.affine((m[0, 3] + 3.0, m[1, 3] - 2.0, m[2, 3]), (1.1, 0.9, 1.0), ih.rotation((0, 1, 0.3), 20.0 * g))) for g, k, m in inst]
    rays = ih.general_rays(rtc, po, iq.bounds_meshes(scenes), inst, m=8192, seed=5)
    dev, top, inner = iq.build(rtc, mode, scenes, inst)
    before = iq.copy(rtc, rays)
    top.intersect1M(before)
    for g, _, m in moved:
        top.set_instance_transform(g, m)  # rtcSetGeometryTransform + rtcCommitGeometry
    top.commit()
    after = iq.copy(rtc, rays)
    top.intersect1M(after)
    dev2, fresh, inner2 = iq.build(rtc, mode, scenes, moved)
    want = iq.copy(rtc, rays)
    fresh.intersect1M(want)
    assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()
    assert int((want["geomID"] != INVALID).sum()) > 500
    iq.release(dev2, fresh, inner2)
    iq.release(dev, top, inner)


# ---- 11. the C example -------------------------------------------------------------------------------------------------------------------------
def test_instance_quads_example_runs(tmp_path):
    exe = str(tmp_path / "instance_quads_min")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "instance_quads_min.c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instance_quads_min: ok" in out.stdout
