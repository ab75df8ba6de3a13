"""Line segments and flat curves below an instance (device config inst_hair=1): the hair form of the two-level kernel
(embree-compressed_amd/csrc/trace_instance_hair.hip), kinds 22 / 23.

The byte-for-byte legs need no oracle arithmetic: with exact transforms (origins and translations on the 2^-10 grid, uniform power-of-two
scales) the instanced scene traced DIRECTLY with the exact local rays - a plain scene, traced by the line, curve and mesh kernels that
exist without instancing - is the expected record of that instance, apart from instID.  The general-transform leg is held to the float64
truth of the line and curve tests (restated in plain float64 in instance_hair_helpers) on the float64 local ray.  tests/instance_hair_helpers.py, tests/instance_subdiv_helpers.py."""
import ctypes as C

import numpy as np
import pytest

import curve_helpers as ch
import deep_stack_helpers as ds
import instance_hair_helpers as ihh
import instance_helpers as ih
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
import instance_subdiv_helpers as isd
import line_helpers as lh
from helpers import INVALID, fill_rays, random_rays_np, random_soup

pytestmark = pytest.mark.gpu

INST = isd.lattice_instances(6)  # power-of-two scales, grid translations: local rays are exact
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL", "RTAMD_CBVH_FORM")


def _check(got, want, what):
    assert got.tobytes() == want.tobytes(), f"{what}: {isd.differing(got, want)} of {len(got)} records differ"


def _trace_both(rtc, top, rays):
    got, occ = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    top.intersect1M(got)
    top.occluded1M(occ)
    return got, occ


# ---- 1. short rays, byte for byte ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["a", "b", "c", "d", "e"])
def test_short_rays_equal_the_instanced_scene_traced_directly(rtc, which, mode):
    scs = ihh.scenes(which)
    meshes = ihh.bounds_meshes(scs)
    times = [k / 8.0 for k in (0, 3, 8, 1, 4, 6, 2, 7, 5)] if which == "e" else None  # the dyadic grid
    rays, owner = isd.short_rays(rtc, meshes, INST, 300, 21 + ord(which), times=times)
    isd.assert_cannot_reach_others(meshes, INST, rays, owner)
    dev, top, inner = ihh.build(rtc, mode, scs, INST)
    assert top.stats()["accelKind"] == imm.kind(mode)
    got, occ = _trace_both(rtc, top, rays)
    want = isd.direct_owned(rtc, inner, INST, rays, owner)
    _check(got, want, f"({which}) mode {mode}, closest hit")
    _check(occ, isd.direct_owned(rtc, inner, INST, rays, owner, occluded=True), f"({which}) mode {mode}, any hit")
    hit = want["geomID"] != INVALID
    per_inst = np.bincount(owner[hit], minlength=len(INST))
    geoms = sorted(np.unique(want["geomID"][hit]).tolist())
    print(f"({which}) mode {mode}: {int(hit.sum())} hits of {len(rays)} rays, per instance {per_inst.tolist()}, geometries {geoms}")
    assert per_inst.min() >= 5 and np.array_equal(want["instID"][hit], np.array([g for g, _, _ in INST])[owner[hit]])
    d = scs["m"]
    expect = [g[4] for g in (d["curves"] or [])] + ([d["lines"][2]] if d["lines"] else [])
    assert set(expect) <= set(geoms), (expect, geoms)  # every hair geometry (every tessellation rate, both bases) is hit
    if which == "d":
        # a later tree wins a bit-identical t: rays along +z onto the axis-aligned squares, whose t is exact in the triangle and in the quad
        # test (everything dyadic) - the quads (geomID 2) come after the coincident triangles (geomID 1) and take the hit
        sq = np.asarray(d["quads"][0], np.float64).reshape(-1, 4, 3)
        local = sq.mean(1) + np.array([0.25, 0.125, -1.0])
        org = np.concatenate([ih.xfm_points(steps[0], local) for _, _, steps in INST])
        zr = rtc.aligned_rayhits(len(org))
        fill_rays(zr, org.astype(np.float32), np.tile(np.array([0, 0, 1], np.float32), (len(org), 1)), tfar=np.repeat([2.0 * steps[0][0][0] for _, _, steps in INST], len(local)).astype(np.float32))
        zowner = np.repeat(np.arange(len(INST)), len(local))
        isd.assert_cannot_reach_others(meshes, INST, zr, zowner)
        zgot = iq.copy(rtc, zr)
        top.intersect1M(zgot)
        _check(zgot, isd.direct_owned(rtc, inner, INST, zr, zowner), "(d) rays along +z")
        on_mesh = np.isin(zgot["geomID"], (1, 2))
        print(f"(d) mode {mode}: {int(on_mesh.sum())} of {len(zr)} rays along +z end on a square, {int((zgot['geomID'] == 2).sum())} of them on the quad")
        assert on_mesh.sum() >= len(zr) // 2 and (zgot["geomID"][on_mesh] == 2).all()
        assert np.array_equal(zgot["tfar"][on_mesh], np.repeat([float(steps[0][0][0]) for _, _, steps in INST], len(local)).astype(np.float32)[on_mesh])
    ihh.release(dev, top, inner)


# ---- 2. crossing rays ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_crossing_rays_equal_the_merged_direct_traces(rtc, mode):
    scs = ihh.scenes("c")
    meshes = ihh.bounds_meshes(scs)
    rays = isd.crossing_rays(rtc, meshes, INST, 2000, 7)
    dev, top, inner = ihh.build(rtc, mode, scs, INST)
    per = isd.direct_all(rtc, inner, INST, rays)
    # the condition: for no ray do two instances' direct hits lie within 1e-6 relative of each other (the lattice is disjoint)
    t = np.sort(np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf).astype(np.float64) for p in per]), axis=0)
    both = np.isfinite(t[1])
    assert np.all(t[1][both] - t[0][both] > 1e-6 * np.abs(t[0][both]))
    want = isd.merge(rays, per, INST)
    got, occ = _trace_both(rtc, top, rays)
    _check(got, want, f"crossing rays, mode {mode}")
    _check(occ, isd.occluded_any(rtc, inner, INST, rays), f"crossing rays, mode {mode}, any hit")
    hit = want["geomID"] != INVALID
    print(f"crossing rays, mode {mode}: {int(hit.sum())} hits in {len(np.unique(want['instID'][hit]))} instances, {int(both.sum())} rays hit two or more")
    assert int(hit.sum()) >= 100 and len(np.unique(want["instID"][hit])) == len(INST)
    ihh.release(dev, top, inner)


# ---- 3. moving instances -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_moving_instances_equal_the_static_instance_at_the_rays_time(rtc, mode):
    """instances with 2 and 3 transform steps (signed axis permutations, power-of-two scales, translations on the grid: world2local(time)
    is exact, which instance_subdiv_helpers.direct asserts), ray times k / 8 and two times outside [0, 1]: byte for byte.
    A time outside [0, 1] extrapolates the transform (still exact) while the instance's box in the top scene is the union over its steps,
    so such a ray may pass the instance by.  Decided on the host: where the direct trace's hit point lies inside that union box (the
    instanced scene's bounds under every step, shrunk by 1e-3 of its extent for the builder's float32 corners) the segment [tnear, tfar]
    meets every box above the instance, the ray enters it and its record must be the direct trace's, for closest and any hit; a ray the
    direct trace misses comes back untouched; only a ray whose direct hit lies outside the union box may come back either way."""
    scs = ihh.scenes("c")
    meshes = ihh.bounds_meshes(scs)
    inst = [(g, k, s[:3]) for g, k, s in im.exact_instances(6)]
    assert sorted({len(s) for _, _, s in inst}) == [2, 3]
    rays, owner = isd.short_rays(rtc, meshes, inst, 300, 9, times=[k / 8.0 for k in (0, 3, 8, 1, 4, 6, 2, 7, 5, -2, 11)])
    isd.assert_cannot_reach_others(meshes, inst, rays, owner)
    dev, top, inner = ihh.build(rtc, mode, scs, inst)
    assert top.stats()["accelKind"] == imm.kind(mode)
    got, occ = _trace_both(rtc, top, rays)
    want, wocc = isd.direct_owned(rtc, inner, inst, rays, owner), isd.direct_owned(rtc, inner, inst, rays, owner, occluded=True)
    inside = (rays["time"] >= 0) & (rays["time"] <= 1)
    out, whit = ~inside, want["geomID"] != INVALID
    o = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1).astype(np.float64)
    d = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1).astype(np.float64)
    point = o + want["tfar"].astype(np.float64)[:, None] * d  # (of the direct hit; used where there is one)
    in_box = np.zeros(len(rays), bool)
    for i, (_, key, steps) in enumerate(inst):
        lo, hi = (x.astype(np.float64) for x in inner[key].bounds())
        corners = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)])
        w = np.concatenate([ih.xfm_points(m, corners) for m in steps])
        blo, bhi = w.min(0), w.max(0)
        margin = 1e-3 * (bhi - blo)
        in_box |= (owner == i) & whit & ((point >= blo + margin) & (point <= bhi - margin)).all(1)
    must = inside | ~whit | in_box
    _check(got[must], want[must], f"moving instances, mode {mode}")
    _check(occ[must], wocc[must], f"moving instances, mode {mode}, any hit")
    same = lambda a, b: (a.view(np.uint8).reshape(-1, a.dtype.itemsize) == b.view(np.uint8).reshape(-1, a.dtype.itemsize)).all(1)  # noqa: E731
    rest = ~must  # outside times, the direct hit outside the union box
    assert (same(got[rest], want[rest]) | same(got[rest], rays[rest])).all() and (same(occ[rest], wocc[rest]) | same(occ[rest], iq.occ_of(rtc, rays)[rest])).all()
    held = out & in_box
    print(f"moving instances, mode {mode}: {int(out.sum())} rays with times outside [0, 1], {int((out & whit).sum())} of them hit in the direct trace, "
          f"{int(held.sum())} of those inside the union box (held to the direct trace), {int(rest.sum())} outside it")
    assert held.sum() >= 20 and len(np.unique(rays["time"][held])) == 2
    hit = got["geomID"] != INVALID
    per_inst = np.bincount(owner[hit], minlength=len(inst))
    print(f"moving instances, mode {mode}: {int(hit.sum())} hits of {len(rays)} rays, per instance {per_inst.tolist()}, {len(np.unique(rays['time'][hit]))} times")
    assert per_inst.min() >= 5 and len(np.unique(rays["time"][hit])) >= 9
    ihh.release(dev, top, inner)


# ---- 4. general transforms against the float64 truth ------------------------------------------------------------------------------------------
GENERAL_SEED = 5  # chosen so that the truth alone sets aside at most 2 % of the rays (checked below, on the CPU)


def _general_instances():
    """rotation x uniform scale x translation (radii are not affine under other maps)"""
    out = []
    for i, (axis, deg, s, t) in enumerate((((0, 0, 1), 30.0, 1.5, (0, 0, 0)), ((1, 2, 3), 77.0, 0.75, (30, 4, -3)), ((1, -1, 0.5), 140.0, 2.0, (-5, 36, 9)),
                                           ((0.2, 1, 0), 251.0, 1.0, (28, 33, 30)))):
        out.append((i, "m", [ih.affine(t, (s, s, s), ih.rotation(np.array(axis, np.float64), deg))]))
    return out


def _truth(d, inst, rays, radius_scale):
    """per ray the nearest hit over all instances in float64 on the float64 local ray (instance_hair_helpers.lines_truth64 / curves_truth64:
    the closed forms of line_helpers / curve_helpers in plain float64, inputs unrounded): dict of hit, inst, geomID, primID, t, u, v"""
    m = len(rays)
    o = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1).astype(np.float64)
    dd = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1).astype(np.float64)
    best = {"hit": np.zeros(m, bool), "inst": np.full(m, -1), "geomID": np.full(m, -1), "primID": np.full(m, -1), "t": np.full(m, np.inf), "u": np.zeros(m), "v": np.zeros(m)}
    for gid, _, steps in inst:
        w = np.linalg.inv(np.vstack([np.asarray(steps[0], np.float64).reshape(3, 4), [0, 0, 0, 1]]))[:3]
        lo, ld = o @ w[:, :3].T + w[:, 3], dd @ w[:, :3].T
        found = []
        if d.get("lines") is not None:
            v, idx, lgid = d["lines"]
            v0, v1 = (x.astype(np.float64).copy() for x in lh.ends(v, idx))
            v0[:, 3] *= radius_scale
            v1[:, 3] *= radius_scale
            r = ihh.lines_truth64(v0, v1, lo, ld)
            found.append((r["hit"], np.full(m, lgid), r["seg"], r["t"], r["u"], np.zeros(m)))
        if d.get("curves"):
            groups = []
            for v, idx, basis, rate, cgid in d["curves"]:
                cp = ch.native(v, idx, basis).astype(np.float64)
                cp[..., 3] *= radius_scale
                groups.append((cp, rate, cgid))
            r = ihh.curves_truth64(groups, lo, ld)
            found.append((r["hit"], r["geomID"], r["primID"], r["t"], r["u"], r["v"]))
        for hit, g, p, t, u, v in found:
            sel = hit & (t < best["t"])
            for k, a in (("inst", np.full(m, gid)), ("geomID", g), ("primID", p), ("t", t), ("u", u), ("v", v)):
                best[k][sel] = a[sel]
            best["hit"] |= sel
    return best


@pytest.mark.parametrize("which", ["a", "b"])
def test_general_transforms_against_the_float64_truth(rtc, which):
    """IDs exact, t within 1e-4 relative, u and v within 1e-4 (the contract of the line and curve tests: curve_helpers.compare).  A ray is set
    aside only when the truth itself changes its hit / miss, instance or primitive under radii scaled by (1 +- 1e-3): at most 2 %."""
    d = ihh.scenes(which)["m"]
    if which == "b":
        d = ihh.desc(curves=[d["curves"][2], d["curves"][5]])  # Bezier at rate 4, B-spline at rate 9 (the second pass)
    scs = {"m": d}
    inst = _general_instances()
    rays = isd.crossing_rays(rtc, ihh.bounds_meshes(scs), inst, 1200, GENERAL_SEED)
    want = _truth(d, inst, rays, 1.0)
    aside = np.zeros(len(rays), bool)
    for s in (1.0 + 1e-3, 1.0 - 1e-3):
        other = _truth(d, inst, rays, s)
        aside |= (other["hit"] != want["hit"]) | (other["hit"] & want["hit"] & ((other["inst"] != want["inst"]) | (other["geomID"] != want["geomID"]) | (other["primID"] != want["primID"])))
    print(f"general transforms ({which}): {int(want['hit'].sum())} hits of {len(rays)} rays in the truth, {int(aside.sum())} rays set aside")
    assert aside.sum() <= 0.02 * len(rays) and want["hit"].sum() >= 100 and len(np.unique(want["inst"][want["hit"]])) == len(inst)
    for mode in (0, 1):
        dev, top, inner = ihh.build(rtc, mode, scs, inst)
        got, occ = _trace_both(rtc, top, rays)
        keep = ~aside
        gh = got["geomID"] != INVALID
        assert np.array_equal(gh[keep], want["hit"][keep]), int((gh[keep] != want["hit"][keep]).sum())
        h = keep & gh
        for f, k in (("instID", "inst"), ("geomID", "geomID"), ("primID", "primID")):
            assert np.array_equal(got[f][h].astype(np.int64), want[k][h]), f
        et = np.abs(got["tfar"][h].astype(np.float64) - want["t"][h]) / np.abs(want["t"][h])
        eu, ev = np.abs(got["u"][h].astype(np.float64) - want["u"][h]), np.abs(got["v"][h].astype(np.float64) - want["v"][h])
        print(f"general transforms ({which}) mode {mode}: {int(h.sum())} hits compared, max error t {et.max():.1e} (relative) u {eu.max():.1e} v {ev.max():.1e}")
        assert et.max() <= 1e-4 and eu.max() <= 1e-4 and ev.max() <= 1e-4
        assert np.array_equal(got["tfar"][~gh], rays["tfar"][~gh])
        assert np.array_equal((occ["tfar"] == -np.inf)[keep], want["hit"][keep])
        ihh.release(dev, top, inner)


# ---- 5. a top scene with hair instances, a subdivision instance and geometry of its own ------------------------------------------------------------
def test_mixed_top_scene_equals_the_merge_of_its_parts(rtc, bomberman):
    scs = ihh.scenes("c")
    sub_mesh = isd.bomberman_faces(bomberman) + (3, 2)
    sv, st = random_soup(256, 5, extent=4.0, size=2.0)
    sv = ih.snap(sv * 4.0) + np.array([0.0, -40.0, 0.0], np.float32)
    places = {"h0": ih.affine((0.0, 0.0, 0.0)), "h1": ih.affine((40.0, 0.0, 0.0), (2.0,) * 3), "sub": ih.affine((0.0, 60.0, 0.0), (0.5,) * 3)}
    dev = rtc.Device(ihh.GPU_CFG)
    hair = ihh.add_scene(rtc, dev, scs["m"], 0)  # (robust: the subdivision accels traverse robustly)
    sub = isd.add_inner(rtc, dev, sub_mesh)
    own = rtc.Scene(dev, iq.flags(0))
    own.add_triangles(sv, st, geom_id=0)
    own.commit()
    top = rtc.Scene(dev, iq.flags(0))
    assert top.add_triangles(sv, st, geom_id=0) == 0
    assert top.add_instance(hair, places["h0"], geom_id=1) == 1 and top.add_instance(hair, places["h1"], geom_id=2) == 2
    assert top.add_instance(sub, places["sub"], geom_id=3) == 3
    top.commit()
    assert len(top.accel_data(rtc.ACCEL_DATA_INSTSUBDIV + 0)) > 0
    boxes_of = {"h": ihh.bounds_meshes(scs)["m"], "m": sub_mesh, "s": (sv,)}
    inst = [(1, "h", [places["h0"]]), (2, "h", [places["h1"]]), (3, "m", [places["sub"]]), (INVALID, "s", [ih.affine()])]
    rays = isd.crossing_rays(rtc, boxes_of, inst, 2000, 13)
    per = [isd.direct(rtc, sc, gid, steps, rays) for sc, (gid, _, steps) in zip((hair, hair, sub, own), inst)]
    t = np.sort(np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf).astype(np.float64) for p in per]), axis=0)
    both = np.isfinite(t[1])
    assert np.all(t[1][both] - t[0][both] > 1e-6 * np.abs(t[0][both]))
    want = isd.merge(rays, per, inst)
    got, occ = _trace_both(rtc, top, rays)
    _check(got, want, "mixed top scene")
    hit = want["geomID"] != INVALID
    counts = [int((hit & (want["instID"] == g)).sum()) for g in (1, 2, 3, INVALID)]
    print(f"mixed top scene: hits per hair instance 1, 2, the subdivision instance and the top scene's own mesh {counts}")
    assert min(counts) >= 20
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    for s in (top, hair, sub, own):
        s.release()
    dev.release()


# ---- 6. every entry path gives the bytes of one device-resident rtcIntersect1M; service=1 --------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (ih.HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_entry_paths_are_bit_identical(rtc, mode):
    import torch
    scs = ihh.scenes("d")
    m = 20000  # (above tunePipeMinRays: the pipelined host path)
    rays = isd.crossing_rays(rtc, ihh.bounds_meshes(scs), INST, m, 31)
    dev, top, inner = ihh.build(rtc, mode, scs, INST)
    L = top.lib
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    top.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    hit = want["geomID"] != INVALID
    assert int(hit.sum()) > 1000 and len(np.unique(want["geomID"][hit])) >= 4
    to = torch.from_numpy(iq.occ_of(rtc, rays).view(np.uint8).reshape(-1, 48).copy()).cuda()
    top.occluded1M(to)
    torch.cuda.synchronize()
    wocc = to.cpu().numpy().reshape(-1).view(rtc.RAY_DTYPE)
    assert np.array_equal(wocc["tfar"] == -np.inf, hit)
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
    k = 64
    one, o1 = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    for i in range(k):
        top.intersect1(one[i:i + 1])
        top.occluded1(o1[i:i + 1])
    assert one[:k].tobytes() == want[:k].tobytes() and o1[:k].tobytes() == wocc[:k].tobytes()
    p = iq.copy(rtc, rays)
    arr = (C.c_void_p * 256)(*[p[i:i + 1].ctypes.data for i in range(256)])
    ctx = rtc.make_context()
    L.rtcIntersect1Mp(top.handle, C.byref(ctx), arr, 256)
    dev.check("rtcIntersect1Mp")
    assert p[:256].tobytes() == want[:256].tobytes()
    fn = L.rtcIntersect8
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    valid = np.full(8, -1, np.int32)
    for a in range(0, 64, 8):
        pk = _soa(rays[a:a + 8], 8, True)
        fn(valid.ctypes.data, top.handle, C.addressof(ctx), pk.ctypes.data)
        dev.check("rtcIntersect8")
        assert np.array_equal(pk, _soa(want[a:a + 8], 8, True))
    ihh.release(dev, top, inner)
    # two shards on one GPU, and service=1 (no service kernel for instances: the call combiner serves the small calls with identical records)
    for cfg, small in (("gpus=0:0", False), ("service=1", True)):
        dev, top, inner = ihh.build(rtc, mode, scs, INST, cfg + "," + ihh.GPU_CFG)
        g = iq.copy(rtc, rays)
        if small:
            for a in range(0, 2048, 32):
                top.intersect1M(g[a:a + 32])
            assert g[:2048].tobytes() == want[:2048].tobytes()
            assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
        else:
            top.intersect1M(g)
            assert g.tobytes() == want.tobytes()
        ihh.release(dev, top, inner)


# ---- 7. the HBM overflow area ---------------------------------------------------------------------------------------------------------------------
def _needle_scene(radius=0.0002):
    """1024 line segments and 512 curves (straight, rate 4) along the needles of deep_stack_helpers.sliver_soup: unit length in the unit
    cube, so thin that about 60 % of the rays hit nothing"""
    v, _ = ds.sliver_soup(1024, ds.SOUP_SEED, snapped=True, width=0.004)
    lv = np.zeros((2048, 4), np.float32)
    lv[0::2, :3], lv[1::2, :3], lv[:, 3] = v[0::3], v[1::3], radius
    cv0, _ = ds.sliver_soup(512, ds.SOUP_SEED + 1, snapped=True, width=0.004)
    a, b = cv0[0::3].astype(np.float64), cv0[1::3].astype(np.float64)
    cv = np.zeros((2048, 4), np.float32)
    for k in range(4):
        cv[k::4, :3] = a + (b - a) * (k / 3.0)
    cv[:, 3] = radius
    return {"m": ihh.desc(curves=[(cv, np.arange(0, 2048, 4, dtype=np.uint32), "bezier", 4, 0)], lines=(lv, np.arange(0, 2048, 2, dtype=np.uint32), 1))}


def test_needle_hair_spills_to_hbm_and_agrees_with_the_direct_traces(rtc, monkeypatch):
    """The 1024 long thin line segments and 512 long thin curves of _needle_scene(), with overlapping boxes, under the three overlapping instances of
    deep_stack_helpers.deep_instances(): a ray stacks most children of most nodes on both levels.  Precondition, measured on the host from
    the accel the kernel traverses (instance_hair_helpers.simulate_stack: the walk of a ray that hits nothing): of the sampled rays that
    the GPU reports as misses at least 10 % of the sample have written stack slots beyond the 16 in LDS."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    sample = 200
    scs = _needle_scene()
    inst = isd.static(ds.deep_instances())
    meshes = ihh.bounds_meshes(scs)
    lo, hi = isd.world_boxes(meshes, inst)[0]
    org, dirs = random_rays_np(4000, lo.astype(np.float32), hi.astype(np.float32), ds.GPU_RAY_SEED)
    rays = ds.rays_of(rtc, ds.snap(org), ih.snap(dirs * 4.0))
    dev, top, inner = ihh.build(rtc, 1, scs, inst)
    st = top.stats()
    assert st["accelKind"] == 23 and ds.stack_capacity(st["maxDepth"]) > 16
    got, occ = _trace_both(rtc, top, rays)
    assert dev.error() == 0  # the `overflow` word stayed clear: no entry was dropped
    o = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1)[:sample]
    d = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1)[:sample]
    deepest = ihh.simulate_stack(top.accel_data(0).view(ih.NODE_DT), top.accel_root(), top.accel_data(2), len(inst), o, d)
    miss = got["geomID"][:sample] == INVALID
    deep = int((miss & (deepest >= 16)).sum())
    print(f"needle hair: maxDepth {st['maxDepth']}, {int(miss.sum())} of {sample} sampled rays miss, {deep} of them pass slot 16, deepest slot {int(deepest.max())}")
    assert deep >= sample // 10 and deepest.max() < ds.stack_capacity(st["maxDepth"])
    per = isd.direct_all(rtc, inner, inst, rays)
    t = np.sort(np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf).astype(np.float64) for p in per]), axis=0)
    with np.errstate(invalid="ignore"):
        clear = ~(np.isfinite(t[1]) & (t[1] - t[0] <= 1e-6 * np.abs(t[0])))  # (the instances overlap: a ray whose two nearest instances tie is left out)
    assert clear.sum() >= 0.99 * len(rays)
    want = isd.merge(rays, per, inst)
    _check(got[clear], want[clear], "needle hair")
    hit = want["geomID"] != INVALID
    assert np.array_equal((occ["tfar"] == -np.inf)[clear], hit[clear])
    print(f"needle hair: {int(hit.sum())} hits of {len(rays)} rays")
    assert int(hit.sum()) >= 200
    ihh.release(dev, top, inner)
    for k, val in {"RTAMD_CHUNK": "32", "RTAMD_REFILL_BATCH": "1", "RTAMD_LEAF_BATCH": "64"}.items():  # small queue shares repeat the bytes
        monkeypatch.setenv(k, val)
    dev, top, inner = ihh.build(rtc, 1, scs, inst)
    g2, o2 = _trace_both(rtc, top, rays)
    assert g2.tobytes() == got.tobytes() and o2.tobytes() == occ.tobytes() and dev.error() == 0
    ihh.release(dev, top, inner)


# ---- 8. invalid rays; refusals at the call ----------------------------------------------------------------------------------------------------------
def test_invalid_rays_come_back_untouched(rtc):
    scs = ihh.scenes("c")
    rays = isd.crossing_rays(rtc, ihh.bounds_meshes(scs), INST, 1024, 3)
    dev, top, inner = ihh.build(rtc, 1, scs, INST)
    good = iq.copy(rtc, rays)
    top.intersect1M(good)
    bad = iq.copy(rtc, rays)
    k = np.arange(len(rays)) % 4
    bad["tnear"][k == 0], bad["tfar"][k == 0] = 2.0, 1.0  # tnear > tfar
    bad["org_x"][k == 1] = np.nan
    bad["dir_y"][k == 2] = np.nan
    src = bad.copy()
    top.intersect1M(bad)
    for c in (0, 1, 2):
        assert bad[k == c].tobytes() == src[k == c].tobytes(), c
    assert bad[k == 3].tobytes() == good[k == 3].tobytes() and (good["geomID"][k == 3] != INVALID).sum() > 10
    occ = iq.occ_of(rtc, src)
    occ["tfar"][k == 3] = -1.0  # tfar < 0: an any-hit ray that is already occluded
    osrc = occ.copy()
    top.occluded1M(occ)
    assert occ.tobytes() == osrc.tobytes()
    ihh.release(dev, top, inner)


def test_context_filter_and_counted_batches_are_refused_at_the_call(rtc):
    for cfg, text in ((ihh.GPU_CFG, "RTCIntersectContext::filter is not supported on a scene with instances"), (ihh.GPU_CFG + ",inst_filters=1", ihh.REFUSE_CONTEXT)):
        dev, top, inner = ihh.build(rtc, 1, ihh.scenes("a"), [(0, "m", [ih.affine()])], cfg)
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
            assert log and log[-1][0] == rtc.RTC_ERROR_INVALID_OPERATION and text in log[-1][1], log
        for counted, recs in ((top.intersect1M_counted, rh), (top.occluded1M_counted, occ)):
            with pytest.raises(rtc.RTCError) as e:
                counted(recs)
            assert e.value.code == rtc.RTC_ERROR_INVALID_OPERATION
            assert "counted batches are not supported on a scene with instances" in log[-1][1], log
        assert rh.tobytes() == src.tobytes() and occ.tobytes() == osrc.tobytes()  # records untouched
        ihh.release(dev, top, inner)
