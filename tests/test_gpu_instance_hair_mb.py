"""Line segments and flat curves with time steps below an instance (device config inst_hair=1,inst_hair_mb=1): the HAIRMB form of the
two-level kernel (embree-compressed_amd/csrc/trace_instance_hair_mb.hip), kinds 22 / 23.

The method is that of tests/test_gpu_instance_hair.py.  With exact transforms (origins and translations on the 2^-10 grid, uniform
power-of-two scales) the instanced scene traced DIRECTLY with the exact local rays and the same ray.time - a plain scene, traced by the
top-level motion-blur line and curve kernels that exist without instancing - is the expected record of that instance, apart from instID.
Vertices and their per-step offsets lie on the 2^-10 grid, times on k / 8.  The general-transform leg is held to the float64 truth of the
line and curve tests on vertices interpolated in float64 at the ray's time.  tests/instance_hair_mb_helpers.py."""
import ctypes as C

import numpy as np
import pytest

import curve_helpers as ch
import deep_stack_helpers as ds
import instance_hair_helpers as ihh
import instance_hair_mb_helpers as ihm
import instance_helpers as ih
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
import instance_subdiv_helpers as isd
import line_helpers as lh
from helpers import INVALID, fill_rays, random_rays_np, random_soup

pytestmark = pytest.mark.gpu

INST = isd.lattice_instances(6)  # power-of-two scales, grid translations: local rays are exact
EIGHTHS = [k / 8.0 for k in (0, 3, 8, 1, 4, 6, 2, 7, 5)]
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL", "RTAMD_CBVH_FORM")


def _check(got, want, what):
    assert got.tobytes() == want.tobytes(), f"{what}: {isd.differing(got, want)} of {len(got)} records differ"


def _trace_both(rtc, top, rays):
    got, occ = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    top.intersect1M(got)
    top.occluded1M(occ)
    return got, occ


def _aimed_rays(rtc, local_points, tfar_local=3.0, seed=1):
    """per instance of INST one ray per local point: from 2 local units away in a dyadic direction straight at the point, times k / 8
    (0 and 1 among them); returns (rays, owner)"""
    rng = np.random.RandomState(seed)
    p = ih.snap(local_points).astype(np.float64)
    d = np.round(rng.uniform(-1, 1, p.shape) * 8.0) / 8.0
    d[(d == 0).all(1)] = (0.5, -0.25, 1.0)
    d /= np.abs(d).max(1, keepdims=True)  # the largest component +-1, the others multiples of 1/8 over it... kept dyadic below
    d = np.round(d * 256.0) / 256.0
    org_l = p - 2.0 * d
    orgs, dirs, tf, owner = [], [], [], []
    for i, (_, _, steps) in enumerate(INST):
        s = float(steps[0][0][0])
        orgs.append(ih.xfm_points(steps[0], org_l))
        dirs.append(d * s)  # the local direction is d again: the same t in every instance
        tf.append(np.full(len(p), tfar_local))
        owner.append(np.full(len(p), i))
    rays = rtc.aligned_rayhits(len(p) * len(INST))
    fill_rays(rays, np.concatenate(orgs).astype(np.float32), np.concatenate(dirs).astype(np.float32), tfar=np.concatenate(tf).astype(np.float32))
    rays["time"] = np.asarray(EIGHTHS, np.float32)[np.arange(len(rays)) % len(EIGHTHS)]
    return rays, np.concatenate(owner)


# ---- 1. and 2. short rays, byte for byte; ties --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["a", "b", "c", "d"])
def test_short_rays_equal_the_instanced_scene_traced_directly(rtc, which, mode):
    scs = ihm.scenes(which)
    d = scs["m"]
    meshes = ihm.bounds_meshes(scs)
    rays, owner = isd.short_rays(rtc, meshes, INST, 300, 41 + ord(which), times=EIGHTHS)
    isd.assert_cannot_reach_others(meshes, INST, rays, owner)
    dev, top, inner = ihm.build(rtc, mode, scs, INST)
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
    assert set(ihm.moving_gids(d)) <= set(geoms), (ihm.moving_gids(d), geoms)  # every moving-hair geometry is hit
    if which == "b":  # three steps: hits in both time segments and exactly at 0.5
        t = rays["time"][hit]
        assert (t < 0.5).any() and (t > 0.5).any() and (t == 0.5).any()
    if which == "d":
        # ties: the moving geometry's steps equal the static geometry's vertices, everything dyadic: lerp is exact, both trees give the
        # bit-identical t and the motion-blur tree, which comes later, owns the hit
        lv, lidx, _ = d["lines"]
        v0, v1 = lh.ends(lv, lidx)
        cp = ch.native(d["curves"][0][0], d["curves"][0][1], "bezier")
        for name, pts, static_gid, moving_gid in (("lines", (v0[:, :3] + v1[:, :3]) / 2, 0, 1), ("curves", (cp[:, 0, :3] + 3 * cp[:, 1, :3] + 3 * cp[:, 2, :3] + cp[:, 3, :3]) / 8, 2, 3)):
            ar, aowner = _aimed_rays(rtc, pts)
            isd.assert_cannot_reach_others(meshes, INST, ar, aowner)
            agot, aocc = _trace_both(rtc, top, ar)
            _check(agot, isd.direct_owned(rtc, inner, INST, ar, aowner), f"(d) rays aimed at the {name}")
            _check(aocc, isd.direct_owned(rtc, inner, INST, ar, aowner, occluded=True), f"(d) rays aimed at the {name}, any hit")
            on = np.isin(agot["geomID"], (static_gid, moving_gid))
            print(f"(d) mode {mode}: {int(on.sum())} of {len(ar)} rays aimed at the {name} end on them, {int((agot['geomID'] == moving_gid).sum())} on the moving geometry")
            assert on.sum() >= len(ar) // 2 and (agot["geomID"][on] == moving_gid).all()
    ihm.release(dev, top, inner)


# ---- 3. crossing rays ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_crossing_rays_equal_the_merged_direct_traces(rtc, mode):
    scs = ihm.scenes("c")
    meshes = ihm.bounds_meshes(scs)
    rays = isd.crossing_rays(rtc, meshes, INST, 2000, 7)
    rays["time"] = np.asarray(EIGHTHS, np.float32)[np.arange(len(rays)) % len(EIGHTHS)]
    dev, top, inner = ihm.build(rtc, mode, scs, INST)
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
    ihm.release(dev, top, inner)


# ---- 4. moving instances -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_moving_instances_equal_the_static_instance_at_the_rays_time(rtc, mode):
    """instances with 2 and 3 transform steps (signed axis permutations, power-of-two scales, translations on the grid: world2local(time)
    is exact, which instance_subdiv_helpers.direct asserts) over moving hair, ray times k / 8 and two times outside [0, 1]: per ray the
    record of the still-moving instanced scene traced directly with the local ray of the instance at that time - a static instance at that
    time - byte for byte.  Ray construction and margin are those of tests/test_gpu_instance_hair.py leg 3.
    A time outside [0, 1] extrapolates the transform (still exact) AND, in the leaf, the hair's first / last time segment, while the
    instance's box in the top scene is the union over its steps of the instanced scene's bounds.  Decided on the host: where the direct
    trace's hit point lies inside that union box (the moving-hair scene's bounds under every transform step, shrunk by 1e-3 of its extent
    for the builder's float32 corners) the segment [tnear, tfar] meets every box above the instance, the ray enters it and its record must
    be the direct trace's, for closest and any hit; a ray the direct trace misses comes back untouched; only a ray whose direct hit lies
    outside the union box may come back either way."""
    scs = {"m": ihm.desc(lines_mb=ihm.moving_strands(2), curves_mb=ihm.moving_curve_geometries(3, first_gid=1))}
    meshes = ihm.bounds_meshes(scs)
    inst = [(g, k, s[:3]) for g, k, s in im.exact_instances(6)]
    assert sorted({len(s) for _, _, s in inst}) == [2, 3]
    rays, owner = isd.short_rays(rtc, meshes, inst, 300, 9, times=EIGHTHS + [-2 / 8.0, 11 / 8.0])
    isd.assert_cannot_reach_others(meshes, inst, rays, owner)
    dev, top, inner = ihm.build(rtc, mode, scs, inst)
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
    hit = inside & (got["geomID"] != INVALID)
    per_inst = np.bincount(owner[hit], minlength=len(inst))
    print(f"moving instances, mode {mode}: {int(hit.sum())} hits of {len(rays)} rays, per instance {per_inst.tolist()}, {len(np.unique(rays['time'][hit]))} times")
    assert per_inst.min() >= 5 and len(np.unique(rays["time"][hit])) == 9 and set(np.unique(got["geomID"][hit]).tolist()) >= set(range(5))
    ihm.release(dev, top, inner)


# ---- 5. general transforms against the float64 truth ------------------------------------------------------------------------------------------
GENERAL_SEED = {"a": 5, "b": 5}  # chosen so that the truth alone sets aside at most 2 % of the rays (checked below, on the CPU)


def _general_instances():
    """rotation x uniform scale x translation (radii are not affine under other maps)"""
    out = []
    for i, (axis, deg, s, t) in enumerate((((0, 0, 1), 30.0, 1.5, (0, 0, 0)), ((1, 2, 3), 77.0, 0.75, (30, 4, -3)), ((1, -1, 0.5), 140.0, 2.0, (-5, 36, 9)),
                                           ((0.2, 1, 0), 251.0, 1.0, (28, 33, 30)))):
        out.append((i, "m", [ih.affine(t, (s, s, s), ih.rotation(np.array(axis, np.float64), deg))]))
    return out


def _truth(d, inst, rays, radius_scale):
    """per ray the nearest hit over all instances in float64: instance_hair_helpers.lines_truth64 / curves_truth64 on vertices interpolated
    in float64 at the ray's time (instance_hair_mb_helpers.steps_at64), on the float64 local ray.
    The segments of a strand share their end points.  Where the nearest point of the ray's axis lies beyond a segment's end, u clips to 0
    or 1 and the hit point IS the shared vertex: the neighbouring segment gives the same point and the same t, and which of the two owns
    the hit is not a property of the geometry (lines_truth64 takes the lower index of an equal t).  For such a hit the truth names both:
    alt_prim / alt_u hold the neighbour and its u (1 - u), -1 elsewhere."""
    m = len(rays)
    o = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1).astype(np.float64)
    dd = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1).astype(np.float64)
    best = {"hit": np.zeros(m, bool), "inst": np.full(m, -1), "geomID": np.full(m, -1), "primID": np.full(m, -1), "t": np.full(m, np.inf), "u": np.zeros(m), "v": np.zeros(m),
            "alt_prim": np.full(m, -1), "alt_u": np.zeros(m)}
    for gid, _, steps in inst:
        w = np.linalg.inv(np.vstack([np.asarray(steps[0], np.float64).reshape(3, 4), [0, 0, 0, 1]]))[:3]
        lo, ld = o @ w[:, :3].T + w[:, 3], dd @ w[:, :3].T
        for time in np.unique(rays["time"]):
            sel = np.nonzero(rays["time"] == time)[0]
            found = []
            if d.get("lines_mb") is not None:
                vsteps, idx, lgid = d["lines_mb"]
                v = ihm.steps_at64(vsteps, float(time))
                i64 = np.asarray(idx, np.int64)
                v0, v1 = v[i64].copy(), v[i64 + 1].copy()
                v0[:, 3] *= radius_scale
                v1[:, 3] *= radius_scale
                r = ihh.lines_truth64(v0, v1, lo[sel], ld[sel])
                alt, alt_u = np.full(len(sel), -1), np.zeros(len(sel))
                for k in np.nonzero(r["hit"] & ((r["u"] == 0.0) | (r["u"] == 1.0)))[0]:  # the hit point is an end point: shared with a neighbour?
                    s0 = int(r["seg"][k])
                    nb = s0 + 1 if r["u"][k] == 1.0 else s0 - 1
                    if 0 <= nb < len(i64) and i64[nb] - i64[s0] == nb - s0:
                        rr = ihh.lines_truth64(v0[nb:nb + 1], v1[nb:nb + 1], lo[sel[k]:sel[k] + 1], ld[sel[k]:sel[k] + 1])
                        if rr["hit"][0] and rr["u"][0] == 1.0 - r["u"][k] and abs(rr["t"][0] - r["t"][k]) <= 1e-12 * abs(r["t"][k]):
                            alt[k], alt_u[k] = nb, rr["u"][0]
                found.append((r["hit"], np.full(len(sel), lgid), r["seg"], r["t"], r["u"], np.zeros(len(sel)), alt, alt_u))
            groups = []
            for vsteps, idx, basis, rate, cgid in (d.get("curves_mb") or []):
                nat = [ch.bspline_to_bezier(ch.control_points(s, idx).astype(np.float64), np.float64) if basis == "bspline" else ch.control_points(s, idx).astype(np.float64) for s in vsteps]
                cp = ihm.steps_at64(nat, float(time))  # (the conversion is linear: interpolating the native points is interpolating the vertices)
                cp[..., 3] *= radius_scale
                groups.append((cp, rate, cgid))
            if groups:
                r = ihh.curves_truth64(groups, lo[sel], ld[sel])
                found.append((r["hit"], r["geomID"], r["primID"], r["t"], r["u"], r["v"], np.full(len(sel), -1), np.zeros(len(sel))))
            for hit, g, p, t, u, v, ap, au in found:
                take = hit & (t < best["t"][sel])
                rows = sel[take]
                for k, a in (("inst", np.full(len(sel), gid)), ("geomID", g), ("primID", p), ("t", t), ("u", u), ("v", v), ("alt_prim", ap), ("alt_u", au)):
                    best[k][rows] = np.asarray(a)[take]
                best["hit"][rows] = True
    return best


@pytest.mark.parametrize("which", ["a", "b"])
def test_general_transforms_against_the_float64_truth(rtc, which):
    """IDs exact, t within 1e-4 relative, u and v within 1e-4 (the contract of the line and curve tests: curve_helpers.compare).  A ray is set
    aside only when the truth itself changes its hit / miss, instance or primitive under radii scaled by (1 +- 1e-3): at most 2 %."""
    d = ihm.scenes(which)["m"]
    if which == "b":
        g = ihm.moving_curve_geometries(3, n=24)
        d = ihm.desc(curves_mb=[g[2], g[3]])  # B-spline at rate 4, Bezier at rate 9 (the second pass), three steps, 24 curves each
    scs = {"m": d}
    inst = _general_instances()
    rays = isd.crossing_rays(rtc, ihm.bounds_meshes(scs), inst, 1200, GENERAL_SEED[which])
    rays["time"] = np.asarray(EIGHTHS, np.float32)[np.arange(len(rays)) % len(EIGHTHS)]
    want = _truth(d, inst, rays, 1.0)
    aside = np.zeros(len(rays), bool)
    for s in (1.0 + 1e-3, 1.0 - 1e-3):
        other = _truth(d, inst, rays, s)
        same_prim = (other["primID"] == want["primID"]) | ((want["alt_prim"] >= 0) & (other["primID"] == want["alt_prim"]))  # (a shared end point: either owner)
        aside |= (other["hit"] != want["hit"]) | (other["hit"] & want["hit"] & ((other["inst"] != want["inst"]) | (other["geomID"] != want["geomID"]) | ~same_prim))
    print(f"general transforms ({which}): {int(want['hit'].sum())} hits of {len(rays)} rays in the truth, {int(aside.sum())} rays set aside")
    assert aside.sum() <= 0.02 * len(rays) and want["hit"].sum() >= 100 and len(np.unique(want["inst"][want["hit"]])) == len(inst)
    # a condition on the inputs, from the truth alone: hits at an end point that two segments share - the only hits whose primID may be
    # either of two - are at most 5 % of the hits, so that a kernel that names the neighbour as a rule cannot pass on them
    shared = want["hit"] & (want["alt_prim"] >= 0)
    print(f"general transforms ({which}): {int(shared.sum())} of the truth's hits lie at an end point two segments share")
    assert shared.sum() <= 0.05 * want["hit"].sum()
    for mode in (0, 1):
        dev, top, inner = ihm.build(rtc, mode, scs, inst)
        got, occ = _trace_both(rtc, top, rays)
        keep = ~aside
        gh = got["geomID"] != INVALID
        assert np.array_equal(gh[keep], want["hit"][keep]), int((gh[keep] != want["hit"][keep]).sum())
        h = keep & gh
        for f, k in (("instID", "inst"), ("geomID", "geomID")):
            assert np.array_equal(got[f][h].astype(np.int64), want[k][h]), f
        gp = got["primID"].astype(np.int64)
        other_owner = h & (want["alt_prim"] >= 0) & (gp == want["alt_prim"])  # the hit point is an end point two segments share: the neighbour owns it
        assert np.array_equal(gp[h & ~other_owner], want["primID"][h & ~other_owner]), "primID"
        assert other_owner.sum() <= shared.sum() <= 0.05 * want["hit"].sum()
        want_u = np.where(other_owner, want["alt_u"], want["u"])
        et = np.abs(got["tfar"][h].astype(np.float64) - want["t"][h]) / np.abs(want["t"][h])
        eu, ev = np.abs(got["u"][h].astype(np.float64) - want_u[h]), np.abs(got["v"][h].astype(np.float64) - want["v"][h])
        print(f"general transforms ({which}) mode {mode}: {int((want['alt_prim'] >= 0).sum())} hits at shared end points, {int(other_owner.sum())} of them owned by the neighbour")
        print(f"general transforms ({which}) mode {mode}: {int(h.sum())} hits compared, max error t {et.max():.1e} (relative) u {eu.max():.1e} v {ev.max():.1e}")
        assert et.max() <= 1e-4 and eu.max() <= 1e-4 and ev.max() <= 1e-4
        assert np.array_equal(got["tfar"][~gh], rays["tfar"][~gh])
        assert np.array_equal((occ["tfar"] == -np.inf)[keep], want["hit"][keep])
        ihm.release(dev, top, inner)


# ---- 6. times outside the shutter and NaN ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_times_outside_the_shutter_and_nan_equal_the_direct_trace(rtc, mode):
    """time = -0.5 and 1.5 extrapolate the first / last segment, a NaN time makes every interpolated point NaN: whatever the top-level
    leaves do with them, the instanced trace does the same (static instances: the ray enters whatever its time)"""
    scs = {"m": ihm.desc(lines_mb=ihm.moving_strands(2), curves_mb=ihm.moving_curve_geometries(3, first_gid=1))}
    meshes = ihm.bounds_meshes(scs)
    rays, owner = isd.short_rays(rtc, meshes, INST, 300, 17, times=[-0.5, 1.5, np.nan, 0.5])
    isd.assert_cannot_reach_others(meshes, INST, rays, owner)
    dev, top, inner = ihm.build(rtc, mode, scs, INST)
    got, occ = _trace_both(rtc, top, rays)
    want = isd.direct_owned(rtc, inner, INST, rays, owner)
    _check(got, want, f"odd times, mode {mode}")
    _check(occ, isd.direct_owned(rtc, inner, INST, rays, owner, occluded=True), f"odd times, mode {mode}, any hit")
    hit = want["geomID"] != INVALID
    nan = np.isnan(rays["time"])
    counts = [int((hit & (rays["time"] == t)).sum()) for t in (-0.5, 1.5)]
    print(f"odd times, mode {mode}: hits at time -0.5 and 1.5 {counts}, at NaN {int((hit & nan).sum())} of {int(nan.sum())}")
    assert min(counts) >= 20 and not (hit & nan).any()
    ihm.release(dev, top, inner)


# ---- 7. a top scene with moving-hair instances, a static-hair instance, a subdivision instance and geometry of its own ------------------------------
def test_mixed_top_scene_equals_the_merge_of_its_parts(rtc, bomberman):
    scs = ihm.scenes("c")
    static_hair = ihh.scenes("c")["m"]
    sub_mesh = isd.bomberman_faces(bomberman) + (3, 2)
    sv, st = random_soup(256, 5, extent=4.0, size=2.0)
    sv = ih.snap(sv * 4.0) + np.array([0.0, -40.0, 0.0], np.float32)
    places = {"h0": ih.affine((0.0, 0.0, 0.0)), "h1": ih.affine((40.0, 0.0, 0.0), (2.0,) * 3), "s": ih.affine((0.0, 0.0, 60.0)), "sub": ih.affine((0.0, 60.0, 0.0), (0.5,) * 3)}
    dev = rtc.Device(ihm.GPU_CFG)
    hair = ihm.add_scene(rtc, dev, scs["m"], 0)  # (robust: the subdivision accels traverse robustly)
    still = ihh.add_scene(rtc, dev, static_hair, 0)
    sub = isd.add_inner(rtc, dev, sub_mesh)
    own = rtc.Scene(dev, iq.flags(0))
    own.add_triangles(sv, st, geom_id=0)
    own.commit()
    top = rtc.Scene(dev, iq.flags(0))
    assert top.add_triangles(sv, st, geom_id=0) == 0
    assert top.add_instance(hair, places["h0"], geom_id=1) == 1 and top.add_instance(hair, places["h1"], geom_id=2) == 2
    assert top.add_instance(sub, places["sub"], geom_id=3) == 3 and top.add_instance(still, places["s"], geom_id=4) == 4
    top.commit()
    assert len(top.accel_data(rtc.ACCEL_DATA_INSTSUBDIV + 0)) > 0
    boxes_of = {"h": ihm.bounds_meshes(scs)["m"], "t": ihh.bounds_meshes({"m": static_hair})["m"], "m": sub_mesh, "s": (sv,)}
    inst = [(1, "h", [places["h0"]]), (2, "h", [places["h1"]]), (3, "m", [places["sub"]]), (4, "t", [places["s"]]), (INVALID, "s", [ih.affine()])]
    rays = isd.crossing_rays(rtc, boxes_of, inst, 2500, 13)
    rays["time"] = np.asarray(EIGHTHS, np.float32)[np.arange(len(rays)) % len(EIGHTHS)]
    per = [isd.direct(rtc, sc, gid, steps, rays) for sc, (gid, _, steps) in zip((hair, hair, sub, still, own), inst)]
    t = np.sort(np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf).astype(np.float64) for p in per]), axis=0)
    both = np.isfinite(t[1])
    assert np.all(t[1][both] - t[0][both] > 1e-6 * np.abs(t[0][both]))
    want = isd.merge(rays, per, inst)
    got, occ = _trace_both(rtc, top, rays)
    _check(got, want, "mixed top scene")
    hit = want["geomID"] != INVALID
    counts = [int((hit & (want["instID"] == g)).sum()) for g in (1, 2, 3, 4, INVALID)]
    print(f"mixed top scene: hits per moving-hair instance 1, 2, the subdivision instance, the static-hair instance and the top scene's own mesh {counts}")
    assert min(counts) >= 20
    assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    for s in (top, hair, still, sub, own):
        s.release()
    dev.release()


# ---- 8. every entry path gives the bytes of one device-resident rtcIntersect1M; service=1 --------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (ih.HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_entry_paths_are_bit_identical(rtc, mode):
    import torch
    scs = ihm.scenes("c")
    m = 20000  # (above tunePipeMinRays: the pipelined host path)
    rays = isd.crossing_rays(rtc, ihm.bounds_meshes(scs), INST, m, 31)
    rays["time"] = np.asarray(EIGHTHS, np.float32)[np.arange(m) % len(EIGHTHS)]
    dev, top, inner = ihm.build(rtc, mode, scs, INST)
    L = top.lib
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    top.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    hit = want["geomID"] != INVALID
    assert int(hit.sum()) > 1000 and len(np.unique(want["geomID"][hit])) >= 8
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
    ctx = rtc.make_context()
    p = iq.copy(rtc, rays)
    arr = (C.c_void_p * 256)(*[p[i:i + 1].ctypes.data for i in range(256)])
    L.rtcIntersect1Mp(top.handle, C.byref(ctx), arr, 256)
    dev.check("rtcIntersect1Mp")
    assert p[:256].tobytes() == want[:256].tobytes()
    # rtcIntersectNM (streams of SoA packets of 4) and rtcIntersectNp (one SoA packet with a pointer per component)
    n_nm = 64
    pk = np.ascontiguousarray(np.stack([_soa(rays[a:a + 4], 4, True) for a in range(0, n_nm, 4)]))
    fn = L.rtcIntersectNM
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_size_t]
    fn(top.handle, C.addressof(ctx), pk.ctypes.data, 4, n_nm // 4, pk[0].nbytes)
    dev.check("rtcIntersectNM")
    assert np.array_equal(pk, np.stack([_soa(want[a:a + 4], 4, True) for a in range(0, n_nm, 4)]))
    cols = _soa(rays, 128, True)
    ptrs = (C.c_void_p * len(cols))(*[cols[i].ctypes.data for i in range(len(cols))])
    fn = L.rtcIntersectNp
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
    fn(top.handle, C.addressof(ctx), C.addressof(ptrs), 128)
    dev.check("rtcIntersectNp")
    assert np.array_equal(cols, _soa(want, 128, True))
    for width in (4, 8, 16):
        fn = getattr(L, "rtcIntersect%d" % width)
        fn.restype = None
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        valid = np.full(width, -1, np.int32)
        for a in range(0, 64, width):
            pk = _soa(rays[a:a + width], width, True)
            fn(valid.ctypes.data, top.handle, C.addressof(ctx), pk.ctypes.data)
            dev.check("rtcIntersect%d" % width)
            assert np.array_equal(pk, _soa(want[a:a + width], width, True))
    ihm.release(dev, top, inner)
    # two shards on one GPU, and service=1 (no service kernel for instances: the call combiner serves the small calls with identical records)
    for cfg, small in (("gpus=0:0", False), ("service=1", True)):
        dev, top, inner = ihm.build(rtc, mode, scs, INST, cfg + "," + ihm.GPU_CFG)
        g = iq.copy(rtc, rays)
        if small:
            for a in range(0, 2048, 32):
                top.intersect1M(g[a:a + 32])
            assert g[:2048].tobytes() == want[:2048].tobytes()
            assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
        else:
            top.intersect1M(g)
            assert g.tobytes() == want.tobytes()
        ihm.release(dev, top, inner)


# ---- 9. the HBM overflow area ---------------------------------------------------------------------------------------------------------------------
def _needle_scene(radius=0.0002):
    """1024 two-step line segments and 512 two-step curves (straight, rate 4) along the needles of deep_stack_helpers.sliver_soup: unit
    length in the unit cube, so thin that most rays hit nothing; step 1 is step 0 moved by 2^-8 along x"""
    v, _ = ds.sliver_soup(1024, ds.SOUP_SEED, snapped=True, width=0.004)
    lv = np.zeros((2048, 4), np.float32)
    lv[0::2, :3], lv[1::2, :3], lv[:, 3] = v[0::3], v[1::3], radius
    cv0, _ = ds.sliver_soup(512, ds.SOUP_SEED + 1, snapped=True, width=0.004)
    a, b = cv0[0::3].astype(np.float64), cv0[1::3].astype(np.float64)
    cv = np.zeros((2048, 4), np.float32)
    for k in range(4):
        cv[k::4, :3] = a + (b - a) * (k / 3.0)
    cv[:, 3] = radius
    move = np.array([1.0 / 256.0, 0, 0, 0], np.float32)
    return {"m": ihm.desc(curves_mb=[([cv, cv + move], np.arange(0, 2048, 4, dtype=np.uint32), "bezier", 4, 0)], lines_mb=([lv, lv + move], np.arange(0, 2048, 2, dtype=np.uint32), 1))}


def test_needle_moving_hair_spills_to_hbm_and_agrees_with_the_direct_traces(rtc, monkeypatch):
    """tests/test_gpu_instance_hair.py leg 7 over moving hair: the needles under the three overlapping instances of
    deep_stack_helpers.deep_instances(); a ray stacks most children of most nodes on both levels.  Precondition, measured on the host from
    the accel the kernel traverses (instance_hair_mb_helpers.simulate_stack): of the sampled rays that the GPU reports as misses at least
    10 % of the sample have written stack slots beyond the 16 in LDS."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    sample = 200
    scs = _needle_scene()
    inst = isd.static(ds.deep_instances())
    meshes = ihm.bounds_meshes(scs)
    lo, hi = isd.world_boxes(meshes, inst)[0]
    org, dirs = random_rays_np(4000, lo.astype(np.float32), hi.astype(np.float32), ds.GPU_RAY_SEED)
    rays = ds.rays_of(rtc, ds.snap(org), ih.snap(dirs * 4.0))
    rays["time"] = np.asarray(EIGHTHS, np.float32)[np.arange(len(rays)) % len(EIGHTHS)]
    dev, top, inner = ihm.build(rtc, 1, scs, inst)
    st = top.stats()
    assert st["accelKind"] == 23 and ds.stack_capacity(st["maxDepth"]) > 16
    got, occ = _trace_both(rtc, top, rays)
    assert dev.error() == 0  # the `overflow` word stayed clear: no entry was dropped
    o = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1)[:sample]
    d = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1)[:sample]
    deepest, _ = ihm.simulate_stack(top.accel_data(0).view(ih.NODE_DT), top.accel_root(), top.accel_data(2), len(inst), o, d)
    miss = got["geomID"][:sample] == INVALID
    deep = int((miss & (deepest >= 16)).sum())
    print(f"needle moving hair: maxDepth {st['maxDepth']}, {int(miss.sum())} of {sample} sampled rays miss, {deep} of them pass slot 16, deepest slot {int(deepest.max())}")
    assert deep >= sample // 10 and deepest.max() < ds.stack_capacity(st["maxDepth"])
    per = isd.direct_all(rtc, inner, inst, rays)
    t = np.sort(np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf).astype(np.float64) for p in per]), axis=0)
    with np.errstate(invalid="ignore"):
        clear = ~(np.isfinite(t[1]) & (t[1] - t[0] <= 1e-6 * np.abs(t[0])))  # (the instances overlap: a ray whose two nearest instances tie is left out)
    assert clear.sum() >= 0.99 * len(rays)
    want = isd.merge(rays, per, inst)
    _check(got[clear], want[clear], "needle moving hair")
    hit = want["geomID"] != INVALID
    assert np.array_equal((occ["tfar"] == -np.inf)[clear], hit[clear])
    print(f"needle moving hair: {int(hit.sum())} hits of {len(rays)} rays")
    assert int(hit.sum()) >= 200
    ihm.release(dev, top, inner)
    for k, val in {"RTAMD_CHUNK": "32", "RTAMD_REFILL_BATCH": "1", "RTAMD_LEAF_BATCH": "64"}.items():  # small queue shares repeat the bytes
        monkeypatch.setenv(k, val)
    dev, top, inner = ihm.build(rtc, 1, scs, inst)
    g2, o2 = _trace_both(rtc, top, rays)
    assert g2.tobytes() == got.tobytes() and o2.tobytes() == occ.tobytes() and dev.error() == 0
    ihm.release(dev, top, inner)


# ---- 10. invalid rays; refusals at the call ----------------------------------------------------------------------------------------------------------
def test_invalid_rays_come_back_untouched(rtc):
    scs = ihm.scenes("c")
    rays = isd.crossing_rays(rtc, ihm.bounds_meshes(scs), INST, 1024, 3)
    rays["time"] = 0.375
    dev, top, inner = ihm.build(rtc, 1, scs, INST)
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
    ihm.release(dev, top, inner)


def test_context_filter_and_counted_batches_are_refused_at_the_call(rtc):
    for cfg, text in ((ihm.GPU_CFG, "RTCIntersectContext::filter is not supported on a scene with instances"), (ihm.GPU_CFG + ",inst_filters=1", ihh.REFUSE_CONTEXT)):
        dev, top, inner = ihm.build(rtc, 1, ihm.scenes("a"), [(0, "m", [ih.affine()])], cfg)
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
        ihm.release(dev, top, inner)
