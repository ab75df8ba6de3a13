"""Shared by tests/test_host_edge_rays.py and tests/test_gpu_edge_rays.py: the hard rays of tests/test_gpu_degenerate_rays.py and
tests/test_gpu_secondary.py for the accels that came after them - quads, motion-blur triangles and quads, instances - and the expected
records of every case, all of them from the CPU oracle (no product kernel takes part in an expected side).

edge_rays() is `_degenerate_rays` of test_gpu_degenerate_rays.py with its absolute numbers (3.0 in front of the box, tnear 7.5, tfar up
to 40: sized for the unscaled bomberman, 700 across) made relative to the diagonal of the box; bounce() is `_bounce` of
test_gpu_secondary.py with the primary's time inherited and origins that may be snapped to the 2^-10 grid."""
import numpy as np

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
from helpers import INVALID, fill_rays

F32 = np.float32
ROBUST = 4  # RTC_SCENE_FLAG_ROBUST
TIMES = ds.TIMES  # 0, 1/4, 1/2, 3/4, 1
UNIT = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F32)
BENT = np.array([[0, 0, 0], [1, 0, 0.5], [1, 1, 0.125], [0, 1, 0.25]], F32)  # non-planar, on the grid
Q1 = np.array([[0, 1, 2, 3]], np.uint32)


# ---- 1. the ray families ------------------------------------------------------------------------------------------------------------------
def edge_rays(rtc, lo, hi, n_grid, seed, snapped=False, m=6000, k=3000):
    """RAYHIT records over the box [lo, hi] (diagonal D):
      * 6 n_grid^2 axis-parallel rays, from planes D / 128 in front of the six sides, on the (j + 0.37) / n_grid lattice;
      * m rays from inside the box with ONE random direction component exactly zero; every fifth direction scaled by 2^-10 and every
        fifth + 1 by 256 (powers of two: what is exact stays exact); every third tnear = 0.01 D, every seventh + 1 tnear = 1e30;
        every fourth tfar = rand * 0.06 D;
      * k rays that start exactly on a face of the box and point inwards along the axis.
    snapped: origins on the 2^-10 grid (instance_helpers.snap) - lo and hi are then expected on it."""
    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    diag = float(np.linalg.norm(ext))
    front = diag / 128.0
    org, dirs, tnear, tfar = [], [], [], []
    g = (np.arange(n_grid) + 0.37) / n_grid
    for axis in range(3):
        a, b = [j for j in range(3) if j != axis]
        for sign in (1.0, -1.0):
            o = np.zeros((n_grid * n_grid, 3), np.float64)
            o[:, a] = lo[a] + np.repeat(g, n_grid) * ext[a]
            o[:, b] = lo[b] + np.tile(g, n_grid) * ext[b]
            o[:, axis] = (lo[axis] - front) if sign > 0 else (hi[axis] + front)
            d = np.zeros((len(o), 3), F32)
            d[:, axis] = sign
            org.append(o); dirs.append(d)
            tnear.append(np.zeros(len(o), F32)); tfar.append(np.full(len(o), np.inf, F32))
    o = lo + rng.rand(m, 3) * ext
    d = (rng.rand(m, 3).astype(F32) - F32(0.5))
    d[np.arange(m), rng.randint(0, 3, m)] = 0.0
    d[::5] *= F32(2.0 ** -10)
    d[1::5] *= F32(256.0)
    org.append(o); dirs.append(d)
    tn = np.zeros(m, F32)
    tn[::3] = 0.01 * diag   # hits in front of tnear do not count
    tn[1::7] = 1e30         # tnear > tfar for finite tfar -> skipped, else nothing in range
    tf = np.full(m, np.inf, F32)
    tf[::4] = (rng.rand(len(tf[::4])) * 0.06 * diag).astype(F32)  # short rays
    tnear.append(tn); tfar.append(tf)
    o = lo + rng.rand(k, 3) * ext
    ax = rng.randint(0, 3, k)
    side = rng.randint(0, 2, k)
    o[np.arange(k), ax] = np.where(side == 0, lo[ax], hi[ax])
    d = np.zeros((k, 3), F32)
    d[np.arange(k), ax] = np.where(side == 0, 1.0, -1.0)
    org.append(o); dirs.append(d)
    tnear.append(np.zeros(k, F32)); tfar.append(np.full(k, np.inf, F32))
    org, dirs = np.concatenate(org), np.concatenate(dirs)
    org = ih.snap(org) if snapped else org.astype(F32)
    rays = rtc.aligned_rayhits(len(org))
    fill_rays(rays, org, dirs, tnear=np.concatenate(tnear), tfar=np.concatenate(tfar))
    return rays


def with_times(rays, times=TIMES):
    rays["time"] = np.asarray(times, F32)[np.arange(len(rays)) % len(times)]
    return rays


def bounce(rtc, primary, seed, snapped=False, light=(50.0, 400.0, -120.0)):
    """diffuse-ish bounce rays (RAYHIT) and shadow rays (RAY) towards a point light from the hit points of `primary`, tnear = 0.001,
    ray.time that of the primary.  snapped: origins on the 2^-10 grid, up to 2^-11 off the surface - some self-hits then land just
    above tnear, legitimate hits for both sides."""
    hit = primary["geomID"] != INVALID
    p = primary[hit]
    n = p.shape[0]
    o = np.stack([p["org_x"] + p["tfar"] * p["dir_x"], p["org_y"] + p["tfar"] * p["dir_y"], p["org_z"] + p["tfar"] * p["dir_z"]], 1).astype(F32)
    if snapped:
        o = ih.snap(o)
    ng = np.stack([p["Ng_x"], p["Ng_y"], p["Ng_z"]], 1).astype(np.float64)
    ng /= np.maximum(np.linalg.norm(ng, axis=1, keepdims=True), 1e-30)
    d_in = np.stack([p["dir_x"], p["dir_y"], p["dir_z"]], 1)
    ng[(ng * d_in).sum(1) > 0] *= -1  # face the incoming ray
    rng = np.random.RandomState(seed)
    r = rng.normal(size=(n, 3))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    d = ng + 0.999 * r  # cosine-like lobe around the normal, including grazing directions
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sec = rtc.aligned_rayhits(n)
    fill_rays(sec, o, d.astype(F32), tnear=0.001, tfar=np.inf)
    sec["time"] = p["time"]
    ld = np.asarray(light, np.float64)[None, :] - o
    dist = np.linalg.norm(ld, axis=1)
    sh = rtc.aligned_rays(n)
    fill_rays(sh, o, (ld / dist[:, None]).astype(F32), tnear=0.001, tfar=dist.astype(F32))
    sh["time"] = p["time"]
    return sec, sh


def light_of(lo, hi):
    """the point light of test_gpu_secondary.py, (50, 400, -120) beside a mesh 700 across, relative to the box"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return (lo + hi) / 2 + np.array([0.07, 0.57, -0.17]) * np.linalg.norm(hi - lo)


# ---- 2. meshes and scenes -----------------------------------------------------------------------------------------------------------------
def nonplanar_quads(verts, quads):
    """per quad: the normals of its two split triangles, cross(v1 - v0, v3 - v0) and cross(v3 - v2, v1 - v2), differ in direction:
    |1 - cos| > 1e-6 in float64 (a degenerate quad counts as non-planar)"""
    v = np.asarray(verts, np.float64)[np.asarray(quads)]
    na = np.cross(v[:, 1] - v[:, 0], v[:, 3] - v[:, 0])
    nb = np.cross(v[:, 3] - v[:, 2], v[:, 1] - v[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = (na * nb).sum(1) / (np.linalg.norm(na, axis=1) * np.linalg.norm(nb, axis=1))
    return ~(np.abs(1.0 - cos) <= 1e-6)


def nonplanar_over_time(steps, quads, times=TIMES):
    """non-planar at any of `times` (two planar steps lerp into a non-planar quad when the quad turns)"""
    out = np.zeros(len(quads), bool)
    for t in times:
        out |= nonplanar_quads(ds.at_time(steps, t), quads)
    return out


def static_quads(bomberman):
    """the 727 quads of test_bomberman_quads_1m_parity (unscaled)"""
    v, fs, fi = bomberman
    assert (fs == 4).all() and len(fs) == 727
    return v, fi.reshape(-1, 4).astype(np.uint32)


def two_steps(bomberman, quads):
    """the `two_steps` data of test_gpu_motion_blur.py / test_gpu_quad_motion_blur.py: scaled by 0.0625 and snapped; step 1 rotated by 20
    degrees about y and moved by 0.3 x the extent along x.  Returns ([step 0, step 1], indices)."""
    v, q = static_quads(bomberman)
    s0 = ds.snap(v * ih.SCALE)
    ext = s0.max(0) - s0.min(0)
    s1 = ds.snap(ds.rot_y(s0, 20.0) + np.array([0.3 * ext[0], 0.0, 0.0]))
    idx = q if quads else np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.uint32)  # = rtc.fan_triangulate
    return [s0, s1], idx


def quad_device(rtc, mode, extra=""):
    """as test_gpu_quads.py: mode 0 = robust scene (Pluecker, kind 8), mode 1 = the explicit quad4v accel (Moeller, kind 9)"""
    cfg = "" if mode == 0 else "quad_accel=bvh8.quad4v"
    if extra:
        cfg = (cfg + "," + extra) if cfg else extra
    return rtc.Device(cfg), (ROBUST if mode == 0 else 0)


def top_scene(rtc, what, mode, data, extra=""):
    """a committed top-level scene: what = 'quads' (verts, quads), 'tri.mb' / 'quad.mb' ([steps], indices)"""
    if what == "quads":
        dev, flags = quad_device(rtc, mode, extra)
    else:
        dev, flags = rtc.Device(extra), (ROBUST if mode == 0 else 0)
    sc = rtc.Scene(dev, flags)
    {"quads": sc.add_quads, "tri.mb": sc.add_triangles_mb, "quad.mb": sc.add_quads_mb}[what](*data)
    sc.commit()
    assert sc.stats()["accelKind"] == {"quads": 8, "tri.mb": 10, "quad.mb": 12}[what] + mode
    return dev, sc


def top_data(what, bomberman):
    return static_quads(bomberman) if what == "quads" else two_steps(bomberman, what == "quad.mb")


def top_bounds(what, data):
    return ds.bounds(data[0]) if what == "quads" else ds.bounds(*data[0])


def top_oracle(rtc, po, what, data, rays, mode):
    """(want, isb) of a top-level scene: the split oracle with the B mapping for quads, one static oracle scene per time for the moving meshes"""
    if what != "quads":
        return ds.oracle_per_time(rtc, po, data[0], data[1], rays, mode, nthreads=16)
    want = iq.copy(rtc, rays)
    orc = iq.split_oracle(po, data[0], data[1], mode)
    orc.intersect1M(want, nthreads=16)
    orc.free()
    return want, iq.map_b(want)


def top_nonplanar(what, data):
    if what == "tri.mb":
        return None
    return nonplanar_quads(*data) if what == "quads" else nonplanar_over_time(*data)


def top_edge_rays(rtc, what, data):
    """section 2 of the suite: n_grid 70 on the static quads, 24 over the bounds of both steps, times cycling through TIMES"""
    lo, hi = top_bounds(what, data)
    if what == "quads":
        return edge_rays(rtc, lo, hi, 70, 4)
    return with_times(edge_rays(rtc, lo, hi, 24, 4))


def top_primaries(rtc, po, what, data, m=200_000, seed=51):
    lo, hi = top_bounds(what, data)
    rays = rtc.aligned_rayhits(m)
    rays[:] = po.make_random_rays(m, lo, hi, seed=seed)
    return rays if what == "quads" else with_times(rays)


# ---- instances --------------------------------------------------------------------------------------------------------------------------
def instance_sets(which):
    """'exact': im.exact_instances(6), moving, signed axis permutations times power-of-two scales; 'grid': the nine static
    iq.grid_instances(9); 'general': im.general_instances() (rotations, non-uniform scales, moving)"""
    if which == "exact":
        return im.exact_instances(6)
    if which == "grid":
        return [(g, k, [m]) for g, k, m in iq.grid_instances(9)]
    return im.general_instances()


def instance_box(scenes, inst):
    """the outward-rounded integer box of all instances over all their steps"""
    flat = [(g, k, s) for g, k, steps in inst for s in steps]
    lo, hi = ih.instances_bounds(imm.bounds_meshes(scenes), flat)
    return np.floor(lo), np.ceil(hi)


def instance_edge_rays(rtc, scenes, inst):
    lo, hi = instance_box(scenes, inst)
    return with_times(edge_rays(rtc, lo, hi, 40, 4, snapped=True, m=3000, k=1500))


def instance_nonplanar(scenes):
    """{geomID: per-quad mask} of the quad parts of scene "m" """
    d, out = scenes["m"], {}
    if d.get("quads") is not None:
        out[d["quads"][2]] = nonplanar_quads(d["quads"][0], d["quads"][1])
    if d.get("quads_mb") is not None:
        out[d["quads_mb"][2]] = nonplanar_over_time(d["quads_mb"][0], d["quads_mb"][1])
    return out


def single_tri_instance(bomberman):
    """a static triangle mesh under one static instance (kinds 14 / 15): (scenes, instances) as instance_quads_helpers describes them"""
    v, q = iq.bomberman_quads(bomberman)
    t = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.uint32)
    return {"m": {"tris": (v, t, 0), "quads": None}}, [(0, "m", ih.affine((3.0, -1.5, 0.25), (2.0, 2.0, 2.0)))]


# ---- checks that need no GPU ----------------------------------------------------------------------------------------------------------------
def occluded_expected(rtc, rays, want):
    """RAY records as rtcOccluded1M must leave them: tfar = -inf exactly where the oracle hits, every other byte as it was"""
    occ = iq.occ_of(rtc, rays)
    occ["tfar"][want["geomID"] != INVALID] = -np.inf
    return occ


def counts(want, rays, gids=None, n_inst=None):
    """what a case exercises, measured on the oracle's records: hits, the smallest number of hits per time / geomID / instance"""
    hit = want["geomID"] != INVALID
    out = {"rays": len(want), "hits": int(hit.sum())}
    out["per_time"] = min(int((hit & (rays["time"] == t)).sum()) for t in np.unique(rays["time"]))
    if gids is not None:
        out["per_geom"] = min(int((want["geomID"][hit] == g).sum()) for g in gids)
    if n_inst is not None:
        out["per_inst"] = min(int((want["instID"][hit] == i).sum()) for i in range(n_inst))
    return out


# ---- the v1-v3 diagonal, closed form ------------------------------------------------------------------------------------------------------
def diagonal_rays(quad, n=64):
    """n rays exactly through the v1-v3 diagonal of `quad` (vertices on the grid), through v1 and v3 themselves among them: targets
    v1 + s (v3 - v1) with s = j / 16, directions axis-parallel and oblique with dyadic components, origins target - 2 d - all exact in
    fp32, so that the ray passes through the diagonal itself and A and B tie.  Returns (org, dirs)."""
    v1, v3 = quad[1].astype(np.float64), quad[3].astype(np.float64)
    dset = np.array([[0, 0, 1], [0, 0, -1], [0.5, 0.25, 1], [-0.25, 0.5, 1], [0.75, -0.5, -1], [1, 1, 1], [0.125, 0, 1], [0, -0.375, 1]], np.float64)
    s = (np.arange(n) % 17) / 16.0  # 0 and 1: the vertices v1 and v3
    tg = v1[None, :] + s[:, None] * (v3 - v1)[None, :]
    d = dset[(np.arange(n) // 17 + np.arange(n)) % len(dset)]
    org = tg - 2.0 * d
    assert np.array_equal(org.astype(F32).astype(np.float64), org) and np.array_equal(tg.astype(F32).astype(np.float64), tg)
    return org.astype(F32), d.astype(F32)


def _soa4(p):
    return np.ascontiguousarray(np.tile(np.asarray(p, F32)[None, :], (4, 1)).T.reshape(-1))  # x[4], y[4], z[4]: the quad in all four lanes


def diagonal_expected(rtc, po, quad, org, dirs, mode, prefer_b=False):
    """The records of the single quad `quad` from the oracle's block entry points, as test_block_semantics_against_the_oracle_blocks
    reads them: A = (v0, v1, v3) in lanes 0-3, B = (v2, v1, v3) in lanes 4-7, select_min takes the smaller t and on equal t the lowest
    lane, i.e. A.  prefer_b: the mutation - B on equal t.  Returns (want, want_other, tie, near): want_other = the records with the
    other triangle where both are hit, tie = t bit-identical on A and B, near = both hit within 1e-6 relative but not bit-identical
    (the oracle's rcp is rcpps + Newton: there either candidate is accepted)."""
    L = po.lib()
    blockfn = L.orc_pluecker_block if mode == 0 else L.orc_moeller_block
    v0, v1, v2, v3 = (_soa4(quad[j]) for j in range(4))
    n = len(org)
    want = rtc.aligned_rayhits(n)
    fill_rays(want, org, dirs)
    other = want.copy()
    tie, near, isb = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    out = np.zeros(6, F32)

    def put(rec, i, r, b):
        rec["geomID"][i], rec["primID"][i], rec["tfar"][i] = 0, 0, r[0]
        if b:  # the B mapping
            rec["u"][i], rec["v"][i] = F32(1) - r[2], F32(1) - r[1]
            rec["Ng_x"][i], rec["Ng_y"][i], rec["Ng_z"][i] = -r[3:6]
        else:
            rec["u"][i], rec["v"][i] = r[1], r[2]
            rec["Ng_x"][i], rec["Ng_y"][i], rec["Ng_z"][i] = r[3:6]

    for i in range(n):
        o, d = np.ascontiguousarray(org[i]), np.ascontiguousarray(dirs[i])
        la = blockfn(v0.ctypes.data, v1.ctypes.data, v3.ctypes.data, o.ctypes.data, d.ctypes.data, 0.0, np.inf, out.ctypes.data)
        ra = out.copy()
        lb = blockfn(v2.ctypes.data, v1.ctypes.data, v3.ctypes.data, o.ctypes.data, d.ctypes.data, 0.0, np.inf, out.ctypes.data)
        rb = out.copy()
        if la < 0 and lb < 0:
            continue
        both = la >= 0 and lb >= 0
        tie[i] = both and ra[0] == rb[0]
        near[i] = both and not tie[i] and abs(float(ra[0]) - float(rb[0])) <= 1e-6 * abs(float(ra[0]))
        useb = la < 0 or (lb >= 0 and (rb[0] <= ra[0] if prefer_b else rb[0] < ra[0]))
        isb[i] = useb
        put(want, i, rb if useb else ra, useb)
        if both:
            put(other, i, ra if useb else rb, not useb)
        else:
            other[i] = want[i]
    return want, other, tie, near, isb


# ---- the kinds the pipelined and the sharded host paths trace besides triangles and cBVH blobs ------------------------------------------------
HOST_KINDS = ("quad.mb", "inst.meshmb")


def host_scene(rtc, cfg, bomberman, kind):
    """(device, committed scene) on a device created from `cfg`: 'quad.mb' = the two-step quads (Moeller), 'inst.meshmb' = imm.scenes_c
    under im.general_instances() (Pluecker); the scene's release() also releases the instanced scenes"""
    if kind == "quad.mb":
        return top_scene(rtc, "quad.mb", 1, two_steps(bomberman, True), cfg)
    dev, top, inner = imm.build(rtc, 0, imm.scenes_c(bomberman), im.general_instances(), cfg)
    assert top.stats()["accelKind"] == imm.kind(0)
    release_top = top.release

    def release():
        release_top()
        for s in inner.values():
            s.release()

    top.release = release
    return dev, top


def host_bounds(bomberman, kind):
    """the box the rays of a host-path test are drawn from"""
    if kind == "quad.mb":
        return ds.bounds(*two_steps(bomberman, True)[0])
    if kind == "inst.meshmb":
        inst = im.general_instances()
        lo, hi = ih.instances_bounds(imm.bounds_meshes(imm.scenes_c(bomberman)), [(g, k, s) for g, k, steps in inst for s in steps])
        return lo.astype(F32), hi.astype(F32)
    return bomberman[0].min(0), bomberman[0].max(0)


def host_rays(po, kind, n, lo, hi, seed):
    """po.make_random_rays; on the kinds that read it, ray.time random in [0, 1]"""
    rays = po.make_random_rays(n, lo, hi, seed=seed)
    if kind in HOST_KINDS:
        rays["time"] = np.random.RandomState(seed + 1000).rand(n).astype(F32)
    return rays
