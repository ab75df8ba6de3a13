"""Shared by tests/test_host_instance_filters.py and tests/test_gpu_instance_filters.py: filter functions on instanced meshes (device
config inst_filters=1).

Two families of scenes:
 * the quad stack of tests/test_gpu_filters.py (NQ unit quads at z = 0..NQ-1, geomID = z, two triangles each, rays along +z) as the
   INSTANCED scene, placed by translations on the 2^-10 grid, so that the local ray is exact and every t is the closed form;
 * small multi-geometry scenes (four layers of the 4 x 4 grid mesh of tests/mb_linear_helpers.py) under the general transforms of
   instance_helpers.general_instances(), for the equivalence "a filter that rejects the hits on the geometries of a set R" == "the same
   top scene, unfiltered, with the geometries of R disabled in the instanced scene".  That anchor needs neither the code under test nor
   hand-made expectations; what it does need is that no ray has two candidates at a bit-identical t (the two sides have different
   trees, and a tie goes to the candidate met first): such rays are counted with the oracle alone - the layers split into triangles
   at the ray's time, traced per instance with the instance's local rays, ties between instances counted by
   instance_helpers.equal_t_ties - and set aside; the seed is pinned so that they stay below 1 % (asserted in equivalence_case, on the CPU)."""
import ctypes as C

import numpy as np

import instance_helpers as ih
import instance_mb_helpers as imb
import mb_linear_helpers as mbl

INVALID = 0xFFFFFFFF
NQ = 5
SQUARE = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
SQUARE_TRIS = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)  # primID 0 covers y < x, primID 1 y > x
ROBUST_CFG = "tri_accel=bvh8.triangle4v"
HOST_CFG = "gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,inst_accel=default"


def cfg(robust=False, key=True, extra=""):
    return ",".join(p for p in ("inst_filters=1" if key else "", ROBUST_CFG if robust else "", extra) if p)


# ---- what a callback sees ----------------------------------------------------------------------------------------------------------
class Args:
    """the fields of RTCFilterFunctionNArguments for N = 1"""

    def __init__(self, rtc, args):
        a = args.contents
        self.a = a
        self.rayf = C.cast(a.ray, C.POINTER(C.c_float * 12)).contents
        self.rayu = C.cast(a.ray, C.POINTER(C.c_uint * 12)).contents
        self.hit = C.cast(a.hit, C.POINTER(C.c_uint * 8)).contents
        self.ctx = C.cast(a.context, C.POINTER(rtc.RTCIntersectContext)).contents

    x = property(lambda s: s.rayf[0])
    y = property(lambda s: s.rayf[1])
    tfar = property(lambda s: s.rayf[8])
    ray_id = property(lambda s: s.rayu[10])
    prim = property(lambda s: s.hit[5])
    geom = property(lambda s: s.hit[6])
    inst = property(lambda s: s.hit[7])

    def reject(self):
        self.a.valid[0] = 0


CALLBACK_ERRORS = []  # an exception inside a ctypes callback is printed and dropped: collected here, checked by the tests after the call


def filter_func(rtc, body):
    """FILTER_FUNC around body(Args); what body raises (a failed assert) lands in CALLBACK_ERRORS"""
    def wrapper(args):
        try:
            body(Args(rtc, args))
        except BaseException as e:  # noqa: B902
            CALLBACK_ERRORS.append(e)
    return rtc.FILTER_FUNC(wrapper)


def context_with(rtc, fn, inst_id=INVALID):
    ctx = rtc.make_context(inst_id=inst_id)
    ctx.filter = C.cast(fn, C.c_void_p)
    return ctx


# ---- the instanced quad stack --------------------------------------------------------------------------------------------------------
def stack_scene(rtc, dev, quads=False, nq=NQ):
    """the stack as a scene of its own; quads: RTC_GEOMETRY_TYPE_QUAD geometries (one quad each) instead of two triangles"""
    sc = rtc.Scene(dev)
    for z in range(nq):
        v = (SQUARE + (0, 0, z)).astype(np.float32)
        g = sc.add_quads(v, np.array([[0, 1, 2, 3]], np.uint32)) if quads else sc.add_triangles(v, SQUARE_TRIS)
        assert g == z
    return sc


def stack_top(rtc, config, places, intersect=None, occluded=None, filtered=range(NQ), extra=None, quads=False, nq=NQ):
    """device(config), the stack with `intersect` / `occluded` on the geometries `filtered`, and a top scene with one instance per entry of
    places = [(geomID, translation)].  Returns (dev, top, inner)."""
    dev = rtc.Device(config)
    inner = stack_scene(rtc, dev, quads, nq)
    if intersect is not None or occluded is not None:
        for g in filtered:
            inner.set_filters(g, intersect=intersect, occluded=occluded)
    inner.commit()
    top = rtc.Scene(dev)
    for gid, t in places:
        assert top.add_instance(inner, ih.affine(t), geom_id=gid) == gid
    if extra:
        extra(top)
    top.commit()
    return dev, top, inner


def release(dev, top, inner):
    top.release()
    inner.release()
    dev.release()


def stack_rays(rtc, n, places, seed=1):
    """ray i goes through instance places[i % len(places)] along +z from z = -1 (of that instance), x and y on the 2^-10 grid inside
    (0.05, 0.95) and off the diagonals; ray.id = i.  Returns (rayhits, local x, local y, index into places)."""
    rng = np.random.RandomState(seed)
    which = np.arange(n) % len(places)
    xl = ih.snap(rng.rand(n) * 0.9 + 0.05)
    yl = ih.snap(rng.rand(n) * 0.9 + 0.05)
    yl = np.where(np.abs(yl - xl) < 2.0 ** -9, yl + np.float32(2.0 ** -8) * np.where(yl < 0.5, 1, -1), yl).astype(np.float32)
    yl = np.where(np.abs(yl + xl - 1) < 2.0 ** -9, yl + np.float32(2.0 ** -8) * np.where(yl < 0.5, 1, -1), yl).astype(np.float32)
    t = np.array([places[k][1] for k in which], np.float64)
    org = np.stack([xl + t[:, 0], yl + t[:, 1], t[:, 2] - 1.0], 1)
    assert np.array_equal(org.astype(np.float32).astype(np.float64), org)
    rh = rtc.aligned_rayhits(n)
    rh["org_x"], rh["org_y"], rh["org_z"] = org[:, 0], org[:, 1], org[:, 2]
    rh["dir_x"], rh["dir_y"], rh["dir_z"] = 0, 0, 1
    rh["tnear"], rh["tfar"], rh["time"] = 0, np.inf, 0
    rh["mask"], rh["id"], rh["flags"] = 0xFFFFFFFF, np.arange(n), 0
    rh["geomID"] = rh["primID"] = rh["instID"] = INVALID
    return rh, xl, yl, which


def occ_of(rtc, rays):
    occ = rtc.aligned_rays(len(rays))
    for f in occ.dtype.names:
        occ[f] = rays[f]
    return occ


def copy_of(rtc, rays):
    out = rtc.aligned_rayhits(len(rays))
    out[:] = rays
    return out


# ---- equivalence with disabled geometry ----------------------------------------------------------------------------------------------
EQ_RAYS = 3000
EQ_SEED = 41
EQ_TIMES = 8  # ray times are multiples of 1 / 8
EQ_KINDS = {"tri": (14, 15), "triquad": (16, 17), "triquad_xfmb": (20, 21), "meshmb": (22, 23), "meshmb_linear": (30, 31)}
EQ_CFG = {"meshmb_linear": "mb_bounds=linear,inst_mb_bounds=linear"}
EQ_REJECTED = {"tri": (1, 3), "triquad": (1, 2), "triquad_xfmb": (1, 2), "meshmb": (1, 3), "meshmb_linear": (1, 3)}
ROBUST_FLAG = 4  # RTC_SCENE_FLAG_ROBUST: mode 0 = Pluecker / robust, mode 1 = Moeller / fast


def eq_pieces(form):
    """[(type "tri" | "quad", geomID, [vertices per time step], indices)]: four layers of the warped 4 x 4 grid mesh of
    mb_linear_helpers (32 triangles or 16 quads each), scaled by 8 and 3 apart in z, on the 2^-10 grid; a ray through the stack meets all
    four, so that rejecting the geometries of R uncovers what lies behind them.  Which layers are quads or have a second time step is the
    form's: "tri" 14 / 15, "triquad" 16 / 17 (and 20 / 21 with a moving instance), "meshmb" 22 / 23 (and 30 / 31 under linear bounds)."""
    vt, t = mbl.grid_tris(4)
    _, q = mbl.grid_quads(4)
    layer = lambda k: ih.snap(vt.astype(np.float64) * 8.0 + (0.0, 0.0, 3.0 * k))  # noqa: E731
    moved = lambda v: ih.snap(v.astype(np.float64) + (0.5, -0.25, 0.75))  # noqa: E731
    if form == "tri":
        return [("tri", k, [layer(k)], t) for k in range(4)]
    if form in ("triquad", "triquad_xfmb"):
        return [("tri", 0, [layer(0)], t), ("tri", 1, [layer(1)], t), ("quad", 2, [layer(2)], q), ("quad", 3, [layer(3)], q)]
    assert form in ("meshmb", "meshmb_linear")
    return [("tri", 0, [layer(0)], t), ("tri", 1, [layer(1), moved(layer(1))], t), ("quad", 2, [layer(2)], q), ("quad", 3, [layer(3), moved(layer(3))], q)]


def eq_instances(form):
    """instance_helpers.general_instances(); in the form with instance steps instance 4 moves (a second step 3 further along x)"""
    out = []
    for g, _, m in ih.general_instances():
        steps = [m]
        if form == "triquad_xfmb" and g == 4:
            m1 = m.copy()
            m1[0, 3] += np.float32(3.0)
            steps.append(m1)
        out.append((g, steps))
    return out


def eq_rays(rtc, po, pieces, instances, m=EQ_RAYS, seed=EQ_SEED):
    """random rays through the instances' common box (instance_helpers.general_rays), ray times multiples of 1 / EQ_TIMES"""
    allv = np.concatenate([v for _, _, steps, _ in pieces for v in steps])
    rays = ih.general_rays(rtc, po, {"m": (allv,)}, [(g, "m", steps[0]) for g, steps in instances], m=m, seed=seed)
    rays["time"] = (np.random.RandomState(seed).randint(0, EQ_TIMES + 1, m) / float(EQ_TIMES)).astype(np.float32)
    rays["id"] = np.arange(m)
    return rays


def eq_build(rtc, config, mode, pieces, instances, intersect=None, disabled=()):
    """-> (dev, top, inner): the instanced scene of `pieces` (with `intersect` on every geometry, the geometries `disabled` disabled)
    below `instances`"""
    dev = rtc.Device(config)
    flags = ROBUST_FLAG if mode == 0 else 0
    inner = rtc.Scene(dev, flags)
    for typ, gid, steps, idx in pieces:
        if typ == "tri":
            g = inner.add_triangles(steps[0], idx, geom_id=gid) if len(steps) == 1 else inner.add_triangles_mb(steps, idx, geom_id=gid)
        else:
            g = inner.add_quads(steps[0], idx, geom_id=gid) if len(steps) == 1 else inner.add_quads_mb(steps, idx, geom_id=gid)
        assert g == gid
        if intersect is not None:
            inner.set_filters(gid, intersect=intersect)
        if gid in disabled:
            inner.set_enabled(gid, False)
    inner.commit()
    top = rtc.Scene(dev, flags)
    for gid, steps in instances:
        g = top.add_instance(inner, steps[0], geom_id=gid) if len(steps) == 1 else top.add_instance_mb(inner, steps, geom_id=gid)
        assert g == gid
    top.commit()
    return dev, top, inner


def _split_triangles(pieces, time, skip=()):
    """all pieces as one triangle soup at `time` (vertices interpolated as the kernels do, mb_linear_helpers.lerp_vertex; quads split
    into (v0, v1, v3) and (v2, v1, v3)): (verts, tris, geomIDs)"""
    verts, tris, gids, base = [], [], [], 0
    for typ, gid, steps, idx in pieces:
        if gid in skip:
            continue
        v = steps[0] if len(steps) == 1 else mbl.lerp_vertex(steps[0], steps[1], np.float32(time))
        t = idx if typ == "tri" else np.concatenate([idx[:, [0, 1, 3]], idx[:, [2, 1, 3]]])
        verts.append(np.asarray(v, np.float32))
        tris.append(t.astype(np.uint32) + base)
        gids.append(np.full(len(t), gid, np.uint32))
        base += len(v)
    return np.concatenate(verts), np.concatenate(tris), np.concatenate(gids)


def eq_oracle_per_instance(rtc, po, pieces, instances, rays, mode, skip=()):
    """per[i] = the oracle's closest hit of every ray on instance i alone: local rays at the ray's time, the triangle soup at that time"""
    timed = any(len(steps) > 1 for _, _, steps, _ in pieces)
    groups = [(tau, rays["time"] == np.float32(tau)) for tau in np.arange(EQ_TIMES + 1) / float(EQ_TIMES)] if timed else [(0.0, np.ones(len(rays), bool))]
    per = [rtc.aligned_rayhits(len(rays)) for _ in instances]
    for tau, sel in groups:
        if not sel.any():
            continue
        v, t, g = _split_triangles(pieces, tau, skip)
        orc = po.TriangleScene(v, t, mode, g)
        for i, (gid, steps) in enumerate(instances):
            sub = rtc.aligned_rayhits(int(sel.sum()))
            if len(steps) == 1:
                sub[:] = ih.local_rays(rays[sel], ih.world2local(steps[0]))
            else:
                w2l, ok = imb.world2local_at(steps, rays["time"][sel])
                sub[:] = imb.local_rays(rays[sel], w2l, ok)
            orc.intersect1M(sub, inst_id=gid, nthreads=8)
            per[i][sel] = sub
        orc.free()
    return per


def tie_mask(per):
    """rays for which two instances report the same t (the rays instance_helpers.equal_t_ties counts)"""
    t = np.sort(np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf) for p in per]), axis=0)
    m = np.isfinite(t[0]) & (t[0] == t[1])
    assert int(m.sum()) == ih.equal_t_ties(per)
    return m


def equivalence_case(rtc, po, form, mode):
    """-> (pieces, instances, rays, R, aside): the CPU part.  aside = rays with a tie at a bit-identical t on either side (all
    geometries; without those of R), by the oracle alone; at most 1 % of the rays, and the case must have rays that hit behind a rejected
    layer for the check to mean anything."""
    pieces, instances = eq_pieces(form), eq_instances(form)
    rays = eq_rays(rtc, po, pieces, instances)
    rejected = EQ_REJECTED[form]
    full = eq_oracle_per_instance(rtc, po, pieces, instances, rays, mode)
    reduced = eq_oracle_per_instance(rtc, po, pieces, instances, rays, mode, skip=rejected)
    aside = tie_mask(full) | tie_mask(reduced)
    assert aside.sum() <= 0.01 * len(rays), (form, mode, int(aside.sum()))
    first = np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf) for p in full])
    best = np.argmin(first, axis=0)
    gid = np.stack([p["geomID"] for p in full])[best, np.arange(len(rays))]
    uncovered = np.isfinite(first.min(0)) & np.isin(gid, rejected) & np.isfinite(np.stack([np.where(p["geomID"] != INVALID, p["tfar"], np.inf) for p in reduced]).min(0))
    assert uncovered.sum() >= 50, (form, mode, int(uncovered.sum()))
    return pieces, instances, rays, rejected, aside
