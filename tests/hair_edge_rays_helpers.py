"""Shared by tests/test_host_hair_edge_rays.py and tests/test_gpu_hair_edge_rays.py: the hard rays of tests/edge_rays_helpers.py
(edge_rays, with_times, bounce - as they are) over the unit cube every pinned hair input lives in, for the hair family: line segments
(kinds 36 / 37), flat curves (42 / 43, Bezier at rate 4 and the same control points read as a B-spline at rate 9), round curves (42 / 43
with round_curves=1), their motion-blur forms (38 .. 41, 44 .. 47) and hair below instances (22 / 23 with inst_hair=1).

Every expected side is the float64 truth the kind already has - line_helpers.closest, curve_helpers.closest, round_curve_helpers.truth,
line_mb_helpers.moving_truth, curve_mb_helpers.moving_truth, instance_hair_helpers.lines_truth64 / curves_truth64 - never a product
kernel.  check() compares under the kind's own rules (curve_helpers.compare, round_curve_helpers.compare: hit / miss and IDs exact, t
within 1e-4 relative, u and v within 1e-4 absolute, at most 0.5 % of the rays left out and only by the truth's own conditions), and adds
what the parity tests of the kinds add: Ng, a miss comes back untouched, occluded sets tfar = -inf exactly where the truth hits and
leaves every other byte alone.  Truths are computed once per process and shared by the parametrisations."""
import numpy as np

import curve_helpers as ch
import curve_mb_helpers as cmh
import edge_rays_helpers as er
import instance_hair_helpers as ihh
import instance_helpers as ih
import instance_mb_helpers as im
import line_helpers as lh
import line_mb_helpers as lmh
import round_curve_helpers as rh
from helpers import INVALID

F32 = np.float32
GID = 7
LO, HI = np.zeros(3), np.ones(3)
STATIC = ("lines", "curves", "bspline", "round")
MOVING = ("lines.mb", "curves.mb")
# The kinds that take the surface-origin rays.  Round curves do not: a ray that starts ON a tube has its closest approach, 0, at its
# origin, and the grazing rule of round_curve_helpers.truth (a miss whose closest approach is within 1e-4 of 0 is left out) leaves out
# every miss among them - 380 of the 685 bounce rays of input (b), far over the 0.5 % cap, measured on the truth alone.  Nor is there a
# self-intersection rule on a tube to decide the root at the origin: with tnear = 0 the exit root at t = 0 +- rounding is in or out by
# an ulp.  The flat kinds have `t > tnear + 2 r s`, which removes the ambiguity, and keep the cap (1 ray of 3239, 1 of 1078).
SURFACE = ("lines", "curves", "bspline") + MOVING
SCALES = (-20, -10, 10, 20)  # the exponents of the direction-scale cases
TIMES = er.TIMES
SHORT = 1e-2  # |dir| below this: the rays the Newton bound of the tube leaf is short for
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def fields(rays):
    """(org [m, 3], dirs [m, 3], tnear [m], tfar [m]) of RAY / RAYHIT records, float32"""
    return (np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1), np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1),
            rays["tnear"].copy(), rays["tfar"].copy())


def copy(rtc, rays):
    out = rtc.aligned_rayhits(len(rays)) if "geomID" in rays.dtype.names else rtc.aligned_rays(len(rays))
    out[:] = rays
    return out


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def geometry(kind):
    """what a kind traces: dict of cfg (device config), add(scene), org / dirs (its pinned rays) and, for the moving kinds, times"""
    def make():
        if kind == "lines":
            v, idx, org, dirs = lh.tuft_and_rays()
            return {"cfg": "", "add": lambda s: s.add_lines(v, idx, geom_id=GID), "v": v, "idx": idx, "org": org, "dirs": dirs}
        if kind in ("curves", "bspline"):
            v, idx, org, dirs = ch.hair_and_rays()
            basis, rate = ("bezier", 4) if kind == "curves" else ("bspline", 9)
            return {"cfg": "", "add": lambda s: s.add_curves(v, idx, basis=basis, tessellation_rate=rate, geom_id=GID), "cp": ch.native(v, idx, basis), "N": rate,
                    "org": org, "dirs": dirs}
        if kind == "round":
            v, idx, org, dirs = rh.pinned("b")
            return {"cfg": "round_curves=1", "add": lambda s: s.add_round_curves(v, idx, geom_id=GID), "cp": ch.native(v, idx), "org": org, "dirs": dirs}
        if kind == "lines.mb":
            steps, idx, org, dirs = lmh.tuft_steps(2)
            return {"cfg": "", "add": lambda s: s.add_lines_mb(steps, idx, geom_id=GID), "steps": steps, "idx": idx, "org": org, "dirs": dirs,
                    "times": lmh.round_robin_times(len(org), 2)}
        if kind == "curves.mb":
            steps, idx, org, dirs = cmh.hair_steps(2)
            return {"cfg": "", "add": lambda s: s.add_curves_mb(steps, idx, tessellation_rate=4, geom_id=GID), "nat": cmh.native_steps(steps, idx), "N": 4,
                    "org": org, "dirs": dirs, "times": cmh.round_robin_times(len(org), 2)}
        raise KeyError(kind)
    return _once(("geometry", kind), make)


# ---- truths ---------------------------------------------------------------------------------------------------------------------------
def _norm_lines(c):
    """line_helpers.closest in the shape curve_helpers.compare reads"""
    m = len(c["hit"])
    c = dict(c)
    c.update(geomID=np.full(m, GID, np.int64), primID=c["seg"].astype(np.int64), v=np.zeros(m))
    return c


def truth(kind, org, dirs, tnear, tfar, times=None, self_rule=True):
    """the kind's float64 truth of the rays, in one shape: hit, geomID (GID), primID, t, u, v, Ng and the kind's left-out conditions (`out`)"""
    g = geometry(kind)
    if kind == "lines":
        v0, v1 = lh.ends(g["v"], g["idx"])
        c = _norm_lines(lh.closest(v0, v1, org, dirs, tnear, tfar, np.float64, self_rule=self_rule))
    elif kind in ("curves", "bspline"):
        c = dict(ch.closest([(g["cp"], g["N"], GID)], org, dirs, tnear, tfar, np.float64))
    elif kind == "round":
        return rh.truth([(g["cp"], GID)], org, dirs, tnear, tfar)
    elif kind == "lines.mb":
        c = _norm_lines(lmh.moving_truth(g["steps"], g["idx"], org, dirs, times, np.float64, tnear=tnear, tfar=tfar))
    elif kind == "curves.mb":
        c = dict(cmh.moving_truth(g["nat"], g["N"], org, dirs, times, np.float64, geom_id=GID, tnear=tnear, tfar=tfar))
    else:
        raise KeyError(kind)
    c["out"] = c["near_edge"] | c["near_tie"]
    return c


def restated(kind, org, dirs, tnear, tfar, reference_bound=False):
    """the float32 restatement of the kind's leaf, in the shape of truth() (static lines, flat curves and round curves have one);
    reference_bound: the tube leaf's Newton with the reference's bound 16 ulp |dir|"""
    g = geometry(kind)
    if kind == "lines":
        v0, v1 = lh.ends(g["v"], g["idx"])
        return _norm_lines(lh.closest(v0, v1, org, dirs, tnear, tfar, np.float32))
    if kind in ("curves", "bspline"):
        return dict(ch.closest([(g["cp"], g["N"], GID)], org, dirs, tnear, tfar, np.float32))
    return rh.restate([(g["cp"], GID)], org, dirs, tnear, tfar, np.float32, reference_bound=reference_bound)


def records_of(rtc, rays, c):
    """RAYHIT records of `rays` with the hits of a truth / restatement dict written in"""
    out = copy(rtc, rays)
    h = c["hit"]
    out["tfar"][h] = c["t"][h]
    out["geomID"][h], out["primID"][h] = c["geomID"][h], c["primID"][h]
    out["u"][h], out["v"][h] = c["u"][h], np.asarray(c.get("v", np.zeros(len(h))))[h]
    out["Ng_x"][h], out["Ng_y"][h], out["Ng_z"][h] = c["Ng"][h, 0], c["Ng"][h, 1], c["Ng"][h, 2]
    if "inst" in c:
        out["instID"][h] = c["inst"][h]
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def degenerate_rays(rtc, kind):
    """er.edge_rays over the unit cube, seed 7: n_grid 16, m 2000, k 1000 (4536 rays); round curves n_grid 12, m 1500, k 600 (2964 rays:
    the truth costs 3 ms a ray, and a smaller set breaks the 0.5 % cap on grazing rays alone).  The moving kinds: times cycling k / 4"""
    rays = er.edge_rays(rtc, LO, HI, 12, 7, m=1500, k=600) if kind == "round" else er.edge_rays(rtc, LO, HI, 16, 7, m=2000, k=1000)
    return er.with_times(rays) if kind in MOVING else rays


def degenerate_case(rtc, kind):
    """(rays, truth) of the degenerate family; the rays are the caller's to change, the truth is shared"""
    rays = degenerate_rays(rtc, kind)
    return rays, _once(("degenerate", kind), lambda: truth(kind, *fields(rays), times=rays["time"] if kind in MOVING else None))


def pinned_truth(kind):
    """the truth of the kind's pinned rays, tnear 0 and tfar inf (the kinds' own caches where they have one)"""
    def make():
        g = geometry(kind)
        if kind == "round":
            c = dict(rh.pinned_truth("b"))
            c["geomID"] = np.where(c["hit"], GID, -1)
            return c
        if kind == "curves":
            c = dict(ch.hair_truth(4))
            c.update(geomID=np.full(len(c["hit"]), GID, np.int64), out=c["near_edge"] | c["near_tie"])
            return c
        m = len(g["org"])
        return truth(kind, g["org"], g["dirs"], np.zeros(m, F32), np.full(m, np.inf, F32), times=g.get("times"))
    return _once(("pinned", kind), make)


def pinned_rays(rtc, kind, exponent=0):
    g = geometry(kind)
    rays = lh.rays_of(rtc, g["org"], (g["dirs"] * F32(2.0 ** exponent)).astype(F32))
    if "times" in g:
        rays["time"] = g["times"]
    return rays


def scaled_case(rtc, kind, exponent):
    """the pinned rays with dir multiplied by 2^exponent - exact, so the expected side is the pinned truth with t divided by the same
    factor: u, v, the IDs and the direction of Ng are unchanged, and no truth is computed"""
    c = dict(pinned_truth(kind))
    c["t"] = c["t"] / 2.0 ** exponent
    if "dirs" in c:  # round_curve_helpers.compare evaluates the normal at org + t dirs
        c["dirs"] = c["dirs"] * 2.0 ** exponent
    return pinned_rays(rtc, kind, exponent), c


def bounce_rays(rtc, primary, tnear):
    """er.bounce from the hits of `primary` towards er.light_of the unit cube, the bounce and the shadow rays with `tnear`"""
    sec, sh = er.bounce(rtc, primary, 11, light=er.light_of(LO, HI))
    sec["tnear"], sh["tnear"] = tnear, tnear
    return sec, sh


def as_rayhits(rtc, sh):
    """RAY records as RAYHIT records: a shadow ray is occluded iff it hits"""
    full = lh.rays_of(rtc, np.zeros((len(sh), 3), F32), np.zeros((len(sh), 3), F32))
    for f in sh.dtype.names:
        full[f] = sh[f]
    return full


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------
def check(kind, got, rays, want, what, occ=None):
    """`got` (RAYHIT records: a kernel's or records_of a restatement) against the truth `want` on `rays`; occ: the RAY records occluded1M
    left of the same rays.  Returns {"hits", "out", "t", "u"}; raises AssertionError where the contract is missed."""
    gh = got["geomID"] != INVALID
    geom, prim = np.where(gh, got["geomID"].astype(np.int64), -1), np.where(gh, got["primID"].astype(np.int64), -1)
    ng = np.stack([got["Ng_x"], got["Ng_y"], got["Ng_z"]], 1)
    if kind == "round":
        left, mt, mu, _ = rh.compare(gh, geom, prim, got["tfar"], got["u"], got["v"], ng, want, what)
    else:
        left, mt, mu, _ = ch.compare(gh, geom, prim, got["tfar"], got["u"], got["v"], want, what)
    keep = ~want["out"]
    h = want["hit"] & keep
    inst = want["inst"] if "inst" in want else np.full(len(keep), INVALID, np.int64)
    assert np.array_equal(got["instID"][h].astype(np.int64), inst[h]), what
    if kind in ("lines", "lines.mb"):
        assert ng[h].tobytes() == want["Ng"][h].astype(F32).tobytes(), what  # v1 - v0 in float32
    elif kind in ("curves", "bspline", "curves.mb"):
        # eval_du(u) at the kernel's own u, up to 1e-4 off the truth's: |dNg| <= 1e-4 max |eval_dudu| + the roundings (test_gpu_curves.py)
        cp = want["cp"][..., :3].astype(np.float64)
        dd = 6.0 * np.maximum(np.abs(cp[:, 0] - 2 * cp[:, 1] + cp[:, 2]), np.abs(cp[:, 1] - 2 * cp[:, 2] + cp[:, 3])).max(1)
        tol = 1e-4 * dd + 1e-5 * np.linalg.norm(want["Ng"], axis=1)
        assert (np.abs(ng[h].astype(np.float64) - want["Ng"][h]).max(1) <= tol[h]).all(), what
    miss = ~want["hit"] & keep
    assert got[miss].tobytes() == rays[miss].tobytes(), f"{what}: a miss came back changed"
    if occ is not None:
        wocc = occ.copy()
        for f in occ.dtype.names:
            wocc[f] = rays[f]
        wocc["tfar"][want["hit"]] = -np.inf
        assert occ[keep].tobytes() == wocc[keep].tobytes(), f"{what}: occluded"
    return {"hits": int(want["hit"].sum()), "out": left, "t": mt, "u": mu}


def short_hits(want, rays):
    """truth hits among the rays with |dir| < SHORT"""
    d = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1).astype(np.float64)
    return int((want["hit"] & ~want["out"] & (np.linalg.norm(d, axis=1) < SHORT)).sum())


# ---- invalid rays ---------------------------------------------------------------------------------------------------------------------
# field, value, and whether the record itself must come back byte for byte.  tnear = -inf is a VALID ray whose window starts at -inf:
# its own answer is not checked here, only that it leaves its batch-mates alone.
POISON = [("org_x", np.nan, True), ("org_y", np.inf, True), ("org_z", -np.inf, True), ("dir_x", np.nan, True), ("dir_y", np.inf, True), ("dir_z", -np.inf, True),
          ("tnear", np.nan, True), ("tnear", np.inf, True), ("tnear", -np.inf, False), ("tfar", np.nan, True), ("tfar", -np.inf, True), ("dir", 0.0, True)]
POISON_TIMES = [("time", np.inf, False), ("time", -3.0, False), ("time", 7.0, False)]


def poisoned(rtc, rays, moving):
    """(dirty, bad [indices], exact [per bad index: the record must come back untouched]): every 97th record from 50 on poisoned, the
    list above in turn.  NaN time and times just outside the shutter are fixed by the moving kinds' own tests and are not repeated."""
    kinds = POISON + (POISON_TIMES if moving else [])
    bad = np.arange(50, len(rays), 97)[: 2 * len(kinds)]
    dirty = copy(rtc, rays)
    exact = np.zeros(len(bad), bool)
    for j, i in enumerate(bad):
        f, v, e = kinds[j % len(kinds)]
        exact[j] = e
        if f == "dir":
            dirty["dir_x"][i] = dirty["dir_y"][i] = dirty["dir_z"][i] = 0.0
        else:
            dirty[f][i] = v
    return dirty, bad, exact


# ---- hair below instances -----------------------------------------------------------------------------------------------------------------
def instance_scene(which):
    """'a': instance_hair_helpers.scenes('a'), 96 line segments; 'b': two of the curve geometries of scenes('b'), Bezier at rate 4 and
    B-spline at rate 9 (the leaf's second pass) - as test_general_transforms_against_the_float64_truth takes them"""
    d = ihh.scenes(which)["m"]
    if which == "b":
        d = ihh.desc(curves=[d["curves"][2], d["curves"][5]])
    return {"m": d}


def instance_box(scs, inst):
    flat = [(g, k, s) for g, k, steps in inst for s in steps]
    lo, hi = ih.instances_bounds(ihh.bounds_meshes(scs), flat)
    return np.floor(lo), np.ceil(hi)


def instance_rays(rtc, scs, inst, n_grid=48, m=6000, k=3000):
    """the degenerate family over the instances' integer box, origins snapped to the 2^-10 grid, times k / 4.  The box is some 150
    across and holds six tufts 8 to 32 across: the family is taken three times as dense per axis as over the unit cube, or a tuft meets a
    handful of rays only"""
    lo, hi = instance_box(scs, inst)
    return er.with_times(er.edge_rays(rtc, lo, hi, n_grid, 7, snapped=True, m=m, k=k))


def instance_truth(scs, inst, rays):
    """per instance the EXACT local ray (instance_mb_helpers.local_rays asserts it: signed axis permutations times power-of-two scales,
    everything on the 2^-10 grid, times k / 4) through lines_truth64 / curves_truth64 with the ray's own tnear / tfar - the ray parameter
    is kept across the frame change - merged by smallest t.  A ray is left out where one instance's truth leaves it out, or where the
    nearest hits of two instances lie within 1e-4 relative in t."""
    d = scs["m"]
    m = len(rays)
    tn, tf = rays["tnear"].astype(np.float64), rays["tfar"].astype(np.float64)
    best = {"hit": np.zeros(m, bool), "inst": np.full(m, -1, np.int64), "geomID": np.full(m, -1, np.int64), "primID": np.full(m, -1, np.int64), "t": np.full(m, np.inf),
            "u": np.zeros(m), "v": np.zeros(m)}
    out = np.zeros(m, bool)
    second = np.full(m, np.inf)
    pts = ihh.points(d)  # every point of the scene with the radii added on all sides; a tenth of the extent more: a ray that passes this
    pad = 0.1 * (pts.max(0) - pts.min(0))  # box by has no candidate and none within 1e-4 of an edge, and is not handed to the truths
    blo, bhi = pts.min(0) - pad, pts.max(0) + pad
    for gid, _, steps in inst:
        w, ok = im.world2local_at(steps, rays["time"])
        assert ok.all()
        loc = im.local_rays(rays, w, ok, exact=True)
        lo, ld, _, _ = fields(loc)
        lo, ld = lo.astype(np.float64), ld.astype(np.float64)
        with np.errstate(all="ignore"):
            t1, t2 = (blo - lo) / ld, (bhi - lo) / ld
        inside = (lo >= blo) & (lo <= bhi)
        tin = np.where(ld != 0, np.minimum(t1, t2), np.where(inside, -np.inf, np.inf)).max(1)
        tout = np.where(ld != 0, np.maximum(t1, t2), np.where(inside, np.inf, -np.inf)).min(1)
        k = np.nonzero((tin <= tout) & (tout >= tn) & (tin <= tf))[0]
        found = []
        if d.get("lines") is not None:
            v, idx, lgid = d["lines"]
            v0, v1 = (x.astype(np.float64) for x in lh.ends(v, idx))
            r = ihh.lines_truth64(v0, v1, lo[k], ld[k], tn[k], tf[k])
            found.append((r, np.full(len(k), lgid), r["seg"], np.zeros(len(k))))
        if d.get("curves"):
            r = ihh.curves_truth64([(ch.native(v, idx, basis).astype(np.float64), rate, cgid) for v, idx, basis, rate, cgid in d["curves"]], lo[k], ld[k], tn[k], tf[k])
            found.append((r, r["geomID"], r["primID"], r["v"]))
        for r, g, p, v in found:
            out[k] |= r["near_edge"] | r["near_tie"]
            t = np.full(m, np.inf)
            t[k] = np.where(r["hit"], r["t"], np.inf)
            sel = t < best["t"]
            second = np.minimum(second, np.where(sel, best["t"], t))
            for key, a in (("inst", np.full(len(k), gid)), ("geomID", g), ("primID", p), ("u", r["u"]), ("v", v)):
                full = np.zeros(m, np.asarray(a).dtype)
                full[k] = a
                best[key][sel] = full[sel]
            best["t"][sel] = t[sel]
            best["hit"] |= sel
    with np.errstate(all="ignore"):
        out |= np.isfinite(second) & (np.abs(second - best["t"]) <= 1e-4 * np.abs(best["t"]))
    best.update(near_edge=out, near_tie=np.zeros(m, bool), out=out)
    return best
