"""Flat Bezier and B-spline curves (RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE / _FLAT_BSPLINE_CURVE) on the GPU: the ribbon leaf of
csrc/trace_curve.hip in its lane-per-ray and octet forms (the leaf has no ray-pool form), under robust and fast traversal.

The oracle has no curve intersector; the truth is the NumPy restatement of intersect_ribbon in tests/curve_helpers.py, all segments of
all curves against all rays in float64 (no BVH).  Exact (`==`) where the inputs are dyadic, the project's 1e-4 contract elsewhere."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import curve_helpers as ch
import deep_stack_helpers as ds
from curve_helpers import ACCEL_CURVE_FAST, ACCEL_CURVE_ROBUST, CURVE_DT, ROBUST
from helpers import INVALID

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")
KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL")
FORMS = {"lane form": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "0", "RTAMD_OCT_LEAF": "0"},    # every node and leaf step one ray per lane
         "octet form": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "32", "RTAMD_OCT_LEAF": "1"},  # 8 lanes per ray wherever the kernel allows it
         "pool asked": {"RTAMD_KERNEL": "pool"}}                                                 # the leaf has no pool form: the lane kernel with its default knobs
MODES = [pytest.param(ROBUST, id="robust"), pytest.param(0, id="fast")]
NEXT = np.nextafter
F = np.float32
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
HITF = ["Ng_x", "Ng_y", "Ng_z", "u", "v", "primID", "geomID", "instID"]


def _knobs(monkeypatch, knobs):
    """the tuning knobs are read when a device is created"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def _scene(rtc, flags, add, cfg=""):
    dev = rtc.Device(cfg)
    sc = rtc.Scene(dev, flags)
    add(sc)
    sc.commit()
    return dev, sc


def _trace(rtc, sc, rh, ctx=None):
    out = rtc.aligned_rayhits(len(rh))
    out[:] = rh
    sc.intersect1M(out, ctx=ctx)
    occ = ch.occ_of(rtc, rh)
    sc.occluded1M(occ, ctx=ctx)
    return out, occ


# ---- 1. closed forms, exact ---------------------------------------------------------------------------------------------------------------
# a straight curve with equally spaced collinear control points: the point at u is (-1.5 + 3 u, 0, 0), its derivative (3, 0, 0); N = 4 cuts it
# at x = -0.75, 0, 0.75.  A second curve 100 higher has all control points equal.
STRAIGHT = np.array([[-1.5, 0, 0, .25], [-.5, 0, 0, .25], [.5, 0, 0, .25], [1.5, 0, 0, .25],
                     [0, 100, 0, .25], [0, 100, 0, .25], [0, 100, 0, .25], [0, 100, 0, .25]], np.float32)
# (org, dir, tnear, tfar) -> None (miss) or (t, u, v)
CLOSED_RAYS = [(((0, 0, -4), (0, 0, 1), 0, np.inf), (4, .5, 0)),                    # the centre: t is the depth of the ribbon, which faces the ray
               (((0, 0, -4), (0, 0, 2), 0, np.inf), (2, .5, 0)),
               (((0, .25, -4), (0, 0, 1), 0, np.inf), (4, .5, 1)),                  # on the edge: max(U, V) <= 0
               (((0, NEXT(F(.25), F(1)), -4), (0, 0, 1), 0, np.inf), None),         # one ulp beyond it
               (((0, -.25, -4), (0, 0, 1), 0, np.inf), (4, .5, -1)),                # the other edge: v = -1
               (((0, -NEXT(F(.25), F(1)), -4), (0, 0, 1), 0, np.inf), None),
               (((-.75, 0, -4), (0, 0, 1), 0, np.inf), (4, .25, 0)),                # on the boundary of segments 0 and 1: the same u from either
               (((-.75, .125, -4), (0, 0, 1), 0, np.inf), (4, .25, .5)),
               (((-.375, -.125, -4), (0, 0, 1), 0, np.inf), (4, .375, -.5)),        # inside segment 1
               (((.375, 0, -4), (0, 0, 1), 0, np.inf), (4, .625, 0)),               # segment 2
               (((1.125, .0625, -4), (0, 0, 1), 0, np.inf), (4, .875, .25)),        # segment 3
               (((-1.5, 0, -4), (0, 0, 1), 0, np.inf), (4, 0, 0)),                  # the two ends of the curve
               (((1.5, 0, -4), (0, 0, 1), 0, np.inf), (4, 1, 0)),
               (((NEXT(F(1.5), F(2)), 0, -4), (0, 0, 1), 0, np.inf), None),
               (((NEXT(F(-1.5), F(-2)), 0, -4), (0, 0, 1), 0, np.inf), None),
               (((0, 0, -.25), (0, 0, 1), 0, np.inf), None),                        # self intersection: t = 1/4 is not > 0 + 2 * 1/4
               (((0, 0, -.5), (0, 0, 1), 0, np.inf), None),                         # ... nor is 1/2
               (((0, 0, -.75), (0, 0, 1), 0, np.inf), (.75, .5, 0)),
               (((0, 0, -4), (0, 0, 1), 0, 4), (4, .5, 0)),                         # T <= absDen * tfar
               (((0, 0, -4), (0, 0, 1), 0, NEXT(F(4), F(0))), None),
               (((0, 0, -4), (0, 0, 1), 4, np.inf), None),                          # absDen * tnear < T
               (((0, 0, -4), (0, 0, 1), 3, np.inf), (4, .5, 0)),                    # t = 4 > 3 + 2 * 1/4
               (((0, 0, -4), (0, 0, 1), 3.5, np.inf), None),                        # ... but not > 3.5 + 1/2
               (((0, 100, -4), (0, 0, 1), 0, np.inf), None),                        # a curve with all control points equal is never hit
               (((0, 0, -4), (0, 0, 1), 5, 4), None),                               # invalid rays come back untouched: tnear > tfar
               (((np.nan, 0, -4), (0, 0, 1), 0, np.inf), None)]                     # ... NaN origin


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("flags", MODES)
def test_closed_forms_are_exact(rtc, monkeypatch, flags, form):
    _knobs(monkeypatch, FORMS[form])
    dev, sc = _scene(rtc, flags, lambda s: s.add_curves(STRAIGHT, np.array([0, 4], np.uint32), geom_id=5))
    assert sc.stats()["accelKind"] == (ACCEL_CURVE_ROBUST if flags else ACCEL_CURVE_FAST) and sc.stats()["primCount"] == 2
    rh = ch.rays_of(rtc, [r[0][0] for r in CLOSED_RAYS], [r[0][1] for r in CLOSED_RAYS],
                    np.array([r[0][2] for r in CLOSED_RAYS], F), np.array([r[0][3] for r in CLOSED_RAYS], F))
    rh["u"], rh["v"], rh["Ng_x"] = 7, 7, 7  # a miss leaves the hit part as it was
    got, occ = _trace(rtc, sc, rh)
    for i, (_, want) in enumerate(CLOSED_RAYS):
        g = got[i]
        if want is None:
            assert g.tobytes() == rh[i].tobytes(), (i, g)
            assert occ[i].tobytes() == ch.occ_of(rtc, rh[i:i + 1])[0].tobytes(), i
            continue
        t, u, v = want
        assert g["geomID"] == 5 and g["primID"] == 0 and g["instID"] == INVALID, (i, g)
        assert g["tfar"] == F(t) and g["u"] == F(u) and g["v"] == F(v), (i, g)
        assert (g["Ng_x"], g["Ng_y"], g["Ng_z"]) == (3, 0, 0), (i, g)  # eval_du(u) of the control points, not normalised
        assert occ[i]["tfar"] == -np.inf, i
    assert len(CLOSED_RAYS) == 26 and dev.error() == 0
    sc.release()
    dev.release()


# ---- 2. tie and pass rule -----------------------------------------------------------------------------------------------------------------------
def _tie_rays():
    """rays on a 1/64 grid about the middle of the curves below, directions on a 1/32 grid"""
    rng = np.random.default_rng(3)
    org = np.concatenate([rng.uniform(-.4, .4, (40, 1)), rng.uniform(-.1, .1, (40, 1)), np.full((40, 1), -4.)], 1)
    dirs = np.concatenate([np.round(rng.uniform(-.1, .1, (40, 2)) * 32) / 32, np.ones((40, 1))], 1)
    return (np.round(org * 64) / 64).astype(F), dirs.astype(F)


@pytest.mark.parametrize("basis", ["bezier", "bspline"])
@pytest.mark.parametrize("flags", MODES)
def test_coincident_curves_the_last_record_wins(rtc, monkeypatch, flags, basis):
    """5 coincident curves with primIDs of their own in one leaf, two passes per curve (N = 16): every record is tested against the tfar
    the one before it left, and the depth test is `<=`, so the record at the last place of the leaf wins the equal t - in every form, bit
    for bit.  The depth test is the reference's `T <= absDen * tfar`, and the t a record leaves is fl(T / den): where absDen * fl(T / den)
    rounds below T, an identical copy does NOT pass, and the first record keeps the hit.  Which of the two it is, is a matter of one
    rounding, so:
      * a straight curve under axis-parallel rays, where T, den and t are exact (t = 4, den = 3/32, T = 4 den): the last record MUST win,
        in the first pass (segment 3) as in the second (segment 12);
      * a bent curve under 40 rays: the winner and its t are those of the float32 restatement (tests/curve_helpers.py `again`)."""
    straight = np.array([[-1.5, 0, 0, .25], [-.5, 0, 0, .25], [.5, 0, 0, .25], [1.5, 0, 0, .25]], np.float32)
    bent = np.array([[-1.5, 0, 0, .25], [-.5, .25, 0, .125], [.5, -.25, .5, .25], [1.5, 0, 0, .125]], np.float32)
    idx = np.arange(0, 20, 4, dtype=np.uint32)
    xo = np.array([[-.875, .125, -4], [.875, -.0625, -4], [-.84375, 0, 4]], np.float32)  # exact rays: segments 3, 12 and 3 (from behind)
    xd = np.array([[0, 0, 1], [0, 0, 1], [0, 0, -1]], np.float32)
    if basis == "bspline":  # the B-spline curve spans the middle of its control polygon: x in [-0.5, 0.5]; its conversion is not exact
        xo, xd = xo[:0], xd[:0]
    org, dirs = _tie_rays()
    results = {}
    for name, knobs in FORMS.items():
        _knobs(monkeypatch, knobs)
        for cp, o, d, exact in ((straight, xo, xd, True), (bent, org, dirs, False)):
            if not len(o):
                continue
            dev, sc = _scene(rtc, flags, lambda s: s.add_curves(np.tile(cp, (5, 1)), idx, basis=basis, tessellation_rate=16))
            assert sc.accel_root() == (0x80000000 | (5 << 26))  # one leaf
            rec = sc.accel_data(2).view(CURVE_DT)
            got, occ = _trace(rtc, sc, ch.rays_of(rtc, o, d))
            m = len(o)
            c32 = ch.closest([(rec["v"][:1], 16, 0)], o, d, np.zeros(m, F), np.full(m, np.inf, F), np.float32)
            h = c32["hit"]
            if exact:
                assert h.all() and c32["again"].all() and (c32["t"] == 4).all()
                assert (got["primID"] == rec["primID"][4]).all() and (got["tfar"] == 4).all(), (name, got)
            else:
                want = np.where(c32["again"], rec["primID"][4], rec["primID"][0])
                print(f"  {basis}, {name}: {int(h.sum())} hits, the last record wins {int((h & c32['again']).sum())}, the first keeps {int((h & ~c32['again']).sum())}")
                assert int((h & c32["again"]).sum()) >= 8
                assert np.array_equal(got["geomID"] != INVALID, h), name
                assert np.array_equal(got["primID"][h], want[h]) and np.array_equal(got["tfar"][h], c32["t"][h].astype(F)), (name, got["primID"][h], want[h])
            assert np.array_equal(occ["tfar"] == -np.inf, h)
            results.setdefault(exact, {})[name] = got.tobytes()
            sc.release()
            dev.release()
    for r in results.values():
        assert len(set(r.values())) == 1


# ---- 3. the pinned input against the float64 truth -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hair():
    v, idx, org, dirs = ch.hair_and_rays()
    return {"v": v, "idx": idx, "org": org, "dirs": dirs}


def _check_parity(got, occ, rh, truth, what, geom_ids=None):
    """curve_helpers.compare (hit / miss, geomID / primID exact, t within 1e-4 relative, u and v within 1e-4 absolute, at most 0.5 % of
    the rays left out, and only where the float64 truth is within 1e-4 of an edge of a ribbon quad or of a tie); Ng within 1e-4 of the
    truth's eval_du(u) relative to its length; a miss comes back untouched; the any-hit answer agrees"""
    gh = got["geomID"] != INVALID
    geom = got["geomID"].astype(np.int64)
    ch.compare(gh, geom, got["primID"].astype(np.int64), got["tfar"], got["u"], got["v"], truth, what)
    k = ~(truth["near_edge"] | truth["near_tie"])
    h = truth["hit"] & k
    assert (got["instID"][h] == INVALID).all(), what
    # Ng = eval_du(u) at the kernel's own u, which may be 1e-4 off the truth's: |dNg| <= 1e-4 * max |eval_dudu| over the curve (eval_dudu is
    # linear in u: 6 * the larger second difference of the control points) plus the float32 roundings of the evaluation (1e-5 |Ng| is far over)
    ng = np.stack([got["Ng_x"], got["Ng_y"], got["Ng_z"]], 1).astype(np.float64)
    cp = truth["cp"][..., :3].astype(np.float64)
    dd = 6.0 * np.maximum(np.abs(cp[:, 0] - 2 * cp[:, 1] + cp[:, 2]), np.abs(cp[:, 1] - 2 * cp[:, 2] + cp[:, 3])).max(1)
    tol = 1e-4 * dd + 1e-5 * np.linalg.norm(truth["Ng"], axis=1)
    assert (np.abs(ng[h] - truth["Ng"][h]).max(1) <= tol[h]).all(), what
    miss = ~truth["hit"] & k
    assert got[miss].tobytes() == rh[miss].tobytes(), what  # a miss comes back untouched
    assert np.array_equal(occ["tfar"][k] == -np.inf, truth["hit"][k]) and np.array_equal(occ["tfar"][miss], rh["tfar"][miss]), what


@pytest.mark.parametrize("N", [1, 3, 4, 8, 9, 16])
@pytest.mark.parametrize("flags", MODES)
def test_pinned_hair_meets_the_float64_truth(rtc, monkeypatch, hair, flags, N):
    truth = ch.hair_truth(N)
    assert int(truth["hit"].sum()) == ch.HAIR_HITS[N]
    rh = ch.rays_of(rtc, hair["org"], hair["dirs"])
    first = None
    for name, knobs in FORMS.items():
        _knobs(monkeypatch, knobs)
        dev, sc = _scene(rtc, flags, lambda s: s.add_curves(hair["v"], hair["idx"], tessellation_rate=N, geom_id=7))
        got, occ = _trace(rtc, sc, rh)
        if first is None:
            t = dict(truth)
            t["geomID"] = np.full(len(rh), 7)
            _check_parity(got, occ, rh, t, f"hair, N = {N}, {name}")
            first = (got.tobytes(), occ.tobytes())
        else:
            assert (got.tobytes(), occ.tobytes()) == first, name
        assert dev.error() == 0
        sc.release()
        dev.release()


@pytest.mark.parametrize("flags", MODES)
def test_two_geometries_with_rates_of_their_own_in_one_scene(rtc, monkeypatch, hair, flags):
    """the first half of the hair at rate 3, the second half at rate 9: the leaf takes N from the record"""
    v, idx, org, dirs = hair["v"], hair["idx"], hair["org"], hair["dirs"]
    m, half = len(org), len(idx) // 2
    cp = ch.native(v, idx)
    truth = ch.closest([(cp[:half], 3, 1), (cp[half:], 9, 4)], org, dirs, np.zeros(m, F), np.full(m, np.inf, F), np.float64)
    rh = ch.rays_of(rtc, org, dirs)
    first = None
    for name, knobs in FORMS.items():
        _knobs(monkeypatch, knobs)

        def add(s):
            s.add_curves(v, idx[:half], tessellation_rate=3, geom_id=1)
            s.add_curves(v, idx[half:], tessellation_rate=9, geom_id=4)
        dev, sc = _scene(rtc, flags, add)
        got, occ = _trace(rtc, sc, rh)
        if first is None:
            _check_parity(got, occ, rh, truth, f"hair at rates 3 and 9, {name}")
            assert min(int((got["geomID"] == g).sum()) for g in (1, 4)) > 200
            first = (got.tobytes(), occ.tobytes())
        else:
            assert (got.tobytes(), occ.tobytes()) == first, name
        sc.release()
        dev.release()


# ---- 4. B-spline equals Bezier -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES)
def test_a_bspline_geometry_equals_the_bezier_geometry_of_its_converted_points(rtc, hair, flags):
    v, idx, org, dirs = hair["v"], hair["idx"], hair["org"], hair["dirs"]
    rh = ch.rays_of(rtc, org, dirs)
    conv = ch.native(v, idx, "bspline").reshape(-1, 4)  # four points of its own per curve
    dev, a = _scene(rtc, flags, lambda s: s.add_curves(v, idx, basis="bspline", tessellation_rate=5))
    b = rtc.Scene(dev, flags)
    b.add_curves(conv, np.arange(0, len(conv), 4, dtype=np.uint32), basis="bezier", tessellation_rate=5)
    b.commit()
    ga, oa = _trace(rtc, a, rh)
    gb, ob = _trace(rtc, b, rh)
    assert ga.tobytes() == gb.tobytes() and oa.tobytes() == ob.tobytes()
    assert int((ga["geomID"] != INVALID).sum()) > 300  # (the B-spline curve spans the middle of its control polygon only)
    a.release()
    b.release()
    dev.release()


# ---- 5. mixed scenes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES)
def test_mixed_scene_equals_the_accels_traced_in_reference_order(rtc, po, hair, flags):
    """triangles, curves and line segments in one scene = the three accels traced alone one after the other in the reference's order
    (triangles, hair, lines; scene.cpp:650-658): every ray keeps the nearest, and a later accel wins a bit-equal t"""
    rng = np.random.RandomState(4)
    c = rng.rand(200, 1, 3).astype(F)
    tv = (c + (rng.rand(200, 3, 3).astype(F) - 0.5) * 0.1).reshape(-1, 3).astype(F)
    tt = np.arange(600, dtype=np.uint32).reshape(-1, 3)
    lv = np.concatenate([rng.rand(400, 3), rng.uniform(0.004, 0.012, (400, 1))], 1).astype(F)
    lv[1::2, :3] = lv[0::2, :3] + (rng.rand(200, 3).astype(F) - 0.5) * 0.2
    li = np.arange(0, 400, 2, dtype=np.uint32)

    def scene(parts):
        def add(s):
            if "t" in parts:
                s.add_triangles(tv, tt, geom_id=0)
            if "c" in parts:
                s.add_curves(hair["v"], hair["idx"], geom_id=1)
            if "l" in parts:
                s.add_lines(lv, li, geom_id=2)
        return _scene(rtc, flags, add)

    m = 50000
    rays = po.make_random_rays(m, np.zeros(3, F), np.ones(3, F), seed=9)
    dev, sc = scene("tcl")
    got = rtc.aligned_rayhits(m)
    got[:] = rays
    sc.intersect1M(got)
    want = rtc.aligned_rayhits(m)
    want[:] = rays
    for p in "tcl":
        d1, s1 = scene(p)
        s1.intersect1M(want)
        s1.release()
        d1.release()
    assert got.tobytes() == want.tobytes()
    counts = [int((got["geomID"] == g).sum()) for g in range(3)]
    print(f"  hits per geometry (triangles, curves, lines): {counts}")
    assert min(counts) > 100, counts
    sc.release()
    dev.release()


@pytest.mark.parametrize("flags", MODES)
def test_curves_beside_instances_in_a_top_scene(rtc, po, hair, flags):
    """a top scene with curves of its own beside an instance of a scene without curves = the curve accel, then the instance accel"""
    tv = np.array([[.1, .1, .5], [.9, .1, .5], [.5, .9, .45], [.2, .8, .2], [.8, .3, .7]], F)
    tt = np.array([[0, 1, 2], [0, 3, 4], [1, 3, 4]], np.uint32)
    dev = rtc.Device("")
    inner = rtc.Scene(dev, flags)
    inner.add_triangles(tv, tt)
    inner.commit()

    def scene(parts):
        sc = rtc.Scene(dev, flags)
        if "c" in parts:
            sc.add_curves(hair["v"], hair["idx"], geom_id=0)
        if "i" in parts:
            sc.add_instance(inner, geom_id=1)
        sc.commit()
        return sc

    m = 20000
    rays = po.make_random_rays(m, np.zeros(3, F), np.ones(3, F), seed=5)
    got, want = rtc.aligned_rayhits(m), rtc.aligned_rayhits(m)
    got[:] = rays
    want[:] = rays
    sc = scene("ci")
    assert sc.stats()["accelKind"] == (ACCEL_CURVE_ROBUST if flags else ACCEL_CURVE_FAST)
    sc.intersect1M(got)
    sc.release()
    for p in "ci":
        s1 = scene(p)
        s1.intersect1M(want)
        s1.release()
    assert got.tobytes() == want.tobytes()
    on_curves = int(((got["geomID"] == 0) & (got["instID"] == INVALID)).sum())
    on_inst = int((got["instID"] == 1).sum())
    print(f"  {on_curves} hits on the scene's own curves, {on_inst} below the instance")
    assert on_curves > 500 and on_inst > 1000
    inner.release()
    dev.release()


# ---- 6. filters -------------------------------------------------------------------------------------------------------------------------------------
def _ray_fields(args):
    ray = C.cast(args.contents.ray, C.POINTER(C.c_float * 12)).contents
    hit = C.cast(args.contents.hit, C.POINTER(C.c_uint * 8)).contents
    hitf = C.cast(args.contents.hit, C.POINTER(C.c_float * 8)).contents
    return ray, hit, hitf


@pytest.mark.parametrize("flags", MODES)
def test_filters_reject_every_second_curve_and_the_next_candidate_is_found(rtc, hair, flags):
    """An intersect filter, an occluded filter and a context filter that reject the odd primIDs: the records are those of the scene built
    without those curves, primIDs mapped back.  The callbacks get the geometry's user data and the candidate."""
    v, idx = hair["v"], hair["idx"]
    rh = ch.rays_of(rtc, hair["org"], hair["dirs"])
    USER = 0x5EED0
    seen, bad = [], []

    @rtc.FILTER_FUNC
    def flt(args):
        ray, hit, hitf = _ray_fields(args)
        prim = hit[5]
        seen.append((ray[0], prim, ray[8], hitf[3]))
        if not (args.contents.geometryUserPtr == USER and args.contents.N == 1 and hit[6] == 7 and -1.0 <= hitf[4] <= 1.0 and 0.0 <= hitf[3] <= 1.0 and hit[7] == INVALID):
            bad.append((prim, hit[6], hitf[3], hitf[4]))
        if prim & 1:
            args.contents.valid[0] = 0

    dev0, ref = _scene(rtc, flags, lambda s: s.add_curves(v, idx[0::2], tessellation_rate=6, geom_id=7))
    want, wocc = _trace(rtc, ref, rh)
    wh = want["geomID"] != INVALID
    want["primID"][wh] *= 2  # back to the primIDs of the full geometry
    assert int(wh.sum()) > 400

    def full(s):
        assert s.add_curves(v, idx, tessellation_rate=6, geom_id=7) == 7
        s.set_user_data(7, USER)

    dev, sc = _scene(rtc, flags, full)
    assert sc.filter_flags() == 0
    sc.set_filters(7, intersect=flt, occluded=flt)
    sc.commit()
    assert sc.filter_flags() == rtc.RTCAMD_SCENE_FILTER_MESH_INTERSECT | rtc.RTCAMD_SCENE_FILTER_MESH_OCCLUDED
    got, occ = _trace(rtc, sc, rh)
    assert got.tobytes() == want.tobytes() and occ.tobytes() == wocc.tobytes()
    assert not bad, bad[:3]
    rejected = sum(1 for s in seen if s[1] & 1)
    print(f"  {len(seen)} callbacks, {rejected} rejections")
    assert rejected > 100
    sc.release()
    dev.release()
    # the context filter alone
    dev, sc = _scene(rtc, flags, full)
    ctx = rtc.make_context()
    ctx.filter = C.cast(flt, C.c_void_p)
    got, occ = _trace(rtc, sc, rh, ctx=ctx)
    assert got.tobytes() == want.tobytes() and occ.tobytes() == wocc.tobytes()
    assert not bad, bad[:3]
    sc.release()
    dev.release()
    ref.release()
    dev0.release()


@pytest.mark.parametrize("flags", MODES)
def test_a_rejected_quad_leaves_the_other_quads_of_the_same_curve(rtc, flags):
    """A curve bent into a U, seen from the side: the ray crosses two ribbon quads of ONE curve.  A filter that rejects the first candidate
    it is shown per ray (whatever it is) must be shown the second quad of the same curve next: the rejected candidate is (geomID, primID,
    t), not the curve."""
    u_turn = np.array([[-1, 0, 0, .125], [-1, 0, 2, .125], [1, 0, 2, .125], [1, 0, 0, .125]], np.float32)
    org = np.array([[-4, 0, .5], [4, .03125, .75]], np.float32)
    dirs = np.array([[1, 0, 0], [-1, 0, 0]], np.float32)
    rh = ch.rays_of(rtc, org, dirs)
    dev, sc = _scene(rtc, flags, lambda s: s.add_curves(u_turn, np.array([0], np.uint32), tessellation_rate=16, geom_id=0))
    plain, _ = _trace(rtc, sc, rh)
    assert (plain["geomID"] == 0).all()
    shown = {}

    @rtc.FILTER_FUNC
    def flt(args):
        ray, hit, hitf = _ray_fields(args)
        s = shown.setdefault(ray[1], [])
        s.append((hit[5], ray[8], hitf[3]))
        if len(s) == 1:
            args.contents.valid[0] = 0

    sc.set_filters(0, intersect=flt)
    sc.commit()
    got = rtc.aligned_rayhits(2)
    got[:] = rh
    sc.intersect1M(got)
    for i in range(2):
        s = shown[float(org[i, 1])]
        assert len(s) == 2 and s[0][0] == 0 and s[1][0] == 0, s        # the same curve twice
        assert s[0][1] == plain["tfar"][i] and s[1][1] > s[0][1] + 1.0  # first the near arm of the U, then the far one
        assert got["tfar"][i] == F(s[1][1]) and got["u"][i] == F(s[1][2]) and got["primID"][i] == 0
        assert (s[0][2] < .5) != (s[1][2] < .5)                         # the two arms lie in the two halves of the parameter range
    sc.release()
    dev.release()


# ---- 7. entry paths ------------------------------------------------------------------------------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("flags", MODES)
def test_entry_paths_are_bit_identical(rtc, po, hair, flags):
    import torch

    def scene(extra=""):
        return _scene(rtc, flags, lambda s: s.add_curves(hair["v"], hair["idx"], tessellation_rate=9), extra)

    m = 40000
    rays = po.make_random_rays(m, np.zeros(3, F), np.ones(3, F), seed=21)
    dev, sc = scene()
    L = sc.lib
    # device-resident batch = the reference answer
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()
    sc.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    nh = int((want["geomID"] != INVALID).sum())
    assert nh > 1000, nh
    # host, pipelined (>= 16 k rays)
    h = rtc.aligned_rayhits(m)
    h[:] = rays
    sc.intersect1M(h)
    assert h.tobytes() == want.tobytes()
    # host, small batches (<= 512 rays: zero-copy)
    s = rtc.aligned_rayhits(m)
    s[:] = rays
    for a in range(0, 4096, 500):
        sc.intersect1M(s[a:a + 500])
    assert s[:4096].tobytes() == want[:4096].tobytes()
    # instrumented twins (counted batches)
    c = rtc.aligned_rayhits(m)
    c[:] = rays
    cnt = sc.intersect1M_counted(c)
    assert c.tobytes() == want.tobytes()
    assert cnt["rays"] == m and cnt["hits"] == nh and cnt["primTests"] > 0
    wocc = ch.occ_of(rtc, rays)
    sc.occluded1M(wocc)
    co = ch.occ_of(rtc, rays)
    ocnt = sc.occluded1M_counted(co)
    assert co.tobytes() == wocc.tobytes() and np.array_equal(wocc["tfar"] == -np.inf, want["geomID"] != INVALID)
    assert ocnt["rays"] == m and ocnt["hits"] == nh and ocnt["primTests"] > 0
    # multi-threaded rtcIntersect1 / rtcOccluded1 (call combiner)
    k = 2048
    g = rtc.aligned_rayhits(k)
    g[:] = rays[:k]
    go = ch.occ_of(rtc, rays[:k])
    errors = []

    def worker(i0):
        try:
            for i in range(i0, k, 16):
                sc.intersect1(g[i:i + 1])
                sc.occluded1(go[i:i + 1])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(16)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[0]
    assert g.tobytes() == want[:k].tobytes() and go.tobytes() == wocc[:k].tobytes()
    # packets of 4, 8 and 16 and their occluded twins
    ctx = rtc.make_context()
    for W in (4, 8, 16):
        fn_i, fn_o = getattr(L, f"rtcIntersect{W}"), getattr(L, f"rtcOccluded{W}")
        for fn in (fn_i, fn_o):
            fn.restype = None
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        valid = np.full(W, -1, np.int32)
        for p in range(0, 128, W):
            pk = _soa(rays[p:p + W], W, True)
            fn_i(valid.ctypes.data, sc.handle, C.addressof(ctx), pk.ctypes.data)
            dev.check("packet")
            assert np.array_equal(pk, _soa(want[p:p + W], W, True))
            pko = _soa(rays[p:p + W], W, False)
            fn_o(valid.ctypes.data, sc.handle, C.addressof(ctx), pko.ctypes.data)
            dev.check("packet occluded")
            assert np.array_equal(pko[8], wocc["tfar"][p:p + W].view(np.uint32))
    # the SoA pointer stream and its occluded twin
    n = 300
    cols = {f: np.ascontiguousarray(rays[f][1500:1500 + n]) for f in RAYF + HITF[:-1]}
    inst = np.full(n, INVALID, np.uint32)

    class Np(C.Structure):
        _fields_ = [(f, C.c_void_p) for f in RAYF + HITF]

    a = Np(*[cols[f].ctypes.data for f in RAYF + HITF[:-1]], inst.ctypes.data)
    L.rtcIntersectNp.restype = None
    L.rtcIntersectNp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
    L.rtcIntersectNp(sc.handle, C.addressof(ctx), C.addressof(a), n)
    dev.check("rtcIntersectNp")
    w = want[1500:1500 + n]
    for f in ("tfar", "geomID", "primID", "u", "v", "Ng_x", "Ng_y", "Ng_z"):
        assert np.array_equal(cols[f].view(np.uint32), w[f].view(np.uint32)), f
    ocols = {f: np.ascontiguousarray(rays[f][1500:1500 + n]) for f in RAYF}

    class NpRay(C.Structure):
        _fields_ = [(f, C.c_void_p) for f in RAYF]

    b = NpRay(*[ocols[f].ctypes.data for f in RAYF])
    L.rtcOccludedNp.restype = None
    L.rtcOccludedNp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
    L.rtcOccludedNp(sc.handle, C.addressof(ctx), C.addressof(b), n)
    dev.check("rtcOccludedNp")
    assert np.array_equal(ocols["tfar"].view(np.uint32), wocc["tfar"][1500:1500 + n].view(np.uint32))
    sc.release()
    dev.release()
    # service=1: the curve accel has no service kernel, the calls fall back to the combiner and agree
    dev, sc = scene("service=1")
    sv = rtc.aligned_rayhits(k)
    sv[:] = rays[:k]
    for i in range(0, k, 32):
        sc.intersect1M(sv[i:i + 32])
    assert sv.tobytes() == want[:k].tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    sc.release()
    dev.release()


# ---- 8. the overflow area of the traversal stack ------------------------------------------------------------------------------------------------------------
MIN_SPILLS = 0.05 * ds.GPU_RAYS  # as tests/test_gpu_deep_stack.py: every ray above slot 16 pushes at least one entry to HBM


@pytest.mark.parametrize("flags", MODES)
def test_lane_and_octet_forms_agree_beyond_the_lds_stack(rtc, monkeypatch, flags):
    """A soup of needles as long as the cube they lie in (tests/deep_stack_helpers.py), as straight curves of radius 0.01: node boxes
    overlap everywhere and rays carry their stacks into the HBM overflow area, which the counted twin's stackSpills must show."""
    tv, tt = ds.sliver_soup(ds.N_SLIVERS, ds.SOUP_SEED)
    ends = tv.reshape(-1, 3, 3)[:, :2].astype(np.float64)  # v0, v1 of every needle
    p = np.stack([ends[:, 0] + (ends[:, 1] - ends[:, 0]) * k / 3.0 for k in range(4)], 1).reshape(-1, 3)
    v = np.concatenate([p, np.full((len(p), 1), 0.01)], 1).astype(F)
    idx = np.arange(0, len(v), 4, dtype=np.uint32)
    lo, hi = ds.bounds(p.astype(F))
    from helpers import random_rays_np
    org, dirs = random_rays_np(ds.GPU_RAYS, lo, hi, ds.GPU_RAY_SEED)
    rh = ds.rays_of(rtc, org, dirs)
    first = None
    for name, knobs in FORMS.items():
        _knobs(monkeypatch, knobs)
        dev, sc = _scene(rtc, flags, lambda s: s.add_curves(v, idx, tessellation_rate=2))
        assert sc.stats()["maxDepth"] >= 3
        got, occ = _trace(rtc, sc, rh)
        c = ds.copy_of(rtc, rh)
        cnt = sc.intersect1M_counted(c)
        assert c.tobytes() == got.tobytes(), f"{name}: the instrumented twin differs from the plain kernel"
        print(f"  needle curves, {name}: stackSpills {cnt['stackSpills']} ({len(rh)} rays), {int((got['geomID'] != INVALID).sum())} hits")
        assert cnt["stackSpills"] >= MIN_SPILLS, (name, cnt["stackSpills"])
        if first is None:
            assert int((got["geomID"] != INVALID).sum()) > ds.GPU_RAYS // 2
            first = (name, got.tobytes(), occ.tobytes())
        else:
            assert got.tobytes() == first[1], f"closest hit, {name} differs from {first[0]}"
            assert occ.tobytes() == first[2], f"any hit, {name} differs from {first[0]}"
        assert dev.error() == 0  # the `overflow` word stayed clear: no entry was dropped
        sc.release()
        dev.release()


# ---- 9. the C example -----------------------------------------------------------------------------------------------------------------------------------------
def test_curve_hair_example_runs(tmp_path):
    exe = str(tmp_path / "curve_hair_min")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "curve_hair_min.c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "curve_hair_min: ok" in out.stdout
