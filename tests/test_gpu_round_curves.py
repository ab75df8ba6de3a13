"""Round Bezier and B-spline curves (RTC_GEOMETRY_TYPE_ROUND_BEZIER_CURVE / _ROUND_BSPLINE_CURVE, device config round_curves=1) on the GPU:
the tube leaf of csrc/trace_round_curve.hip (octet form only, no ray-pool form), under robust and fast traversal and with the node steps
of the lane kernel in lane form (RTAMD_OCT_MAX=0) and in octet form (RTAMD_OCT_MAX=32).

The truth is the two-scan float64 truth of tests/round_curve_helpers.py, written from the surface's definition; closed forms where the
answer is known.  The project's 1e-4 contract throughout, hits and misses exact."""
import ctypes as C
import threading

import numpy as np
import pytest

import curve_helpers as ch
import deep_stack_helpers as ds
import round_curve_helpers as rh
from helpers import INVALID
from round_curve_helpers import ACCEL_CURVE_FAST, ACCEL_CURVE_ROBUST, CURVE_DT, ROBUST

pytestmark = pytest.mark.gpu

KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL")
FORMS = {"lane node steps": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "0"}, "octet node steps": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "32"}}
MODES = [pytest.param(ROBUST, id="robust"), pytest.param(0, id="fast")]
CFG = "round_curves=1"
F = np.float32
INF = np.inf
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
HITF = ["Ng_x", "Ng_y", "Ng_z", "u", "v", "primID", "geomID", "instID"]


def _knobs(monkeypatch, knobs):
    """the tuning knobs are read when a device is created"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def _scene(rtc, flags, add, cfg=CFG):
    dev = rtc.Device(cfg)
    sc = rtc.Scene(dev, flags)
    add(sc)
    sc.commit()
    return dev, sc


def _trace(rtc, sc, rays, ctx=None):
    out = rtc.aligned_rayhits(len(rays))
    out[:] = rays
    sc.intersect1M(out, ctx=ctx)
    occ = ch.occ_of(rtc, rays)
    sc.occluded1M(occ, ctx=ctx)
    return out, occ


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------------------------
# the straight tube of the flat tests: axis along x from -1.5 to 1.5, the point at u is (-1.5 + 3 u, 0, 0); radius 0.25.  A second curve
# 100 higher has all control points equal.  The tapered tube has the same axis and the radii 0.1, 0.2, 0.3, 0.4: r(u) = 0.1 + 0.3 u
STRAIGHT = np.array([[-1.5, 0, 0, .25], [-.5, 0, 0, .25], [.5, 0, 0, .25], [1.5, 0, 0, .25],
                     [0, 100, 0, .25], [0, 100, 0, .25], [0, 100, 0, .25], [0, 100, 0, .25]], F)
TAPER = np.array([[-1.5, 0, 0, .1], [-.5, 0, 0, .2], [.5, 0, 0, .3], [1.5, 0, 0, .4]], F)
# (org, dir, tnear, tfar) -> None (miss) or (t, u or None, Ng direction or None)
CLOSED_STRAIGHT = [(((0, 0, -4), (0, 0, 1), 0, INF), (3.75, .5, (0, 0, -1))),
                   (((0, 0, -4), (0, 0, 2), 0, INF), (1.875, .5, (0, 0, -1))),
                   (((0, 0, 0), (0, 0, 1), 0, INF), (.25, .5, (0, 0, 1))),        # origin inside: the exit hit
                   (((0, 0, -4), (0, 0, 1), 0, 3.7), None),
                   (((0, 0, -4), (0, 0, 1), 0, 3.8), (3.75, .5, None)),
                   (((0, 0, -4), (0, 0, 1), 3.8, INF), (4.25, .5, (0, 0, 1))),    # the back
                   (((0, 0, -4), (0, 0, 1), 4.3, INF), None),
                   (((-4, 0, 0), (1, 0, 0), 0, INF), None),                       # along the axis: no end caps
                   (((-4, .1, 0), (1, 0, 0), 0, INF), None),
                   (((1.6, 0, -4), (0, 0, 1), 0, INF), None),
                   (((1.4, 0, -4), (0, 0, 1), 0, INF), (3.75, 29 / 30, None)),
                   (((0, .2, -4), (0, 0, 1), 0, INF), (3.85, .5, (0, .8, -.6))),
                   (((0, .26, -4), (0, 0, 1), 0, INF), None),
                   (((-4, 0, -4), (1, 0, 1), 0, INF), (3.75, 5 / 12, None)),
                   (((0, 100, -4), (0, 0, 1), 0, INF), None),                     # a curve with four equal control points is never hit
                   (((0, 0, -4), (0, 0, 1), 5, 4), None),                         # invalid rays come back untouched: tnear > tfar
                   (((np.nan, 0, -4), (0, 0, 1), 0, INF), None)]                  # ... NaN origin
CLOSED_TAPER = [(((0, 0, -4), (0, 0, 1), 0, INF), (3.75, .5, None)),              # what tells this surface from a sphere sweep: the disc of
                (((.75, 0, -4), (0, 0, 1), 0, INF), (3.675, .75, None)),          # parameter u has the radius r(u), and the ray meets it at
                (((-.75, 0, -4), (0, 0, 1), 0, INF), (3.825, .25, None)),         # x = -1.5 + 3 u exactly
                (((-4, 0, 0), (1, 0, 0), 0, INF), None),                          # axis rays from either end
                (((4, 0, 0), (-1, 0, 0), 0, INF), None)]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("shape", ["straight", "taper"])
def test_closed_forms(rtc, monkeypatch, flags, form, shape):
    _knobs(monkeypatch, FORMS[form])
    v, idx, cases = (STRAIGHT, np.array([0, 4], np.uint32), CLOSED_STRAIGHT) if shape == "straight" else (TAPER, np.array([0], np.uint32), CLOSED_TAPER)
    dev, sc = _scene(rtc, flags, lambda s: s.add_round_curves(v, idx, geom_id=5))
    assert sc.stats()["accelKind"] == (ACCEL_CURVE_ROBUST if flags else ACCEL_CURVE_FAST) and sc.stats()["primCount"] == len(idx)
    assert dev.get_property(99) == 1
    rays = ch.rays_of(rtc, [r[0][0] for r in cases], [r[0][1] for r in cases], np.array([r[0][2] for r in cases], F), np.array([r[0][3] for r in cases], F))
    rays["u"], rays["v"], rays["Ng_x"] = 7, 7, 7  # a miss leaves the hit part as it was
    got, occ = _trace(rtc, sc, rays)
    for i, (_, want) in enumerate(cases):
        g = got[i]
        if want is None:
            assert g.tobytes() == rays[i].tobytes(), (i, g)
            assert occ[i].tobytes() == ch.occ_of(rtc, rays[i:i + 1])[0].tobytes(), i
            continue
        t, u, ng = want
        assert g["geomID"] == 5 and g["primID"] == 0 and g["instID"] == INVALID and g["v"] == 0, (i, g)
        assert abs(float(g["tfar"]) - t) <= 1e-4 * t and abs(float(g["u"]) - u) <= 1e-4, (i, g)
        if ng is not None:
            n = np.array([g["Ng_x"], g["Ng_y"], g["Ng_z"]], np.float64)
            assert np.abs(n / np.linalg.norm(n) - np.array(ng)).max() <= 1e-3, (i, g)
        assert occ[i]["tfar"] == -np.inf, i
    assert dev.error() == 0
    sc.release()
    dev.release()


# ---- 2. parity ---------------------------------------------------------------------------------------------------------------------------
def _check_parity(got, occ, rays, truth, what):
    gh = got["geomID"] != INVALID
    ng = np.stack([got["Ng_x"], got["Ng_y"], got["Ng_z"]], 1)
    rh.compare(gh, got["geomID"].astype(np.int64), got["primID"].astype(np.int64), got["tfar"], got["u"], got["v"], ng, truth, what)
    k = ~truth["out"]
    assert (got["instID"][truth["hit"] & k] == INVALID).all(), what
    miss = ~truth["hit"] & k
    assert got[miss].tobytes() == rays[miss].tobytes(), what  # a miss comes back untouched
    assert np.array_equal(occ["tfar"][k] == -np.inf, truth["hit"][k]) and np.array_equal(occ["tfar"][miss], rays["tfar"][miss]), what  # any hit equals `truth hit`


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("flags", MODES)
def test_pinned_inputs_meet_the_float64_truth(rtc, monkeypatch, flags, which):
    v, idx, org, dirs = rh.pinned(which)
    truth = dict(rh.pinned_truth(which))
    assert int(truth["hit"].sum()) == rh.HAIR_HITS[which] and int(truth["out"].sum()) == rh.HAIR_LEFT_OUT[which]
    truth["geomID"] = np.where(truth["hit"], 7, -1)
    rays = ch.rays_of(rtc, org, dirs)
    first = None
    for name, knobs in FORMS.items():
        _knobs(monkeypatch, knobs)
        dev, sc = _scene(rtc, flags, lambda s: s.add_round_curves(v, idx, geom_id=7))
        got, occ = _trace(rtc, sc, rays)
        if first is None:
            _check_parity(got, occ, rays, truth, f"input ({which}), Bezier, {name}")
            first = (got.tobytes(), occ.tobytes())
        else:
            assert (got.tobytes(), occ.tobytes()) == first, name
        assert dev.error() == 0
        sc.release()
        dev.release()
    # B-spline input whose converted control points are the same hair (up to the float32 rounding of the conversion, one ulp): the curves
    # that have a valid B-spline form - no negative control radius, round_curve_helpers.bspline_of - as one B-spline geometry, the others
    # beside it as they are.  The truth is the hair's, with the IDs of the two geometries
    bv, bidx, ok = rh.bspline_of(v, idx)
    sub, rest = np.nonzero(ok)[0], np.nonzero(~ok)[0]
    assert len(sub) > 100 and np.abs(ch.native(bv, bidx[sub], "bspline") - ch.native(v, idx[sub])).max() <= 5e-7

    def add(s):
        s.add_round_curves(bv, bidx[sub], basis="bspline", geom_id=7)
        s.add_round_curves(v, idx[rest], geom_id=8)
    dev, sc = _scene(rtc, flags, add)
    assert sc.stats()["primCount"] == len(idx)
    tb = dict(truth)
    where = np.zeros(len(idx), np.int64)
    where[sub], where[rest] = np.arange(len(sub)), np.arange(len(rest))
    tb["geomID"] = np.where(truth["hit"], np.where(ok[truth["primID"]], 7, 8), -1)
    tb["primID"] = np.where(truth["hit"], where[truth["primID"]], -1)
    got, occ = _trace(rtc, sc, rays)
    _check_parity(got, occ, rays, tb, f"input ({which}), B-spline and Bezier geometries")
    assert int((got["geomID"] == 7).sum()) > 100
    sc.release()
    dev.release()


# ---- 3. mixed scenes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("flags", MODES)
def test_mixed_scene_gives_the_nearest_of_the_separate_scenes(rtc, po, monkeypatch, flags, form):
    """round curves, flat curves, line segments and a triangle mesh in one scene: each ray's answer is the nearest of the four scenes'
    answers (the round curves are traced last; no two answers of these inputs have a bit-equal t)"""
    _knobs(monkeypatch, FORMS[form])
    v, idx, _, _ = ch.hair_and_rays()
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
                s.add_curves(v, idx[:256], geom_id=1)
            if "l" in parts:
                s.add_lines(lv, li, geom_id=2)
            if "r" in parts:
                s.add_round_curves(v, idx[256:], geom_id=3)
        return _scene(rtc, flags, add)

    m = 30000
    rays = po.make_random_rays(m, np.zeros(3, F), np.ones(3, F), seed=9)
    dev, sc = scene("tclr")
    got = rtc.aligned_rayhits(m)
    got[:] = rays
    sc.intersect1M(got)
    want = rtc.aligned_rayhits(m)
    want[:] = rays
    ts = []
    for p in "tclr":
        d1, s1 = scene(p)
        one = rtc.aligned_rayhits(m)
        one[:] = rays
        s1.intersect1M(one)
        ts.append(one.copy())
        s1.release()
        d1.release()
    tf = np.stack([x["tfar"] for x in ts], 1)
    hit = np.stack([x["geomID"] != INVALID for x in ts], 1)
    tf = np.where(hit, tf, np.inf)
    best = tf.argmin(1)
    assert not ((np.sort(tf, 1)[:, 0] == np.sort(tf, 1)[:, 1]) & hit.any(1)).any()  # no bit-equal t between two accels
    for k in range(4):
        sel = (best == k) & hit.any(1)
        want[sel] = ts[k][sel]
    assert got.tobytes() == want.tobytes()
    counts = [int((got["geomID"] == g).sum()) for g in range(4)]
    print(f"  hits per geometry (triangles, flat curves, lines, round curves): {counts}")
    assert min(counts) > 100, counts
    sc.release()
    dev.release()


def _gentle_hair(n):
    """n gently bent curves in the unit cube - control points 1/3 of the length (0.1 to 0.2) apart along a line, each moved by a normal
    offset of sigma 0.004, radii 0.004 to 0.012: the radius of curvature stays far above the radius, no tube folds - and the 1024 ray
    origins of curve_helpers.hair_and_rays(seed 6) on the sphere around the cube"""
    rng = np.random.default_rng(60 + n)
    p = 0.2 + 0.6 * rng.random((n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ln = rng.uniform(0.1, 0.2, n)
    v = np.zeros((4 * n, 4), F)
    for k in range(4):
        v[k::4, :3] = p + d * ln[:, None] * (k / 3.0) + rng.normal(scale=0.004, size=(n, 3))
        v[k::4, 3] = rng.uniform(0.004, 0.012, n)
    _, _, org, dirs = ch.hair_and_rays(1, 1024, 6)
    return v, np.arange(0, 4 * n, 4, dtype=np.uint32), org, dirs


def _aim_offsets():
    """offsets from a curve's middle for 1024 rays: two in three within a normal cloud of sigma 0.001, well inside the radii (0.004 to 0.012),
    every third a further 0.05 off in a random direction, well outside - few rays graze a tube, so the rules leave few out"""
    rng = np.random.default_rng(2)
    off = rng.normal(scale=0.001, size=(1024, 3))
    far = rng.normal(size=(1024, 3))
    far *= 0.05 / np.linalg.norm(far, axis=1, keepdims=True)
    off[2::3] += far[2::3]
    return off


_LEAF_TRUTH = {}


def _leaf_input(n):
    """n curves and 1024 rays aimed at them, with the truth: computed once per n"""
    if n not in _LEAF_TRUTH:
        v, idx, org, dirs = _gentle_hair(n)
        org, dirs = org.copy(), dirs.copy()
        cp = ch.native(v, idx)
        mid = cp[:, :, :3].mean(1)
        dirs[:] = (mid[np.arange(1024) % n] + _aim_offsets() - org).astype(F)
        _LEAF_TRUTH[n] = (v, idx, org, dirs, rh.truth([(cp, 3)], org, dirs, np.zeros(1024, F), np.full(1024, np.inf, F)))
    return _LEAF_TRUTH[n]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", [1, 7, 8, 9])
@pytest.mark.parametrize("flags", MODES)
def test_leaf_sizes_around_the_octet_pass(rtc, monkeypatch, flags, n, form):
    """1, 7, 8 and 9 curves - one leaf up to 8, two from 9 on - under the whole contract of the parity test"""
    _knobs(monkeypatch, FORMS[form])
    v, idx, org, dirs, truth = _leaf_input(n)
    assert int(truth["hit"].sum()) > 100
    dev, sc = _scene(rtc, flags, lambda s: s.add_round_curves(v, idx, geom_id=3))
    assert sc.stats()["primCount"] == n
    rays = ch.rays_of(rtc, org, dirs)
    got, occ = _trace(rtc, sc, rays)
    _check_parity(got, occ, rays, truth, f"{n} curves, {form}")
    assert dev.error() == 0
    sc.release()
    dev.release()


# ---- 4. filters --------------------------------------------------------------------------------------------------------------------------
def _ray_fields(args):
    ray = C.cast(args.contents.ray, C.POINTER(C.c_float * 12)).contents
    hit = C.cast(args.contents.hit, C.POINTER(C.c_uint * 8)).contents
    hitf = C.cast(args.contents.hit, C.POINTER(C.c_float * 8)).contents
    return ray, hit, hitf


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("flags", MODES)
def test_filters_see_front_and_back_of_one_tube(rtc, monkeypatch, flags, form):
    """An intersect filter that rejects the first candidate of the straight tube's centre ray: the answer becomes the back, t 4.25, on the
    same (geomID, primID) - the exclusion list of the slot is keyed by t.  An occluded filter that rejects everything: not occluded.  A
    context filter that rejects the tube's geomID: a miss."""
    _knobs(monkeypatch, FORMS[form])
    rays = ch.rays_of(rtc, [(0, 0, -4)], [(0, 0, 1)])
    dev, sc = _scene(rtc, flags, lambda s: s.add_round_curves(STRAIGHT[:4], np.array([0], np.uint32), geom_id=5))
    shown = []

    @rtc.FILTER_FUNC
    def first_rejected(args):
        ray, hit, hitf = _ray_fields(args)
        shown.append((hit[6], hit[5], ray[8]))
        if len(shown) == 1:
            args.contents.valid[0] = 0

    @rtc.FILTER_FUNC
    def all_rejected(args):
        args.contents.valid[0] = 0

    sc.set_filters(5, intersect=first_rejected, occluded=all_rejected)
    sc.commit()
    got, occ = _trace(rtc, sc, rays)
    assert len(shown) == 2 and shown[0][:2] == (5, 0) and shown[1][:2] == (5, 0), shown
    assert abs(shown[0][2] - 3.75) <= 3.75e-4 and abs(shown[1][2] - 4.25) <= 4.25e-4
    assert got["geomID"][0] == 5 and got["primID"][0] == 0 and abs(float(got["tfar"][0]) - 4.25) <= 4.25e-4
    assert occ["tfar"][0] == rays["tfar"][0]  # not occluded
    sc.release()
    dev.release()
    dev, sc = _scene(rtc, flags, lambda s: s.add_round_curves(STRAIGHT[:4], np.array([0], np.uint32), geom_id=5))

    @rtc.FILTER_FUNC
    def no_tube(args):
        _, hit, _ = _ray_fields(args)
        if hit[6] == 5:
            args.contents.valid[0] = 0

    ctx = rtc.make_context()
    ctx.filter = C.cast(no_tube, C.c_void_p)
    got, occ = _trace(rtc, sc, rays, ctx=ctx)
    assert got.tobytes() == rays.tobytes() and occ["tfar"][0] == rays["tfar"][0]
    sc.release()
    dev.release()


# ---- 5. entry paths and limits -------------------------------------------------------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("flags", MODES)
def test_entry_paths_are_bit_identical(rtc, po, monkeypatch, flags, form):
    import torch
    _knobs(monkeypatch, FORMS[form])
    v, idx, _, _ = ch.hair_and_rays()

    def scene(extra=""):
        return _scene(rtc, flags, lambda s: s.add_round_curves(v, idx), CFG + extra)

    m = 40000
    rays = po.make_random_rays(m, np.zeros(3, F), np.ones(3, F), seed=21)
    dev, sc = scene()
    L = sc.lib
    t = torch.from_numpy(rays.view(np.uint8).reshape(-1, 80).copy()).cuda()  # device-resident batch = the reference answer
    sc.intersect1M(t)
    torch.cuda.synchronize()
    want = t.cpu().numpy().reshape(-1).view(rays.dtype)
    nh = int((want["geomID"] != INVALID).sum())
    assert nh > 1000, nh
    h = rtc.aligned_rayhits(m)  # host, pipelined
    h[:] = rays
    sc.intersect1M(h)
    assert h.tobytes() == want.tobytes()
    s = rtc.aligned_rayhits(m)  # host, small batches
    s[:] = rays
    for a in range(0, 4096, 500):
        sc.intersect1M(s[a:a + 500])
    assert s[:4096].tobytes() == want[:4096].tobytes()
    c = rtc.aligned_rayhits(m)  # instrumented twins
    c[:] = rays
    cnt = sc.intersect1M_counted(c)
    assert c.tobytes() == want.tobytes()
    assert cnt["rays"] == m and cnt["hits"] == nh and cnt["primTests"] > 0
    wocc = ch.occ_of(rtc, rays)
    sc.occluded1M(wocc)
    co = ch.occ_of(rtc, rays)
    ocnt = sc.occluded1M_counted(co)
    assert co.tobytes() == wocc.tobytes() and np.array_equal(wocc["tfar"] == -np.inf, want["geomID"] != INVALID)
    assert ocnt["rays"] == m and ocnt["hits"] == nh and 0 < ocnt["primTests"] <= cnt["primTests"]
    k = 2048  # multi-threaded rtcIntersect1 / rtcOccluded1 (call combiner)
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
    ctx = rtc.make_context()  # packets of 4, 8 and 16 and their occluded twins
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
    n = 300  # the SoA pointer stream and its occluded twin
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
    # service=1: the kinds 42 / 43 have no service kernel, the calls go through the call combiner and agree
    dev, sc = scene(",service=1")
    sv = rtc.aligned_rayhits(k)
    sv[:] = rays[:k]
    for i in range(0, k, 32):
        sc.intersect1M(sv[i:i + 32])
    assert sv.tobytes() == want[:k].tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    sc.release()
    dev.release()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("flags", MODES)
def test_a_counted_batch_counts_the_records_visited(rtc, monkeypatch, flags, form):
    """three curves make one leaf, the root: every valid ray visits it, and a closest-hit ray visits all three records"""
    _knobs(monkeypatch, FORMS[form])
    v, idx, org, dirs = ch.hair_and_rays(3, 1000, 8)
    dev, sc = _scene(rtc, flags, lambda s: s.add_round_curves(v, idx))
    assert sc.accel_root() == (0x80000000 | (3 << 26))
    rays = ch.rays_of(rtc, org, dirs)
    c = rtc.aligned_rayhits(len(rays))
    c[:] = rays
    cnt = sc.intersect1M_counted(c)
    assert cnt["rays"] == 1000 and cnt["primTests"] == 3 * 1000, cnt
    got, _ = _trace(rtc, sc, rays)
    assert c.tobytes() == got.tobytes()
    sc.release()
    dev.release()


MIN_SPILLS = 0.05 * ds.GPU_RAYS  # as tests/test_gpu_deep_stack.py: every ray above slot 16 pushes at least one entry to HBM


@pytest.mark.parametrize("flags", MODES)
def test_node_step_forms_agree_beyond_the_lds_stack(rtc, monkeypatch, flags):
    """A soup of needles as long as the cube they lie in (tests/deep_stack_helpers.py), as straight tubes of radius 0.01: node boxes overlap
    everywhere and rays carry their stacks into the HBM overflow area, which the counted twin's stackSpills must show."""
    tv, tt = ds.sliver_soup(ds.N_SLIVERS, ds.SOUP_SEED)
    ends = tv.reshape(-1, 3, 3)[:, :2].astype(np.float64)
    p = np.stack([ends[:, 0] + (ends[:, 1] - ends[:, 0]) * k / 3.0 for k in range(4)], 1).reshape(-1, 3)
    v = np.concatenate([p, np.full((len(p), 1), 0.01)], 1).astype(F)
    idx = np.arange(0, len(v), 4, dtype=np.uint32)
    lo, hi = ds.bounds(p.astype(F))
    from helpers import random_rays_np
    org, dirs = random_rays_np(ds.GPU_RAYS, lo, hi, ds.GPU_RAY_SEED)
    rays = ds.rays_of(rtc, org, dirs)
    first = None
    for name, knobs in FORMS.items():
        _knobs(monkeypatch, knobs)
        dev, sc = _scene(rtc, flags, lambda s: s.add_round_curves(v, idx))
        assert sc.stats()["maxDepth"] >= 3
        got, occ = _trace(rtc, sc, rays)
        c = ds.copy_of(rtc, rays)
        cnt = sc.intersect1M_counted(c)
        assert c.tobytes() == got.tobytes(), f"{name}: the instrumented twin differs from the plain kernel"
        print(f"  needle tubes, {name}: stackSpills {cnt['stackSpills']} ({len(rays)} rays), {int((got['geomID'] != INVALID).sum())} hits")
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
