"""Motion blur on flat Bezier and B-spline curves on the GPU: the leaf of csrc/trace_curve_mb.hip in its lane-per-ray and octet forms, under
robust and fast traversal, under swept node boxes (kinds 44 / 45) and time-dependent ones (mb_bounds=linear, kinds 46 / 47).

The pinned inputs are exact in float32 at every ray time (tests/curve_mb_helpers.py), so the moving scene is held to the STATIC curve
kernel on the control points at the ray's time bit for bit, and to the float64 truth of tests/curve_helpers.py under the project's 1e-4
contract (curve_helpers.compare)."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import curve_helpers as ch
import curve_mb_helpers as mh
import deep_stack_helpers as ds
from curve_mb_helpers import CURVEMB_DT
from helpers import INVALID
from line_helpers import ROBUST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")
KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL")
FORMS = {"lane form": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "0", "RTAMD_OCT_LEAF": "0"},    # every node and leaf step one ray per lane
         "octet form": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "32", "RTAMD_OCT_LEAF": "1"}}  # 8 lanes per ray wherever the kernel allows it
BOUNDS = {"swept": "", "linear": "mb_bounds=linear"}
MODES = [pytest.param(ROBUST, id="robust"), pytest.param(0, id="fast")]
KIND = {(ROBUST, "swept"): 44, (0, "swept"): 45, (ROBUST, "linear"): 46, (0, "linear"): 47}
RAYF = ["org_x", "org_y", "org_z", "tnear", "dir_x", "dir_y", "dir_z", "time", "tfar", "mask", "id", "flags"]
HITF = ["Ng_x", "Ng_y", "Ng_z", "u", "v", "primID", "geomID", "instID"]
NEXT = np.nextafter
F = np.float32


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


def _rays(rtc, org, dirs, times, tnear=0.0, tfar=np.inf):
    rh = ch.rays_of(rtc, org, dirs, tnear, tfar)
    rh["time"] = times
    return rh


# ---- 1. bit-identity with the static curve kernel ------------------------------------------------------------------------------------
_STATIC = {}


def _static_reference(rtc, flags, mv, N, rh):
    """every ray against a static add_curves scene of the control points at its time, traced by the static curve kernel (default knobs)"""
    key = (flags, len(mv["steps"]), N)
    if key not in _STATIC:
        want, wocc = rh.copy(), ch.occ_of(rtc, rh)
        for t in np.unique(mv["times"]):
            sel = np.nonzero(mv["times"] == t)[0]
            dev, sc = _scene(rtc, flags, lambda s: s.add_curves(mh.at_time(mv["steps"], t), mv["idx"], tessellation_rate=N, geom_id=7))
            g, o = _trace(rtc, sc, rh[sel])
            want[sel], wocc[sel] = g, o
            sc.release()
            dev.release()
        _STATIC[key] = (want, wocc)
    return _STATIC[key]


@pytest.mark.parametrize("nsteps,N", [(2, 4), (5, 4), (2, 9), (5, 9)])
@pytest.mark.parametrize("flags", MODES)
def test_moving_hair_is_bit_identical_to_the_static_kernel_at_the_rays_time(rtc, monkeypatch, flags, nsteps, N):
    """geomID, primID and the bits of t, u, v and Ng of every ray, and the occluded answer, in the lane and octet forms, under swept and
    linear bounds.  A ray is left out only where the truth's two nearest candidates are within 1e-4 in t (the two scenes have different
    trees), at most 0.5 %.  N = 9 takes a second pass per curve."""
    mv = mh.hair_mb_truth(nsteps, N)
    assert int(mv["hit"].sum()) == mh.HAIR_MB_HITS[(nsteps, N)]
    _knobs(monkeypatch, {})
    rh = _rays(rtc, mv["org"], mv["dirs"], mv["times"])
    want, wocc = _static_reference(rtc, flags, mv, N, rh)
    out = mv["near_tie"]
    assert out.sum() <= 0.005 * len(rh)
    k = ~out
    assert int((want["geomID"] != INVALID).sum()) > 800
    for bname, bcfg in BOUNDS.items():
        for fname, knobs in FORMS.items():
            _knobs(monkeypatch, knobs)
            dev, sc = _scene(rtc, flags, lambda s: s.add_curves_mb(mv["steps"], mv["idx"], tessellation_rate=N, geom_id=7), bcfg)
            assert sc.stats()["accelKind"] == KIND[(flags, bname)] and sc.stats()["primCount"] == (nsteps - 1) * len(mv["idx"])
            got, occ = _trace(rtc, sc, rh)
            what = f"{nsteps} steps, N = {N}, {bname}, {fname}"
            for f in ("geomID", "primID", "tfar", "u", "v", "Ng_x", "Ng_y", "Ng_z", "instID"):
                assert np.array_equal(got[f][k].view(np.uint32), want[f][k].view(np.uint32)), (what, f, int((got[f][k].view(np.uint32) != want[f][k].view(np.uint32)).sum()))
            assert got[k].tobytes() == want[k].tobytes(), what
            assert np.array_equal(occ["tfar"][k] == -np.inf, got["geomID"][k] != INVALID) and occ[k].tobytes() == wocc[k].tobytes(), what
            assert dev.error() == 0
            sc.release()
            dev.release()


# ---- 2. the float64 truth ------------------------------------------------------------------------------------------------------------
def _check_parity(got, occ, rh, truth, what, geom_id=7):
    """curve_helpers.compare (hit / miss, geomID / primID exact, t within 1e-4 relative, u and v within 1e-4 absolute, at most 0.5 % of
    the rays left out, and only where the float64 truth is within 1e-4 of an edge of a ribbon quad or of a tie); Ng within 1e-4 of the
    truth's eval_du(u) (tests/test_gpu_curves.py); a miss comes back untouched; the any-hit answer agrees"""
    t = dict(truth)
    t["geomID"] = np.full(len(rh), geom_id)
    gh = got["geomID"] != INVALID
    ch.compare(gh, got["geomID"].astype(np.int64), got["primID"].astype(np.int64), got["tfar"], got["u"], got["v"], t, what)
    k = ~(t["near_edge"] | t["near_tie"])
    h = t["hit"] & k
    assert (got["instID"][h] == INVALID).all(), what
    ng = np.stack([got["Ng_x"], got["Ng_y"], got["Ng_z"]], 1).astype(np.float64)
    cp = t["cp"][..., :3].astype(np.float64)
    dd = 6.0 * np.maximum(np.abs(cp[:, 0] - 2 * cp[:, 1] + cp[:, 2]), np.abs(cp[:, 1] - 2 * cp[:, 2] + cp[:, 3])).max(1)
    tol = 1e-4 * dd + 1e-5 * np.linalg.norm(t["Ng"], axis=1)
    assert (np.abs(ng[h] - t["Ng"][h]).max(1) <= tol[h]).all(), what
    miss = ~t["hit"] & k
    assert got[miss].tobytes() == rh[miss].tobytes(), what  # a miss comes back untouched
    assert np.array_equal(occ["tfar"][k] == -np.inf, t["hit"][k]) and np.array_equal(occ["tfar"][miss], rh["tfar"][miss]), what


@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("nsteps", [2, 5])
@pytest.mark.parametrize("N", [1, 4, 9, 16])
@pytest.mark.parametrize("basis", ["bezier", "bspline"])
def test_moving_hair_meets_the_float64_truth(rtc, monkeypatch, basis, N, nsteps, bounds):
    """Bezier and B-spline input (for B-spline the truth converts every step to Bezier points and interpolates those); robust traversal
    for the odd rates, fast for the even ones"""
    _knobs(monkeypatch, {})
    flags = ROBUST if N & 1 else 0
    mv = mh.hair_mb_truth(nsteps, N, basis)
    rh = _rays(rtc, mv["org"], mv["dirs"], mv["times"])
    dev, sc = _scene(rtc, flags, lambda s: s.add_curves_mb(mv["steps"], mv["idx"], basis=basis, tessellation_rate=N, geom_id=7), BOUNDS[bounds])
    assert sc.stats()["accelKind"] == KIND[(flags, bounds)]
    got, occ = _trace(rtc, sc, rh)
    _check_parity(got, occ, rh, mv, f"moving hair, {basis}, N = {N}, {nsteps} steps, {bounds}")
    assert int(mv["hit"].sum()) > 300 and dev.error() == 0
    sc.release()
    dev.release()


# ---- 3. closed forms, exact ----------------------------------------------------------------------------------------------------------
# curve 0: the straight curve of tests/test_gpu_curves.py along x (the point at u is (-1.5 + 3 u, 0, 0)), radius 1/4 at step 0 and 1/2 at
# step 1, moved by 8 along x: at time t its centre is (8 t, 0, 0), its radius (1 + t) / 4.  curve 1, 100 up in y, is mirrored through
# (0, 100, 0) between the steps: at time 1/2 all four control points coincide there - a zero derivative, a NaN normal, no hit.
_A = np.array([[-1.5, 0, 0, .25], [-.5, 0, 0, .25], [.5, 0, 0, .25], [1.5, 0, 0, .25]], F)
_B = np.array([[-1, 100, 0, .25], [-.5, 100.5, 0, .25], [.5, 99.5, .5, .25], [1, 100, 0, .25]], F)
CLOSED = [np.concatenate([_A, _B]), np.concatenate([_A + np.array([8, 0, 0, .25], F), np.concatenate([-_B[:, :3] + np.array([0, 200, 0], F), _B[:, 3:]], 1)])]
# (org, dir, time) -> None (miss) or (t, u, v)
CLOSED_RAYS = [(((0, 0, -4), (0, 0, 1), 0.0), (4, .5, 0)),                        # where the ribbon is at time 0 ...
               (((2, 0, -4), (0, 0, 1), 0.25), (4, .5, 0)),                      # ... 1/4
               (((4, 0, -4), (0, 0, 2), 0.5), (2, .5, 0)),                       # ... 1/2
               (((8, 0, -4), (0, 0, 1), 1.0), (4, .5, 0)),                       # ... 1
               (((8, 0, -4), (0, 0, 1), 0.0), None),                             # and nowhere else
               (((0, 0, -4), (0, 0, 1), 1.0), None),
               (((0, 0, -4), (0, 0, 1), 0.5), None),
               (((4, 0, -4), (0, 0, 1), 0.25), None),
               (((2.375, 0, -4), (0, 0, 1), 0.25), (4, .625, 0)),                # u along the interpolated axis: x from 1/2 to 7/2
               (((4, .375, -4), (0, 0, 1), 0.5), (4, .5, 1)),                    # grazing at the interpolated radius 3/8: max(U, V) <= 0
               (((4, NEXT(F(.375), F(0)), -4), (0, 0, 1), 0.5), (4, None, None)),  # ... from inside
               (((4, NEXT(F(.375), F(1)), -4), (0, 0, 1), 0.5), None),           # ... one ulp outside
               (((4, -.375, -4), (0, 0, 1), 0.5), (4, .5, -1)),
               (((4, -NEXT(F(.375), F(1)), -4), (0, 0, 1), 0.5), None),
               (((2, .3125, -4), (0, 0, 1), 0.25), (4, .5, 1)),                  # radius 5/16 at time 1/4
               (((2, NEXT(F(.3125), F(1)), -4), (0, 0, 1), 0.25), None),
               (((0, .25, -4), (0, 0, 1), 0.0), (4, .5, 1)),                     # radius 1/4 at time 0, 1/2 at time 1
               (((0, NEXT(F(.25), F(1)), -4), (0, 0, 1), 0.0), None),
               (((8, .5, -4), (0, 0, 1), 1.0), (4, .5, 1)),
               (((8, NEXT(F(.5), F(1)), -4), (0, 0, 1), 1.0), None),
               (((6.5, 0, -4), (0, 0, 1), 1.0), (4, 0, 0)),                      # the two ends of the curve at time 1
               (((9.5, 0, -4), (0, 0, 1), 1.0), (4, 1, 0)),
               (((NEXT(F(9.5), F(10)), 0, -4), (0, 0, 1), 1.0), None),
               (((0, 100, -4), (0, 0, 1), 0.5), None),                           # curve 1 at time 1/2: all control points equal, never hit
               (((0, 100, -4), (0, 0, 1), np.nan), None)]                        # a NaN time misses


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("flags", MODES)
def test_closed_forms_are_exact(rtc, monkeypatch, flags, bounds, form):
    _knobs(monkeypatch, FORMS[form])
    dev, sc = _scene(rtc, flags, lambda s: s.add_curves_mb(CLOSED, np.array([0, 4], np.uint32), geom_id=5), BOUNDS[bounds])
    assert sc.stats()["accelKind"] == KIND[(flags, bounds)] and sc.stats()["primCount"] == 2
    mid = mh.at_time(CLOSED, 0.5)
    assert (mid[4:, :3] == np.array([0, 100, 0], F)).all()  # curve 1 at time 1/2
    rh = _rays(rtc, [r[0][0] for r in CLOSED_RAYS], [r[0][1] for r in CLOSED_RAYS], np.array([r[0][2] for r in CLOSED_RAYS], F))
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
        assert g["tfar"] == F(t), (i, g)
        assert (g["u"] == F(u) and g["v"] == F(v)) if v is not None else (abs(g["u"] - .5) < 1e-6 and .999 < g["v"] <= 1), (i, g)  # (one ulp inside the edge: v = 2 V - 1 may round to 1)
        assert (g["Ng_x"], g["Ng_y"], g["Ng_z"]) == (3, 0, 0), (i, g)  # eval_du(u) of the interpolated control points, not normalised
        assert occ[i]["tfar"] == -np.inf, i
    # curve 1 where it is at time 1/4: hit (its derivative is not zero there), and the moving scene equals the static one on at_time()
    # (a little off its middle: the ray through (0, 100) meets the joint of two ribbon quads end on, which neither quad's edge test takes)
    q = _rays(rtc, [(.125, 100.0625, -4)] * 2, [(0, 0, 1)] * 2, np.array([0.25, 0.75], F))
    g1, o1 = _trace(rtc, sc, q)
    assert (g1["primID"] == 1).all() and (o1["tfar"] == -np.inf).all()
    for i, t in enumerate((0.25, 0.75)):
        d2, s2 = _scene(rtc, flags, lambda s: s.add_curves(mh.at_time(CLOSED, t), np.array([0, 4], np.uint32), geom_id=5))
        g2, _ = _trace(rtc, s2, q[i:i + 1])
        assert g2.tobytes() == g1[i:i + 1].tobytes(), (i, g1[i], g2)
        s2.release()
        d2.release()
    assert dev.error() == 0
    sc.release()
    dev.release()


# ---- 4. tie and pass rule ------------------------------------------------------------------------------------------------------------
def _tie_rays():
    """the rays of tests/test_gpu_curves.py: on a 1/64 grid about the middle of the curves below, directions on a 1/32 grid"""
    rng = np.random.default_rng(3)
    org = np.concatenate([rng.uniform(-.4, .4, (40, 1)), rng.uniform(-.1, .1, (40, 1)), np.full((40, 1), -4.)], 1)
    dirs = np.concatenate([np.round(rng.uniform(-.1, .1, (40, 2)) * 32) / 32, np.ones((40, 1))], 1)
    return (np.round(org * 64) / 64).astype(F), dirs.astype(F)


@pytest.mark.parametrize("flags", MODES)
def test_coincident_moving_curves_the_last_record_wins(rtc, monkeypatch, flags):
    """5 coincident moving curves with primIDs of their own in one leaf, two passes per curve (N = 16): the record and pass rule of the
    static leaf on the interpolated control points.  Every record is tested against the tfar the one before it left with `T <= absDen *
    tfar`: the record at the last place of the leaf wins the equal t where absDen * fl(T / den) does not round below T (curve_helpers
    `again`), otherwise the first keeps it - in every form and under both bounds, bit for bit."""
    s0 = np.array([[-1.5, 0, 0, .25], [-.5, .25, 0, .125], [.5, -.25, .5, .25], [1.5, 0, 0, .125]], F)
    s1 = np.array([[-1.5, .125, 0, .125], [-.5, 0, .25, .25], [.5, 0, .25, .125], [1.5, -.125, 0, .25]], F)
    idx = np.arange(0, 20, 4, dtype=np.uint32)
    org, dirs = _tie_rays()
    times = np.where(np.arange(len(org)) % 2 == 0, 0.25, 0.75).astype(F)
    m = len(org)
    results = {}
    for bname, bcfg in BOUNDS.items():
        for name, knobs in FORMS.items():
            _knobs(monkeypatch, knobs)
            dev, sc = _scene(rtc, flags, lambda s: s.add_curves_mb([np.tile(s0, (5, 1)), np.tile(s1, (5, 1))], idx, tessellation_rate=16), bcfg)
            assert sc.accel_root() == (0x80000000 | (5 << 26))  # one leaf
            rec = sc.accel_data(2).view(CURVEMB_DT)
            got, occ = _trace(rtc, sc, _rays(rtc, org, dirs, times))
            won = 0
            for t in (0.25, 0.75):
                sel = np.nonzero(times == F(t))[0]
                cp, take = mh.interpolated_records(rec, t)
                assert take.all() and np.array_equal(cp[0], mh.at_time([s0, s1], t))
                c32 = ch.closest([(cp[:1], 16, 0)], org[sel], dirs[sel], np.zeros(len(sel), F), np.full(len(sel), np.inf, F), np.float32)
                h = c32["hit"]
                want = np.where(c32["again"], rec["primID"][4], rec["primID"][0])
                won += int((h & c32["again"]).sum())
                assert np.array_equal(got["geomID"][sel] != INVALID, h), (bname, name)
                assert np.array_equal(got["primID"][sel][h], want[h]) and np.array_equal(got["tfar"][sel][h], c32["t"][h].astype(F)), (bname, name, t)
                assert np.array_equal(occ["tfar"][sel] == -np.inf, h)
            print(f"  {bname}, {name}: the last record wins {won} of {m} rays")
            assert won >= 8
            results[(bname, name)] = got.tobytes()
            sc.release()
            dev.release()
    assert len(set(results.values())) == 1


# ---- 5. time-segment selection -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES)
def test_only_the_records_of_the_rays_time_segment_take_part(rtc, monkeypatch, flags):
    """Three time steps, five coincident curves that move by 4 along y and back: every (curve, time segment) pair has the same swept and the
    same mid-segment box, so the builder cannot part them - ONE leaf of ten records that mixes both time segments.  Beside them a curve
    that is far away (x = 1000) in the first time segment and comes to x = 4 at the last step.  A record of the other segment takes no part: where only
    the other segment's records would put a curve nothing is hit, and the counted twin tests the N quads of the five records of the
    ray's segment, not of all ten."""
    copies, N = 5, 4
    a = np.tile(_A, (copies, 1))
    b = a + np.array([0, 4, 0, 0], F)
    far0 = _A + np.array([1000, 0, 0, 0], F)
    far2 = _A + np.array([4, 0, 0, 0], F)
    steps = [np.concatenate([a, far0]), np.concatenate([b, far0]), np.concatenate([a, far2])]
    idx = np.arange(0, 4 * copies, 4, dtype=np.uint32)
    # times 0, 1/8 (segment 0, f = 1/4: y = 1), 5/8 (segment 1, f = 1/4: y = 3), 1 (segment 1, f = 1), 1/2 (the joint: segment 1, f = 0)
    org = np.array([[0, 0, -4], [0, 1, -4], [0, 3, -4], [0, 0, -4], [0, 4, -4]], F)
    dirs = np.tile(np.array([[0, 0, 1]], F), (5, 1))
    times = np.array([0.0, 0.125, 0.625, 1.0, 0.5], F)
    results = {}
    for bname, bcfg in BOUNDS.items():
        for name, knobs in FORMS.items():
            _knobs(monkeypatch, knobs)
            dev, sc = _scene(rtc, flags, lambda s: (s.add_curves_mb(steps, idx, tessellation_rate=N, geom_id=0),
                                                    s.add_curves_mb(steps, np.array([4 * copies], np.uint32), tessellation_rate=N, geom_id=1)), bcfg)
            rec = sc.accel_data(2).view(CURVEMB_DT)
            assert len(rec) == 2 * copies + 2 and sorted(rec["segment"].tolist()) == [0] * (copies + 1) + [1] * (copies + 1)
            rh = _rays(rtc, org, dirs, times)
            got, occ = _trace(rtc, sc, rh)
            assert (got["geomID"] == 0).all() and (got["tfar"] == 4).all() and (got["u"] == .5).all() and (occ["tfar"] == -np.inf).all(), (bname, name, got)
            # at time 1/8 nothing is at y = 3 (where the second segment's records are at THEIR f = 1/4), at time 5/8 nothing at y = 1
            miss = _rays(rtc, org[[2, 1]], dirs[:2], times[[1, 2]])
            g2, _ = _trace(rtc, sc, miss)
            assert (g2["geomID"] == INVALID).all(), (bname, name)
            # the far curve: in segment 0 it stays at x = 1000; in segment 1 it comes from there to x = 4 (time 1) - at time 1/2 it is not at x = 4
            q = _rays(rtc, [(1000, 0, -4), (4, 0, -4), (4, 0, -4), (1000, 0, -4)], [(0, 0, 1)] * 4, np.array([0.25, 1.0, 0.5, 1.0], F))
            g3, _ = _trace(rtc, sc, q)
            assert g3["geomID"].tolist() == [1, 1, INVALID, INVALID], (bname, name, g3)
            # counted: each of the 5 rays meets the one leaf of the coincident curves and tests the 5 records of its own segment, N quads
            # each (and, under swept boxes, possibly the far curve's record of its segment); all ten would be twice as many
            c = rh.copy()
            cnt = sc.intersect1M_counted(c)
            assert c.tobytes() == got.tobytes()
            print(f"  {bname}, {name}: primTests {cnt['primTests']} for {len(rh)} rays, {copies} records of {N} quads per ray and segment")
            assert len(rh) * copies * N <= cnt["primTests"] <= len(rh) * (copies + 1) * N, (bname, name, cnt["primTests"])
            results[(bname, name)] = got.tobytes()
            sc.release()
            dev.release()
    assert len(set(results.values())) == 1


# ---- 6. a fast mover -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES)
def test_fast_mover_is_hit_only_where_it_is_and_linear_bounds_test_less(rtc, monkeypatch, flags):
    """The hair moves by 16 x its extent along x between two steps.  Every second ray aims where the hair is at the ray's time, the others
    where it is half a shutter away.  Hits are those of the truth at the ray's time; the counted twin under mb_bounds=linear tests
    strictly fewer ribbon quads and visits strictly fewer leaves than under swept boxes, with byte-identical records."""
    _knobs(monkeypatch, {})
    v, idx, org, dirs = ch.hair_and_rays()
    m = len(org)
    s0 = mh.snap16(v).astype(F)
    s1 = s0.copy()
    s1[:, 0] += 16
    steps = [s0, s1]
    i = np.arange(m)
    times = ((i % 5) / 4.0).astype(F)
    aim = np.where(i % 2 == 0, times, (((i + 2) % 5) / 4.0)).astype(F)
    org = org.copy()
    org[:, 0] += 16 * aim
    truth = mh.moving_truth(mh.native_steps(steps, idx), 4, org, dirs, times, np.float64)
    on, off = truth["hit"][i % 2 == 0], truth["hit"][i % 2 == 1]
    print(f"  truth: {int(on.sum())} of {len(on)} rays aimed at the hair's place hit, {int(off.sum())} of {len(off)} aimed elsewhere")
    assert on.sum() > 400 and off.sum() < on.sum() // 8
    rh = _rays(rtc, org, dirs, times)
    res = {}
    for bname, bcfg in BOUNDS.items():
        dev, sc = _scene(rtc, flags, lambda s: s.add_curves_mb(steps, idx, geom_id=7), bcfg)
        got, occ = _trace(rtc, sc, rh)
        _check_parity(got, occ, rh, truth, f"fast mover, {bname}")
        c = rh.copy()
        cnt = sc.intersect1M_counted(c)
        assert c.tobytes() == got.tobytes()
        res[bname] = (got.tobytes(), occ.tobytes(), cnt)
        sc.release()
        dev.release()
    sw, li = res["swept"][2], res["linear"][2]
    print(f"  primTests swept {sw['primTests']} linear {li['primTests']}, leafVisits swept {sw['leafVisits']} linear {li['leafVisits']}, "
          f"nodeVisits swept {sw['nodeVisits']} linear {li['nodeVisits']}")
    assert res["swept"][:2] == res["linear"][:2]
    assert li["primTests"] < sw["primTests"] and li["leafVisits"] < sw["leafVisits"]


# ---- 7. times outside the shutter, and NaN -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("flags", MODES)
def test_times_outside_the_shutter_extrapolate_and_a_nan_time_misses(rtc, monkeypatch, flags, bounds):
    _knobs(monkeypatch, {})
    mv = mh.hair_mb_truth(2, 4)
    m = 1024
    org, dirs = mv["org"][:m], mv["dirs"][:m]
    times = mv["times"][:m].copy()
    odd = np.arange(m) % 8
    times[odd == 1], times[odd == 3], times[odd == 5] = -0.25, 1.5, np.nan
    special = np.isin(odd, (1, 3, 5))
    rh = _rays(rtc, org, dirs, times)
    dev, sc = _scene(rtc, flags, lambda s: s.add_curves_mb(mv["steps"], mv["idx"], geom_id=7), BOUNDS[bounds])
    got, occ = _trace(rtc, sc, rh)
    # the NaN rays miss and come back untouched
    nan = np.isnan(times)
    assert nan.sum() == m // 8 and got[nan].tobytes() == rh[nan].tobytes() and occ[nan].tobytes() == ch.occ_of(rtc, rh)[nan].tobytes()
    # an out-of-range ray reports nothing that is not a hit of the extrapolated first / last segment (the node boxes do not follow the
    # extrapolation, so it may miss what the extrapolated geometry would give)
    n_hits = 0
    for t in (-0.25, 1.5):
        sel = np.nonzero(times == F(t))[0]
        cp = ch.native(mh.at_time(mv["steps"], t), mv["idx"])
        valid, T, U, V, _, _ = ch.candidates(cp, 4, org[sel], dirs[sel], np.zeros(len(sel), F), np.full(len(sel), np.inf, F), np.float32)
        for j, i in enumerate(sel):
            if got["geomID"][i] == INVALID:
                assert got[i].tobytes() == rh[i].tobytes() and occ["tfar"][i] == rh["tfar"][i]
                continue
            p = int(got["primID"][i])
            n_hits += 1
            near = np.abs(T[j, p].astype(np.float64) - float(got["tfar"][i])) <= 1e-4 * abs(float(got["tfar"][i]))
            assert got["geomID"][i] == 7 and (valid[j, p] & near).any(), (t, i, got[i])
            q = int(np.nonzero(valid[j, p] & near)[0][0])
            assert abs(float(got["u"][i]) - float(U[j, p, q])) <= 1e-4 and abs(float(got["v"][i]) - float(V[j, p, q])) <= 1e-4 and occ["tfar"][i] == -np.inf
    print(f"  {bounds}: {n_hits} hits of {int((special & ~nan).sum())} rays outside the shutter")
    assert n_hits > 20
    # every other record equals the batch traced without them
    rest = ~special
    g2, o2 = _trace(rtc, sc, rh[rest])
    assert got[rest].tobytes() == g2.tobytes() and occ[rest].tobytes() == o2.tobytes()
    assert dev.error() == 0
    sc.release()
    dev.release()


# ---- 8. mixed scenes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("flags", MODES)
def test_mixed_scene_equals_the_accels_traced_in_reference_order(rtc, po, flags, bounds):
    """triangles, static curves, moving curves, line segments and moving line segments in one scene = the five accels traced alone one
    after the other in the reference's order (triangles, hair, motion-blur hair, lines, motion-blur lines; scene.cpp:650-660): every ray
    keeps the nearest, and a later accel wins a bit-equal t"""
    rng = np.random.RandomState(4)
    c = rng.rand(200, 1, 3).astype(F)
    tv = (c + (rng.rand(200, 3, 3).astype(F) - 0.5) * 0.1).reshape(-1, 3).astype(F)
    tt = np.arange(600, dtype=np.uint32).reshape(-1, 3)
    lv = np.concatenate([rng.rand(400, 3), rng.uniform(0.004, 0.012, (400, 1))], 1).astype(F)
    lv[1::2, :3] = lv[0::2, :3] + (rng.rand(200, 3).astype(F) - 0.5) * 0.2
    li = np.arange(0, 400, 2, dtype=np.uint32)
    lv2 = lv + np.array([.25, .125, 0, .002], F)
    hv, hidx, _, _ = ch.hair_and_rays()
    mv = mh.hair_mb_truth(2, 4)
    msteps = [s * np.array([1, 1, 1, 1], F) + np.array([-.125, 0, .125, 0], F) for s in mv["steps"]]

    def scene(parts):
        def add(s):
            if "t" in parts:
                s.add_triangles(tv, tt, geom_id=0)
            if "c" in parts:
                s.add_curves(hv[:1024], hidx[:256], geom_id=1)
            if "C" in parts:
                s.add_curves_mb(msteps, mv["idx"], geom_id=2)
            if "l" in parts:
                s.add_lines(lv, li, geom_id=3)
            if "L" in parts:
                s.add_lines_mb([lv, lv2], li, geom_id=4)
        return _scene(rtc, flags, add, BOUNDS[bounds])

    m = 50000
    rays = po.make_random_rays(m, np.zeros(3, F), np.ones(3, F), seed=9)
    rays["time"] = (np.random.RandomState(4).randint(0, 17, m) / 16.0).astype(F)
    dev, sc = scene("tcClL")
    got = rtc.aligned_rayhits(m)
    got[:] = rays
    sc.intersect1M(got)
    want = rtc.aligned_rayhits(m)
    want[:] = rays
    for p in "tcClL":
        d1, s1 = scene(p)
        s1.intersect1M(want)
        s1.release()
        d1.release()
    assert got.tobytes() == want.tobytes()
    counts = [int((got["geomID"] == g).sum()) for g in range(5)]
    print(f"  hits per geometry (triangles, curves, moving curves, lines, moving lines): {counts}")
    assert min(counts) > 100, counts
    sc.release()
    dev.release()


@pytest.mark.parametrize("flags", MODES)
def test_moving_curves_beside_instances_in_a_top_scene(rtc, po, flags):
    """a top scene with moving curves of its own beside an instance of a scene without curves = the motion-blur curve accel, then the
    instance accel"""
    tv = np.array([[.1, .1, .5], [.9, .1, .5], [.5, .9, .45], [.2, .8, .2], [.8, .3, .7]], F)
    tt = np.array([[0, 1, 2], [0, 3, 4], [1, 3, 4]], np.uint32)
    mv = mh.hair_mb_truth(2, 4)
    dev = rtc.Device("")
    inner = rtc.Scene(dev, flags)
    inner.add_triangles(tv, tt)
    inner.commit()

    def scene(parts):
        sc = rtc.Scene(dev, flags)
        if "c" in parts:
            sc.add_curves_mb(mv["steps"], mv["idx"], geom_id=0)
        if "i" in parts:
            sc.add_instance(inner, geom_id=1)
        sc.commit()
        return sc

    m = 20000
    rays = po.make_random_rays(m, np.zeros(3, F), np.ones(3, F), seed=5)
    rays["time"] = (np.random.RandomState(6).randint(0, 9, m) / 8.0).astype(F)
    got, want = rtc.aligned_rayhits(m), rtc.aligned_rayhits(m)
    got[:] = rays
    want[:] = rays
    sc = scene("ci")
    assert sc.stats()["accelKind"] == KIND[(flags, "swept")]
    sc.intersect1M(got)
    sc.release()
    for p in "ci":
        s1 = scene(p)
        s1.intersect1M(want)
        s1.release()
    assert got.tobytes() == want.tobytes()
    on_curves = int(((got["geomID"] == 0) & (got["instID"] == INVALID)).sum())
    on_inst = int((got["instID"] == 1).sum())
    print(f"  {on_curves} hits on the scene's own moving curves, {on_inst} below the instance")
    assert on_curves > 300 and on_inst > 1000
    inner.release()
    dev.release()


# ---- 9. filters ----------------------------------------------------------------------------------------------------------------------
def _ray_fields(args):
    ray = C.cast(args.contents.ray, C.POINTER(C.c_float * 12)).contents
    hit = C.cast(args.contents.hit, C.POINTER(C.c_uint * 8)).contents
    hitf = C.cast(args.contents.hit, C.POINTER(C.c_float * 8)).contents
    return ray, hit, hitf


@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("flags", MODES)
def test_filters_reject_every_second_curve_and_the_next_candidate_is_found(rtc, flags, bounds):
    """An intersect filter, an occluded filter and a context filter that reject the odd primIDs: the records are those of the moving scene
    built without those curves, primIDs mapped back.  The callbacks get the geometry's user data and the candidate."""
    mv = mh.hair_mb_truth(5, 4)
    steps, idx = mv["steps"], mv["idx"]
    rh = _rays(rtc, mv["org"], mv["dirs"], mv["times"])
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

    dev0, ref = _scene(rtc, flags, lambda s: s.add_curves_mb(steps, idx[0::2], tessellation_rate=6, geom_id=7), BOUNDS[bounds])
    want, wocc = _trace(rtc, ref, rh)
    wh = want["geomID"] != INVALID
    want["primID"][wh] *= 2  # back to the primIDs of the full geometry
    assert int(wh.sum()) > 300

    def full(s):
        assert s.add_curves_mb(steps, idx, tessellation_rate=6, geom_id=7) == 7
        s.set_user_data(7, USER)

    dev, sc = _scene(rtc, flags, full, BOUNDS[bounds])
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
    dev, sc = _scene(rtc, flags, full, BOUNDS[bounds])
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
    """A moving curve bent into a U, seen from the side: the ray crosses two ribbon quads of ONE curve (one record: its time segment).  A
    filter that rejects the first candidate it is shown per ray must be shown the second quad of the same curve next: the rejected
    candidate is (geomID, primID, t), not the curve."""
    u0 = np.array([[-1, 0, 0, .125], [-1, 0, 2, .125], [1, 0, 2, .125], [1, 0, 0, .125]], F)
    u1 = u0 + np.array([0, 0, .5, 0], F)
    org = np.array([[-4, 0, .5], [4, .03125, .75]], F)
    dirs = np.array([[1, 0, 0], [-1, 0, 0]], F)
    rh = _rays(rtc, org, dirs, np.array([0.25, 0.5], F))
    dev, sc = _scene(rtc, flags, lambda s: s.add_curves_mb([u0, u1], np.array([0], np.uint32), tessellation_rate=16, geom_id=0))
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


# ---- 10. entry paths -----------------------------------------------------------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("flags", MODES)
def test_entry_paths_are_bit_identical(rtc, po, flags):
    import torch

    mv = mh.hair_mb_truth(5, 4)

    def scene(extra=""):
        return _scene(rtc, flags, lambda s: s.add_curves_mb(mv["steps"], mv["idx"]), extra)

    m = 40000
    lo = np.min([s[:, :3].min(0) for s in mv["steps"]], 0)
    hi = np.max([s[:, :3].max(0) for s in mv["steps"]], 0)
    rays = po.make_random_rays(m, lo, hi, seed=21)
    rays["time"] = np.random.RandomState(8).rand(m).astype(F)
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
    # instrumented twins
    c = rtc.aligned_rayhits(m)
    c[:] = rays
    cnt = sc.intersect1M_counted(c)
    assert c.tobytes() == want.tobytes()
    assert cnt["rays"] == m and cnt["hits"] == nh and cnt["primTests"] > 0
    occ = ch.occ_of(rtc, rays)
    sc.occluded1M(occ)
    co = ch.occ_of(rtc, rays)
    ocnt = sc.occluded1M_counted(co)
    assert co.tobytes() == occ.tobytes() and np.array_equal(occ["tfar"] == -np.inf, want["geomID"] != INVALID)
    assert ocnt["rays"] == m and ocnt["hits"] == nh and ocnt["primTests"] > 0
    # multi-threaded rtcIntersect1 (call combiner)
    k = 2048
    g = rtc.aligned_rayhits(k)
    g[:] = rays[:k]
    errors = []

    def worker(i0):
        try:
            for i in range(i0, k, 16):
                sc.intersect1(g[i:i + 1])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(16)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[0]
    assert g.tobytes() == want[:k].tobytes()
    # SOA packets carry a time per lane; streams of packets; the SOA pointer stream
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
            assert np.array_equal(pko[8], occ["tfar"][p:p + W].view(np.uint32))
    N, M = 8, 16
    buf = np.zeros((M, 20 * N), np.uint32)
    for j in range(M):
        buf[j] = _soa(rays[1024 + j * N: 1024 + (j + 1) * N], N, True).ravel()
    L.rtcIntersectNM.restype = None
    L.rtcIntersectNM.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_size_t]
    L.rtcIntersectNM(sc.handle, C.addressof(ctx), buf.ctypes.data, N, M, 20 * N * 4)
    dev.check("rtcIntersectNM")
    for j in range(M):
        assert np.array_equal(buf[j].reshape(20, N), _soa(want[1024 + j * N: 1024 + (j + 1) * N], N, True))
    kk = 300
    cols = {f: np.ascontiguousarray(rays[f][1500:1500 + kk]) for f in RAYF + HITF[:-1]}
    inst = np.full(kk, INVALID, np.uint32)

    class Np(C.Structure):
        _fields_ = [(f, C.c_void_p) for f in RAYF + HITF]

    a = Np(*[cols[f].ctypes.data for f in RAYF + HITF[:-1]], inst.ctypes.data)
    L.rtcIntersectNp.restype = None
    L.rtcIntersectNp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
    L.rtcIntersectNp(sc.handle, C.addressof(ctx), C.addressof(a), kk)
    dev.check("rtcIntersectNp")
    w = want[1500:1500 + kk]
    for f in ("tfar", "geomID", "primID", "u", "v", "Ng_x", "Ng_y", "Ng_z"):
        assert np.array_equal(cols[f].view(np.uint32), w[f].view(np.uint32)), f
    sc.release()
    dev.release()
    # service=1: the motion-blur curve accel has no service kernel, the calls fall back to the combiner and agree
    dev, sc = scene("service=1")
    sv = rtc.aligned_rayhits(k)
    sv[:] = rays[:k]
    for i in range(0, k, 32):
        sc.intersect1M(sv[i:i + 32])
    assert sv.tobytes() == want[:k].tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    sc.release()
    dev.release()


# ---- 11. the overflow area of the traversal stack ------------------------------------------------------------------------------------
MIN_SPILLS = 0.05 * ds.GPU_RAYS  # as tests/test_gpu_deep_stack.py: every ray above slot 16 pushes at least one entry to HBM


@pytest.mark.parametrize("flags", MODES)
def test_forms_agree_beyond_the_lds_stack(rtc, monkeypatch, flags):
    """The needle soup of tests/deep_stack_helpers.py as straight moving curves of radius 0.01 (a move by 1/64 along x over two steps):
    node boxes overlap everywhere and rays carry their stacks into the HBM overflow area, which the counted twin's stackSpills must show."""
    tv, _ = ds.sliver_soup(ds.N_SLIVERS, ds.SOUP_SEED)
    ends = tv.reshape(-1, 3, 3)[:, :2].astype(np.float64)  # v0, v1 of every needle
    p = np.stack([ends[:, 0] + (ends[:, 1] - ends[:, 0]) * k / 3.0 for k in range(4)], 1).reshape(-1, 3)
    s0 = np.concatenate([p, np.full((len(p), 1), 0.01)], 1).astype(F)
    s1 = s0.copy()
    s1[:, 0] += F(1 / 64)
    idx = np.arange(0, len(s0), 4, dtype=np.uint32)
    lo, hi = ds.bounds(p.astype(F))
    from helpers import random_rays_np
    org, dirs = random_rays_np(ds.GPU_RAYS, lo, hi, ds.GPU_RAY_SEED)
    rh = ds.rays_of(rtc, org, dirs)
    rh["time"] = ((np.arange(len(rh)) % 5) / 4.0).astype(F)
    first = None
    for bname, bcfg in BOUNDS.items():
        for name, knobs in FORMS.items():
            _knobs(monkeypatch, knobs)
            dev, sc = _scene(rtc, flags, lambda s: s.add_curves_mb([s0, s1], idx, tessellation_rate=2), bcfg)
            assert sc.stats()["maxDepth"] >= 3
            got, occ = _trace(rtc, sc, rh)
            c = ds.copy_of(rtc, rh)
            cnt = sc.intersect1M_counted(c)
            assert c.tobytes() == got.tobytes(), f"{bname}, {name}: the instrumented twin differs from the plain kernel"
            print(f"  moving needle curves, {bname}, {name}: stackSpills {cnt['stackSpills']} ({len(rh)} rays), {int((got['geomID'] != INVALID).sum())} hits")
            assert cnt["stackSpills"] >= MIN_SPILLS, (bname, name, cnt["stackSpills"])
            if first is None:
                assert int((got["geomID"] != INVALID).sum()) > ds.GPU_RAYS // 2
                first = (f"{bname}, {name}", got.tobytes(), occ.tobytes())
            else:
                assert got.tobytes() == first[1], f"closest hit, {bname}, {name} differs from {first[0]}"
                assert occ.tobytes() == first[2], f"any hit, {bname}, {name} differs from {first[0]}"
            assert dev.error() == 0  # the `overflow` word stayed clear: no entry was dropped
            sc.release()
            dev.release()


# ---- 12. the C example ---------------------------------------------------------------------------------------------------------------
def test_curve_motion_blur_example_runs(tmp_path):
    exe = str(tmp_path / "curve_motion_blur_min")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "curve_motion_blur_min.c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "curve_motion_blur_min: ok" in out.stdout
