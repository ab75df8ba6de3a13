"""Motion blur on line segments (flat linear curves with time steps) on the GPU: the leaf of csrc/trace_line_mb.hip in its lane-per-ray
and octet forms, under robust and fast traversal, under swept node boxes (kinds 38 / 39) and time-dependent ones (mb_bounds=linear,
kinds 40 / 41).

The pinned inputs are exact in float32 at every ray time (tests/line_mb_helpers.py), so the moving scene is held to the STATIC line
kernel on the geometry at the ray's time bit for bit, and to the float64 truth of tests/line_helpers.py under the project's 1e-4 contract."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import deep_stack_helpers as ds
import line_helpers as lh
import line_mb_helpers as mh
from helpers import INVALID
from line_helpers import ROBUST
from line_mb_helpers import LINEMB_DT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")
KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL")
FORMS = {"lane form": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "0", "RTAMD_OCT_LEAF": "0"},    # every node and leaf step one ray per lane
         "octet form": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "32", "RTAMD_OCT_LEAF": "1"}}  # 8 lanes per ray wherever the kernel allows it
BOUNDS = {"swept": "", "linear": "mb_bounds=linear"}
MODES = [pytest.param(ROBUST, id="robust"), pytest.param(0, id="fast")]
KIND = {(ROBUST, "swept"): 38, (0, "swept"): 39, (ROBUST, "linear"): 40, (0, "linear"): 41}
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
    occ = lh.occ_of(rtc, rh)
    sc.occluded1M(occ, ctx=ctx)
    return out, occ


def _rays(rtc, org, dirs, times, tnear=0.0, tfar=np.inf):
    rh = lh.rays_of(rtc, org, dirs, tnear, tfar)
    rh["time"] = times
    return rh


# ---- the pinned moving tuft -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moving():
    """nsteps -> the pinned moving tuft, its rays with round-robin times, and the float64 truth, computed once"""
    out = {}
    for n in (2, 5):
        steps, idx, org, dirs = mh.tuft_steps(n)
        times = mh.round_robin_times(len(org), n)
        out[n] = {"steps": steps, "idx": idx, "org": org, "dirs": dirs, "times": times, "f64": mh.moving_truth(steps, idx, org, dirs, times, np.float64)}
        assert int(out[n]["f64"]["hit"].sum()) == mh.TUFT_MB_HITS[n]
    return out


_STATIC = {}


def _static_reference(rtc, flags, nsteps, mv, rh):
    """every ray against a static add_lines scene of the geometry at its time, traced by the static line kernel (default knobs)"""
    if (flags, nsteps) not in _STATIC:
        want, wocc = rh.copy(), lh.occ_of(rtc, rh)
        for t in np.unique(mv["times"]):
            sel = np.nonzero(mv["times"] == t)[0]
            dev, sc = _scene(rtc, flags, lambda s: s.add_lines(mh.at_time(mv["steps"], t), mv["idx"], geom_id=7))
            g, o = _trace(rtc, sc, rh[sel])
            want[sel], wocc[sel] = g, o
            sc.release()
            dev.release()
        _STATIC[(flags, nsteps)] = (want, wocc)
    return _STATIC[(flags, nsteps)]


# ---- 1. bit-identity with the static line kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsteps", [2, 5])
@pytest.mark.parametrize("flags", MODES)
def test_moving_scene_is_bit_identical_to_the_static_kernel_at_the_rays_time(rtc, monkeypatch, moving, flags, nsteps):
    """geomID, primID and the bits of t, u and Ng of every ray, in the lane and octet forms, under swept and linear bounds.  A ray may be
    left out only where the truth's two nearest candidates are within 1e-4 in t (the two scenes have different trees), at most 0.5 %."""
    mv = moving[nsteps]
    _knobs(monkeypatch, {})
    rh = _rays(rtc, mv["org"], mv["dirs"], mv["times"])
    want, wocc = _static_reference(rtc, flags, nsteps, mv, rh)
    out = mv["f64"]["near_tie"]
    assert out.sum() <= 0.005 * len(rh)
    k = ~out
    assert int((want["geomID"] != INVALID).sum()) > 2000
    for bname, bcfg in BOUNDS.items():
        for fname, knobs in FORMS.items():
            _knobs(monkeypatch, knobs)
            dev, sc = _scene(rtc, flags, lambda s: s.add_lines_mb(mv["steps"], mv["idx"], geom_id=7), bcfg)
            assert sc.stats()["accelKind"] == KIND[(flags, bname)] and sc.stats()["primCount"] == (nsteps - 1) * len(mv["idx"])
            got, occ = _trace(rtc, sc, rh)
            what = f"{nsteps} steps, {bname}, {fname}"
            for f in ("geomID", "primID", "tfar", "u", "v", "Ng_x", "Ng_y", "Ng_z", "instID"):
                assert np.array_equal(got[f][k].view(np.uint32), want[f][k].view(np.uint32)), (what, f, int((got[f][k].view(np.uint32) != want[f][k].view(np.uint32)).sum()))
            assert got[k].tobytes() == want[k].tobytes(), what
            assert np.array_equal(occ["tfar"][k] == -np.inf, got["geomID"][k] != INVALID) and occ[k].tobytes() == wocc[k].tobytes(), what
            assert dev.error() == 0
            sc.release()
            dev.release()


# ---- 2. the float64 truth ----------------------------------------------------------------------------------------------------------------
def _check_parity(got, occ, rh, truth, geom_id, what, cap=0.005):
    """hit / miss, geomID / primID exact, t within 1e-4 relative, u within 1e-4 absolute, v = 0; a ray is left out only where the float64
    truth has a segment within 1e-4 of `d2 <= r2` or its two nearest candidates within 1e-4 in t, at most the share `cap` of the rays"""
    out = truth["near_edge"] | truth["near_tie"]
    assert out.sum() <= cap * len(got), (what, int(out.sum()))
    k = ~out
    hit = truth["hit"]
    gh = got["geomID"] != INVALID
    seg = truth["seg"]
    dt = np.abs(got["tfar"][hit & k].astype(np.float64) - truth["t"][hit & k]) / np.abs(truth["t"][hit & k])
    du = np.abs(got["u"][hit & k].astype(np.float64) - truth["u"][hit & k])
    print(f"  {what}: {int(hit.sum())} hits of {len(got)}, {int(out.sum())} rays left out, hit/miss differs on {int((gh != hit)[k].sum())}, IDs on "
          f"{int((got['primID'] != seg)[hit & k & gh].sum())}, t to {dt.max():.3g} relative, u to {du.max():.3g}")
    assert np.array_equal(gh[k], hit[k]), what
    h = hit & k
    assert (got["geomID"][h] == geom_id).all() and np.array_equal(got["primID"][h], seg[h].astype(np.uint32)) and (got["instID"][h] == INVALID).all(), what
    assert (dt <= 1e-4).all() and (du <= 1e-4).all() and (got["v"][h] == 0).all(), (what, dt.max(), du.max())
    miss = ~hit & k
    assert got[miss].tobytes() == rh[miss].tobytes(), what  # a miss comes back untouched
    assert np.array_equal(occ["tfar"][k] == -np.inf, hit[k]) and np.array_equal(occ["tfar"][miss], rh["tfar"][miss]), what


@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("nsteps", [2, 5])
@pytest.mark.parametrize("flags", MODES)
def test_moving_tuft_meets_the_float64_truth(rtc, monkeypatch, moving, flags, nsteps, bounds):
    _knobs(monkeypatch, {})
    mv = moving[nsteps]
    rh = _rays(rtc, mv["org"], mv["dirs"], mv["times"])
    dev, sc = _scene(rtc, flags, lambda s: s.add_lines_mb(mv["steps"], mv["idx"], geom_id=7), BOUNDS[bounds])
    got, occ = _trace(rtc, sc, rh)
    _check_parity(got, occ, rh, mv["f64"], 7, f"moving tuft, {nsteps} steps, {bounds}")
    assert dev.error() == 0
    sc.release()
    dev.release()


# ---- 3. closed forms, exact --------------------------------------------------------------------------------------------------------------
# segment 0 along x, radius 1/4 at step 0 and 1/2 at step 1, moved by 8 along x: at time t its centre is (8 t, 0, 0), its radius (1 + t) / 4
# segment 1 (100 up in y) turns end over end: at time 1/2 both ends are at (0, 100, 0) - a zero-length segment
CLOSED = [np.array([[-1, 0, 0, .25], [1, 0, 0, .25], [-1, 100, 0, .25], [1, 100, 0, .25]], F),
          np.array([[7, 0, 0, .5], [9, 0, 0, .5], [1, 100, 0, .25], [-1, 100, 0, .25]], F)]
# (org, dir, time) -> None (miss) or (primID, t, u, Ng_x)
CLOSED_RAYS = [(((0, 0, -4), (0, 0, 1), 0.0), (0, 4, .5, 2)),                      # where the segment is at time 0 ...
               (((2, 0, -4), (0, 0, 1), 0.25), (0, 4, .5, 2)),                    # ... 1/4
               (((4, 0, -4), (0, 0, 2), 0.5), (0, 2, .5, 2)),                     # ... 1/2; t is the depth of the axis point
               (((8, 0, -4), (0, 0, 1), 1.0), (0, 4, .5, 2)),                     # ... 1
               (((8, 0, -4), (0, 0, 1), 0.0), None),                              # and nowhere else: where it is at time 1, at time 0
               (((0, 0, -4), (0, 0, 1), 1.0), None),
               (((0, 0, -4), (0, 0, 1), 0.5), None),
               (((4, 0, -4), (0, 0, 1), 0.25), None),
               (((2.5, 0, -4), (0, 0, 1), 0.25), (0, 4, .75, 2)),                 # u along the interpolated axis: x from 1 to 3
               (((4, .375, -4), (0, 0, 1), 0.5), (0, 4, .5, 2)),                  # grazing at the interpolated radius 3/8: d2 <= r2
               (((4, NEXT(F(.375), F(0)), -4), (0, 0, 1), 0.5), (0, 4, .5, 2)),   # ... from inside
               (((4, NEXT(F(.375), F(1)), -4), (0, 0, 1), 0.5), None),            # ... from outside
               (((2, .3125, -4), (0, 0, 1), 0.25), (0, 4, .5, 2)),                # radius 5/16 at time 1/4
               (((2, NEXT(F(.3125), F(1)), -4), (0, 0, 1), 0.25), None),
               (((0, .25, -4), (0, 0, 1), 0.0), (0, 4, .5, 2)),                   # radius 1/4 at time 0, 1/2 at time 1
               (((0, NEXT(F(.25), F(1)), -4), (0, 0, 1), 0.0), None),
               (((8, .5, -4), (0, 0, 1), 1.0), (0, 4, .5, 2)),
               (((8, NEXT(F(.5), F(1)), -4), (0, 0, 1), 1.0), None),
               (((0, 100, -4), (0, 0, 1), 0.0), (1, 4, .5, 2)),                   # segment 1 at time 0 ...
               (((0, 100, -4), (0, 0, 1), 1.0), (1, 4, .5, -2)),                  # ... at time 1, turned round
               (((0, 100, -4), (0, 0, 1), 0.25), (1, 4, .5, 1)),                  # ... at time 1/4: from -1/2 to 1/2
               (((0, 100, -4), (0, 0, 1), 0.5), None)]                            # ... a zero-length segment at time 1/2 is not hit


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("flags", MODES)
def test_closed_forms_are_exact(rtc, monkeypatch, flags, bounds, form):
    _knobs(monkeypatch, FORMS[form])
    dev, sc = _scene(rtc, flags, lambda s: s.add_lines_mb(CLOSED, np.array([0, 2], np.uint32), geom_id=5), BOUNDS[bounds])
    assert sc.stats()["accelKind"] == KIND[(flags, bounds)] and sc.stats()["primCount"] == 2
    rh = _rays(rtc, [r[0][0] for r in CLOSED_RAYS], [r[0][1] for r in CLOSED_RAYS], np.array([r[0][2] for r in CLOSED_RAYS], F))
    rh["u"], rh["v"], rh["Ng_x"] = 7, 7, 7  # a miss leaves the hit part as it was
    got, occ = _trace(rtc, sc, rh)
    for i, (_, want) in enumerate(CLOSED_RAYS):
        g = got[i]
        if want is None:
            assert g.tobytes() == rh[i].tobytes(), (i, g)
            assert occ[i].tobytes() == lh.occ_of(rtc, rh[i:i + 1])[0].tobytes(), i
            continue
        prim, t, u, ngx = want
        assert g["geomID"] == 5 and g["primID"] == prim and g["instID"] == INVALID, (i, g)
        assert g["tfar"] == F(t) and g["u"] == F(u) and g["v"] == 0, (i, g)
        assert (g["Ng_x"], g["Ng_y"], g["Ng_z"]) == (ngx, 0, 0), (i, g)  # v1 - v0 at the ray's time, not normalised
        assert occ[i]["tfar"] == -np.inf, i
    assert dev.error() == 0
    sc.release()
    dev.release()


# ---- 4. block rule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [8, 5])
@pytest.mark.parametrize("flags", MODES)
def test_coincident_moving_segments_follow_the_block_rule_in_both_forms(rtc, monkeypatch, flags, copies):
    """`copies` coincident moving segments with primIDs of their own: one leaf, two blocks (the second partial for 5).  Inside a block the
    lowest lane wins the equal t, the later block wins it with `t <= tfar`: the record at place 4 of the leaf, on the interpolated records."""
    s0 = np.tile(np.array([[-1, 0, 0, .25], [1, 0, 0, .125]], F), (copies, 1))
    s1 = np.tile(np.array([[-.5, .25, 0, .5], [1.5, .25, 0, .25]], F), (copies, 1))
    org = np.array([[0, 0, -4], [.5, .125, -3], [-.75, 0, 5]], F)
    dirs = np.array([[0, 0, 1], [-.125, 0, 1], [.25, .03125, -2]], F)
    times = np.array([0.25, 0.5, 0.75], F)
    results = {}
    for bname, bcfg in BOUNDS.items():
        for name, knobs in FORMS.items():
            _knobs(monkeypatch, knobs)
            dev, sc = _scene(rtc, flags, lambda s: s.add_lines_mb([s0, s1], np.arange(0, 2 * copies, 2, dtype=np.uint32)), bcfg)
            assert sc.accel_root() == (0x80000000 | (copies << 26))  # one leaf
            rec = sc.accel_data(2).view(LINEMB_DT)
            got, occ = _trace(rtc, sc, _rays(rtc, org, dirs, times))
            for i in range(len(org)):
                prim, t = mh.leaf_rule_mb(rec, org[i], dirs[i], times[i])
                assert prim == rec["primID"][4] and got["primID"][i] == prim and abs(got["tfar"][i] - t) <= 1e-5 * t, (bname, name, i, got[i], prim, t)
            assert (occ["tfar"] == -np.inf).all()
            results[(bname, name)] = got.tobytes()
            sc.release()
            dev.release()
    assert len(set(results.values())) == 1


@pytest.mark.parametrize("flags", MODES)
def test_only_the_records_of_the_rays_time_segment_take_part(rtc, monkeypatch, flags):
    """Three time steps, five coincident segments that move by 4 along y and back: every (segment, time segment) pair has the same swept and
    the same mid-segment box, so the builder cannot part them - ONE leaf of ten records that mixes both time segments.  A record of the
    other segment keeps its place in its block and takes no part: the winner is what the block rule names on the records that accept the
    ray's time, and where only the other segment's records would put the geometry nothing is hit."""
    copies = 5
    a = np.tile(np.array([[-1, 0, 0, .25], [1, 0, 0, .125]], F), (copies, 1))
    b = np.tile(np.array([[-1, 4, 0, .25], [1, 4, 0, .125]], F), (copies, 1))
    c = a
    # times 0, 1/8 (segment 0, f = 1/4: y = 1), 5/8 (segment 1, f = 1/4: y = 3), 1 (segment 1, f = 1), 1/2 (the joint: segment 1, f = 0)
    org = np.array([[0, 0, -4], [0, 1, -4], [0, 3, -4], [0, 0, -4], [0, 4, -4]], F)
    dirs = np.tile(np.array([[0, 0, 1]], F), (5, 1))
    times = np.array([0.0, 0.125, 0.625, 1.0, 0.5], F)
    results = {}
    for bname, bcfg in BOUNDS.items():
        for name, knobs in FORMS.items():
            _knobs(monkeypatch, knobs)
            dev, sc = _scene(rtc, flags, lambda s: s.add_lines_mb([a, b, c], np.arange(0, 2 * copies, 2, dtype=np.uint32)), bcfg)
            assert sc.accel_root() == (0x80000000 | (2 * copies << 26))
            rec = sc.accel_data(2).view(LINEMB_DT)
            assert sorted(rec["segment"].tolist()) == [0] * copies + [1] * copies
            got, _ = _trace(rtc, sc, _rays(rtc, org, dirs, times))
            for i in range(len(org)):
                prim, t = mh.leaf_rule_mb(rec, org[i], dirs[i], times[i])
                assert prim is not None and got["primID"][i] == prim and got["tfar"][i] == 4, (bname, name, i, got[i], prim, t)
            # at time 1/8 nothing is at y = 3 (where the second segment's records are at THEIR f = 1/4), at time 5/8 nothing at y = 1
            miss = _rays(rtc, org[[2, 1]], dirs[:2], times[[1, 2]])
            g2, _ = _trace(rtc, sc, miss)
            assert (g2["geomID"] == INVALID).all(), (bname, name)
            results[(bname, name)] = got.tobytes()
            sc.release()
            dev.release()
    assert len(set(results.values())) == 1


# ---- 5. a fast mover -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES)
def test_fast_mover_is_hit_only_where_it_is_and_linear_bounds_test_less(rtc, monkeypatch, flags):
    """The tuft moves by 16 x its extent along x between two steps.  Every second ray aims where the tuft is at the ray's time, the others
    where it is half a shutter away.  Hits are those of the truth at the ray's time; the counted twin under mb_bounds=linear tests
    strictly fewer primitives and visits strictly fewer leaves than under swept boxes, with byte-identical records."""
    _knobs(monkeypatch, {})
    v, idx, org, dirs = lh.tuft_and_rays()
    m = 2048
    s0 = np.concatenate([mh.snap(v[:, :3]), mh.snap(v[:, 3])[:, None]], 1).astype(F)
    s1 = s0.copy()
    s1[:, 0] += 16
    steps = [s0, s1]
    i = np.arange(m)
    times = ((i % 5) / 4.0).astype(F)
    aim = np.where(i % 2 == 0, times, (((i + 2) % 5) / 4.0)).astype(F)
    org = org[:m].copy()
    org[:, 0] += 16 * aim
    dirs = dirs[:m]
    truth = mh.moving_truth(steps, idx, org, dirs, times, np.float64)
    on, off = truth["hit"][i % 2 == 0], truth["hit"][i % 2 == 1]
    print(f"  truth: {int(on.sum())} of {len(on)} rays aimed at the tuft's place hit, {int(off.sum())} of {len(off)} aimed elsewhere")
    assert on.sum() > 600 and off.sum() < on.sum() // 8
    rh = _rays(rtc, org, dirs, times)
    res = {}
    for bname, bcfg in BOUNDS.items():
        dev, sc = _scene(rtc, flags, lambda s: s.add_lines_mb(steps, idx, geom_id=7), bcfg)
        got, occ = _trace(rtc, sc, rh)
        _check_parity(got, occ, rh, truth, 7, f"fast mover, {bname}")
        c = rh.copy()
        cnt = sc.intersect1M_counted(c)
        assert c.tobytes() == got.tobytes()
        res[bname] = (got.tobytes(), occ.tobytes(), cnt)
        sc.release()
        dev.release()
    sw, li = res["swept"][2], res["linear"][2]
    print(f"  primTests swept {sw['primTests']} linear {li['primTests']} ({sw['primTests'] / max(li['primTests'], 1):.2f} x), "
          f"leafVisits swept {sw['leafVisits']} linear {li['leafVisits']} ({sw['leafVisits'] / max(li['leafVisits'], 1):.2f} x), "
          f"nodeVisits swept {sw['nodeVisits']} linear {li['nodeVisits']}")
    assert res["swept"][:2] == res["linear"][:2]
    assert li["primTests"] < sw["primTests"] and li["leafVisits"] < sw["leafVisits"]


# ---- 6. times outside the shutter, and NaN ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("flags", MODES)
def test_times_outside_the_shutter_extrapolate_and_a_nan_time_misses(rtc, monkeypatch, moving, flags, bounds):
    _knobs(monkeypatch, {})
    mv = moving[2]
    m = 1024
    org, dirs = mv["org"][:m], mv["dirs"][:m]
    times = mv["times"][:m].copy()
    odd = np.arange(m) % 8
    times[odd == 1], times[odd == 3], times[odd == 5] = -0.25, 1.5, np.nan
    special = np.isin(odd, (1, 3, 5))
    rh = _rays(rtc, org, dirs, times)
    dev, sc = _scene(rtc, flags, lambda s: s.add_lines_mb(mv["steps"], mv["idx"], geom_id=7), BOUNDS[bounds])
    got, occ = _trace(rtc, sc, rh)
    # the NaN rays miss and come back untouched
    nan = np.isnan(times)
    assert got[nan].tobytes() == rh[nan].tobytes() and occ[nan].tobytes() == lh.occ_of(rtc, rh)[nan].tobytes()
    # an out-of-range ray reports nothing that is not a hit of the extrapolated first / last segment (the node boxes do not follow the
    # extrapolation, so it may miss what the extrapolated geometry would give)
    n_hits = 0
    for t in (-0.25, 1.5):
        sel = np.nonzero(times == F(t))[0]
        v0, v1 = lh.ends(mh.at_time(mv["steps"], t), mv["idx"])
        valid, T, U, _ = lh.candidates(v0, v1, org[sel], dirs[sel], np.zeros(len(sel), F), np.full(len(sel), np.inf, F), np.float32)
        for j, i in enumerate(sel):
            if got["geomID"][i] == INVALID:
                assert got[i].tobytes() == rh[i].tobytes() and occ["tfar"][i] == rh["tfar"][i]
                continue
            p = int(got["primID"][i])
            n_hits += 1
            assert got["geomID"][i] == 7 and valid[j, p] and abs(float(got["tfar"][i]) - float(T[j, p])) <= 1e-4 * abs(float(T[j, p])), (t, i, got[i])
            assert abs(float(got["u"][i]) - float(U[j, p])) <= 1e-4 and occ["tfar"][i] == -np.inf
    print(f"  {bounds}: {n_hits} hits of {int((special & ~nan).sum())} rays outside the shutter")
    assert n_hits > 20
    # every other record equals the batch traced without them
    rest = ~special
    g2, o2 = _trace(rtc, sc, rh[rest])
    assert got[rest].tobytes() == g2.tobytes() and occ[rest].tobytes() == o2.tobytes()
    assert dev.error() == 0
    sc.release()
    dev.release()


# ---- 7. mixed scene ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("flags", MODES)
def test_mixed_scene_equals_the_accels_traced_in_reference_order(rtc, po, bomberman_tris, moving, flags, bounds):
    """triangles, static lines, moving lines and a mesh instance in one top scene = the four accels traced alone one after the other in
    the reference's order (triangles, lines, motion-blur lines, instances): every ray keeps the nearest, a later accel wins a bit-equal t"""
    verts, tris = bomberman_tris
    lo, hi = verts.min(0), verts.max(0)
    ext = float(np.max(hi - lo))

    def place(v4, shift):  # the tuft over the mesh's bounds
        out = v4.copy()
        out[:, :3] = (lo + (out[:, :3] + shift) * (hi - lo)).astype(F)
        out[:, 3] *= ext / 8
        return out

    mv = moving[2]
    static = place(lh.tuft_and_rays()[0], np.array([0, .25, 0]))
    steps = [place(s, np.array([-.25 + .5 * k, 0, 0])) for k, s in enumerate(mv["steps"])]
    dev = rtc.Device(BOUNDS[bounds])
    inner = rtc.Scene(dev, flags)
    inner.add_triangles(verts, tris)
    inner.commit()
    up = np.array([0, float(hi[1] - lo[1]), 0], F)  # the instance: the mesh once more, on top of itself
    xfm = np.array([[1, 0, 0, up[0]], [0, 1, 0, up[1]], [0, 0, 1, up[2]]], F)

    def scene(parts):
        sc = rtc.Scene(dev, flags)
        if "t" in parts:
            sc.add_triangles(verts, tris, geom_id=0)
        if "l" in parts:
            sc.add_lines(static, mv["idx"], geom_id=1)
        if "m" in parts:
            sc.add_lines_mb(steps, mv["idx"], geom_id=2)
        if "i" in parts:
            sc.add_instance(inner, xfm, geom_id=3)
        sc.commit()
        return sc

    m = 50000
    rays = po.make_random_rays(m, lo, hi + up, seed=9)
    rays["time"] = (np.random.RandomState(4).randint(0, 17, m) / 16.0).astype(F)
    got, want = rtc.aligned_rayhits(m), rtc.aligned_rayhits(m)
    got[:] = rays
    want[:] = rays
    sc = scene("tlmi")
    sc.intersect1M(got)
    sc.release()
    for p in "tlmi":
        s1 = scene(p)
        s1.intersect1M(want)
        s1.release()
    assert got.tobytes() == want.tobytes()
    counts = [int(((got["geomID"] == g) & (got["instID"] == INVALID)).sum()) for g in range(3)] + [int((got["instID"] == 3).sum())]
    print(f"  hits (triangles, static lines, moving lines, below the instance): {counts}")
    assert min(counts) > 100, counts
    inner.release()
    dev.release()


# ---- 8. filters --------------------------------------------------------------------------------------------------------------------------
def _ray_fields(args):
    ray = C.cast(args.contents.ray, C.POINTER(C.c_float * 12)).contents
    hit = C.cast(args.contents.hit, C.POINTER(C.c_uint * 8)).contents
    hitf = C.cast(args.contents.hit, C.POINTER(C.c_float * 8)).contents
    return ray, hit, hitf


@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("flags", MODES)
def test_filters_see_the_candidates_and_reject_every_second_segment(rtc, moving, flags, bounds):
    """An intersect filter, an occluded filter and a context filter that reject the odd primIDs: the records are those of the moving scene
    built without those segments, primIDs mapped back.  The callbacks get the geometry's user data and the candidate."""
    mv = moving[5]
    steps, idx = mv["steps"], mv["idx"]
    n = 1024
    rh = _rays(rtc, mv["org"][:n], mv["dirs"][:n], mv["times"][:n])
    USER = 0x5EED0
    seen, bad = [], []

    @rtc.FILTER_FUNC
    def flt(args):
        ray, hit, hitf = _ray_fields(args)
        prim = hit[5]
        seen.append((ray[0], prim, ray[8], hitf[3]))
        if not (args.contents.geometryUserPtr == USER and args.contents.N == 1 and hit[6] == 7 and hitf[4] == 0.0 and 0.0 <= hitf[3] <= 1.0 and hit[7] == INVALID):
            bad.append((prim, hit[6], hitf[4]))
        if prim & 1:
            args.contents.valid[0] = 0

    dev0, ref = _scene(rtc, flags, lambda s: s.add_lines_mb(steps, idx[0::2], geom_id=7), BOUNDS[bounds])
    want, wocc = _trace(rtc, ref, rh)
    wh = want["geomID"] != INVALID
    want["primID"][wh] *= 2  # back to the primIDs of the full geometry
    assert int(wh.sum()) > n // 3

    def full(s):
        assert s.add_lines_mb(steps, idx, geom_id=7) == 7
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
    shown = {(s[0], s[1]): (s[2], s[3]) for s in seen}  # every closest hit was shown to the intersect filter with its t and u
    for r in got[wh][:200]:
        assert shown[(float(r["org_x"]), int(r["primID"]))] == (float(r["tfar"]), float(r["u"]))
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


# ---- 9. entry paths ----------------------------------------------------------------------------------------------------------------------
def _soa(aos, n, with_hit):
    fields = RAYF + (HITF if with_hit else [])
    out = np.zeros((len(fields), n), np.uint32)
    for k, f in enumerate(fields):
        out[k] = aos[f][:n].view(np.uint32)
    return out


@pytest.mark.parametrize("flags", MODES)
def test_entry_paths_are_bit_identical(rtc, po, moving, flags):
    import torch

    mv = moving[5]

    def scene(extra=""):
        return _scene(rtc, flags, lambda s: s.add_lines_mb(mv["steps"], mv["idx"]), extra)

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
    occ = lh.occ_of(rtc, rays)
    sc.occluded1M(occ)
    co = lh.occ_of(rtc, rays)
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
    # service=1: the motion-blur line accel has no service kernel, the calls fall back to the combiner and agree
    dev, sc = scene("service=1")
    sv = rtc.aligned_rayhits(k)
    sv[:] = rays[:k]
    for i in range(0, k, 32):
        sc.intersect1M(sv[i:i + 32])
    assert sv.tobytes() == want[:k].tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    sc.release()
    dev.release()


# ---- 10. the overflow area of the traversal stack ------------------------------------------------------------------------------------------
MIN_SPILLS = 0.05 * ds.GPU_RAYS  # as tests/test_gpu_deep_stack.py: every ray above slot 16 pushes at least one entry to HBM


@pytest.mark.parametrize("flags", MODES)
def test_forms_agree_beyond_the_lds_stack(rtc, monkeypatch, flags):
    """The needle soup of tests/deep_stack_helpers.py as moving segments of radius 0.01 (a move by 1/64 along x over two steps): node boxes
    overlap everywhere and rays carry their stacks into the HBM overflow area, which the counted twin's stackSpills must show."""
    tv, _ = ds.sliver_soup(ds.N_SLIVERS, ds.SOUP_SEED)
    p = tv.reshape(-1, 3, 3)[:, :2].reshape(-1, 3)  # v0, v1 of every needle
    s0 = np.concatenate([p, np.full((len(p), 1), 0.01, F)], 1).astype(F)
    s1 = s0.copy()
    s1[:, 0] += F(1 / 64)
    idx = np.arange(0, len(s0), 2, dtype=np.uint32)
    lo, hi = ds.bounds(p)
    from helpers import random_rays_np
    org, dirs = random_rays_np(ds.GPU_RAYS, lo, hi, ds.GPU_RAY_SEED)
    rh = ds.rays_of(rtc, org, dirs)
    rh["time"] = ((np.arange(len(rh)) % 5) / 4.0).astype(F)
    first = None
    for bname, bcfg in BOUNDS.items():
        for name, knobs in FORMS.items():
            _knobs(monkeypatch, knobs)
            dev, sc = _scene(rtc, flags, lambda s: s.add_lines_mb([s0, s1], idx), bcfg)
            assert sc.stats()["maxDepth"] >= 3
            got, occ = _trace(rtc, sc, rh)
            c = ds.copy_of(rtc, rh)
            cnt = sc.intersect1M_counted(c)
            assert c.tobytes() == got.tobytes(), f"{bname}, {name}: the instrumented twin differs from the plain kernel"
            print(f"  moving needle segments, {bname}, {name}: stackSpills {cnt['stackSpills']} ({len(rh)} rays), {int((got['geomID'] != INVALID).sum())} hits")
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


# ---- 11. the C example -------------------------------------------------------------------------------------------------------------------
def test_line_motion_blur_example_runs(tmp_path):
    exe = str(tmp_path / "line_motion_blur_min")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "line_motion_blur_min.c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "line_motion_blur_min: ok" in out.stdout
