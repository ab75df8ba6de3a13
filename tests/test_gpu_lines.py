"""Line segments (RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE) on the GPU: the line leaf of csrc/trace_line.hip in its lane-per-ray, octet and
ray-pool forms, under robust and fast traversal.

The oracle has no line intersector; the truth is the NumPy restatement of LineIntersector1::intersect in tests/line_helpers.py, all
segments against all rays in float64 (no BVH).  Exact (`==`) where the inputs are dyadic, the project's 1e-4 contract elsewhere."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import deep_stack_helpers as ds
import line_helpers as lh
from helpers import INVALID
from line_helpers import ACCEL_LINE_FAST, ACCEL_LINE_ROBUST, LINE_DT, ROBUST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "embree-compressed_amd", "lib")
KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL")
FORMS = {"lane form": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "0", "RTAMD_OCT_LEAF": "0"},    # every node and leaf step one ray per lane
         "octet form": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "32", "RTAMD_OCT_LEAF": "1"},  # 8 lanes per ray wherever the kernel allows it
         "ray-pool kernel": {"RTAMD_KERNEL": "pool"}}
MODES = [pytest.param(ROBUST, id="robust"), pytest.param(0, id="fast")]
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
    got = rh.copy()
    out = rtc.aligned_rayhits(len(rh))
    out[:] = got
    sc.intersect1M(out, ctx=ctx)
    occ = lh.occ_of(rtc, rh)
    sc.occluded1M(occ, ctx=ctx)
    return out, occ


# ---- 1. closed forms, exact ---------------------------------------------------------------------------------------------------------------
# five segments, 100 apart in y, primID = the variant
CLOSED = np.array([[-1, 0, 0, .25], [1, 0, 0, .25],        # 0: radius 1/4
                   [-1, 100, 0, .5], [1, 100, 0, 0],       # 1: radii 1/2 -> 0
                   [-1, 200, 0, .25], [1, 200, 0, 2.5],    # 2: end radius 5/2
                   [-1, 300, 0, .25], [1, 300, 0, 1.5],    # 3: end radius 3/2
                   [0, 400, 0, .25], [0, 400, 0, .25]], np.float32)  # 4: zero length
# (org, dir, tnear, tfar) -> None (miss) or (primID, t, u)
CLOSED_RAYS = [(((0, 0, -4), (0, 0, 1), 0, np.inf), (0, 4, .5)),                 # t is the depth of the axis point, not 3.75: flat
               (((0, 0, -4), (0, 0, 2), 0, np.inf), (0, 2, .5)),
               (((0, .25, -4), (0, 0, 1), 0, np.inf), (0, 4, .5)),               # d2 <= r2
               (((0, NEXT(F(.25), F(1)), -4), (0, 0, 1), 0, np.inf), None),
               (((0, 100.25, -4), (0, 0, 1), 0, np.inf), (1, 4, .5)),            # the cone's radius at u = 1/2 is 1/4
               (((0, NEXT(F(100.25), F(200)), -4), (0, 0, 1), 0, np.inf), None),
               (((3, 0, -4), (0, 0, 1), 0, np.inf), None),                       # u clamped to 1: two away from the end, radius 1/4
               (((3, 200, -8), (0, 0, 1), 0, np.inf), (2, 8, 1)),                # ... inside the end radius 5/2
               (((3, 300, -8), (0, 0, 1), 0, np.inf), None),                     # ... outside the end radius 3/2
               (((0, 0, -.25), (0, 0, 1), 0, np.inf), None),                     # self intersection: t = 1/4 is not > 0 + 2 * 1/4
               (((0, 0, -.5), (0, 0, 1), 0, np.inf), None),                      # ... nor is 1/2
               (((0, 0, -.75), (0, 0, 1), 0, np.inf), (0, .75, .5)),
               (((0, 0, -4), (0, 0, 1), 0, 4), (0, 4, .5)),                      # t <= tfar
               (((0, 0, -4), (0, 0, 1), 0, NEXT(F(4), F(0))), None),
               (((0, 0, -4), (0, 0, 1), 4, np.inf), None),                       # tnear < t
               (((0, 0, -4), (0, 0, 1), 3, np.inf), (0, 4, .5)),                 # t = 4 > 3 + 2 * 1/4
               (((0, 0, -4), (0, 0, 1), 3.5, np.inf), None),                     # ... but not > 3.5 + 1/2
               (((0, 400, -4), (0, 0, 1), 0, np.inf), None),                     # a zero-length segment is never hit
               (((0, 0, -4), (0, 0, 1), 5, 4), None),                            # invalid rays come back untouched: tnear > tfar
               (((np.nan, 0, -4), (0, 0, 1), 0, np.inf), None)]                  # ... NaN origin


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("flags", MODES)
def test_closed_forms_are_exact(rtc, monkeypatch, flags, form):
    _knobs(monkeypatch, FORMS[form])
    dev, sc = _scene(rtc, flags, lambda s: s.add_lines(CLOSED, np.arange(0, 10, 2, dtype=np.uint32), geom_id=5))
    assert sc.stats()["accelKind"] == (ACCEL_LINE_ROBUST if flags else ACCEL_LINE_FAST) and sc.stats()["primCount"] == 5
    n = len(CLOSED_RAYS)
    rh = lh.rays_of(rtc, [r[0][0] for r in CLOSED_RAYS], [r[0][1] for r in CLOSED_RAYS],
                    np.array([r[0][2] for r in CLOSED_RAYS], F), np.array([r[0][3] for r in CLOSED_RAYS], F))
    rh["u"], rh["v"], rh["Ng_x"] = 7, 7, 7  # a miss leaves the hit part as it was
    got, occ = _trace(rtc, sc, rh)
    for i, (_, want) in enumerate(CLOSED_RAYS):
        g = got[i]
        if want is None:
            assert g.tobytes() == rh[i].tobytes(), (i, g)
            assert occ[i].tobytes() == lh.occ_of(rtc, rh[i:i + 1])[0].tobytes(), i
            continue
        prim, t, u = want
        assert g["geomID"] == 5 and g["primID"] == prim and g["instID"] == INVALID, (i, g)
        assert g["tfar"] == F(t) and g["u"] == F(u) and g["v"] == 0, (i, g)
        assert (g["Ng_x"], g["Ng_y"], g["Ng_z"]) == (2, 0, 0), (i, g)  # v1 - v0, not normalised
        assert occ[i]["tfar"] == -np.inf, i
    assert n == 20 and dev.error() == 0
    sc.release()
    dev.release()


# ---- 2. block and tie rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [8, 5])
@pytest.mark.parametrize("flags", MODES)
def test_coincident_segments_follow_the_block_rule_in_every_form(rtc, monkeypatch, flags, copies):
    """`copies` coincident segments with primIDs of their own: one leaf, two blocks (the second partial for 5).  Inside a block the lowest
    lane wins the equal t, the later block wins it with `t <= tfar`: the record at place 4 of the leaf."""
    v = np.tile(np.array([[-1, 0, 0, .25], [1, 0, 0, .125]], np.float32), (copies, 1))
    org = np.array([[0, 0, -4], [.5, .125, -3], [-.75, 0, 5]], np.float32)
    dirs = np.array([[0, 0, 1], [-.125, 0, 1], [.25, .03125, -2]], np.float32)
    results = {}
    for name, knobs in FORMS.items():
        _knobs(monkeypatch, knobs)
        dev, sc = _scene(rtc, flags, lambda s: s.add_lines(v, np.arange(0, 2 * copies, 2, dtype=np.uint32)))
        assert sc.accel_root() == (0x80000000 | (copies << 26))  # one leaf
        rec = sc.accel_data(2).view(LINE_DT)
        got, occ = _trace(rtc, sc, lh.rays_of(rtc, org, dirs))
        for i in range(len(org)):
            prim, t = lh.leaf_rule(rec, org[i], dirs[i], 0.0, np.inf)
            assert prim == rec["primID"][4] and got["primID"][i] == prim and abs(got["tfar"][i] - t) <= 1e-5 * t, (name, i, got[i], prim, t)
        assert (occ["tfar"] == -np.inf).all()
        results[name] = got.tobytes()
        sc.release()
        dev.release()
    assert len(set(results.values())) == 1


# ---- 3. parity on the pinned random tuft ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tuft():
    """the pinned input with its float64 truth and the float32 restatement, computed once"""
    v, idx, org, dirs = lh.tuft_and_rays()
    v0, v1 = lh.ends(v, idx)
    m = len(org)
    tn, tf = np.zeros(m, F), np.full(m, np.inf, F)
    return {"v": v, "idx": idx, "org": org, "dirs": dirs, "f64": lh.closest(v0, v1, org, dirs, tn, tf, np.float64),
            "f32": lh.closest(v0, v1, org, dirs, tn, tf, np.float32)}


def _check_parity(got, occ, rh, truth, geom_id, what, cap=0.005):
    """hit / miss, geomID / primID exact, t within 1e-4 relative, u within 1e-4 absolute, v = 0, Ng bit-equal to v1 - v0 in float32; a ray
    is left out only where the float64 truth has a segment within 1e-4 of `d2 <= r2` or its two nearest candidates within 1e-4 in t, and at
    most the share `cap` of the rays may be (0.5 % on the tuft)"""
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
    ng = np.stack([got["Ng_x"], got["Ng_y"], got["Ng_z"]], 1)
    assert ng[h].tobytes() == truth["Ng"][h].astype(F).tobytes(), what
    miss = ~hit & k
    assert got[miss].tobytes() == rh[miss].tobytes(), what  # a miss comes back untouched
    assert np.array_equal(occ["tfar"][k] == -np.inf, hit[k]) and np.array_equal(occ["tfar"][miss], rh["tfar"][miss]), what


@pytest.mark.parametrize("flags", MODES)
def test_random_tuft_meets_the_float64_truth(rtc, monkeypatch, tuft, flags):
    a, b = tuft["f64"], tuft["f32"]
    # the reference arithmetic itself, in float32 on the CPU, needs no ray left out (tests/test_host_lines.py has the figures)
    h = a["hit"]
    assert int(h.sum()) == lh.TUFT_HITS and np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["seg"][h], b["seg"][h])
    assert not (a["near_edge"] | a["near_tie"]).any()
    assert (np.abs(a["t"][h] - b["t"][h]) <= 1e-4 * np.abs(a["t"][h])).all() and (np.abs(a["u"][h] - b["u"][h]) <= 1e-4).all()
    rh = lh.rays_of(rtc, tuft["org"], tuft["dirs"])
    first = None
    for name, knobs in FORMS.items():
        _knobs(monkeypatch, knobs)
        dev, sc = _scene(rtc, flags, lambda s: s.add_lines(tuft["v"], tuft["idx"], geom_id=7))
        got, occ = _trace(rtc, sc, rh)
        if first is None:
            _check_parity(got, occ, rh, a, 7, f"tuft, {name}")
            first = (got.tobytes(), occ.tobytes())
        else:
            assert (got.tobytes(), occ.tobytes()) == first, name
        assert dev.error() == 0
        sc.release()
        dev.release()


# ---- 4. mixed scene --------------------------------------------------------------------------------------------------------------------------------
def _random_quads(n, seed, lo, hi):
    rng = np.random.RandomState(seed)
    c = (lo + rng.rand(n, 1, 3) * (hi - lo)).astype(F)
    size = 0.1 * float(np.max(hi - lo))
    v = (c + (rng.rand(n, 4, 3).astype(F) - 0.5) * size).astype(F).reshape(-1, 3)
    return v, np.arange(4 * n, dtype=np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("flags", MODES)
def test_mixed_scene_equals_the_accels_traced_in_reference_order(rtc, po, bomberman_tris, tuft, flags):
    """triangles, quads and lines in one scene = the three accels traced alone one after the other in the reference's order (triangles,
    quads, lines; scene.cpp:650-663): every ray keeps the nearest, and a later accel wins a bit-equal t"""
    verts, tris = bomberman_tris
    lo, hi = verts.min(0), verts.max(0)
    ext = float(np.max(hi - lo))
    lv = tuft["v"].copy()  # the tuft over the mesh's bounds, radii at an eighth of the largest extent's share
    lv[:, :3] = (lo + lv[:, :3] * (hi - lo)).astype(F)
    lv[:, 3] *= ext / 8
    qv, qq = _random_quads(64, 6, lo, hi)

    def scene(parts):
        def add(s):
            if "t" in parts:
                s.add_triangles(verts, tris, geom_id=0)
            if "q" in parts:
                s.add_quads(qv, qq, geom_id=1)
            if "l" in parts:
                s.add_lines(lv, tuft["idx"], geom_id=2)
        return _scene(rtc, flags, add)

    m = 100000
    rays = po.make_random_rays(m, lo, hi, seed=9)
    dev, sc = scene("tql")
    got = rtc.aligned_rayhits(m)
    got[:] = rays
    sc.intersect1M(got)
    want = rtc.aligned_rayhits(m)
    want[:] = rays
    for p in "tql":
        d1, s1 = scene(p)
        s1.intersect1M(want)
        s1.release()
        d1.release()
    assert got.tobytes() == want.tobytes()
    counts = [int((got["geomID"] == g).sum()) for g in range(3)]
    print(f"  hits per geometry (triangles, quads, lines): {counts}")
    assert min(counts) > 100, counts
    sc.release()
    dev.release()


@pytest.mark.parametrize("flags", MODES)
def test_lines_beside_instances_in_a_top_scene(rtc, po, tuft, flags):
    """a top scene with lines of its own beside an instance = the line accel, then the instance accel (the reference's order)"""
    tv = np.array([[.1, .1, .5], [.9, .1, .5], [.5, .9, .45], [.2, .8, .2], [.8, .3, .7]], F)
    tt = np.array([[0, 1, 2], [0, 3, 4], [1, 3, 4]], np.uint32)
    dev = rtc.Device("")
    inner = rtc.Scene(dev, flags)
    inner.add_triangles(tv, tt)
    inner.commit()

    def scene(parts):
        sc = rtc.Scene(dev, flags)
        if "l" in parts:
            sc.add_lines(tuft["v"], tuft["idx"], geom_id=0)
        if "i" in parts:
            sc.add_instance(inner, geom_id=1)
        sc.commit()
        return sc

    m = 20000
    rays = po.make_random_rays(m, np.zeros(3, F), np.ones(3, F), seed=5)
    got, want = rtc.aligned_rayhits(m), rtc.aligned_rayhits(m)
    got[:] = rays
    want[:] = rays
    sc = scene("li")
    assert sc.stats()["accelKind"] == (ACCEL_LINE_ROBUST if flags else ACCEL_LINE_FAST)
    sc.intersect1M(got)
    sc.release()
    for p in "li":
        s1 = scene(p)
        s1.intersect1M(want)
        s1.release()
    assert got.tobytes() == want.tobytes()
    on_lines = int(((got["geomID"] == 0) & (got["instID"] == INVALID)).sum())
    on_inst = int((got["instID"] == 1).sum())
    print(f"  {on_lines} hits on the scene's own lines, {on_inst} below the instance")
    assert on_lines > 1000 and on_inst > 1000
    inner.release()
    dev.release()


# ---- 5. filters -------------------------------------------------------------------------------------------------------------------------------------
def _ray_fields(args):
    ray = C.cast(args.contents.ray, C.POINTER(C.c_float * 12)).contents
    hit = C.cast(args.contents.hit, C.POINTER(C.c_uint * 8)).contents
    hitf = C.cast(args.contents.hit, C.POINTER(C.c_float * 8)).contents
    return ray, hit, hitf


@pytest.mark.parametrize("flags", MODES)
def test_filters_see_the_candidates_and_reject_every_second_segment(rtc, tuft, flags):
    """An intersect filter, an occluded filter and a context filter that reject the odd primIDs: the records are those of the scene built
    without those segments, primIDs mapped back.  The callbacks get the geometry's user data and the candidate (geomID, primID, t, u, v = 0, Ng)."""
    v, idx = tuft["v"], tuft["idx"]
    n = 1024
    rh = lh.rays_of(rtc, tuft["org"][:n], tuft["dirs"][:n])
    ng = (v[idx + 1, :3] - v[idx, :3]).astype(F)
    USER = 0x5EED0
    seen, bad = [], []

    @rtc.FILTER_FUNC
    def flt(args):
        ray, hit, hitf = _ray_fields(args)
        prim = hit[5]
        seen.append((ray[0], prim, ray[8], hitf[3]))
        if not (args.contents.geometryUserPtr == USER and args.contents.N == 1 and hit[6] == 7 and hitf[4] == 0.0 and 0.0 <= hitf[3] <= 1.0 and
                (hitf[0], hitf[1], hitf[2]) == tuple(ng[prim]) and hit[7] == INVALID):
            bad.append((prim, hit[6], hitf[4], tuple(hitf[0:3])))
        if prim & 1:
            args.contents.valid[0] = 0

    even = idx[0::2]
    dev0, ref = _scene(rtc, flags, lambda s: s.add_lines(v, even, geom_id=7))
    want, wocc = _trace(rtc, ref, rh)
    wh = want["geomID"] != INVALID
    want["primID"][wh] *= 2  # back to the primIDs of the full geometry
    assert int(wh.sum()) > n // 3

    def full(s):
        assert s.add_lines(v, idx, geom_id=7) == 7
        s.set_user_data(7, USER)

    # geometry filters
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
    # every closest hit was shown to the intersect filter with its t and u
    shown = {(s[0], s[1]): (s[2], s[3]) for s in seen}
    for r in got[wh][:200]:
        assert shown[(float(r["org_x"]), int(r["primID"]))] == (float(r["tfar"]), float(r["u"]))
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


# ---- 6. entry paths ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES)
def test_entry_paths_are_bit_identical(rtc, po, tuft, flags):
    import torch

    def scene(extra=""):
        return _scene(rtc, flags, lambda s: s.add_lines(tuft["v"], tuft["idx"]), extra)

    m = 40000
    rays = po.make_random_rays(m, np.zeros(3, F), np.ones(3, F), seed=21)
    dev, sc = scene()
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
    sc.release()
    dev.release()
    # service=1: the line accel has no service kernel, the calls fall back to the combiner and agree
    dev, sc = scene("service=1")
    sv = rtc.aligned_rayhits(k)
    sv[:] = rays[:k]
    for i in range(0, k, 32):
        sc.intersect1M(sv[i:i + 32])
    assert sv.tobytes() == want[:k].tobytes()
    assert dev.get_property(rtc.RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS) == 0
    sc.release()
    dev.release()


# ---- 7. the overflow area of the traversal stack ------------------------------------------------------------------------------------------------------------
MIN_SPILLS = 0.05 * ds.GPU_RAYS  # as tests/test_gpu_deep_stack.py: every ray above slot 16 pushes at least one entry to HBM


@pytest.mark.parametrize("flags", MODES)
def test_lane_octet_and_pool_kernels_agree_beyond_the_lds_stack(rtc, monkeypatch, flags):
    """A soup of needles as long as the cube they lie in (tests/deep_stack_helpers.py), as segments of radius 0.01: node boxes overlap
    everywhere and rays carry their stacks into the HBM overflow area, which the counted twin's stackSpills must show."""
    tv, tt = ds.sliver_soup(ds.N_SLIVERS, ds.SOUP_SEED)
    p = tv.reshape(-1, 3, 3)[:, :2].reshape(-1, 3)  # v0, v1 of every needle
    v = np.concatenate([p, np.full((len(p), 1), 0.01, F)], 1).astype(F)
    idx = np.arange(0, len(v), 2, dtype=np.uint32)
    lo, hi = ds.bounds(p)
    from helpers import random_rays_np
    org, dirs = random_rays_np(ds.GPU_RAYS, lo, hi, ds.GPU_RAY_SEED)
    rh = ds.rays_of(rtc, org, dirs)
    first = None
    for name, knobs in FORMS.items():
        _knobs(monkeypatch, knobs)
        dev, sc = _scene(rtc, flags, lambda s: s.add_lines(v, idx))
        assert sc.stats()["maxDepth"] >= 3
        got, occ = _trace(rtc, sc, rh)
        c = ds.copy_of(rtc, rh)
        cnt = sc.intersect1M_counted(c)
        assert c.tobytes() == got.tobytes(), f"{name}: the instrumented twin differs from the plain kernel"
        print(f"  needle segments, {name}: stackSpills {cnt['stackSpills']} ({len(rh)} rays), {int((got['geomID'] != INVALID).sum())} hits")
        assert cnt["stackSpills"] >= MIN_SPILLS, (name, cnt["stackSpills"])
        if first is None:
            # A share of the rays against the truth.  Rays set aside: a ray crosses the ribbons of about N * 2 r * L * pi / 4 = 8192 *
            # 0.02 * 0.785 = 130 needles per unit of its length, and a crossing lies within 1e-4 of `d2 <= r2` (|d| / r within 5e-5 of 1,
            # from either side) with probability 1e-4 each side: about 2 % of the rays have some segment there - not only the nearest
            # counts - and twice that is the cap (measured: 5 of 512)
            k = 512
            v0, v1 = lh.ends(v, idx)
            truth = lh.closest(v0, v1, org[:k], dirs[:k], rh["tnear"][:k], rh["tfar"][:k], np.float64)
            _check_parity(got[:k], occ[:k], rh[:k], truth, 0, f"needle segments, {name}", cap=0.04)
            assert int((got["geomID"] != INVALID).sum()) > ds.GPU_RAYS // 2
            first = (name, got.tobytes(), occ.tobytes())
        else:
            assert got.tobytes() == first[1], f"closest hit, {name} differs from {first[0]}"
            assert occ.tobytes() == first[2], f"any hit, {name} differs from {first[0]}"
        assert dev.error() == 0  # the `overflow` word stayed clear: no entry was dropped
        sc.release()
        dev.release()


# ---- 8. the C example -----------------------------------------------------------------------------------------------------------------------------------------
def test_line_segments_example_runs(tmp_path):
    exe = str(tmp_path / "line_segments_min")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200112L", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "line_segments_min.c"), "-L" + LIBDIR, "-lembree3", "-lm", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "line_segments_min: ok" in out.stdout
