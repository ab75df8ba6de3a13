"""The hard rays on the hair family: line segments (kinds 36 / 37), flat curves (42 / 43), round curves (42 / 43 with round_curves=1), their
motion-blur forms (38 .. 41, 44 .. 47) and hair below instances (22 / 23 with inst_hair=1).  The kinds' own files trace random rays that
come in from a sphere, directions about 2 long, tnear 0, tfar inf; the leaves have code of their own on the rays of
tests/test_gpu_edge_rays.py: line_space() builds the ray frame from dir (an axis-parallel dir is an exact tie of `l0 > l1`) and the
depth scale 1 / |dir| enters every t, `t > tnear + 2 r s` is what a bounce ray from a hair meets first, the tube leaf shifts the ray to a
reference point, cuts cylinders with an eps relative to |dir|^2 and accepts a Newton candidate under bounds tied to |dir|, and the
instance leaf re-derives all of it in local space.

Rays, scenes, truths and the comparison are those of tests/hair_edge_rays_helpers.py: every expected side is the kind's float64 truth,
never a product kernel; tests/test_host_hair_edge_rays.py runs the float32 restatements of the leaves through the same comparison and
shows that two deliberately wrong expected sides fail it.  Every mode (robust, fast) and every kernel form the kind's own parity test
enumerates; the forms must be bit-identical to one another.

Invalid rays - why no poisoned field can index memory or keep a loop running, read off the leaves before the first run (the node steps,
the traversal stack, time_segment and the instance leaf are those of tests/test_gpu_edge_rays.py, whose text holds here as it stands):
  * the line leaf (trace_line.hip.h) and the ribbon leaf (trace_curve.hip.h) loop over the records of the leaf - first and count come
    from the leaf reference - and, the ribbon leaf, over the segments of a record - N comes from the record; every address is formed
    from those and from the ray's index in the batch (the exclusion list), never from a ray value.  A ray value enters line_space() and
    the products after it only: a NaN or infinite org / dir gives a NaN frame or NaN ray-space points, `d2 <= r2`, `max(U, V) <= 0` and
    the depth tests are comparisons, false on NaN, and the candidate is dropped.  dir = 0 gives s = inf and a NaN frame: the same.
  * the tube leaf (trace_round_curve.hip.h): three levels, unrolled at compile time, and five Newton steps; the record loop runs over the
    leaf's count.  The only data-dependent loop, `while (__ballot(cand))`, clears one candidate lane per octet and turn - the selected
    lane is the lowest with `tlo == tmin`, and a lane is a candidate only after `tlo + dt <= tfar`, false for a NaN tlo or dt, so the
    minimum is taken over numbers - at most seven turns per level.  A NaN or infinite org or dir makes dt NaN or infinite and the shifted
    control points NaN: `D >= 0` fails and no candidate is formed; Newton returns through `!(th > tnear && th < tfar)` on NaN.
  * the moving leaves add time_segment (a comparison, no index) and a lerp of the record's two ends; under mb_bounds=linear the node
    step (trace_loop.hip.h) takes the ray's time clamped to [0, 1], a NaN as 0, as the weight of a lerp of the planes - no index either.
  * tnear NaN, tnear > tfar, tfar NaN or -inf: the ray fails `tnear <= tfar` and is never started.
No field was left out.  tnear = -inf is a valid ray (its window starts at -inf): it is in the batch, but what it reports is not held
to anything here; every other poisoned record must come back byte for byte."""
import numpy as np
import pytest

import hair_edge_rays_helpers as he
import instance_hair_helpers as ihh
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import line_helpers as lh
from helpers import INVALID

pytestmark = pytest.mark.gpu

ROBUST = 4
MODES = [pytest.param(ROBUST, id="robust"), pytest.param(0, id="fast")]
KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL", "RTAMD_CBVH_FORM")
LANE = {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "0", "RTAMD_OCT_LEAF": "0"}
OCTET = {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "32", "RTAMD_OCT_LEAF": "1"}
POOL = {"RTAMD_KERNEL": "pool"}
# as the parity test of each kind enumerates them (the tube leaf is octet-only: lane and octet NODE steps)
FORMS = {"lines": {"lane form": LANE, "octet form": OCTET, "ray-pool kernel": POOL},
         "curves": {"lane form": LANE, "octet form": OCTET, "pool asked": POOL}, "bspline": {"lane form": LANE, "octet form": OCTET, "pool asked": POOL},
         "round": {"lane node steps": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "0"}, "octet node steps": {"RTAMD_KERNEL": "lane", "RTAMD_OCT_MAX": "32"}},
         "lines.mb": {"lane form": LANE, "octet form": OCTET}, "curves.mb": {"lane form": LANE, "octet form": OCTET}}
BOUNDS = {"swept": "", "linear": "mb_bounds=linear"}
ACCEL = {"lines": 36, "curves": 42, "bspline": 42, "round": 42, ("lines.mb", "swept"): 38, ("lines.mb", "linear"): 40, ("curves.mb", "swept"): 44,
         ("curves.mb", "linear"): 46}  # the robust kind; the fast one is one higher
KIND_BOUNDS = [(k, "swept") for k in he.STATIC] + [(k, b) for k in he.MOVING for b in BOUNDS]  # node boxes over time are a choice of the moving kinds


def _knobs(monkeypatch, knobs):
    """the tuning knobs are read when a device is created"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def _scene(rtc, kind, flags, bounds="swept"):
    g = he.geometry(kind)
    dev = rtc.Device(",".join(x for x in (g["cfg"], BOUNDS[bounds]) if x))
    sc = rtc.Scene(dev, flags)
    g["add"](sc)
    sc.commit()
    assert sc.stats()["accelKind"] == ACCEL[(kind, bounds) if kind in he.MOVING else kind] + (0 if flags else 1)
    return dev, sc


def _trace(rtc, sc, rays):
    got, occ = he.copy(rtc, rays), lh.occ_of(rtc, rays)
    sc.intersect1M(got)
    sc.occluded1M(occ)
    return got, occ


def _forms(rtc, monkeypatch, kind, flags, rays, bounds="swept"):
    """intersect1M and occluded1M of `rays` in every form of the kind: the first form's records, the others bit-identical to them"""
    first = None
    for name, knobs in FORMS[kind].items():
        _knobs(monkeypatch, knobs)
        dev, sc = _scene(rtc, kind, flags, bounds)
        got, occ = _trace(rtc, sc, rays)
        assert dev.error() == 0, name
        if first is None:
            first = (got, occ)
        else:
            assert got.tobytes() == first[0].tobytes() and occ.tobytes() == first[1].tobytes(), f"{kind}: {name} differs from {next(iter(FORMS[kind]))}"
        sc.release()
        dev.release()
    return first


def _short_floor(kind, want, rays, what):
    """round curves: at least 30 compared truth hits among the rays with |dir| < 1e-2 - the rays the Newton bound 16 ulp |dir| was short
    for (the CPU counts: 38 on the degenerate family, every hit of the pinned rays scaled down)"""
    if kind == "round":
        n = he.short_hits(want, rays)
        print(f"{what}: {n} compared truth hits with |dir| < {he.SHORT}")
        assert n >= 30, (what, n)


# ---- 1. degenerate rays -------------------------------------------------------------------------------------------------------------------
# hits of the float64 truth (tests/test_host_hair_edge_rays.py has them from the CPU alone)
DEGENERATE_HITS = {"lines": 2784, "curves": 1736, "bspline": 817, "round": 682, "lines.mb": 2801, "curves.mb": 1798}


@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("kind", he.STATIC)
def test_degenerate_rays(rtc, monkeypatch, kind, flags):
    """edge_rays over the unit cube, seed 7: axis-parallel rays from all six sides, one direction component exactly zero with every fifth
    direction scaled by 2^-10 and every fifth + 1 by 256, tnear windows, tnear = 1e30, short tfar, origins exactly on a face of the cube"""
    rays, want = he.degenerate_case(rtc, kind)
    assert int(want["hit"].sum()) >= DEGENERATE_HITS[kind] // 2
    what = f"degenerate rays, {kind}, {'robust' if flags else 'fast'}"
    _short_floor(kind, want, rays, what)
    got, occ = _forms(rtc, monkeypatch, kind, flags, rays)
    he.check(kind, got, rays, want, what, occ)


@pytest.mark.parametrize("bounds", list(BOUNDS))
@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("kind", he.MOVING)
def test_degenerate_rays_on_moving_hair(rtc, monkeypatch, kind, flags, bounds):
    """the same family, ray times cycling through k / 4, on the two-step tuft and hair under swept and time-dependent node boxes"""
    rays, want = he.degenerate_case(rtc, kind)
    assert int(want["hit"].sum()) >= DEGENERATE_HITS[kind] // 2 and min(int((want["hit"] & (rays["time"] == t)).sum()) for t in he.TIMES) >= 100
    got, occ = _forms(rtc, monkeypatch, kind, flags, rays, bounds)
    he.check(kind, got, rays, want, f"degenerate rays, {kind}, {'robust' if flags else 'fast'}, {bounds}", occ)


# ---- 2. direction scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("kind,bounds", KIND_BOUNDS)
def test_directions_scaled_by_powers_of_two(rtc, monkeypatch, kind, flags, bounds):
    """the kind's pinned rays with dir times 2^-20, 2^-10, 2^10, 2^20, one batch: the expected side is the pinned truth with t divided by
    the same factor"""
    cases = [he.scaled_case(rtc, kind, e) for e in he.SCALES]
    rays = he.copy(rtc, np.concatenate([r for r, _ in cases]))
    got, occ = _forms(rtc, monkeypatch, kind, flags, rays, bounds)
    m = len(cases[0][0])
    for j, (e, (r, want)) in enumerate(zip(he.SCALES, cases)):
        what = f"dir * 2^{e}, {kind}, {'robust' if flags else 'fast'}, {bounds}"
        assert int(want["hit"].sum()) >= 300
        if e < 0:
            _short_floor(kind, want, r, what)
        he.check(kind, got[j * m:(j + 1) * m], r, want, what, occ[j * m:(j + 1) * m])


# ---- 3. rays that start on a hair -----------------------------------------------------------------------------------------------------------
def _surface_case(rtc, kind):
    """bounce and shadow rays, tnear 0 and 0.001, from the hits of the KERNEL's primaries on the pinned rays (robust scene, default
    knobs; the flat kinds report the tangent as Ng - whatever direction bounce() derives from it, the origin lies on a primitive), and
    their truths: computed once, shared by modes, bounds and forms"""
    def make():
        dev, sc = _scene(rtc, kind, ROBUST)
        prim = he.pinned_rays(rtc, kind)
        sc.intersect1M(prim)
        sc.release()
        dev.release()
        out = []
        for tnear in (0.0, 0.001):
            sec, sh = he.bounce_rays(rtc, prim, tnear)
            shfull = he.as_rayhits(rtc, sh)
            times = sec["time"] if kind in he.MOVING else None
            out.append((tnear, sec, he.truth(kind, *he.fields(sec), times=times), shfull, he.truth(kind, *he.fields(shfull), times=times)))
        return out
    return he._once(("surface", kind), make)


@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("kind,bounds", [kb for kb in KIND_BOUNDS if kb[0] in he.SURFACE])
def test_surface_origin_rays(rtc, monkeypatch, kind, flags, bounds):
    """bounce rays and, through occluded, shadow rays that start on a hair, tnear 0 and 0.001: what they meet first is the hair they
    start on and its rule `t > tnear + 2 r s`.  Round curves are not among the kinds (hair_edge_rays_helpers.SURFACE says why)."""
    for p in KNOBS:
        monkeypatch.delenv(p, raising=False)
    cases = _surface_case(rtc, kind)
    n = len(cases[0][1])
    rays = he.copy(rtc, np.concatenate([x for _, sec, _, shfull, _ in cases for x in (sec, shfull)]))
    got, occ = _forms(rtc, monkeypatch, kind, flags, rays, bounds)
    for j, (tnear, sec, want, shfull, wsh) in enumerate(cases):
        what = f"tnear {tnear}, {kind}, {'robust' if flags else 'fast'}, {bounds}"
        a, b = 2 * j * n, (2 * j + 1) * n
        assert 0 < int(want["hit"].sum()) < n and 0 < int(wsh["hit"].sum()) < n, what
        he.check(kind, got[a:a + n], sec, want, "bounce rays, " + what, occ[a:a + n])
        he.check(kind, got[b:b + n], shfull, wsh, "shadow rays, " + what, occ[b:b + n])


# ---- 4. invalid rays leave their batch-mates alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES)
@pytest.mark.parametrize("kind,bounds", KIND_BOUNDS)
def test_invalid_rays_leave_the_others_alone(rtc, monkeypatch, kind, flags, bounds):
    """poisoned records among the kind's pinned rays (hair_edge_rays_helpers.POISON: NaN and +-inf in org, dir, tnear, tfar, dir = 0,
    tfar = -inf, and on the moving kinds time = +inf, -3, 7): they come back byte for byte (tnear = -inf apart), the others are the
    records of the batch traced without them.  Why none of them can fault: the module docstring."""
    clean = he.pinned_rays(rtc, kind)
    dirty, bad, exact = he.poisoned(rtc, clean, kind in he.MOVING)
    keep = np.ones(len(clean), bool)
    keep[bad] = False
    want, wocc = _forms(rtc, monkeypatch, kind, flags, he.copy(rtc, clean[keep]), bounds)
    got, occ = _forms(rtc, monkeypatch, kind, flags, dirty, bounds)
    nh = int((want["geomID"] != INVALID).sum())
    print(f"invalid rays, {kind}: {len(bad)} poisoned records, {nh} hits among the other {int(keep.sum())}")
    assert nh > 300  # the B-spline reading of the hair spans the middle of each control polygon only: 469 hits, the other kinds above 600
    src = lh.occ_of(rtc, dirty)
    same = bad[exact]
    assert got[same].tobytes() == dirty[same].tobytes() and occ[same].tobytes() == src[same].tobytes()
    assert got[keep].tobytes() == want.tobytes() and occ[keep].tobytes() == wocc.tobytes()


# ---- 5. hair below instances ------------------------------------------------------------------------------------------------------------------
INSTANCE_HITS = {"a": 1095, "b": 1283}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["a", "b"])
def test_degenerate_rays_on_instanced_hair(rtc, monkeypatch, which, mode):
    """line segments (a) and flat curves (b: Bezier at rate 4, B-spline at rate 9) under six moving instances - signed axis permutations
    times power-of-two scales: an axis-parallel world ray becomes an axis-parallel local ray along ANOTHER axis, and its |dir| is scaled,
    which moves 2 r s.  The expected side: hair_edge_rays_helpers.instance_truth."""
    for p in KNOBS:
        monkeypatch.delenv(p, raising=False)
    scs = he.instance_scene(which)
    inst = im.exact_instances(6)
    rays = he.instance_rays(rtc, scs, inst)
    want = he._once(("instanced", which), lambda: he.instance_truth(scs, inst, rays))
    per_inst = np.bincount(want["inst"][want["hit"]], minlength=len(inst))
    assert int(want["hit"].sum()) >= INSTANCE_HITS[which] // 2 and per_inst.min() >= 5, per_inst
    dev, top, inner = ihh.build(rtc, mode, scs, inst)
    assert top.stats()["accelKind"] == imm.kind(mode)
    got, occ = _trace(rtc, top, rays)
    assert dev.error() == 0
    he.check("inst", got, rays, want, f"degenerate rays, instanced hair ({which}), mode {mode}", occ)
    assert (got["instID"][got["geomID"] == INVALID] == INVALID).all()
    ihh.release(dev, top, inner)
