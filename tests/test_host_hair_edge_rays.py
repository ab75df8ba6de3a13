"""The inputs of tests/test_gpu_hair_edge_rays.py, measured on the CPU alone: for the kinds whose leaf has a float32 restatement (line
segments, flat curves, round curves) the restatement against the float64 truth on the same ray families under the same comparison
(hair_edge_rays_helpers.check) - which pins the counts the floors of the GPU tests are derived from and shows that the inputs keep the
0.5 % cap without any kernel - and two deliberately wrong expected sides, which must fail that comparison: one without the
self-intersection rule `t > tnear + 2 r s`, one that ignores tnear.

The round-curve restatement carries the Newton bound of the leaf, |g| < 16 ulp max(|dir|, largest |component| of the relative control
points).  With the bound the reference has, 16 ulp |dir|, restatement and kernel alike lost hits of short directions: on the pinned rays of
input (b) scaled by 2^-20, 201 hit flips and 31 wrong primIDs (test_the_reference_newton_bound_loses_hits_of_short_directions keeps that
measurement); on the degenerate family the kernel had 6 hit flips and t off by up to 3.8e-2 among the 38 short-direction hits."""
import numpy as np
import pytest

import hair_edge_rays_helpers as he
import instance_mb_helpers as im
from helpers import INVALID

F32 = np.float32
# (rays, hits of the truth, rays its rules leave out) of the degenerate family
DEGENERATE = {"lines": (4536, 2784, 0), "curves": (4536, 1736, 0), "bspline": (4536, 817, 0), "round": (2964, 682, 9)}


def _restated_check(rtc, kind, rays, want, what):
    got = he.records_of(rtc, rays, he.restated(kind, *he.fields(rays)))
    return he.check(kind, got, rays, want, what)


@pytest.mark.parametrize("kind", he.STATIC)
def test_degenerate_rays_restatement_meets_the_truth(rtc, kind):
    rays, want = he.degenerate_case(rtc, kind)
    fig = _restated_check(rtc, kind, rays, want, f"degenerate rays, {kind}, float32 restatement")
    n, hits, left = DEGENERATE[kind]
    print(f"degenerate rays, {kind}: {fig}, short-direction hits {he.short_hits(want, rays)}")
    assert len(rays) == n and fig["out"] <= 0.005 * n and fig["hits"] == hits and fig["out"] == left
    if kind == "round":
        assert he.short_hits(want, rays) == 38


@pytest.mark.parametrize("exponent", he.SCALES)
@pytest.mark.parametrize("kind", he.STATIC)
def test_scaled_directions_restatement_meets_the_scaled_truth(rtc, kind, exponent):
    rays, want = he.scaled_case(rtc, kind, exponent)
    fig = _restated_check(rtc, kind, rays, want, f"dir * 2^{exponent}, {kind}, float32 restatement")
    assert fig["hits"] >= 300
    if kind == "round" and exponent < 0:
        assert he.short_hits(want, rays) >= 30


@pytest.mark.parametrize("tnear", [0.0, 0.001])
@pytest.mark.parametrize("kind", [k for k in he.SURFACE if k in he.STATIC])
def test_bounce_rays_restatement_meets_the_truth(rtc, kind, tnear):
    """bounce and shadow rays from the hits of the pinned truth (the GPU test takes the kernel's own primary hits); why round curves
    are not among them: hair_edge_rays_helpers.SURFACE"""
    prim = he.records_of(rtc, he.pinned_rays(rtc, kind), he.pinned_truth(kind))
    sec, sh = he.bounce_rays(rtc, prim, tnear)
    shfull = he.as_rayhits(rtc, sh)
    for name, rays in (("bounce", sec), ("shadow", shfull)):
        want = he.truth(kind, *he.fields(rays))
        fig = _restated_check(rtc, kind, rays, want, f"{name} rays, tnear {tnear}, {kind}, float32 restatement")
        assert 0 < fig["hits"] < len(rays)


def _fails(kind, got, rays, wrong, what):
    with pytest.raises(AssertionError):
        he.check(kind, got, rays, wrong, what)
    return True


def test_a_truth_without_the_self_intersection_rule_fails(rtc):
    """bounce rays with tnear 0 from the tuft's hits: every origin lies on a segment, and without `t > tnear + 2 r s` that segment
    itself is the nearest hit of most of them"""
    prim = he.records_of(rtc, he.pinned_rays(rtc, "lines"), he.pinned_truth("lines"))
    sec, _ = he.bounce_rays(rtc, prim, 0.0)
    got = he.records_of(rtc, sec, he.restated("lines", *he.fields(sec)))
    wrong = he.truth("lines", *he.fields(sec), self_rule=False)
    assert int(wrong["hit"].sum()) > int((got["geomID"] != INVALID).sum()) + 100
    assert _fails("lines", got, sec, wrong, "no self-intersection rule")


@pytest.mark.parametrize("kind", ["lines", "curves", "round"])
def test_a_truth_that_ignores_tnear_fails(rtc, kind):
    rays, want = he.degenerate_case(rtc, kind)
    org, dirs, tnear, tfar = he.fields(rays)
    got = he.records_of(rtc, rays, he.restated(kind, org, dirs, tnear, tfar))
    # (tnear = 1e30 stays: with a finite tfar such a ray is invalid, which is not what this mutation is about)
    wrong = he.truth(kind, org, dirs, np.where(tnear < 1e29, F32(0), tnear).astype(F32), tfar)
    assert int((wrong["hit"] != want["hit"]).sum() + (wrong["hit"] & want["hit"] & (wrong["primID"] != want["primID"])).sum()) >= 5
    assert _fails(kind, got, rays, wrong, "tnear ignored")


def test_the_reference_newton_bound_loses_hits_of_short_directions(rtc):
    """the restatement with the reference's bound |g| < 16 ulp |dir| on the pinned rays of input (b) scaled by 2^-20: hit flips and
    wrong primIDs by the hundred (measured: 201 and 31), and the comparison fails - the GPU tests would fail on a leaf that kept it"""
    rays, want = he.scaled_case(rtc, "round", -20)
    c = he.restated("round", *he.fields(rays), reference_bound=True)
    keep = ~want["out"]
    flips = int((c["hit"] != want["hit"])[keep].sum())
    ids = int((c["hit"] & want["hit"] & keep & (c["primID"] != want["primID"])).sum())
    print(f"reference bound, dir * 2^-20: {flips} hit flips, {ids} wrong primIDs")
    assert flips >= 100 and ids >= 10
    assert _fails("round", he.records_of(rtc, rays, c), rays, want, "reference bound")


@pytest.mark.parametrize("kind", he.MOVING)
def test_moving_degenerate_rays_keep_the_cap(rtc, kind):
    rays, want = he.degenerate_case(rtc, kind)
    hits = [int((want["hit"] & (rays["time"] == t)).sum()) for t in he.TIMES]
    print(f"degenerate rays, {kind}: {int(want['hit'].sum())} hits, per time {hits}, {int(want['out'].sum())} rays left out")
    assert len(rays) == 4536 and want["out"].sum() <= 0.005 * len(rays) and min(hits) >= 300  # measured: 549 / 352 at the least, 2 rays left out
    assert int(want["hit"].sum()) == {"lines.mb": 2801, "curves.mb": 1798}[kind]


@pytest.mark.parametrize("which", ["a", "b"])
def test_instanced_hair_case_counts(rtc, which):
    scs = he.instance_scene(which)
    inst = im.exact_instances(6)
    rays = he.instance_rays(rtc, scs, inst)
    want = he.instance_truth(scs, inst, rays)
    per_inst = np.bincount(want["inst"][want["hit"]], minlength=len(inst))
    print(f"instanced hair ({which}): {int(want['hit'].sum())} hits of {len(rays)} rays, per instance {per_inst.tolist()}, {int(want['out'].sum())} rays left out")
    assert want["out"].sum() <= 0.005 * len(rays) and per_inst.min() >= 10  # measured: 34 / 1 rays left out, 16 / 19 hits on the least hit instance
    assert int(want["hit"].sum()) == {"a": 1095, "b": 1283}[which]
