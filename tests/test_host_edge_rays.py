"""The inputs of tests/test_gpu_edge_rays.py, measured on the CPU oracle alone: the counts its floors are derived from, the v1-v3
diagonal finding on the ground quad, the set-aside share of the general-transform leg - and three mutations: a deliberately wrong
expected side (B preferred on a tie, tnear ignored inside an instance, the time of bounce rays zeroed) must differ from the right one
under helpers.compare_hits, i.e. the GPU tests would fail on a kernel that made that mistake."""
import numpy as np
import pytest

import deep_stack_helpers as ds
import edge_rays_helpers as er
import instance_helpers as ih
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
from helpers import INVALID, compare_hits


def _near(count, pinned):
    return abs(count - pinned) <= pinned // 100


def _diagonal(want):
    hit = want["geomID"] != INVALID
    return hit & (np.abs(want["u"].astype(np.float64) + want["v"] - 1.0) < 1e-4)


def _differs(a, b):
    with pytest.raises(AssertionError):
        compare_hits(a, b)
    return True


# ---- the ray families ---------------------------------------------------------------------------------------------------------------------
def test_edge_ray_families(rtc):
    lo, hi = np.array([-2.0, 0.0, 1.0]), np.array([6.0, 3.0, 5.0])
    diag = float(np.linalg.norm(hi - lo))
    r = er.edge_rays(rtc, lo, hi, 5, 3, snapped=True, m=70, k=30)
    assert len(r) == 6 * 25 + 100
    o = np.stack([r["org_x"], r["org_y"], r["org_z"]], 1).astype(np.float64)
    d = np.stack([r["dir_x"], r["dir_y"], r["dir_z"]], 1)
    assert np.array_equal(o * 1024.0, np.round(o * 1024.0))  # on the 2^-10 grid
    assert ((d[:150] != 0).sum(1) == 1).all() and (np.abs(d[:150]).sum(1) == 1).all()  # axis-parallel, all six directions
    assert len(np.unique(d[:150], axis=0)) == 6
    outside = ((o[:150] < lo) | (o[:150] > hi)).sum(1)
    assert (outside == 1).all()
    mid = d[150:220]
    assert ((mid == 0).sum(1) >= 1).all() and ((mid != 0).sum(1) == 2).all()  # one zero component
    assert np.abs(mid[::5]).max() < 2.0 ** -10 and np.abs(mid[1::5]).max() > 1.0
    tn, tf = r["tnear"][150:220], r["tfar"][150:220]
    assert (tn[::3][tn[::3] < 1e29] == np.float32(0.01 * diag)).all() and (tn[1::7] == np.float32(1e30)).all()
    assert (tf[::4] <= 0.06 * diag).all() and np.isinf(np.delete(tf, np.arange(0, 70, 4))).all()
    face = o[220:]
    assert (((face == lo) | (face == hi)).sum(1) >= 1).all() and ((d[220:] != 0).sum(1) == 1).all()
    inwards = face + d[220:] * 0.5
    assert ((inwards >= lo) & (inwards <= hi)).all()
    u = er.edge_rays(rtc, lo + 0.3, hi + 0.3, 5, 3, m=70, k=30)
    assert len(u) == len(r) and u.dtype == r.dtype


# ---- section 2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_static_quad_case_and_the_ground_plane_diagonal(rtc, po, bomberman, mode):
    data = er.top_data("quads", bomberman)
    rays = er.top_edge_rays(rtc, "quads", data)
    want, isb = er.top_oracle(rtc, po, "quads", data, rays, mode)
    hits = int((want["geomID"] != INVALID).sum())
    assert len(rays) == 38_400 and hits == 12_437
    dg = _diagonal(want)
    bent = er.nonplanar_quads(*data)
    assert int(bent.sum()) == 353 and not bent[0]
    # 140 near-diagonal hits, 1.13 %: beyond the 1 % cap - all on quad 0, the planar ground quad, none on a non-planar quad
    assert int(dg.sum()) == 140 and int(dg.sum()) >= hits // 100 and (want["primID"][dg] == 0).all()
    assert int((dg & (want["u"] + want["v"] == np.float32(1))).sum()) >= 32  # u + v == 1 exactly (measured: 63)
    with pytest.raises(AssertionError):
        ds.quad_allowances(want.copy(), want.copy(), isb, mode)  # the unrestricted allowance breaks its cap on the oracle alone
    assert ds.quad_allowances(want.copy(), want.copy(), isb, mode, nonplanar=bent) == 0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["tri.mb", "quad.mb"])
def test_motion_blur_case_counts(rtc, po, bomberman, what, mode):
    data = er.top_data(what, bomberman)
    rays = er.top_edge_rays(rtc, what, data)
    want, isb = er.top_oracle(rtc, po, what, data, rays, mode)
    c = er.counts(want, rays)
    assert c == {"rays": 12_456, "hits": 1_877, "per_time": 357}, c
    if what == "quad.mb":
        assert ds.quad_allowances(want.copy(), want.copy(), isb, mode, nonplanar=er.top_nonplanar(what, data)) <= 1


def test_quad_allowances_restricts_the_normal_allowance_to_non_planar_quads(rtc):
    want = rtc.aligned_rayhits(400)
    want["geomID"], want["primID"], want["u"], want["v"] = 7, np.arange(400) % 2, 0.25, 0.25
    want["u"][:3], want["v"][:3] = 0.5, 0.5  # three hits on the diagonal: quads 0, 1, 0
    want["Ng_z"] = 1.0
    got = want.copy()
    got["Ng_z"][:3] = -1.0
    w = want.copy()
    assert ds.quad_allowances(got, w, np.zeros(400, bool), 0) == 3 and (w["Ng_z"][:3] == -1).all()  # unchanged default
    for mask in (np.array([False, True]), {7: np.array([False, True])}):
        w = want.copy()
        assert ds.quad_allowances(got, w, np.zeros(400, bool), 0, nonplanar=mask) == 1
        assert w["Ng_z"][1] == -1 and w["Ng_z"][0] == 1 and w["Ng_z"][2] == 1
    w = want.copy()
    assert ds.quad_allowances(got, w, np.zeros(400, bool), 0, nonplanar={9: np.array([True, True])}) == 0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["exact", "grid"])
def test_instance_case_counts_and_the_tnear_mutation(rtc, po, bomberman, which, mode):
    scenes = imm.scenes_c(bomberman)
    inst = er.instance_sets(which)
    rays = er.instance_edge_rays(rtc, scenes, inst)
    want, per, isb, _ = imm.oracle_instances(rtc, po, scenes, inst, rays, mode, exact=True)  # asserts the local rays exact
    c = er.counts(want, rays, (3, 5, 7, 9), len(inst))
    pinned = {"exact": {"rays": 14_100, "hits": 6_240, "per_time": 1_221, "per_geom": 1_031, "per_inst": 121},
              "grid": {"rays": 14_100, "hits": 7_435, "per_time": 1_416, "per_geom": 1_433, "per_inst": 79}}[which]
    assert c == pinned, c
    hit = want["geomID"] != INVALID
    assert (want["instID"][~hit] == INVALID).all() and ih.equal_t_ties(per) == 0
    assert ds.quad_allowances(want.copy(), want.copy(), isb, mode, imm.quad_gids(scenes), er.instance_nonplanar(scenes)) == 0
    if which == "exact" and mode == 0:
        # mutation: tnear ignored after entering an instance
        r0 = iq.copy(rtc, rays)
        r0["tnear"] = 0
        wrong = imm.oracle_instances(rtc, po, scenes, inst, r0, mode, exact=True)[0]
        wrong["tnear"] = rays["tnear"]
        assert _differs(wrong, want)


# ---- the closed form on the diagonal ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", ["unit", "bent"])
def test_diagonal_rays_tie_and_the_b_preferred_mutation(rtc, po, shape, mode):
    quad = er.UNIT if shape == "unit" else er.BENT
    assert bool(er.nonplanar_quads(quad, er.Q1)[0]) == (shape == "bent")
    org, dirs = er.diagonal_rays(quad)
    assert len(org) == 64 and len(np.unique(dirs, axis=0)) == 8
    want, other, tie, near, isb = er.diagonal_expected(rtc, po, quad, org, dirs, mode)
    assert (want["geomID"] == 0).all() and tie.all() and not near.any() and not isb.any()
    assert np.abs(want["u"].astype(np.float64) + want["v"] - 1.0).max() < 1e-6  # on the diagonal
    assert int((want["u"] == 0).sum()) >= 3 and int((want["v"] == 0).sum()) >= 3  # through v3 and through v1
    wrong, _, _, _, wb = er.diagonal_expected(rtc, po, quad, org, dirs, mode, prefer_b=True)
    assert wb.all()
    if shape == "bent":  # mutation: B-lane tie preferred over A - B's normal differs on a non-planar quad
        assert _differs(wrong, want)


# ---- section 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["quads", "tri.mb", "quad.mb"])
def test_surface_ray_counts_and_the_time_mutation(rtc, po, bomberman, what):
    mode = 0
    data = er.top_data(what, bomberman)
    lo, hi = er.top_bounds(what, data)
    prim = er.top_primaries(rtc, po, what, data)
    pw, _ = er.top_oracle(rtc, po, what, data, prim, mode)
    sec, sh = er.bounce(rtc, pw, 11, snapped=True, light=er.light_of(lo, hi))
    assert np.isfinite(sh["tfar"]).all() and (sec["tnear"] == np.float32(0.001)).all()
    want, _ = er.top_oracle(rtc, po, what, data, sec, mode)
    hit = want["geomID"] != INVALID
    near = int((hit & (want["tfar"] < 0.01)).sum())
    pinned = {"quads": (45_479, 3_199, 327), "tri.mb": (25_547, 2_089, 163), "quad.mb": (25_546, 2_065, 169)}[what]
    assert _near(len(sec), pinned[0]) and _near(int(hit.sum()), pinned[1]) and near >= pinned[2] // 2, (len(sec), int(hit.sum()), near)
    if what != "quads":
        assert len(np.unique(sec["time"])) == 5 and np.array_equal(sec["time"], pw["time"][pw["geomID"] != INVALID])
        # mutation: the time of the bounce rays zeroed
        s0 = iq.copy(rtc, sec)
        s0["time"] = 0
        wrong, _ = er.top_oracle(rtc, po, what, data, s0, mode)
        wrong["time"] = sec["time"]
        assert _differs(wrong, want)


def test_general_instance_surface_rays_stay_within_the_set_aside_cap(rtc, po, bomberman):
    mode = 0
    scenes = imm.scenes_c(bomberman)
    inst = er.instance_sets("general")
    lo, hi = er.instance_box(scenes, inst)
    prim = imm.rays_with_times(rtc, po, scenes, inst, 20_000, 53, denom=4)
    pw = imm.oracle_instances(rtc, po, scenes, inst, prim, mode)[0]
    sec, sh = er.bounce(rtc, pw, 11, snapped=True, light=er.light_of(lo, hi))
    want, per, _, want_tri = imm.oracle_instances(rtc, po, scenes, inst, sec, mode)
    aside = iq.quad_set_aside(want, per, want_tri, imm.quad_gids(scenes))
    hit = want["geomID"] != INVALID
    assert _near(len(sec), 10_587) and _near(int(hit.sum()), 5_464) and int((hit & (want["tfar"] < 0.01)).sum()) >= 500  # measured: 1 054
    assert aside.sum() <= 0.02 * len(sec)  # measured: 2
