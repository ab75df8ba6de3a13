"""The hard rays on the accels that came after the triangle and subdivision kernels: static quads (kinds 8 / 9), motion-blur triangles
(10 / 11) and quads (12 / 13), and instances of all of them (14 .. 23).  tests/test_gpu_degenerate_rays.py and
tests/test_gpu_secondary.py stop at triangles and subdivision accels; the kernels here have code of their own on exactly these rays: the
instance leaf re-derives the ray's reciprocals and octant in local space (a world ray with a zero direction component becomes a local
ray with ANOTHER zero component under a signed axis permutation) and keeps tnear / tfar across the frame change, the Quad4v leaf ranks A
and B lanes that tie on the v1-v3 diagonal, the motion-blur leaves interpolate vertices before the same edge tests.

Rays, scenes and expected records are those of tests/edge_rays_helpers.py; every expected side is the CPU oracle's (one static oracle
scene per ray time, the split-triangle scene with the B mapping for quads, local rays per instance merged by smallest t), never a
product kernel's.  tests/test_host_edge_rays.py pins the counts of the oracle's records the floors below are derived from, and shows that
three deliberately wrong expected sides fail.  Bar: IDs exact, t / u / v / Ng within 1e-4 (helpers.compare_hits) after
deep_stack_helpers.quad_allowances; occluded: tfar = -inf exactly where the oracle hits and every other byte of the record untouched.

Finding (the inputs', not the kernels'): on the static-quad case 140 of the oracle's 12 437 hits (1.13 %) lie within 1e-4 of a v1-v3
diagonal, 63 of them with u + v == 1 exactly - all on quad 0, the square ground plane: the +y lattice rays have equal x and z lattice
fractions and run exactly along its diagonal.  That breaks the 1 % cap of the normal allowance on the oracle alone.  The quad is planar,
its two split normals agree, so the allowance is not needed there: quad_allowances takes it for NON-PLANAR quads only (353 of the 727;
0 near-diagonal hits on them), and the ground plane's ties (A and B tie, the lowest lane - A - wins) are compared like any other hit.

Invalid rays (section 4) - why no poisoned field can index out of bounds, read off the kernels before the first run:
  * org / dir / tnear / tfar NaN or infinite: they reach slab tests and edge tests only.  fmaxf / fminf drop a NaN operand, so a NaN slab
    distance leaves tN = tnear, tF = tfar: the ray may enter every child of every node, never more - the stack holds at most 7 entries
    per level plus the markers, which is what launch_on reserves (7 (maxDepth + 1) + 2); a push beyond it is dropped behind a bounds
    check and raises the overflow flag (dev.error() != 0, which the test would report), a pop beyond it returns EMPTY.  The octant
    (TravRay::negx: !(r >= 0)) only selects between two words already loaded.  Leaf records are addressed by the leaf reference, never by
    a ray value; a tnear NaN fails `tnear <= tfar` and the ray is skipped.
  * time (NaN, +inf, -3, 7): time_segment (trace_mb.hip.h) only COMPARES clamp(floor(time S), 0, S - 1) with the record's segment - no
    index is formed; fmaxf(NaN, 0) = 0.  instance_time_segment (instance_xfm.h) does index InstanceStep[itime], [itime + 1] with the same
    clamp: itime lies in [0, S - 1] for every input (NaN -> 0, +inf -> S - 1), and an instance with S segments owns S + 1 steps.  ftime
    is then NaN / inf / outside [0, 1]: the lerped matrix is non-finite or extrapolated; instance_invert refuses a result that is not
    finite (the ray does not enter, nothing is pushed) and an extrapolated matrix is an ordinary matrix.  Lerped vertices that are NaN
    fail the edge tests.
  * a non-finite local ray inside an instance is the first bullet again, in the instanced scene's trees."""
import numpy as np
import pytest

import deep_stack_helpers as ds
import edge_rays_helpers as er
import instance_helpers as ih
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
from helpers import INVALID, compare_hits, fill_rays

pytestmark = pytest.mark.gpu

TOP = ["quads", "tri.mb", "quad.mb"]


def _parity(rtc, sc, rays, want, isb, mode, what, quads, quad_gids=None, nonplanar=None):
    """intersect1M and occluded1M of `sc` against the oracle's records; returns the kernel's records"""
    hit = want["geomID"] != INVALID
    got = iq.copy(rtc, rays)
    sc.intersect1M(got)
    ghit = got["geomID"] != INVALID
    print(f"{what}: GPU {int(ghit.sum())} hits of {len(rays)} rays, oracle {int(hit.sum())}; {int((isb & hit).sum())} on B triangles")
    want = want.copy()
    if quads:
        nd = ds.quad_allowances(got, want, isb, mode, quad_gids, nonplanar)
        print(f"{what}: kernel's normal taken on {nd} near-diagonal hits of non-planar quads")
    compare_hits(got, want, 1e-4, what)
    assert (got["instID"][~ghit] == INVALID).all()
    occ = iq.occ_of(rtc, rays)
    sc.occluded1M(occ)
    assert occ.tobytes() == er.occluded_expected(rtc, rays, want).tobytes(), f"{what}: occluded"
    return got


def _floors(want, rays, hits, per_time=None, per_geom=None, per_inst=None, gids=None, n_inst=None):
    """a scene that moved out of the rays must not pass silently: at least half of the oracle's hit count, every time / geomID /
    instance at least `per_*` times"""
    c = er.counts(want, rays, gids, n_inst)
    assert c["hits"] >= hits // 2, c
    for key, floor in (("per_time", per_time), ("per_geom", per_geom), ("per_inst", per_inst)):
        if floor is not None:
            assert c[key] >= floor, (key, c)


# ---- 2. degenerate rays -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", TOP)
def test_degenerate_rays_on_quads_and_motion_blur_meshes(rtc, po, bomberman, what, mode):
    """er.edge_rays over the mesh's bounds (n_grid 70 on the 727 static quads, 24 over both steps of the two-step meshes, times cycling
    through 0, 1/4, 1/2, 3/4, 1).  Oracle, both modes alike: static quads 12 437 hits of 38 400 rays; motion-blur triangles / quads
    1 877 of 12 456, at least 357 per time."""
    data = er.top_data(what, bomberman)
    rays = er.top_edge_rays(rtc, what, data)
    want, isb = er.top_oracle(rtc, po, what, data, rays, mode)
    if what == "quads":
        assert len(rays) == 38_400
        _floors(want, rays, 12_437)  # oracle: 12 437
    else:
        assert len(rays) == 12_456
        _floors(want, rays, 1_877, per_time=100)  # oracle: 1 877, 357 at the least populated time
    dev, sc = er.top_scene(rtc, what, mode, data)
    _parity(rtc, sc, rays, want, isb, mode, f"degenerate rays, {what}, mode {mode}", what != "tri.mb", nonplanar=er.top_nonplanar(what, data))
    assert dev.error() == 0
    sc.release()
    dev.release()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("which", ["exact", "grid"])
def test_degenerate_rays_on_instances(rtc, po, bomberman, which, mode):
    """imm.scenes_c (static and motion-blur triangles and quads, geomIDs 3 / 5 / 7 / 9) under (exact) six moving instances - signed axis
    permutations times power-of-two scales: axis-parallel world rays become axis-parallel local rays along OTHER axes - and (grid) nine
    static ones; er.edge_rays(n_grid 40, snapped) over the integer box of all instances over all steps, times k / 4; the local rays are
    exact in fp32 (oracle_instances asserts it).  Oracle, both modes alike: (exact) 6 240 hits of 14 100 rays, at least 1 031 per
    geomID, 1 221 per time, 121 per instance; (grid) 7 435 hits, at least 1 433 per geomID, 1 416 per time - and 79 on the least hit
    instance (instance 6, half size, behind its neighbours; 71 - 79 for other seeds): a floor of 100 per instance is not reachable
    there, the floor is half of the measured count."""
    scenes = imm.scenes_c(bomberman)
    inst = er.instance_sets(which)
    rays = er.instance_edge_rays(rtc, scenes, inst)
    assert len(rays) == 14_100
    want, per, isb, _ = imm.oracle_instances(rtc, po, scenes, inst, rays, mode, exact=True)
    assert ih.equal_t_ties(per) == 0
    if which == "exact":
        _floors(want, rays, 6_240, per_time=100, per_geom=100, per_inst=100, gids=(3, 5, 7, 9), n_inst=6)  # oracle: 6 240; 1 221; 1 031; 121
    else:
        _floors(want, rays, 7_435, per_time=100, per_geom=100, per_inst=39, gids=(3, 5, 7, 9), n_inst=9)  # oracle: 7 435; 1 416; 1 433; 79
    dev, top, inner = imm.build(rtc, mode, scenes, inst)
    assert top.stats()["accelKind"] == imm.kind(mode)
    _parity(rtc, top, rays, want, isb, mode, f"degenerate rays, {which} instances, mode {mode}", True, imm.quad_gids(scenes), er.instance_nonplanar(scenes))
    assert dev.error() == 0
    iq.release(dev, top, inner)


# ---- the tie on the diagonal, closed form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("shape", ["unit", "bent"])
def test_rays_through_the_diagonal_take_triangle_a(rtc, po, shape, moving, mode):
    """One quad, planar (the unit square) or not (er.BENT), static or with two identical time steps; 64 rays exactly through its v1-v3
    diagonal, v1 and v3 among them, axis-parallel and oblique.  Expected: the oracle's block entry points on A = (v0, v1, v3) and
    B = (v2, v1, v3) with the select_min rule - smaller t, on equal t the lowest lane, i.e. A.  Oracle: all 64 rays hit, on all 64 the
    two t are bit-identical (so the "either candidate" escape of test_block_semantics_against_the_oracle_blocks for t within ulps
    covers none of them); on the non-planar quad B's normal differs and preferring B fails (test_host_edge_rays.py)."""
    quad = er.UNIT if shape == "unit" else er.BENT
    org, dirs = er.diagonal_rays(quad)
    want, other, tie, near, isb = er.diagonal_expected(rtc, po, quad, org, dirs, mode)
    assert (want["geomID"] == 0).all() and int(tie.sum()) >= 32 and not isb[tie].any()  # oracle: 64 hits, 64 ties
    if moving:
        dev, sc = er.top_scene(rtc, "quad.mb", mode, ([quad, quad.copy()], er.Q1))
    else:
        dev, sc = er.top_scene(rtc, "quads", mode, (quad, er.Q1))
    rays = iq.copy(rtc, want)
    for f in ("geomID", "primID", "instID"):
        rays[f] = INVALID
    for f in ("Ng_x", "Ng_y", "Ng_z", "u", "v"):
        rays[f] = 0
    rays["tfar"] = np.inf
    if moving:
        er.with_times(rays, (0.0, 0.3, 0.5, 1.0))
        want["time"] = other["time"] = rays["time"]
    got = iq.copy(rtc, rays)
    sc.intersect1M(got)
    print(f"{shape} quad, moving {moving}, mode {mode}: {int((got['geomID'] != INVALID).sum())} hits, {int(tie.sum())} exact ties, {int(near.sum())} within ulps")
    # t within ulps but not equal: the oracle's rcp may rank A and B the other way - either candidate, as the block test does
    for i in np.nonzero(near)[0]:
        d = [np.abs(np.array([got[f][i] - w[f][i] for f in ("Ng_x", "Ng_y", "Ng_z")], np.float64)).max() for w in (want, other)]
        if d[1] < d[0]:
            want[i], isb[i] = other[i], not isb[i]
    if mode == 1:  # Moeller B-lane u / v (deep_stack_helpers.quad_allowances)
        for f in ("u", "v"):
            assert np.all(np.abs(got[f][isb].astype(np.float64) - want[f][isb]) <= 4e-7 + 1e-4 * np.abs(want[f][isb]))
            want[f][isb] = got[f][isb]
    compare_hits(got, want, 1e-4, f"{shape} quad diagonal")
    occ = iq.occ_of(rtc, rays)
    sc.occluded1M(occ)
    assert occ.tobytes() == er.occluded_expected(rtc, rays, want).tobytes()
    sc.release()
    dev.release()


# ---- 3. rays that start on the surface -------------------------------------------------------------------------------------------------------
def _as_rayhits(rtc, sh):
    """the RAY records `sh` as RAYHIT records, for the oracle's intersect entry point: a shadow ray is occluded iff it hits"""
    full = rtc.aligned_rayhits(len(sh))
    fill_rays(full, np.zeros((len(sh), 3), np.float32), np.zeros((len(sh), 3), np.float32))
    for f in sh.dtype.names:
        full[f] = sh[f]
    return full


def _surface_floors(want, wsh, what):
    hit = want["geomID"] != INVALID
    near = int((hit & (want["tfar"] < 0.01)).sum())
    occl = int((wsh["geomID"] != INVALID).sum())
    print(f"{what}: oracle {int(hit.sum())} hits of {len(want)} secondary rays, {near} at t < 0.01, {occl} shadow rays occluded")
    assert 0 < int(hit.sum()) < len(want)
    assert near >= 20
    assert 0 < occl < len(wsh)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", TOP)
def test_surface_origin_rays_on_quads_and_motion_blur_meshes(rtc, po, bomberman, what, mode):
    """Bounce and shadow rays (tnear 0.001, the primary's time, origins snapped: up to 2^-11 off the surface) from the ORACLE's hits of
    200 000 random primaries.  Oracle, mode 0: static quads 45 479 secondaries, 3 199 hits, 327 at t < 0.01, 3 764 occluded;
    motion-blur triangles 25 547 / 2 089 / 163 / 2 600; motion-blur quads 25 546 / 2 065 / 169 / 2 620."""
    data = er.top_data(what, bomberman)
    lo, hi = er.top_bounds(what, data)
    prim = er.top_primaries(rtc, po, what, data)
    pw, _ = er.top_oracle(rtc, po, what, data, prim, mode)
    sec, sh = er.bounce(rtc, pw, 11, snapped=True, light=er.light_of(lo, hi))
    assert len(sec) > 20_000  # oracle: 45 479 / 25 547 / 25 546
    want, isb = er.top_oracle(rtc, po, what, data, sec, mode)
    shfull = _as_rayhits(rtc, sh)
    wsh = er.top_oracle(rtc, po, what, data, shfull, mode)[0]
    _surface_floors(want, wsh, f"surface rays, {what}, mode {mode}")
    if what != "quads":
        assert er.counts(want, sec)["per_time"] >= 100  # oracle: 376 at the least
    dev, sc = er.top_scene(rtc, what, mode, data)
    hit = want["geomID"] != INVALID
    got = iq.copy(rtc, sec)
    sc.intersect1M(got)
    print(f"surface rays, {what}, mode {mode}: GPU {int((got['geomID'] != INVALID).sum())} hits, {int(((got['geomID'] != INVALID) & (got['tfar'] < 0.01)).sum())} at t < 0.01")
    if what != "tri.mb":
        ds.quad_allowances(got, want, isb, mode, nonplanar=er.top_nonplanar(what, data))
    compare_hits(got, want, 1e-4, f"secondary {what}")
    assert hit.any()
    occ = iq.occ_of(rtc, sh)
    sc.occluded1M(occ)
    assert occ.tobytes() == er.occluded_expected(rtc, shfull, wsh).tobytes()
    assert dev.error() == 0
    sc.release()
    dev.release()


def _instance_surface_case(rtc, po, bomberman, which, mode):
    scenes = imm.scenes_c(bomberman)
    inst = er.instance_sets(which)
    exact = which == "grid"
    lo, hi = er.instance_box(scenes, inst)
    prim = imm.rays_with_times(rtc, po, scenes, inst, 20_000, 53, snapped=exact, denom=4)
    pw = imm.oracle_instances(rtc, po, scenes, inst, prim, mode, exact=exact)[0]
    sec, sh = er.bounce(rtc, pw, 11, snapped=True, light=er.light_of(lo, hi))
    want, per, isb, want_tri = imm.oracle_instances(rtc, po, scenes, inst, sec, mode, exact=exact)
    shfull = _as_rayhits(rtc, sh)
    wsh, psh, _, wsh_tri = imm.oracle_instances(rtc, po, scenes, inst, shfull, mode, exact=exact)
    return scenes, inst, sec, sh, shfull, (want, per, isb, want_tri), (wsh, psh, wsh_tri)


@pytest.mark.parametrize("mode", [0, 1])
def test_surface_origin_rays_on_grid_instances(rtc, po, bomberman, mode):
    """imm.scenes_c under the nine static iq.grid_instances: bounce and shadow rays from the oracle's hits of 20 000 snapped primaries,
    origins snapped - the exact leg.  Oracle: 15 006 secondaries, 8 077 hits, 210 at t < 0.01, 9 965 shadow rays occluded."""
    scenes, inst, sec, sh, shfull, (want, per, isb, _), (wsh, _, _) = _instance_surface_case(rtc, po, bomberman, "grid", mode)
    assert len(sec) > 7_000 and ih.equal_t_ties(per) == 0  # oracle: 15 006
    _surface_floors(want, wsh, f"surface rays, grid instances, mode {mode}")
    dev, top, inner = imm.build(rtc, mode, scenes, inst)
    got = iq.copy(rtc, sec)
    top.intersect1M(got)
    print(f"surface rays, grid instances, mode {mode}: GPU {int((got['geomID'] != INVALID).sum())} hits")
    ds.quad_allowances(got, want, isb, mode, imm.quad_gids(scenes), er.instance_nonplanar(scenes))
    compare_hits(got, want, 1e-4, "secondary, grid instances")
    assert (got["instID"][got["geomID"] == INVALID] == INVALID).all()
    occ = iq.occ_of(rtc, sh)
    top.occluded1M(occ)
    assert occ.tobytes() == er.occluded_expected(rtc, shfull, wsh).tobytes()
    assert dev.error() == 0
    iq.release(dev, top, inner)


@pytest.mark.parametrize("mode", [0, 1])
def test_surface_origin_rays_on_general_instances(rtc, po, bomberman, mode):
    """The same under im.general_instances() (rotations, non-uniform scales, moving): tolerance territory, with the set-aside of
    test_general_transforms (iq.quad_set_aside: within 1e-4 of an edge or of a quad's diagonal, or a second instance within 1e-4 in t)
    and its cap of 2 %.  Oracle: 10 587 secondaries, 5 464 hits, 1 054 at t < 0.01, 6 043 occluded; 2 bounce and 2 shadow rays set
    aside."""
    scenes, inst, sec, sh, shfull, (want, per, isb, want_tri), (wsh, psh, wsh_tri) = _instance_surface_case(rtc, po, bomberman, "general", mode)
    gids = imm.quad_gids(scenes)
    aside, aside_sh = iq.quad_set_aside(want, per, want_tri, gids), iq.quad_set_aside(wsh, psh, wsh_tri, gids)
    print(f"surface rays, general instances, mode {mode}: {int(aside.sum())} bounce and {int(aside_sh.sum())} shadow rays set aside")
    assert len(sec) > 5_000 and aside.sum() <= 0.02 * len(sec) and aside_sh.sum() <= 0.02 * len(sh)  # oracle: 10 587; 2; 2
    _surface_floors(want, wsh, f"surface rays, general instances, mode {mode}")
    dev, top, inner = imm.build(rtc, mode, scenes, inst)
    got = iq.copy(rtc, sec)
    top.intersect1M(got)
    print(f"surface rays, general instances, mode {mode}: GPU {int((got['geomID'] != INVALID).sum())} hits")
    keep = ~aside
    if mode == 1:  # Moeller B-lane u / v, as test_general_transforms
        b = isb & keep & (got["geomID"] != INVALID)
        for f in ("u", "v"):
            assert np.all(np.abs(got[f][b].astype(np.float64) - want[f][b]) <= 4e-7 + 1e-4 * np.abs(want[f][b]))
            want[f][b] = got[f][b]
    compare_hits(got[keep], want[keep], 1e-4, "secondary, general instances")
    for k in np.nonzero(aside)[0]:  # a ray set aside is still a miss, or a hit within 1e-4 in t of SOME instance's oracle hit
        if got["geomID"][k] == INVALID:
            assert got["tfar"][k] == sec["tfar"][k]
            continue
        ts = [float(p["tfar"][k]) for p in per if p["geomID"][k] != INVALID]
        assert any(abs(float(got["tfar"][k]) - t) <= 1e-4 * abs(t) for t in ts), (k, got[k], ts)
    occ = iq.occ_of(rtc, sh)
    top.occluded1M(occ)
    keep = ~aside_sh
    assert occ[keep].tobytes() == er.occluded_expected(rtc, shfull, wsh)[keep].tobytes()
    assert dev.error() == 0
    iq.release(dev, top, inner)


# ---- 4. invalid rays leave their batch-mates alone ----------------------------------------------------------------------------------------------
INVALID_SCENES = ["quads", "tri.mb", "quad.mb", "inst.grid", "inst.exact", "inst.tri"]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", INVALID_SCENES)
def test_invalid_rays_leave_the_others_alone(rtc, po, bomberman, what, mode):
    """test_invalid_rays_terminate_and_leave_the_others_alone of test_gpu_degenerate_rays.py, at its size: 40 000 rays, ten of them
    poisoned - NaN / infinite origin, direction, tnear, tfar and, on the scenes that read it, time = NaN, +inf, -3, 7.  The other records
    must be byte for byte those of the clean batch.  What a poisoned ray reports itself is not checked.  Why it cannot fault: the module
    docstring."""
    if what in TOP:
        data = er.top_data(what, bomberman)
        dev, sc = er.top_scene(rtc, what, mode, data)
        lo, hi = er.top_bounds(what, data)
    elif what == "inst.tri":
        scenes, inst = er.single_tri_instance(bomberman)
        dev, sc, inner = iq.build(rtc, mode, scenes, inst)
        assert sc.stats()["accelKind"] == (ih.ACCEL_INST_TRI_PLUECKER if mode == 0 else ih.ACCEL_INST_TRI_MOELLER)
        lo, hi = ih.instances_bounds(iq.bounds_meshes(scenes), inst)
    else:
        scenes = imm.scenes_c(bomberman)
        inst = er.instance_sets(what[5:])
        dev, sc, inner = imm.build(rtc, mode, scenes, inst)
        assert sc.stats()["accelKind"] == imm.kind(mode)
        lo, hi = er.instance_box(scenes, inst)
    timed = what not in ("quads", "inst.tri")
    n = 40_000
    clean = rtc.aligned_rayhits(n)
    clean[:] = po.make_random_rays(n, np.asarray(lo, np.float32), np.asarray(hi, np.float32), seed=91)
    if timed:
        er.with_times(clean)
    want = iq.copy(rtc, clean)
    sc.intersect1M(want)
    nh = int((want["geomID"] != INVALID).sum())
    print(f"invalid rays, {what}, mode {mode}: {nh} hits of the clean batch")
    assert nh > 1000
    bad = np.arange(100, n, 4001)  # ten rays
    fields = ["org_x", "dir_y", "tnear", "tfar", "dir_z", "org_z"]
    values = [np.nan, np.nan, np.nan, np.nan, np.inf, -np.inf]
    if timed:
        fields, values = fields + ["time"] * 4, values + [np.nan, np.inf, -3.0, 7.0]
    assert len(bad) == 10

    def poison(recs):
        for k, i in enumerate(bad):
            recs[fields[k % len(fields)]][i] = values[k % len(fields)]

    dirty = iq.copy(rtc, clean)
    poison(dirty)
    dirty["dir_x"][bad[-1]] = dirty["dir_y"][bad[-1]] = dirty["dir_z"][bad[-1]] = 0.0  # null direction
    sc.intersect1M(dirty)
    keep = np.ones(n, bool)
    keep[bad] = False
    assert dirty[keep].tobytes() == want[keep].tobytes()
    wocc = iq.occ_of(rtc, clean)
    sc.occluded1M(wocc)
    occ = iq.occ_of(rtc, clean)
    poison(occ)
    sc.occluded1M(occ)
    assert occ[keep].tobytes() == wocc[keep].tobytes()
    assert int((wocc["tfar"] == -np.inf).sum()) == nh
    assert dev.error() == 0
    if what in TOP:
        sc.release()
        dev.release()
    else:
        iq.release(dev, sc, inner)
