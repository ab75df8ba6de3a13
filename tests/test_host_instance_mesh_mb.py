"""CPU tests of instanced scenes that hold triangle and quad meshes with time steps (accel kinds 22 / 23) on a
`gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,inst_accel=default` device: when the kinds are chosen, that
static-only scenes keep the kinds 14..21 and their bytes, the layout as accel.h documents it, the stack bound, and what stays refused."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import instance_quads_helpers as iq
from helpers import random_soup
from instance_helpers import EMPTY, INST_DT, LEAF, NODE_DT, TRI_DT

CFG = "gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,inst_accel=default"
CFG_STATIC = "gpu=none,quad_accel=default,inst_accel=default"
ERRFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)
NEW_LIMIT = "triangle and quad meshes only (no subdivision meshes or instances)"


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 0. the build -----------------------------------------------------------------------------------------------------------------------------
def test_the_eight_new_kernel_instantiations_are_present_without_scratch_and_within_their_wave_bound():
    """trace_instance_mesh_mb_kernel<PLUECKER, OCCLUDED, VEC>: any hit 4 waves per SIMD (at most 128 VGPRs), closest-hit Moeller 3 (168),
    closest-hit Pluecker 2 (256); none fewer than 2"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_metadata import kernel_metadata
    md = {n: r for n, r in kernel_metadata(os.path.join(ROOT, "embree-compressed_amd", "lib", "libembree3.so")).items() if n.startswith("trace_instance_mesh_mb_kernel<")}
    caps = {}
    for pluecker, occluded, vec in itertools.product((False, True), repeat=3):
        n = "trace_instance_mesh_mb_kernel<%s>" % ", ".join(str(b).lower() for b in (pluecker, occluded, vec))
        caps[n] = 128 if occluded else (256 if pluecker else 168)
    assert sorted(md) == sorted(caps)
    bad = [(n, md[n]["vgpr"], md[n]["agpr"], md[n]["scratch"]) for n, cap in caps.items() if md[n]["scratch"] != 0 or md[n]["vgpr"] + md[n]["agpr"] > cap]
    assert not bad, bad


class Errors:
    """the messages the device reports through rtcSetDeviceErrorFunction"""

    def __init__(self, dev):
        self.log = []
        self.fn = ERRFN(lambda user, code, msg: self.log.append((code, (msg or b"").decode())))
        dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(self.fn, C.c_void_p), None)
        self.dev = dev

    def expect(self, code, text):
        assert self.dev.error() == code, self.log
        assert self.log and self.log[-1][0] == code and text in self.log[-1][1], self.log
        self.log.clear()


def _random_quads(n, seed):
    rng = np.random.RandomState(seed)
    c = rng.rand(n, 1, 3) * 10.0
    base = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]], np.float64)
    v = (c + base + (rng.rand(n, 4, 3) - 0.5) * 0.2).reshape(-1, 3).astype(np.float32)
    return v, np.arange(4 * n, dtype=np.uint32).reshape(-1, 4)


def _moved(v, nsteps, seed):
    rng = np.random.RandomState(seed)
    shift = rng.rand(3).astype(np.float32) * 0.5
    return [(v + k * shift).astype(np.float32) for k in range(nsteps)]


def _desc(nt=0, ntm=0, nq=0, nqm=0, seed=3, steps=2):
    """an instanced scene with nt static triangles (geomID 0), ntm moving ones (1), nq static quads (2), nqm moving ones (3)"""
    d = imm.desc()
    if nt:
        v, t = random_soup(nt, seed)
        d["tris"] = (v, t, 0)
    if ntm:
        v, t = random_soup(ntm, seed + 1)
        d["tris_mb"] = (_moved(v, steps, seed + 1), t, 1)
    if nq:
        v, q = _random_quads(nq, seed + 2)
        d["quads"] = (v, q, 2)
    if nqm:
        v, q = _random_quads(nqm, seed + 3)
        d["quads_mb"] = (_moved(v, steps + 1, seed + 3), q, 3)
    return d


def _top(rtc, dev, inner, uses, flags=0, moving=()):
    top = rtc.Scene(dev, flags)
    ids = {}
    for i, k in enumerate(uses):
        m = ih.affine((30.0 * i, 0, 0))
        if i in moving:
            ids[top.add_instance_mb(inner[k], [m, ih.affine((30.0 * i, 1.0, 0)), ih.affine((30.0 * i, 2.0, 0.5))])] = k
        else:
            ids[top.add_instance(inner[k], m)] = k
    top.commit()
    return top, ids


# ---- 1. kinds -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(0, 20, 0, 0), (0, 0, 0, 20), (16, 20, 0, 0), (16, 0, 12, 20), (16, 20, 12, 20)])
def test_kinds_22_23_are_chosen_when_an_instanced_scene_has_a_motion_blur_accel(rtc, mode, shape):
    dev = rtc.Device(CFG)
    inner = {"a": imm.add_scene(rtc, dev, _desc(*shape), mode), "s": imm.add_scene(rtc, dev, _desc(16, 0, 12, 0, seed=9), mode)}
    top, _ = _top(rtc, dev, inner, "sas", iq.flags(mode))
    assert top.stats()["accelKind"] == imm.kind(mode) and top.stats()["leafCount"] == 3
    top.release()
    # without the moving scene: the static kinds
    top, _ = _top(rtc, dev, inner, "ss", iq.flags(mode))
    assert top.stats()["accelKind"] == (iq.ACCEL_INST_PLUECKER if mode == 0 else iq.ACCEL_INST_MOELLER)
    top.release()
    for s in inner.values():
        s.release()
    dev.release()


# ---- 2. static-only top scenes: kinds 14..21, the same bytes as without the two *_mb keys -------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("quads,moving", [(False, False), (True, False), (False, True), (True, True)])
def test_static_only_scenes_keep_their_kind_and_every_byte(rtc, mode, quads, moving):
    got = []
    for cfg in (CFG, CFG_STATIC):
        dev = rtc.Device(cfg)
        inner = {"a": imm.add_scene(rtc, dev, _desc(40, 0, 24 if quads else 0, 0), mode), "b": imm.add_scene(rtc, dev, _desc(24, 0, 0, 0, seed=5), mode)}
        top, _ = _top(rtc, dev, inner, "abab", iq.flags(mode), moving=(1, 2) if moving else ())
        st = top.stats()
        got.append((st["accelKind"], top.accel_root(), st["maxDepth"], [top.accel_data(k).tobytes() for k in range(4)]))
        top.release()
        for s in inner.values():
            s.release()
        dev.release()
    assert got[0][0] == (im.kind(mode, quads) if moving else im.static_kind(mode, quads))
    assert got[0] == got[1]


# ---- 3. layout ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_accel_arrays_decode_per_the_documented_layout(rtc, mode):
    # a: all four trees, 5 instances (one of them moving); b: MB quads only; c: static triangles + MB triangles; d: static quads only
    shapes = {"a": (40, 30, 24, 20, 3), "b": (0, 0, 0, 36, 13), "c": (28, 44, 0, 0, 23), "d": (0, 0, 32, 0, 33)}
    descs = {k: _desc(*s[:4], seed=s[4]) for k, s in shapes.items()}
    own = {k: imm.own_accels(rtc, CFG, d, mode) for k, d in descs.items()}
    dev = rtc.Device(CFG)
    inner = {k: imm.add_scene(rtc, dev, d, mode) for k, d in descs.items()}
    uses = "abacadaa"  # first use: a, b, c, d; a is shared by 5 instances
    top, ids = _top(rtc, dev, inner, uses, iq.flags(mode), moving=(2,))
    assert top.stats()["accelKind"] == imm.kind(mode)
    n = len(uses)
    nodes, prims, blobs = top.accel_data(0).view(NODE_DT), top.accel_data(1).view(TRI_DT), top.accel_data(2)
    order = "abcd"
    cat = lambda part: b"".join(own[k][part][1].tobytes() for k in order if own[k][part] is not None)  # noqa: E731
    count = lambda part: sum(len(own[k][part][1]) for k in order if own[k][part] is not None)  # noqa: E731
    recs, quads, steps, scenes, trimb, quadmb, t_off, q_off = imm.split_blobs(blobs, n, count("quads"), 3, 4, count("tris_mb"), count("quads_mb"))
    # every distinct scene once (a is used 5 times), in the order of first use; the records are the source accels' records, byte for byte
    assert prims.tobytes() == cat("tris") and quads.tobytes() == cat("quads")
    assert trimb.tobytes() == cat("tris_mb") and quadmb.tobytes() == cat("quads_mb")
    assert len(trimb) == 30 + 44 and len(quadmb) == 20 * 2 + 36 * 2  # one record per primitive and segment (quads: three steps)
    assert t_off % 96 == 0 and q_off % 128 == 0
    assert not scenes["pad"].any()
    # the instance records name their scene's record; the moving instance its steps
    scene_base = n + len(quads) + len(steps)
    assert sorted(recs["geomID"].tolist()) == sorted(ids)
    for r in recs:
        assert int(r["root"]) - scene_base == order.index(ids[int(r["geomID"])]) and r["pad"][0] == 0
    mv = recs[recs["pad"][:, 1] != 0]
    assert len(mv) == 1 and ids[int(mv[0]["geomID"])] == "a" and int(mv[0]["pad"][1]) == (2 << 24) | (n + len(quads))
    # roots: REF_EMPTY for missing trees; every rebased tree decodes to its source records and is a copy of the source nodes
    bases = {"tris": 0, "quads": n, "tris_mb": t_off // 96, "quads_mb": q_off // 128}
    totals = {"tris": len(prims), "quads": n + len(quads), "tris_mb": t_off // 96 + len(trimb), "quads_mb": q_off // 128 + len(quadmb)}
    fields = {"tris": "triRoot", "tris_mb": "triMBRoot", "quads": "quadRoot", "quads_mb": "quadMBRoot"}
    node_ranges = []
    for si, k in enumerate(order):
        for part in imm.PARTS:  # Scene::commit's order
            root = int(scenes[si][fields[part]])
            o = own[k][part]
            assert (root == EMPTY) == (o is None), (k, part)
            if o is None:
                continue
            assert not (root & LEAF and (root >> 26) & 31 == 0)  # no root looks like a marker
            onodes, orecs, oroot, _ = o
            base = bases[part]
            got, _ = imm.walk(nodes, root)
            want, _ = imm.walk(onodes, oroot)
            assert sorted(got) == sorted((f + base, c) for f, c in want)
            assert all(base <= f and f + c <= base + len(orecs) <= totals[part] for f, c in got)
            assert sum(c for _, c in got) == len(orecs)
            bases[part] += len(orecs)
            if not root & LEAF:
                nb = root - oroot
                node_ranges.append((nb, nb + len(onodes)))
                for a, b in zip(nodes[nb:nb + len(onodes)], onodes):
                    assert a["origin"].tobytes() == b["origin"].tobytes() and a["exp"].tobytes() == b["exp"].tobytes() and a["q"].tobytes() == b["q"].tobytes()
                    for ca, cb in zip(a["child"].tolist(), b["child"].tolist()):
                        assert ca == (cb if cb == EMPTY else (cb + base if cb & LEAF else cb + nb))
    # top-level tree first, then per scene triangle, MB triangle, quad, MB quad nodes, in that order and without gaps
    assert node_ranges == sorted(node_ranges) and node_ranges[-1][1] == len(nodes)
    assert all(a[1] == b[0] for a, b in zip(node_ranges, node_ranges[1:]))
    leaves, _ = imm.walk(nodes[:node_ranges[0][0]], top.accel_root())
    assert sorted(f for f, _ in leaves) == list(range(n)) and all(c == 1 for _, c in leaves)
    assert top.stats()["totalBytes"] == len(nodes) * 96 + len(prims) * 48 + len(blobs)
    top.release()
    for s in inner.values():
        s.release()
    dev.release()


# ---- 4. stack bound ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,trees", [((0, 0, 0, 1500), 1), ((8, 1500, 0, 0), 2), ((8, 0, 40, 1500), 3), ((8, 1500, 40, 700), 4)])
def test_max_depth_equals_the_formula(rtc, shape, trees):
    """maxDepth = top-level depth + 1 (exit marker) + the most pending-tree markers of any scene (its trees - 1) + the deepest tree"""
    d = _desc(*shape, seed=9)
    own = imm.own_accels(rtc, CFG, d, 1)
    deepest = max(o[3] for o in own.values() if o is not None)
    assert deepest >= 2
    dev = rtc.Device(CFG)
    inner = {"a": imm.add_scene(rtc, dev, d, 1), "one": imm.add_scene(rtc, dev, _desc(0, 4, 0, 0, seed=1), 1)}
    top = rtc.Scene(dev)
    for i in range(20):
        top.add_instance(inner["a"], ih.affine((12.0 * i, 0, 0)))
    top.add_instance(inner["one"], ih.affine((0, 40.0, 0)))  # a scene with fewer trees does not lower the bound
    top.commit()
    nodes = top.accel_data(0).view(NODE_DT)
    scenes = imm.split_blobs(top.accel_data(2), 21, shape[2], 0, 2, shape[1] + 4, 2 * shape[3])[3]
    first_inner = min(int(sc[f]) for sc in scenes for f, _ in imm.VISIT if sc[f] != EMPTY and not sc[f] & LEAF)  # the top-level tree ends here
    _, top_levels = imm.walk(nodes[:first_inner], top.accel_root())
    assert top_levels >= 2
    assert top.stats()["maxDepth"] == top_levels + 1 + (trees - 1) + deepest
    top.release()
    for s in inner.values():
        s.release()
    dev.release()


def test_a_walk_of_four_trees_stays_within_the_stack_capacity_and_passes_slot_16_under_markers(rtc):
    """imm.deep_scene() - needle soups (deep_stack_helpers) in all four trees of one instanced scene - under deep_instances(): the CPU
    walk of the exported arrays, with the tree markers, never writes a slot beyond stack_capacity(maxDepth), has three markers stacked
    at once, and - the precondition of the GPU test of the overflow area - at least 10 % of the 300 rays write a slot beyond the 16 in
    LDS, that is into HBM, while at least one tree marker is stacked.  (The markers themselves lie right above the few top-level
    entries, below slot 16; what the GPU test needs is that entries above them go to HBM and come back before a marker is popped.)
    Measured: printed by this test."""
    scenes = imm.deep_scene()
    inst = [(g, k, [m]) for g, k, m in ds.deep_instances()]
    dev, top, inner = imm.build(rtc, 1, scenes, inst, CFG)
    st = top.stats()
    assert st["accelKind"] == imm.ACCEL_INSTMESHMB_MOELLER
    lo, hi = ds.instance_ray_box({"m": {"tris": scenes["m"]["tris"], "quads": scenes["m"]["quads"]}}, ds.deep_instances())
    rng = np.random.RandomState(ds.HOST_RAY_SEED)
    org = lo + rng.rand(ds.HOST_RAYS, 3) * (hi - lo)
    dirs = rng.randn(ds.HOST_RAYS, 3)
    times = np.asarray(ds.TIMES)[np.arange(ds.HOST_RAYS) % len(ds.TIMES)]
    n = imm.DEEP_N
    w = imm.WalkInstances(top, 3, (n, 0, 1, n, n), pluecker=False)
    deepest, markers, marked, _ = imm.simulate_stack(top.accel_data(0).view(NODE_DT), top.accel_root(), org, dirs, times, w)
    share = float((marked >= ds.LDS_STACK).mean())
    print(f"deepest slot {deepest.max()} of {ds.stack_capacity(st['maxDepth'])}, most markers {markers.max()}, "
          f"{100 * share:.1f} % of the rays pass slot {ds.LDS_STACK} with a marker stacked")
    assert deepest.max() < ds.stack_capacity(st["maxDepth"])
    assert markers.max() == 3
    assert share >= 0.10
    iq.release(dev, top, inner)


def test_tree_markers_themselves_reach_the_overflow_area_under_a_deep_top_level(rtc):
    """imm.marker_spill_case(): 128 instances with nearly coinciding bounds.  The precondition of the GPU test of markers in HBM: for at
    least 10 % of 100 rays a tree marker is written to a slot beyond the 16 in LDS (pushed to the overflow column and popped from it
    with the tree's root in the distance word), and no ray writes beyond stack_capacity(maxDepth).  Measured: printed by this test."""
    scenes, inst = imm.marker_spill_case()
    dev, top, inner = imm.build(rtc, 1, scenes, inst, CFG)
    st = top.stats()
    assert st["accelKind"] == imm.ACCEL_INSTMESHMB_MOELLER
    rays = imm.marker_spill_rays(rtc, 100, ds.HOST_RAY_SEED)
    org = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1)
    dirs = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1)
    n = imm.MARKER_N
    w = imm.WalkInstances(top, len(inst), (n, 0, 1, n, n), pluecker=False)
    deepest, markers, _, marker_slot = imm.simulate_stack(top.accel_data(0).view(NODE_DT), top.accel_root(), org, dirs, rays["time"], w)
    share = float((marker_slot >= ds.LDS_STACK).mean())
    print(f"deepest slot {deepest.max()} of {ds.stack_capacity(st['maxDepth'])}, highest marker slot {marker_slot.max()}, "
          f"{100 * share:.1f} % of the rays write a tree marker beyond slot {ds.LDS_STACK}")
    assert deepest.max() < ds.stack_capacity(st["maxDepth"]) and markers.max() == 3
    assert share >= 0.10
    iq.release(dev, top, inner)


# ---- 4b. the pinned inputs of the general-transform GPU test ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_general_transform_inputs_set_aside_at_most_two_percent(rtc, po, bomberman, mode):
    """the oracle alone, for the pinned seed: rays within 1e-4 of an edge, of a quad's diagonal or of a second instance's hit"""
    _, _, rays, want, _, _, aside = imm.general_case(rtc, po, bomberman, mode, imm.GENERAL_SEED)
    hits = int((want["geomID"] != ih.INVALID).sum())
    print(f"mode {mode}: {hits} hits of {len(rays)} rays, {int(aside.sum())} set aside, hits per geomID {[int((want['geomID'] == g).sum()) for g in (3, 5, 7, 9)]}")
    assert hits > 1000 and aside.sum() <= 0.02 * len(rays)
    assert len(np.unique(rays["time"])) == 9


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def _moving_inner(rtc, dev, flags=0):
    sc = rtc.Scene(dev, flags)
    v, t = random_soup(16, 1)
    g = sc.add_triangles_mb(_moved(v, 2, 2), t)
    return sc, g


@pytest.mark.parametrize("cfg", [CFG_STATIC, "gpu=none,quad_accel=default,tri_accel_mb=default,quad_accel_mb=default"])
def test_a_device_without_both_keys_keeps_todays_message_for_time_steps(rtc, cfg):
    dev = rtc.Device(cfg)
    err = Errors(dev)
    sc, _ = _moving_inner(rtc, dev)
    sc.commit()
    top = rtc.Scene(dev)
    top.add_instance(sc)
    top.lib.rtcCommitScene(top.handle)
    if "inst_accel" in cfg:
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "static triangle and quad meshes only (no time steps, subdivision meshes or instances)")
    else:
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "static triangle meshes only (no quads, time steps, subdivision meshes or instances)")
    top.release()
    sc.release()
    dev.release()


@pytest.mark.parametrize("key", ["tri_accel_mb=default", "quad_accel_mb=default"])
def test_one_of_the_two_mb_keys_beside_inst_accel_is_enough(rtc, key):
    dev = rtc.Device("gpu=none,quad_accel=default,inst_accel=default," + key)
    sc, _ = _moving_inner(rtc, dev)
    sc.commit()
    top = rtc.Scene(dev)
    top.add_instance(sc)
    top.commit()
    assert top.stats()["accelKind"] == imm.ACCEL_INSTMESHMB_MOELLER
    top.release()
    sc.release()
    dev.release()


@pytest.mark.parametrize("what", ["subdivision", "instances"])
def test_subdivision_and_nested_instances_are_refused_with_the_remaining_limit(rtc, bomberman, what):
    dev = rtc.Device(CFG)
    err = Errors(dev)
    sc, _ = _moving_inner(rtc, dev)
    leaf = None
    if what == "subdivision":
        v, fs, fi = bomberman
        sc.add_subdiv(v, fs[:8], fi[:32])
    else:
        leaf = rtc.Scene(dev)
        v, t = random_soup(8, 3)
        leaf.add_triangles(v, t)
        leaf.commit()
        sc.add_instance(leaf)
    sc.commit()
    top = rtc.Scene(dev)
    top.add_instance(sc)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, NEW_LIMIT)
    assert "time steps" not in NEW_LIMIT
    top.release()
    sc.release()
    if leaf:
        leaf.release()
    dev.release()


def test_accels_of_one_top_scene_that_disagree_in_arithmetic_are_refused(rtc):
    # within one scene: a robust scene under an explicit (Moeller) motion-blur accel beside its Pluecker triangles
    dev = rtc.Device(CFG.replace("tri_accel_mb=default", "tri_accel_mb=bvh8.triangle4imb"))
    err = Errors(dev)
    sc = rtc.Scene(dev, iq.ROBUST)
    v, t = random_soup(16, 1)
    sc.add_triangles(v, t)
    sc.add_triangles_mb(_moved(v, 2, 2), t)
    sc.commit()
    top = rtc.Scene(dev, iq.ROBUST)
    top.add_instance(sc)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "disagree in kind (Pluecker / robust: triangle; Moeller / fast: motion blur triangle)")
    top.release()
    sc.release()
    dev.release()
    # across scenes: a robust static scene beside a fast moving one
    dev = rtc.Device(CFG)
    err = Errors(dev)
    a = rtc.Scene(dev, iq.ROBUST)
    a.add_triangles(v, t)
    a.commit()
    b, _ = _moving_inner(rtc, dev, 0)
    b.commit()
    for order in ((a, b), (b, a)):
        top = rtc.Scene(dev)
        for s in order:
            top.add_instance(s)
        top.lib.rtcCommitScene(top.handle)
        err_text = "the instanced scenes of one scene disagree in accel kind (Pluecker / robust and Moeller / fast): the scene of instance 1 has "
        # the message names the accels on either side
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, err_text + ("Moeller / fast accels (motion blur triangle), the scene of instance 0 Pluecker / robust ones (triangle)"
                                                                if order[0] is a else "Pluecker / robust accels (triangle), the scene of instance 0 Moeller / fast ones (motion blur triangle)"))
        top.release()
    a.release()
    b.release()
    dev.release()


def test_a_geometry_filter_on_a_moving_mesh_inside_an_instanced_scene_is_refused(rtc):
    dev = rtc.Device(CFG)
    err = Errors(dev)
    sc, g = _moving_inner(rtc, dev)
    keep = rtc.FILTER_FUNC(lambda args: None)
    sc.set_filters(g, intersect=keep)
    sc.commit()
    top = rtc.Scene(dev)
    top.add_instance(sc)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "geometry filter functions inside an instanced scene are not supported")
    top.release()
    sc.release()
    dev.release()
