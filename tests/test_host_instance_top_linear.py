"""CPU tests of time-dependent top-level boxes for moving instances (device config inst_bounds=linear; accel kinds 32 / 33) on a `gpu=none`
device that names every accel key: the key, when the kinds are chosen and what stays byte for byte what it was, the layout as accel.h
documents it, containment of the moving instances at 33 times, tightness at both ends, how many rays still enter a fast mover, the
stack bound and the refusals.
Not tested: the refusal of a top-level node index that would reach the leaf bit, which takes about 2^31 nodes."""
import ctypes as C

import numpy as np
import pytest

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_mb_helpers as im
import instance_mesh_mb_helpers as imm
import instance_mesh_mb_linear_helpers as iml
import instance_quads_helpers as iq
import instance_top_linear_helpers as itl
from helpers import random_soup
from instance_helpers import EMPTY, LEAF, NODE_DT
from mb_linear_helpers import NODEMB_DT, decode_children_mb, walk_paths

BASE = "gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,inst_accel=default"
LIN = BASE + "," + itl.KEY
ALL = BASE + "," + itl.ALL_KEYS
ERRFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)
NEEDS_LINEAR = ("inst_bounds=linear: a scene with moving instances takes instanced scenes with motion blur meshes only when their accels hold time-dependent nodes "
                "(use mb_bounds=linear,inst_mb_bounds=linear beside inst_bounds=linear, or inst_bounds=swept)")


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


def _moved(v, nsteps, shift=(0.25, 0.5, -0.125)):
    return [(v + k * np.asarray(shift, np.float32)).astype(np.float32) for k in range(nsteps)]


def _mb_scene(seed=5):
    """an instanced scene with static and moving triangles and quads"""
    d = itl.soup_scene(60, 40, seed)
    v, t = random_soup(50, seed + 2)
    d["tris_mb"] = (_moved(ih.snap(v), 2), t, 2)
    v, q = itl.random_quads(30, seed + 3)
    d["quads_mb"] = (_moved(v, 3), q, 3)
    return d


def _export(top):
    st = top.stats()
    return (st["accelKind"], top.accel_root(), st["maxDepth"], st["nodeCount"], st["nodeBytes"], st["leafCount"], st["totalBytes"], [top.accel_data(k).tobytes() for k in range(4)])


MOVING = [(0, "m", [ih.affine((0, 0, 0)), ih.affine((3, 1, 0))]), (1, "m", [ih.affine((30, 0, 0))]), (2, "m", [ih.affine((0, 30, 0)), ih.affine((0, 31, 1)), ih.affine((2, 30, 0))])]
STATIC = [(g, k, s[:1]) for g, k, s in MOVING]
# kinds -> (scene, instances, further keys)
KIND_CASES = {
    (18, 19): (lambda: itl.soup_scene(80, 0), MOVING, ""),
    (20, 21): (lambda: itl.soup_scene(80, 40), MOVING, ""),
    (22, 23): (_mb_scene, MOVING, ""),
    (30, 31): (_mb_scene, MOVING, "," + iml.LINEAR),
}


# ---- 1. the key ---------------------------------------------------------------------------------------------------------------------------------
def test_unknown_inst_bounds_is_an_invalid_argument(rtc):
    with pytest.raises(rtc.RTCError) as e:
        rtc.Device("gpu=none,inst_bounds=bogus")
    assert e.value.code == rtc.RTC_ERROR_INVALID_ARGUMENT
    for ok in ("swept", "linear"):
        rtc.Device("gpu=none,inst_bounds=" + ok).release()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kinds", list(KIND_CASES))
def test_swept_and_the_key_absent_give_the_same_bytes(rtc, mode, kinds):
    make, inst, more = KIND_CASES[kinds]
    got = []
    for cfg in (BASE + more, BASE + more + ",inst_bounds=swept"):
        built = imm.build(rtc, mode, {"m": make()}, inst, cfg)
        got.append(_export(built[1]))
        iq.release(*built)
    assert got[0][0] == kinds[mode]
    assert got[0] == got[1]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kinds", [(14, 15), (16, 17), (22, 23), (30, 31)])
def test_without_a_moving_instance_linear_changes_no_byte(rtc, mode, kinds):
    make, _, more = {(14, 15): KIND_CASES[(18, 19)], (16, 17): KIND_CASES[(20, 21)]}.get(kinds, KIND_CASES.get(kinds))
    got = []
    for cfg in (BASE + more, BASE + more + "," + itl.KEY):
        built = imm.build(rtc, mode, {"m": make()}, STATIC, cfg)
        got.append(_export(built[1]))
        iq.release(*built)
    assert got[0][0] == kinds[mode]
    assert got[0] == got[1]


def test_a_host_only_device_honours_the_key_only_with_inst_accel(rtc):
    """a host-only device takes moving instances at all only when its config names inst_accel=: without it the commit refuses them as
    before, whatever inst_bounds says"""
    dev = rtc.Device("gpu=none,inst_bounds=linear")
    err = Errors(dev)
    sc = rtc.Scene(dev)
    sc.add_triangles(*random_soup(20, 1))
    sc.commit()
    top = rtc.Scene(dev)
    top.add_instance_mb(sc, MOVING[0][2])
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "instances with more than one time step are not supported")
    top.release()
    sc.release()
    dev.release()


# ---- 2. kinds and layout ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["tris", "tris and quads", "two scenes", "one instance"])
def test_kinds_and_layout(rtc, mode, what):
    scenes = {"m": itl.soup_scene(80, 0 if what == "tris" else 40, 3), "n": itl.soup_scene(5, 70, 9)}
    if what == "two scenes":
        inst = [(g, "mn"[g % 2], s if g % 3 else s[:1]) for g, _, s in im.exact_instances(11)]
    else:
        scenes.pop("n")
        inst = MOVING[:1] if what == "one instance" else MOVING
    swept, lin = (imm.build(rtc, mode, scenes, inst, cfg) for cfg in (BASE, LIN))
    top, top_s = lin[1], swept[1]
    st = top.stats()
    assert st["accelKind"] == itl.kind(mode) == (32, 33)[mode] and st["leafCount"] == len(inst) and st["nodeBytes"] == 96
    assert top_s.stats()["accelKind"] in (18, 19, 20, 21)
    # -- the node buffer: QNode8s of the static trees | padding | QNodeMB8s, the top-level tree
    nodes8, image_mb, n_mb, first = iml.split_nodes(top)  # sizes, padding, blobOffsets, statistics
    assert st["totalBytes"] == (first + n_mb) * 144 + len(top.accel_data(1)) + len(top.accel_data(2)) + 8
    _, leaves = itl.top_leaves(top)  # the root and every inner reference name QNodeMB8s of the second section
    assert sorted(r for _, r in leaves) == list(range(len(inst)))  # every instance is reached exactly once
    visited = {n for path, _ in leaves for n, _ in path}
    assert visited == set(range(first, first + n_mb))  # no moving meshes below: the section is the top-level tree
    assert st["maxDepth"] >= max(len(p) for p, _ in leaves) + 1
    # -- blobs: the general layout; records, steps and scene records are the swept build's up to leaf order
    cnt = itl.counts(scenes, inst)
    recs, quads, steps, srecs, trimb, quadmb, _, _ = imm.split_blobs(top.accel_data(2), len(inst), *cnt)
    assert len(trimb) == 0 and len(quadmb) == 0 and not srecs["pad"].any()
    blobs_s = top_s.accel_data(2)
    recs_s = blobs_s[:64 * len(inst)].view(ih.INST_DT)
    steps_s = blobs_s[64 * (len(inst) + cnt[0]):].view(im.STEP_DT)
    assert len(steps_s) == cnt[1] and quads.tobytes() == blobs_s[64 * len(inst):64 * (len(inst) + cnt[0])].tobytes()
    assert top.accel_data(1).tobytes() == top_s.accel_data(1).tobytes()
    by_gid = {int(r["geomID"]): r for r in recs_s}
    used = list(dict.fromkeys(k for _, k, _ in inst))
    scene_base = len(inst) + cnt[0] + cnt[1]
    nodes8_s = top_s.accel_data(0).view(NODE_DT)
    top_nodes_s = len(nodes8_s) - len(nodes8)  # the swept build keeps its top-level tree in front of the same static trees
    assert top_nodes_s >= 0
    shift = lambda r: r if r == EMPTY or r & LEAF else r - top_nodes_s  # noqa: E731
    for r in recs:
        g = int(r["geomID"])
        rs = by_gid[g]
        assert r["world2local"].tobytes() == rs["world2local"].tobytes() and r["pad"][0] == 0
        sc = srecs[int(r["root"]) - scene_base]
        assert int(r["root"]) - scene_base == used.index(dict((i, k) for i, k, _ in inst)[g])
        # the scene record holds what the swept record carries in root / pad[0], moved down by the swept build's top-level nodes
        quad_root_s = int(rs["pad"][0]) if cnt[0] else EMPTY
        assert (int(sc["triRoot"]), int(sc["quadRoot"])) == (shift(int(rs["root"])), shift(quad_root_s)) and int(sc["triMBRoot"]) == int(sc["quadMBRoot"]) == EMPTY
        nst = len(dict((i, s) for i, _, s in inst)[g])
        assert (int(r["pad"][1]) >> 24) == (nst - 1 if nst > 1 else 0) and (int(rs["pad"][1]) >> 24) == (int(r["pad"][1]) >> 24)
        if nst > 1:
            a, b = int(r["pad"][1]) & 0xFFFFFF, int(rs["pad"][1]) & 0xFFFFFF
            own = top.accel_data(2).view(im.STEP_DT)[a:a + nst]
            assert own.tobytes() == blobs_s.view(im.STEP_DT)[b:b + nst].tobytes() and not own["pad"].any()
    # the static trees are the swept build's nodes, inner child indices moved down
    for f in ("origin", "exp", "pad", "q"):
        assert nodes8[f].tobytes() == nodes8_s[top_nodes_s:][f].tobytes(), f
    c = nodes8_s[top_nodes_s:]["child"].astype(np.int64)
    inner_ref = (c != EMPTY) & ((c & LEAF) == 0)
    want = c.copy()
    want[inner_ref] -= top_nodes_s
    assert np.array_equal(nodes8["child"].astype(np.int64), want)
    for b in (swept, lin):
        iq.release(*b)


# ---- 3. containment -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", itl.CASES)
def test_every_box_above_an_instance_holds_it_at_33_times(rtc, mode, what):
    """every root-to-leaf path of the top-level tree, at 33 times in [0, 1] (all step times of 2, 3 and 5 steps among them): the box
    decoded with the kernel's fp32 formula holds the float64 images of the eight corners of the instanced scene's bounds under
    lerp(step[k], step[k + 1], f).  A pair-of-ends guess alone fails (c) and (d): checked on the decoded end boxes."""
    scenes = {"m": itl.soup_scene(60, 30, 7)}
    inst = itl.instances(what)
    steps_of = {g: s for g, _, s in inst}
    dev, top, inner = imm.build(rtc, mode, scenes, inst, LIN)
    assert top.stats()["accelKind"] == itl.kind(mode)
    lo, hi = itl.scene_bounds(scenes["m"])
    image_mb, leaves = itl.top_leaves(top)
    recs = top.accel_data(2)[:64 * len(inst)].view(ih.INST_DT)
    assert sorted(r for _, r in leaves) == list(range(len(inst)))
    checks, bad, ends_alone_fail = 0, [], 0
    for path, rec in leaves:
        steps = steps_of[int(recs[rec]["geomID"])]
        for t in itl.TIMES33:
            p = itl.corners_at(lo, hi, steps, t)
            for blo, bhi in itl.path_boxes(image_mb, path, np.float32(t)):
                checks += 1
                if not ((blo <= p).all() and (p <= bhi).all()):
                    bad.append((rec, float(t), blo, bhi, p.min(0), p.max(0)))
        if len(steps) > 2:  # the lerp of the instance's own end boxes alone would not hold its middle steps
            e0, e1 = itl.corners_at(lo, hi, steps, 0.0), itl.corners_at(lo, hi, steps, 1.0)
            for k in range(1, len(steps) - 1):
                t = k / (len(steps) - 1)
                p = itl.corners_at(lo, hi, steps, t)
                glo, ghi = (1 - t) * e0.min(0) + t * e1.min(0), (1 - t) * e0.max(0) + t * e1.max(0)
                ends_alone_fail += not ((glo <= p.min(0)).all() and (p.max(0) <= ghi).all())
    print(f"({what}) mode {mode}: {len(leaves)} instances, {checks} box checks, deepest path {max(len(p) for p, _ in leaves)}")
    assert not bad, bad[:3]
    assert checks >= 33 * len(inst)
    if what in "cd":
        assert ends_alone_fail >= 1
    if what == "e":
        assert max(len(p) for p, _ in leaves) >= 2  # inner QNodeMB8s below the root
    # times outside [0, 1] and NaN clamp: the box of the nearer end, bit for bit
    for node in {n for path, _ in leaves for n, _ in path}:
        for t, end in ((-0.5, 0.0), (1.5, 1.0), (np.inf, 1.0), (-np.inf, 0.0), (np.nan, 0.0)):
            a, b = decode_children_mb(image_mb[node], t), decode_children_mb(image_mb[node], end)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    iq.release(dev, top, inner)


# ---- 4. tightness ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what", ["a", "b", "e"])
def test_leaf_boxes_are_one_to_two_grid_steps_outside_the_step_boxes(rtc, mode, what):
    """the QNodeMB8 guarantee at t = 0 and t = 1 for the leaf box of every two-step instance (its exact step box: the float64 images of
    the corners); a static instance has equal boxes at both ends"""
    scenes = {"m": itl.soup_scene(60, 30, 7)}
    inst = itl.instances(what)
    steps_of = {g: s for g, _, s in inst}
    dev, top, inner = imm.build(rtc, mode, scenes, inst, LIN)
    lo, hi = itl.scene_bounds(scenes["m"])
    image_mb, leaves = itl.top_leaves(top)
    recs = top.accel_data(2)[:64 * len(inst)].view(ih.INST_DT)
    two_step = static = 0
    for path, rec in leaves:
        steps = steps_of[int(recs[rec]["geomID"])]
        node, slot = path[-1]
        s = (image_mb[node]["exp"].astype(np.uint32) << 23).view(np.float32).astype(np.float64)
        b0, b1 = (decode_children_mb(image_mb[node], t) for t in (0.0, 1.0))
        if len(steps) == 1:
            static += 1
            assert b0[0][slot].tobytes() == b1[0][slot].tobytes() and b0[1][slot].tobytes() == b1[1][slot].tobytes()
        if len(steps) == 2:
            two_step += 1
            for t, (blo, bhi) in ((0.0, b0), (1.0, b1)):
                p = itl.corners_at(lo, hi, steps, t)
                dlo, dhi = (p.min(0) - blo[slot].astype(np.float64)) / s, (bhi[slot].astype(np.float64) - p.max(0)) / s
                assert (dlo >= 1.0).all() and (dlo < 2.0).all() and (dhi >= 1.0).all() and (dhi < 2.0).all(), (rec, t, dlo, dhi)
    assert two_step >= 1 and static >= 1
    iq.release(dev, top, inner)


# ---- 5. fewer entries ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_fast_mover_is_entered_by_a_tenth_of_the_rays_the_swept_box_lets_in(rtc):
    """One unit cube, instanced once, translating by D = 10 edges along x over a two-step shutter; 4096 rays along -z from above, x uniform
    over the swept footprint [0, 11], times uniform in [0, 1].  Counted: the rays whose slab test at their time passes the mover's leaf
    box and every box above it, in the tree under inst_bounds=linear and in the swept tree, each exported from its own device (the swept
    tree of a single instance is its leaf: no box at all, every ray enters).  Geometry: 1 / 11; the quantizer pads by at most two steps
    of 1 / 255 of the node extent per side."""
    c = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = np.array([t for a, b, cc, d in faces for t in ((a, b, cc), (a, cc, d))], np.uint32)
    scenes = {"m": imm.desc(tris=(c, tris, 0))}
    D = 10.0
    inst = [(0, "m", [ih.affine((0, 0, 0)), ih.affine((D, 0, 0))])]
    m = 4096
    rng = np.random.RandomState(3)
    org = np.stack([rng.rand(m) * (D + 1.0), rng.rand(m), np.full(m, 5.0)], 1).astype(np.float32).astype(np.float64)
    dirs = np.tile(np.array([0.0, 0.0, -1.0]), (m, 1))
    times = rng.rand(m).astype(np.float32)
    truth = int(((org[:, 0] >= D * times.astype(np.float64)) & (org[:, 0] <= D * times.astype(np.float64) + 1.0)).sum())
    dev, top, inner = imm.build(rtc, 1, scenes, inst, LIN)
    assert top.stats()["accelKind"] == 33
    image_mb, leaves = itl.top_leaves(top)
    (path, rec), = leaves
    assert len(path) == 1  # a root of one child: the mover's box is tested although the tree is one leaf
    ok = np.ones(m, bool)
    for t in np.unique(times):
        sel = times == t
        ok[sel] = itl.passes([(lo[None], hi[None]) for lo, hi in itl.path_boxes(image_mb, path, t)], org[sel], dirs[sel])
    linear = int(ok.sum())
    iq.release(dev, top, inner)
    dev, top, inner = imm.build(rtc, 1, scenes, inst, BASE)
    assert top.stats()["accelKind"] == 19
    nodes = top.accel_data(0).view(NODE_DT)
    root = top.accel_root()
    boxes = []
    for p, first, count in walk_paths(nodes, root):  # (a single instance: the root is the leaf, no path)
        assert (first, count) == (0, 1)
        lo, hi, _ = ds.decode_nodes(nodes)
        boxes = [(lo[n][s][None], hi[n][s][None]) for n, s in p]
    swept = int(itl.passes(boxes, org, dirs).sum())
    iq.release(dev, top, inner)
    print(f"rays that enter the mover: swept {swept}, linear {linear}, truly meeting the cube at their time {truth} of {m} (ratio {linear / swept:.3f}, geometry {1 / 11:.3f})")
    assert truth <= linear
    assert linear <= 0.25 * swept


# ---- 6. stack bound -------------------------------------------------------------------------------------------------------------------------------------------
def test_max_depth_covers_the_deepest_path_of_a_chain_of_nested_instances(rtc):
    """itl.chain_case(): 30 instances with nested boxes over a needle soup.  maxDepth is the formula of every instance kind over the
    QNodeMB8 top level - top-level depth + 1 (exit marker) + 0 pending trees + the soup's depth - and no ray of the host walk writes a
    slot beyond the capacity sized from it; a tenth of the rays or more pass the 16 slots in LDS (the precondition of the GPU test)."""
    scenes, inst = itl.chain_case()
    dev, top, inner = imm.build(rtc, 1, scenes, inst, LIN)
    st = top.stats()
    assert st["accelKind"] == 33
    _, leaves = itl.top_leaves(top)
    top_depth = max(len(p) for p, _ in leaves)
    own = imm.own_accels(rtc, BASE, scenes["m"], 1)["tris"]
    assert top_depth >= 2 and st["maxDepth"] == top_depth + 1 + own[3]
    rays = itl.chain_rays(rtc, 60, ds.HOST_RAY_SEED)
    org = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1)
    dirs = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1)
    w = itl.walk_instances(top, scenes, inst, pluecker=False)
    deepest, markers = itl.simulate_stack(top, org, dirs, rays["time"], w)
    share = float((deepest >= ds.LDS_STACK).mean())
    print(f"deepest slot {deepest.max()} of {ds.stack_capacity(st['maxDepth'])}, {100 * share:.0f} % of the rays pass slot {ds.LDS_STACK}")
    assert deepest.max() < ds.stack_capacity(st["maxDepth"]) and markers.max() == 0
    assert share >= 0.1
    iq.release(dev, top, inner)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_moving_meshes_below_a_moving_instance_need_all_three_keys(rtc, mode):
    d = _mb_scene()
    for cfg in (LIN, LIN + ",mb_bounds=linear", LIN + ",inst_mb_bounds=linear"):
        dev = rtc.Device(cfg)
        err = Errors(dev)
        inner = {"m": imm.add_scene(rtc, dev, d, mode)}
        top = rtc.Scene(dev, iq.flags(mode))
        top.add_instance_mb(inner["m"], MOVING[0][2])
        top.add_instance(inner["m"], MOVING[1][2][0])
        top.lib.rtcCommitScene(top.handle)
        err.expect(rtc.RTC_ERROR_INVALID_OPERATION, NEEDS_LINEAR)
        assert all(k in NEEDS_LINEAR for k in ("mb_bounds=linear", "inst_mb_bounds=linear", "inst_bounds=linear"))
        iq.release(dev, top, inner)
    # static meshes below the moving instance need no other key (above); all three keys: accepted, the motion-blur trees in the QNodeMB8 section
    dev, top, inner = imm.build(rtc, mode, {"m": d}, MOVING, ALL)
    st = top.stats()
    assert st["accelKind"] == itl.kind(mode)
    nodes8, image_mb, n_mb, first = iml.split_nodes(top)
    _, leaves = itl.top_leaves(top)
    top_nodes = {n for path, _ in leaves for n, _ in path}
    nq, ntm, nqm = len(d["quads"][1]), len(d["tris_mb"][1]), 2 * len(d["quads_mb"][1])
    recs, _, _, srecs, trimb, quadmb, t_off, q_off = imm.split_blobs(top.accel_data(2), 3, nq, 5, 1, ntm, nqm)
    own = {p: imm.add_scene(rtc, dev, imm.desc(**{p: d[p]}), mode) for p in ("tris_mb", "quads_mb")}
    mb_nodes = set()
    for field, part, base in (("triMBRoot", "tris_mb", t_off // 96), ("quadMBRoot", "quads_mb", q_off // 128)):
        root = int(srecs[0][field])
        assert not root & LEAF and first <= root < first + n_mb and root not in top_nodes
        onodes = own[part].accel_data(0).view(NODEMB_DT)
        assert own[part].stats()["accelKind"] in (26, 27, 28, 29)
        got = sorted((f, c) for _, f, c in walk_paths(image_mb, root))
        assert got == sorted((f + base, c) for _, f, c in walk_paths(onodes, own[part].accel_root()))
        mb_nodes |= {n for path, _, _ in walk_paths(image_mb, root) for n, _ in path}
    assert top_nodes | mb_nodes == set(range(first, first + n_mb)) and not top_nodes & mb_nodes
    assert min(top_nodes) == first  # the top-level tree leads the section
    for s in own.values():
        s.release()
    iq.release(dev, top, inner)


def test_existing_refusals_keep_their_texts_under_the_key(rtc):
    dev = rtc.Device(LIN + ",subdiv_accel=default")
    err = Errors(dev)
    v, t = random_soup(16, 1)
    a = rtc.Scene(dev)
    a.add_triangles(v, t)
    a.commit()
    # instances below instances
    b = rtc.Scene(dev)
    b.add_instance(a)
    b.commit()
    top = rtc.Scene(dev)
    top.add_instance_mb(b, MOVING[0][2])
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "an instanced scene may hold triangle and quad meshes only (no subdivision meshes or instances)")
    top.release()
    # subdivision beside meshes
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    c = rtc.Scene(dev)
    c.add_triangles(v, t)
    c.add_subdiv(quad, np.array([4], np.uint32), np.arange(4, dtype=np.uint32))
    c.commit()
    top = rtc.Scene(dev)
    top.add_instance_mb(c, MOVING[0][2])
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "an instanced scene that enables subdivision meshes may hold nothing else: the scene of instance 0 also enables a triangle mesh")
    top.release()
    # counted batches, and the context filter without inst_filters=1: refused before anything touches a GPU
    top = rtc.Scene(dev)
    top.add_instance_mb(a, MOVING[0][2])
    top.commit()
    assert top.stats()["accelKind"] == 33
    rh = rtc.aligned_rayhits(8)
    from helpers import fill_rays
    fill_rays(rh, np.zeros((8, 3), np.float32), np.tile(np.array([0, 0, 1], np.float32), (8, 1)))
    with pytest.raises(rtc.RTCError) as e:
        top.intersect1M_counted(rh)
    assert e.value.code == rtc.RTC_ERROR_INVALID_OPERATION
    assert "counted batches are not supported on a scene with instances" in err.log[-1][1], err.log
    fn = rtc.FILTER_FUNC(lambda args: None)
    ctx = rtc.make_context()
    ctx.filter = C.cast(fn, C.c_void_p)
    top.intersect1M(rh, ctx=ctx, check=False)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "RTCIntersectContext::filter is not supported on a scene with instances")
    top.release()
    for s in (a, b, c):
        s.release()
    dev.release()
