"""CPU tests of the linear-bounds motion-blur accels (device config mb_bounds=linear) on a `gpu=none` device: the accel kinds 26..29 and
their 144-byte time-dependent nodes (csrc/accel.h QNodeMB8, read through rtcamdGetAccelData), that every decoded box holds what lies
below it at the ray's time, how tight the boxes are, what the midpoint build does to the tree, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from mb_linear_helpers import (EMPTY, LEAF, NODE_DT, NODEMB_DT, PAD_STEPS, QUAD_ENDS, QUADMB_DT, ROBUST, TRI_ENDS, TRIMB_DT, bomberman_two_steps,
                               curved_steps, decode_children_mb, grid_quads, grid_tris, record_vertices, scales, walk_paths)

TRI_CFG = "gpu=none"
QUAD_CFG = "gpu=none,quad_accel_mb=default"


def _build(rtc, cfg, flags, meshes, quads=False):
    dev = rtc.Device(cfg)
    sc = rtc.Scene(dev, flags)
    for steps, idx in meshes:
        (sc.add_quads_mb if quads else sc.add_triangles_mb)(steps, idx)
    sc.commit()
    return dev, sc


def _arrays(sc, quads, linear):
    nodes = sc.accel_data(0).view(NODEMB_DT if linear else NODE_DT)
    recs = sc.accel_data(2).view(QUADMB_DT if quads else TRIMB_DT)
    return nodes, recs


# ---- 1. kinds and sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsteps", [2, 5])
@pytest.mark.parametrize("quads,flags,kind,swept_kind", [(False, ROBUST, 26, 10), (False, 0, 27, 11), (True, ROBUST, 28, 12), (True, 0, 29, 13)])
def test_kinds_sizes_and_records(rtc, nsteps, quads, flags, kind, swept_kind):
    v, idx = grid_quads(8) if quads else grid_tris(8)
    steps = curved_steps(v, nsteps)
    base = QUAD_CFG if quads else TRI_CFG
    out = {}
    for name, cfg in (("none", base), ("swept", base + ",mb_bounds=swept"), ("linear", base + ",mb_bounds=linear")):
        dev, sc = _build(rtc, cfg, flags, [(steps, idx)], quads)
        st = sc.stats()
        out[name] = (st, sc.accel_data(0).tobytes(), sc.accel_data(2).tobytes(), sc.accel_root(), sc.bounds())
        sc.release()
        dev.release()
    # no key and mb_bounds=swept: today's accel, byte for byte
    assert out["none"][0]["accelKind"] == out["swept"][0]["accelKind"] == swept_kind
    assert out["none"][0]["nodeBytes"] == 96
    assert out["none"][1:4] == out["swept"][1:4]
    st = out["linear"][0]
    rec_bytes = 128 if quads else 96
    assert st["accelKind"] == kind and kind in (rtc.ACCEL_TRIMB_LINEAR_PLUECKER, rtc.ACCEL_TRIMB_LINEAR_MOELLER, rtc.ACCEL_QUADMB_LINEAR_PLUECKER, rtc.ACCEL_QUADMB_LINEAR_MOELLER)
    assert st["nodeBytes"] == 144 and st["nodeCount"] > 0 and len(out["linear"][1]) == st["nodeCount"] * 144
    assert st["primBytes"] == rec_bytes and st["primCount"] == len(idx) * (nsteps - 1)
    assert st["totalBytes"] == st["nodeCount"] * 144 + st["primCount"] * rec_bytes
    # the leaf records, as a set, are the swept build's
    split = lambda b: sorted(b[i:i + rec_bytes] for i in range(0, len(b), rec_bytes))
    assert split(out["linear"][2]) == split(out["swept"][2])
    # the leaves partition the record array in blocks the leaf code knows
    nodes = np.frombuffer(out["linear"][1], NODEMB_DT)
    covered = np.zeros(st["primCount"], np.int32)
    nleaves = 0
    for _, first, count in walk_paths(nodes, out["linear"][3]):
        assert 1 <= count <= 28
        covered[first:first + count] += 1
        nleaves += 1
    assert (covered == 1).all() and nleaves == st["leafCount"]
    # rtcGetSceneBounds: the swept bounds, as before
    for a, b in zip(out["linear"][4], out["swept"][4]):
        assert np.array_equal(a, b)


# ---- 2. containment -------------------------------------------------------------------------------------------------------------
def _containment(nodes, recs, root, ends):
    """every record, at both ends of its segment and at three times inside it: the vertices the kernel forms lie in the box of every
    ancestor as the kernel decodes it at that time -> (checks made, violations)"""
    checks, bad, accepted_ends = 0, [], 0
    for path, first, count in walk_paths(nodes, root):
        for r in recs[first:first + count]:
            S, seg = int(r["numSegments"]), int(r["segment"])
            for k, f in enumerate((0.0, 0.25, 0.5, 0.75, 1.0)):
                t = np.float32((seg + f) / S)
                p = record_vertices(r, ends, t)
                if p is None:  # the segment's last instant belongs to the next segment (floor), or 1 / 3 rounds across a step
                    assert f in (0.0, 1.0) and (S & (S - 1) or f == 1.0), (S, seg, f)
                    continue
                accepted_ends += f in (0.0, 1.0)
                for n, slot in path:
                    lo, hi = decode_children_mb(nodes[n], t)
                    checks += 1
                    if not ((lo[slot] <= p).all() and (p <= hi[slot]).all()):
                        bad.append((n, slot, float(t), lo[slot], hi[slot], p))
    return checks, bad, accepted_ends


@pytest.mark.parametrize("quads", [False, True])
@pytest.mark.parametrize("nsteps", [2, 3, 5])
def test_every_ancestor_box_holds_the_interpolated_vertices(rtc, nsteps, quads):
    v, idx = grid_quads(12) if quads else grid_tris(8)  # (12 x 12 quads: enough records for inner nodes below the root)
    dev, sc = _build(rtc, (QUAD_CFG if quads else TRI_CFG) + ",mb_bounds=linear", 0, [(curved_steps(v, nsteps), idx)], quads)
    nodes, recs = _arrays(sc, quads, True)
    root = sc.accel_root()
    assert not root & LEAF and len(nodes) > 1
    checks, bad, ends = _containment(nodes, recs, root, QUAD_ENDS if quads else TRI_ENDS)
    print(f"{nsteps} steps, {'quads' if quads else 'triangles'}: {len(nodes)} nodes, {checks} box checks, {ends} accepted segment ends")
    assert checks >= 4 * len(recs) and ends >= len(recs)  # every record at four times or more, under one ancestor or more
    assert not bad, bad[:3]
    sc.release()
    dev.release()


def test_boxes_hold_a_two_step_and_a_four_step_mesh_together(rtc):
    v, idx = grid_tris(8)
    a = curved_steps(v, 2)
    b = [s + np.array([3.0, 0.5, 0.25], np.float32) for s in curved_steps(v, 4)]  # overlapping the first mesh, S = 3: step times 1/3, 2/3
    dev, sc = _build(rtc, TRI_CFG + ",mb_bounds=linear", 0, [(a, idx), (b, idx)])
    nodes, recs = _arrays(sc, False, True)
    root = sc.accel_root()
    mixed = 0
    for path, first, count in walk_paths(nodes, root):
        mixed += len(set(recs["numSegments"][first:first + count].tolist())) > 1
    checks, bad, ends = _containment(nodes, recs, root, TRI_ENDS)
    print(f"2-step + 4-step mesh: {len(nodes)} nodes, {mixed} leaves that mix S = 1 and S = 3, {checks} box checks")
    assert sorted(set(recs["numSegments"].tolist())) == [1, 3] and mixed > 0
    assert not bad, bad[:3]
    sc.release()
    dev.release()


# ---- 3. tightness on 2-step meshes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quads", [False, True])
def test_two_step_boxes_are_the_step_bounds_plus_the_stated_padding(rtc, quads):
    v, idx = grid_quads(8) if quads else grid_tris(8)
    dev, sc = _build(rtc, (QUAD_CFG if quads else TRI_CFG) + ",mb_bounds=linear", 0, [(curved_steps(v, 2), idx)], quads)
    nodes, recs = _arrays(sc, quads, True)
    ends = QUAD_ENDS if quads else TRI_ENDS
    # exact bounds, per step, of the records below every (node, slot)
    exact = {}
    for path, first, count in walk_paths(nodes, sc.accel_root()):
        for step in (0, 1):
            pts = np.concatenate([recs[f][first:first + count] for f in ends[step]])
            for key in path:
                lo, hi = exact.setdefault((key, step), (np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)))
                exact[(key, step)] = (np.minimum(lo, pts.min(0)), np.maximum(hi, pts.max(0)))
    worst = 0.0
    for ((n, slot), step), (elo, ehi) in exact.items():
        lo, hi = decode_children_mb(nodes[n], float(step))
        s = scales(nodes[n]).astype(np.float64)
        assert (s > 0).all()
        under, over = (elo.astype(np.float64) - lo[slot]) / s, (hi[slot] - ehi.astype(np.float64)) / s
        worst = max(worst, under.max(), over.max())
        assert (under >= 0).all() and (over >= 0).all(), (n, slot, step)
        assert (under <= PAD_STEPS).all() and (over <= PAD_STEPS).all(), (n, slot, step, under, over)
    print(f"2-step {'quads' if quads else 'triangles'}: {len(exact)} child boxes, largest excess {worst:.3f} grid steps (bound {PAD_STEPS})")
    assert len(exact) > 16
    sc.release()
    dev.release()


# ---- 4. topology ----------------------------------------------------------------------------------------------------------------
def test_the_midpoint_build_keeps_splitting_where_the_swept_build_stops(rtc, bomberman_tris):
    v, tris = bomberman_tris
    steps = bomberman_two_steps(v)
    count = {}
    for name in ("swept", "linear"):
        dev, sc = _build(rtc, TRI_CFG + ",mb_bounds=" + name, ROBUST, [(steps, tris)])
        count[name] = sc.stats()["nodeCount"]
        sc.release()
        dev.release()
    dev, sc = _build(rtc, TRI_CFG, ROBUST, [])
    sc.add_triangles(steps[0], tris)
    sc.commit()
    count["rest"] = sc.stats()["nodeCount"]
    sc.release()
    dev.release()
    print(f"moved 2-step bomberman: {count['swept']} nodes swept, {count['linear']} linear; the mesh at rest {count['rest']}")
    assert count["swept"] == 33  # docs/experiments.md "Motion blur"
    assert count["linear"] > count["swept"]


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------
def test_unknown_mb_bounds_is_an_invalid_argument(rtc):
    with pytest.raises(rtc.RTCError) as e:
        rtc.Device("gpu=none,mb_bounds=bogus")
    assert e.value.code == rtc.RTC_ERROR_INVALID_ARGUMENT


@pytest.mark.parametrize("quads", [False, True])
def test_an_instanced_scene_with_a_linear_accel_is_refused_at_the_top_commit(rtc, quads):
    cfg = "gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,inst_accel=default"
    for bounds, want in (("swept", rtc.RTC_ERROR_NONE), ("linear", rtc.RTC_ERROR_INVALID_OPERATION)):
        dev = rtc.Device(cfg + ",mb_bounds=" + bounds)
        inner = rtc.Scene(dev)
        v, idx = grid_quads(4) if quads else grid_tris(4)
        (inner.add_quads_mb if quads else inner.add_triangles_mb)(curved_steps(v, 2), idx)
        inner.commit()
        assert inner.stats()["accelKind"] == {("swept", False): 11, ("swept", True): 13, ("linear", False): 27, ("linear", True): 29}[(bounds, quads)]
        top = rtc.Scene(dev)
        top.add_instance(inner)
        assert dev.error() == rtc.RTC_ERROR_NONE
        messages = []
        on_error = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)(lambda user, code, msg: messages.append((code, msg.decode())))
        dev.lib.rtcSetDeviceErrorFunction(dev.handle, C.cast(on_error, C.c_void_p), None)
        dev.lib.rtcCommitScene(top.handle)
        assert dev.error() == want
        if want != rtc.RTC_ERROR_NONE:  # the refusal says what to change
            assert len(messages) == 1 and messages[0][0] == want and "mb_bounds=linear" in messages[0][1], messages
        else:
            assert not messages
        dev.lib.rtcSetDeviceErrorFunction(dev.handle, None, None)
        top.release()
        inner.release()
        dev.release()
