"""CPU tests of instanced scenes that hold quad meshes (accel kinds 16 / 17) on a `gpu=none,quad_accel=default,inst_accel=default`
device: the accel's layout as accel.h documents it, the refusals, the config key, and the pinning of the inputs of the GPU parity tests
with the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import instance_helpers as ih
import instance_quads_helpers as iq
from helpers import random_soup
from instance_helpers import EMPTY, INST_DT, INVALID, LEAF, NODE_DT, TRI_DT
from instance_quads_helpers import QUAD_DT, ROBUST

CFG = "gpu=none,quad_accel=default,inst_accel=default"
REF_INST_EXIT, REF_INST_QUADS = 0x80000000, 0x80000001
ERRFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)
GENERAL_ASIDE = {0: 3, 1: 3}  # rays the general-transform GPU test may set aside, per mode (of 10 670 hits)


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


def _random_quads(n, seed, extent=10.0, size=1.0):
    rng = np.random.RandomState(seed)
    c = rng.rand(n, 1, 3) * extent
    v = (c + (rng.rand(n, 4, 3) - 0.5) * size).astype(np.float32).reshape(-1, 3)
    return v, np.arange(4 * n, dtype=np.uint32).reshape(-1, 4)


def _inner(rtc, dev, flags=0, ntris=64, nquads=48, seed=3):
    sc = rtc.Scene(dev, flags)
    if ntris:
        v, t = random_soup(ntris, seed)
        sc.add_triangles(v, t, geom_id=0)
    if nquads:
        v, q = _random_quads(nquads, seed + 1)
        sc.add_quads(v, q, geom_id=1)
    sc.commit()
    return sc


def _own_accels(rtc, flags, ntris, nquads, seed):
    """the triangle and the quad accel of _inner(...) as scenes of their own export them: (nodes, records, root, maxDepth) each"""
    dev = rtc.Device(CFG)
    out = []
    for nt, nq, kind, dt in ((ntris, 0, 1, TRI_DT), (0, nquads, 2, QUAD_DT)):
        if not (nt or nq):
            out.append(None)
            continue
        sc = _inner(rtc, dev, flags, nt, nq, seed)
        out.append((sc.accel_data(0).view(NODE_DT).copy(), sc.accel_data(kind).view(dt).copy(), sc.accel_root(), sc.stats()["maxDepth"]))
        sc.release()
    dev.release()
    return out


def _walk(nodes, root):
    """[(first record, count)] of the leaves reachable from root, and the number of levels of inner nodes above the deepest leaf"""
    if root == EMPTY:
        return [], 0
    if root & LEAF:
        return [(root & 0x3FFFFFF, (root >> 26) & 31)], 0
    out, todo, deepest = [], [(root, 1)], 0
    while todo:
        n, depth = todo.pop()
        deepest = max(deepest, depth)
        for c in nodes[n]["child"].tolist():
            if c == EMPTY:
                continue
            if c & LEAF:
                out.append((c & 0x3FFFFFF, (c >> 26) & 31))
            else:
                todo.append((c, depth + 1))
    return out, deepest


# ---- 1. kinds -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,kind", [(0, iq.ACCEL_INST_MOELLER), (ROBUST, iq.ACCEL_INST_PLUECKER)])
def test_triangles_and_quads_instanced_twice_commit_with_the_new_kinds(rtc, flags, kind):
    dev = rtc.Device(CFG)
    inner = _inner(rtc, dev, flags)
    top = rtc.Scene(dev, flags)
    top.add_instance(inner)
    top.add_instance(inner, ih.affine((30, 0, 0)))
    top.commit()
    st = top.stats()
    assert st["accelKind"] == kind and st["leafCount"] == 2
    assert st["primBytes"] == 64 and st["primCount"] == 2 + 48  # 64-byte records: the instances, then the quads
    top.release()
    inner.release()
    dev.release()


# ---- 2. layout --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, ROBUST])
def test_accel_arrays_decode_per_the_documented_layout(rtc, flags):
    # scene a: triangles + quads, three instances; scene b: quads only, two; scene c: triangles only, one
    shapes = {"a": (64, 48, 3), "b": (0, 30, 5), "c": (40, 0, 7)}
    dev = rtc.Device(CFG)
    inner = {k: _inner(rtc, dev, flags, nt, nq, seed) for k, (nt, nq, seed) in shapes.items()}
    own = {k: _own_accels(rtc, flags, nt, nq, seed) for k, (nt, nq, seed) in shapes.items()}
    top = rtc.Scene(dev, flags)
    use = {}
    for i, k in enumerate("abacab"):  # first use: a, b, c
        use[top.add_instance(inner[k], ih.affine((30.0 * i, 0, 0)))] = k
    top.commit()
    nodes, prims, blobs = top.accel_data(0).view(NODE_DT), top.accel_data(1).view(TRI_DT), top.accel_data(2)
    n = len(use)
    recs, quads = blobs[:64 * n].view(INST_DT), blobs[64 * n:].view(QUAD_DT)
    assert top.stats()["leafCount"] == n and sorted(recs["geomID"].tolist()) == sorted(use)
    # every distinct scene once, in the order of first use
    assert len(prims) == 64 + 40 and len(quads) == 48 + 30
    assert prims.tobytes() == own["a"][0][1].tobytes() + own["c"][0][1].tobytes()
    assert quads.tobytes() == own["a"][1][1].tobytes() + own["b"][1][1].tobytes()
    tri_base, quad_base = {"a": 0, "c": 64}, {"a": n, "b": n + 48}
    roots = {}
    for r in recs:
        k = use[int(r["geomID"])]
        roots.setdefault(k, set()).add((int(r["root"]), int(r["pad"][0])))
        assert r["pad"][1] == 0
    assert all(len(v) == 1 for v in roots.values()) and len({next(iter(v)) for v in roots.values()}) == 3
    node_ranges = []
    for k, (nt, nq, _) in shapes.items():
        troot, qroot = next(iter(roots[k]))
        assert (troot == EMPTY) == (nt == 0) and (qroot == EMPTY) == (nq == 0)
        assert qroot not in (REF_INST_EXIT, REF_INST_QUADS) and troot not in (REF_INST_EXIT, REF_INST_QUADS)
        for root, o, base, total in ((troot, own[k][0], tri_base.get(k), len(prims)), (qroot, own[k][1], quad_base.get(k), n + len(quads))):
            if o is None:
                continue
            onodes, orecs, oroot, _ = o
            # the leaves under the rebased root are the scene's own leaves moved by the base: they land on its own records, in order
            got, _ = _walk(nodes, root)
            want, _ = _walk(onodes, oroot)
            assert sorted(got) == sorted((f + base, c) for f, c in want)
            assert all(base <= f and f + c <= base + len(orecs) <= total for f, c in got)
            assert sum(c for _, c in got) == len(orecs)
            if not root & LEAF:  # its nodes are a copy of the scene's own, child indices moved by the node base
                nb = root - oroot
                node_ranges.append((nb, nb + len(onodes)))
                for a, b in zip(nodes[nb:nb + len(onodes)], onodes):
                    assert a["origin"].tobytes() == b["origin"].tobytes() and a["exp"].tobytes() == b["exp"].tobytes() and a["q"].tobytes() == b["q"].tobytes()
                    for ca, cb in zip(a["child"].tolist(), b["child"].tolist()):
                        assert ca == (cb if cb == EMPTY else (cb + base if cb & LEAF else cb + nb))
    # top-level tree first, then a's triangle nodes, a's quad nodes, b's quad nodes, c's triangle nodes, without gaps
    node_ranges.sort()
    assert node_ranges == sorted(node_ranges, key=lambda r: r[0]) and node_ranges[-1][1] == len(nodes)
    assert all(a[1] == b[0] for a, b in zip(node_ranges, node_ranges[1:]))
    leaves, _ = _walk(nodes[:node_ranges[0][0]], top.accel_root())
    assert sorted(f for f, _ in leaves) == list(range(n)) and all(c == 1 for _, c in leaves)
    assert top.stats()["totalBytes"] == len(nodes) * 96 + len(prims) * 48 + len(blobs)
    top.release()
    for s in inner.values():
        s.release()
    dev.release()


# ---- 3. stack bound ---------------------------------------------------------------------------------------------------------------------------
def test_max_depth_covers_the_markers_and_the_deeper_quad_tree(rtc):
    dev = rtc.Device(CFG)
    inner = _inner(rtc, dev, 0, ntris=8, nquads=2000, seed=9)
    (_, _, _, tdepth), (_, _, _, qdepth) = _own_accels(rtc, 0, 8, 2000, 9)
    assert qdepth > tdepth
    top = rtc.Scene(dev)
    for i in range(20):
        top.add_instance(inner, ih.affine((12.0 * i, 0, 0)))
    top.commit()
    nodes = top.accel_data(0).view(NODE_DT)
    first_inner = min(int(r["pad"][0]) for r in top.accel_data(2)[:64 * 20].view(INST_DT))
    _, top_levels = _walk(nodes[:first_inner], top.accel_root())
    assert top_levels >= 2
    # top-level levels + exit marker + the entry of the pending quad tree + the deeper instanced tree
    assert top.stats()["maxDepth"] >= top_levels + 1 + 1 + qdepth
    top.release()
    inner.release()
    dev.release()


# ---- 4. quads only ------------------------------------------------------------------------------------------------------------------------------
def test_quads_only_instanced_scene_commits_and_is_not_left_out(rtc):
    dev = rtc.Device(CFG)
    inner = _inner(rtc, dev, 0, ntris=0, nquads=48)
    lo, hi = inner.bounds()
    top = rtc.Scene(dev)
    g = top.add_instance(inner, ih.affine((5, 0, 0)))
    top.commit()
    assert top.stats()["accelKind"] == iq.ACCEL_INST_MOELLER
    blobs = top.accel_data(2)
    recs = blobs[:64].view(INST_DT)
    assert recs["geomID"].tolist() == [g] and recs["root"][0] == EMPTY and recs["pad"][0][0] != EMPTY
    assert len(top.accel_data(1)) == 0 and len(blobs[64:].view(QUAD_DT)) == 48
    # the instance's world bounds are the instanced scene's bounds - which are its quads' - moved
    tlo, thi = top.bounds()
    assert np.allclose(tlo, np.asarray(lo) + (5, 0, 0), atol=1e-5) and np.allclose(thi, np.asarray(hi) + (5, 0, 0), atol=1e-5)
    v, _ = _random_quads(48, 4)
    assert np.allclose(lo, v.min(0)) and np.allclose(hi, v.max(0))
    top.release()
    inner.release()
    dev.release()


def test_bounds_of_a_mixed_instanced_scene_include_its_quads(rtc):
    dev = rtc.Device(CFG)
    inner = rtc.Scene(dev)
    inner.add_triangles(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    inner.add_quads(np.array([[5, 5, 5], [6, 5, 5], [6, 6, 5], [5, 6, 7]], np.float32), np.array([[0, 1, 2, 3]], np.uint32))
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance(inner, ih.affine((10, 20, 30)))
    top.commit()
    lo, hi = top.bounds()
    assert np.allclose(lo, (10, 20, 30)) and np.allclose(hi, (16, 26, 37))
    top.release()
    inner.release()
    dev.release()


# ---- 5. / 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_robust_scene_under_an_explicit_quad4v_accel_is_refused(rtc):
    dev = rtc.Device("gpu=none,quad_accel=bvh8.quad4v,inst_accel=default")
    err = Errors(dev)
    inner = _inner(rtc, dev, ROBUST)  # Pluecker triangles beside Moeller quads
    top = rtc.Scene(dev, ROBUST)
    top.add_instance(inner)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "triangle and quad accels of an instanced scene disagree in kind")
    top.release()
    inner.release()
    dev.release()


def test_instanced_scenes_that_disagree_in_kind_are_refused_also_with_quads(rtc):
    dev = rtc.Device(CFG)
    err = Errors(dev)
    a, b = _inner(rtc, dev, ROBUST, ntris=0), _inner(rtc, dev, 0)
    top = rtc.Scene(dev)
    top.add_instance(a)
    top.add_instance(b, ih.affine((30, 0, 0)))
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "disagree in accel kind (Pluecker / robust and Moeller / fast)")
    dev.release()


def test_unknown_instance_accel_name_is_an_invalid_argument(rtc):
    dev = rtc.Device("gpu=none,quad_accel=default,inst_accel=bvh4.object")
    err = Errors(dev)
    sc = rtc.Scene(dev)
    v, t = random_soup(8, 1)
    sc.add_triangles(v, t)
    sc.lib.rtcCommitScene(sc.handle)
    err.expect(rtc.RTC_ERROR_INVALID_ARGUMENT, "unknown instance acceleration structure bvh4.object")
    dev.release()


@pytest.mark.parametrize("what", ["time steps", "subdivision", "instances"])
def test_what_stays_refused_names_the_limit_that_remains(rtc, what):
    dev = rtc.Device(CFG)
    err = Errors(dev)
    inner = _inner(rtc, dev)
    if what == "time steps":
        v, t = random_soup(8, 1)
        inner.add_triangles_mb([v, v + 1], t)
    elif what == "subdivision":
        inner.add_subdiv(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), [4], [0, 1, 2, 3])
        inner.set_levels(2, 1)
    else:
        leaf = _inner(rtc, dev)
        inner.add_instance(leaf)
    inner.commit()
    top = rtc.Scene(dev)
    top.add_instance(inner)
    top.lib.rtcCommitScene(top.handle)
    err.expect(rtc.RTC_ERROR_INVALID_OPERATION, "static triangle and quad meshes only (no time steps, subdivision meshes or instances)")
    dev.release()


# ---- 7. triangle-only accels are untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, ROBUST])
def test_triangle_only_accel_is_byte_identical_with_and_without_the_key(rtc, flags):
    got = []
    for cfg in ("gpu=none", CFG):
        dev = rtc.Device(cfg)
        a, b = _inner(rtc, dev, flags, 64, 0, 3), _inner(rtc, dev, flags, 40, 0, 4)
        top = rtc.Scene(dev, flags)
        for i in range(9):
            top.add_instance((a, b)[i % 2], ih.affine((25.0 * (i % 3), 25.0 * (i // 3), 0), (1.0 + 0.1 * i, 0.75, 1.25), ih.rotation((1, 1 + i % 3, 0.5), 13.0 * i)))
        top.commit()
        st = top.stats()
        got.append(([top.accel_data(k).tobytes() for k in range(4)], st["accelKind"], top.accel_root(), st["maxDepth"]))
        assert st["accelKind"] == (ih.ACCEL_INST_TRI_PLUECKER if flags else ih.ACCEL_INST_TRI_MOELLER)
        assert not top.accel_data(2).view(INST_DT)["pad"].any()
        dev.release()
    assert got[0] == got[1]


# ---- the inputs of the GPU parity tests, pinned with the oracle alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 9])
def test_grid_parity_inputs_are_pinned(rtc, po, bomberman, n, mode):
    scenes = iq.quads_only(bomberman)
    inst = iq.grid_instances(n)
    rays = ih.general_rays(rtc, po, iq.bounds_meshes(scenes), inst, snapped=True, m=iq.PARITY_RAYS, seed=iq.PARITY_SEED[n])
    want, per, isb, _ = iq.oracle_instances(rtc, po, scenes, inst, rays, mode, exact=True)
    hits, diag = int((want["geomID"] != INVALID).sum()), int(iq.diagonal(want).sum())
    print(f"grid parity, {n} instances, mode {mode}: {hits} hits, {int(isb.sum())} on B, {diag} on a diagonal, {ih.equal_t_ties(per)} equal-t ties")
    assert ih.equal_t_ties(per) == 0
    assert hits > (200 if n > 2 else 1000)
    assert diag < hits // 100


@pytest.mark.parametrize("mode", [0, 1])
def test_general_transform_inputs_are_pinned(rtc, po, bomberman, mode):
    scenes = iq.quads_only(bomberman)
    inst = iq.general_instances()
    rays = ih.general_rays(rtc, po, iq.bounds_meshes(scenes), inst, m=iq.GENERAL_RAYS, seed=iq.GENERAL_SEED)
    want, per, isb, want_tri = iq.oracle_instances(rtc, po, scenes, inst, rays, mode)
    hits = int((want["geomID"] != INVALID).sum())
    aside = int(iq.quad_set_aside(want, per, want_tri, [0]).sum())
    print(f"general transforms over quads, mode {mode}: {hits} hits, {aside} rays may be set aside, {ih.equal_t_ties(per)} equal-t ties")
    assert hits > 2000
    assert ih.equal_t_ties(per) == 0
    assert aside <= 0.01 * hits
    assert aside == GENERAL_ASIDE[mode]


def test_overlapping_quads_give_leaves_longer_than_one_block(rtc):
    dev = rtc.Device(CFG)
    v, q = iq.overlapping_quads()
    sc = rtc.Scene(dev)
    sc.add_quads(v, q)
    sc.commit()
    leaves, _ = _walk(sc.accel_data(0).view(NODE_DT), sc.accel_root())
    assert max(c for _, c in leaves) > 4, leaves
    sc.release()
    dev.release()
