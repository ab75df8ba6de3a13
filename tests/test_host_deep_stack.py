"""CPU tests of the inputs of tests/test_gpu_deep_stack.py on `gpu=none` devices: for every accel that file traces, the needle scene of
deep_stack_helpers.py really sends rays into the HBM overflow part of the traversal stack (above slot 16 for the lane kernels, above
slot 8 for the ray-pool kernel), and never past what the host sizes the stack for, 7 * (maxDepth + 1) + 2 entries.

The figures come from deep_stack_helpers.simulate_stack, a float64 walk of the product's own node and record arrays with the kernels'
ordering and culling rules, over 300 rays between random points of the scene's bounds.  The shares are conditions on the INPUTS: if a
change of the builder makes the trees of these scenes shallow, these tests say so before the GPU tests silently stop reaching the
overflow code."""
import numpy as np
import pytest

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_quads_helpers as iq
from helpers import random_rays_np

ABOVE_LDS, ABOVE_POOL = 0.10, 0.50  # shares of the rays that must reach a slot above 16 / above 8


def _measure(what, nodes, root, leaves, lo, hi, max_depth, times=None, instances=None):
    org, dirs = random_rays_np(ds.HOST_RAYS, lo, hi, ds.HOST_RAY_SEED)
    time = 0.0 if times is None else np.asarray(times)[np.arange(ds.HOST_RAYS) % len(times)]
    w = ds.simulate_stack(nodes, root, leaves, org, dirs, time=time, instances=instances)
    a16, a8 = float((w.deepest > ds.LDS_STACK).mean()), float((w.deepest > ds.POOL_STACK).mean())
    print(f"{what}: {100 * a16:.0f} % of {ds.HOST_RAYS} rays above slot 16, {100 * a8:.0f} % above slot 8, deepest slot {int(w.deepest.max())}, "
          f"maxDepth {max_depth} (capacity {ds.stack_capacity(max_depth)}), {100 * float(w.hit.mean()):.0f} % hit, "
          f"{int(w.from_overflow.sum())} final hits in a leaf popped from an overflow slot")
    assert a16 >= ABOVE_LDS, (what, a16)                                # (a)
    assert a8 >= ABOVE_POOL, (what, a8)                                 # (b)
    assert int(w.deepest.max()) <= ds.stack_capacity(max_depth) - 1, what  # (c)
    assert w.hit.mean() > 0.25, what  # the rays do find hits, so tfar shrinks and the distance cull of popped entries is exercised
    return w


def _commit(rtc, cfg, flags, add):
    dev = rtc.Device(cfg)
    sc = rtc.Scene(dev, flags)
    add(sc)
    sc.commit()
    return dev, sc


@pytest.mark.parametrize("cfg,pluecker", [("tri_accel=bvh8.triangle4v", True), ("tri_accel=bvh8.triangle4", False)])
def test_triangle_needles_reach_the_overflow_area(rtc, cfg, pluecker):
    """Measured (n = 8192, seed 7, 300 rays): triangle4v 61 % of the rays above slot 16, 94 % above slot 8, deepest slot 21, maxDepth 4
    (capacity 37); triangle4 the same tree and the same figures.  90 % of the rays hit, 40 final hits came from a leaf popped from an
    overflow slot.  (n = 4096: maxDepth 3, 11 % above slot 16 with these 300 rays and 10.0 % with 600 - on the bar, hence 8192.)"""
    v, t = ds.sliver_soup(ds.N_SLIVERS, ds.SOUP_SEED)
    dev, sc = _commit(rtc, "gpu=none," + cfg, 0, lambda s: s.add_triangles(v, t))
    assert sc.stats()["accelKind"] == (1 if pluecker else 2)
    nodes, recs = sc.accel_data(0).view(ds.NODE_DT), sc.accel_data(1).view(ds.TRI_DT)
    assert len(recs) == ds.N_SLIVERS
    lo, hi = ds.bounds(v)
    _measure(cfg, nodes, sc.accel_root(), ds.tri_leaves(recs, pluecker), lo, hi, sc.stats()["maxDepth"])
    sc.release()
    dev.release()


@pytest.mark.parametrize("mode", [0, 1])
def test_quad_needles_reach_the_overflow_area(rtc, mode):
    """Measured (n = 8192, seed 7, 300 rays), both modes (one tree): 64 % of the rays above slot 16, 94 % above slot 8, deepest slot 21,
    maxDepth 4 (capacity 37), 94 % of the rays hit, 32 final hits in a leaf popped from an overflow slot.  (n = 4096: 11 % above 16.)"""
    v, q = ds.sliver_soup(ds.N_SLIVERS, ds.SOUP_SEED, quads=True)
    cfg = "gpu=none,quad_accel=default" if mode == 0 else "gpu=none,quad_accel=bvh8.quad4v"
    dev, sc = _commit(rtc, cfg, ds.ROBUST if mode == 0 else 0, lambda s: s.add_quads(v, q))
    assert sc.stats()["accelKind"] == (8 if mode == 0 else 9)
    nodes, recs = sc.accel_data(0).view(ds.NODE_DT), sc.accel_data(2).view(ds.QUAD_DT)
    assert len(recs) == ds.N_SLIVERS
    lo, hi = ds.bounds(v)
    _measure(f"quads mode {mode}", nodes, sc.accel_root(), ds.quad_leaves(recs), lo, hi, sc.stats()["maxDepth"])
    sc.release()
    dev.release()


@pytest.mark.parametrize("quads", [False, True])
def test_motion_blur_needles_reach_the_overflow_area(rtc, quads):
    """Measured (n = 8192, seed 7, 2 time steps, 300 rays with times k/4): triangles 64 % of the rays above slot 16, 94 % above slot 8,
    deepest slot 21, maxDepth 4 (capacity 37), 89 % hit, 34 final hits in a leaf popped from an overflow slot; quads 64 %, 93 %, deepest
    slot 21, maxDepth 4, 92 % hit, 33 such hits.  (n = 4096: 13 % above slot 16, both.)"""
    steps, idx = ds.sliver_soup_mb(ds.N_SLIVERS, ds.SOUP_SEED, quads=quads)
    cfg = "gpu=none,quad_accel=default,quad_accel_mb=default" if quads else "gpu=none"
    dev, sc = _commit(rtc, cfg, 0, lambda s: s.add_quads_mb(steps, idx) if quads else s.add_triangles_mb(steps, idx))
    assert sc.stats()["accelKind"] == (13 if quads else 11)
    nodes = sc.accel_data(0).view(ds.NODE_DT)
    recs = sc.accel_data(2).view(ds.QUADMB_DT if quads else ds.TRIMB_DT)
    assert len(recs) == ds.N_SLIVERS
    lo, hi = ds.bounds(*steps)
    _measure("quad MB" if quads else "tri MB", nodes, sc.accel_root(), (ds.quad_mb_leaves if quads else ds.tri_mb_leaves)(recs), lo, hi,
             sc.stats()["maxDepth"], times=ds.TIMES)
    sc.release()
    dev.release()


@pytest.mark.parametrize("kind", ["t", "q", "tq"])
def test_instanced_needles_reach_the_overflow_area(rtc, kind):
    """Three overlapping instances of one needle scene: the stack holds the top-level entries, the exit marker, the marker of the pending
    quad tree ('tq') and the entries of the instanced tree.  Measured (4096 needles, 300 rays drawn from the bounds of the unit-scale
    instance): 't' 77 % of the rays above slot 16, 100 % above slot 8, deepest slot 21, maxDepth 6 (capacity 51), every ray hits,
    14 final hits in a leaf popped from an overflow slot; 'q' 77 %, 100 %, deepest slot 20, maxDepth 6, 17 such hits; 'tq' (2048 + 2048 needles) 55 %, 100 %, deepest slot 20,
    maxDepth 6, 7 such hits."""
    scenes, inst = ds.instanced_scene(kind), ds.deep_instances()
    dev = rtc.Device("gpu=none,quad_accel=default,inst_accel=default")
    inner = {k: iq.add_scene(rtc, dev, d, 1) for k, d in scenes.items()}
    top = rtc.Scene(dev)
    for gid, key, l2w in inst:
        assert top.add_instance(inner[key], l2w, geom_id=gid) == gid
    top.commit()
    st = top.stats()
    has_quads = "q" in kind
    assert st["accelKind"] == (iq.ACCEL_INST_MOELLER if has_quads else ih.ACCEL_INST_TRI_MOELLER)
    nodes, prims, blobs = top.accel_data(0).view(ds.NODE_DT), top.accel_data(1).view(ds.TRI_DT), top.accel_data(2)
    recs, quads = blobs[:64 * len(inst)].view(ds.INST_DT), blobs[64 * len(inst):].view(ds.QUAD_DT)
    # quad leaf references are rebased by the number of InstanceRecords: pad the Leaves so that they index like `blobs`
    ql = ds.quad_leaves(np.concatenate([np.zeros(len(inst), ds.QUAD_DT), quads])) if has_quads else None
    lo, hi = ds.instance_ray_box(scenes, inst)
    _measure(f"instances of '{kind}'", nodes, top.accel_root(), ds.tri_leaves(prims, False), lo, hi, st["maxDepth"],
             instances=ds.Instances(recs, ql, has_quads))
    iq.release(dev, top, inner)
