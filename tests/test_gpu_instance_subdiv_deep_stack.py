"""The HBM overflow part of the traversal stack in the kernels of trace_instance_subdiv.hip, after tests/deep_stack_helpers.py.

A ray's stack lives in LDS up to slot 16 and in a per-lane column of an HBM overflow area beyond that; the host sizes the column from
7 * (maxDepth + 1) + 2, a push beyond it would be dropped behind a bounds check and raise the `overflow` word, which the device
reports as an error.  The scene: 1024 needle quads (deep_stack_helpers.sliver_soup, 0.4 % wide instead of 2 %, so that a good share of
the rays hits nothing) as ONE subdivision mesh - every needle a patch of its own, one grid cell / one cBVH blob each at tessellation
level 1 - under the three overlapping instances of deep_instances().  The node boxes overlap everywhere, so a ray stacks most children
of most nodes on both levels.

Precondition, measured here on the host from the accel the kernels traverse (there is no instrumented twin of these kernels):
deep_stack_helpers.simulate_stack walks the node array without primitive tests, which is exactly the walk of a ray that hits nothing;
of the sampled rays that the GPU reports as misses at least 10 % of the sample must have written stack slots beyond the 16 in LDS.
The records are compared with the instanced scene traced directly (eager: all rays, byte for byte; compressed.leaf: the order-free
classes), the `overflow` word must stay clear (no entry dropped: dev.error() == 0), and small queue shares must repeat the bytes."""
import numpy as np
import pytest

import deep_stack_helpers as ds
import instance_helpers as ih
import instance_quads_helpers as iq
import instance_subdiv_helpers as isd
from helpers import INVALID, random_rays_np

pytestmark = pytest.mark.gpu

KNOBS = ("RTAMD_KERNEL", "RTAMD_OCT_MAX", "RTAMD_OCT_LEAF", "RTAMD_CHUNK", "RTAMD_REFILL_BATCH", "RTAMD_LEAF_BATCH", "RTAMD_CULL", "RTAMD_CBVH_FORM")
SMALL_SHARES = {"RTAMD_CHUNK": "32", "RTAMD_REFILL_BATCH": "1", "RTAMD_LEAF_BATCH": "64"}
N_NEEDLES, WIDTH, SAMPLE = 1024, 0.004, 200


def _knobs(monkeypatch, knobs):
    """the tuning knobs are read when a device is created"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_needle_patches_spill_to_hbm_and_agree_with_the_direct_traces(rtc, monkeypatch, accel):
    _knobs(monkeypatch, {})
    v, q = ds.sliver_soup(N_NEEDLES, ds.SOUP_SEED, quads=True, snapped=True, width=WIDTH)
    meshes = {"m": (v, np.full(N_NEEDLES, 4, np.uint32), q.reshape(-1).astype(np.uint32), 1, 1)}
    inst = isd.static(ds.deep_instances())
    lo, hi = isd.world_boxes(meshes, inst)[0]
    org, dirs = random_rays_np(ds.GPU_RAYS, lo.astype(np.float32), hi.astype(np.float32), ds.GPU_RAY_SEED)
    rays = ds.rays_of(rtc, ds.snap(org), ih.snap(dirs * 4.0))  # origins on the 2^-10 grid, directions too: the local rays are exact
    dev, top, inner = isd.build(rtc, accel, meshes, inst)
    st = top.stats()
    assert st["accelKind"] == isd.KIND[accel] and ds.stack_capacity(st["maxDepth"]) > ds.LDS_STACK
    got, occ = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    top.intersect1M(got)
    top.occluded1M(occ)
    assert dev.error() == 0  # the `overflow` word stayed clear: no entry was dropped
    # the precondition: misses among the first SAMPLE rays whose walk passes slot 16, and none beyond what the host reserved
    nodes, blobs, _ = isd.decode(top, rtc)
    recs = blobs[: len(inst) * 64].view(ih.INST_DT)
    o = np.stack([rays["org_x"], rays["org_y"], rays["org_z"]], 1)[:SAMPLE]
    d = np.stack([rays["dir_x"], rays["dir_y"], rays["dir_z"]], 1)[:SAMPLE]
    walk = ds.simulate_stack(nodes, top.accel_root(), None, o, d, instances=ds.Instances(recs, None, False))
    miss = got["geomID"][:SAMPLE] == INVALID
    deep = int((miss & (walk.deepest >= ds.LDS_STACK)).sum())
    print(f"{accel}: maxDepth {st['maxDepth']}, {int(miss.sum())} of {SAMPLE} sampled rays miss, {deep} of them pass slot {ds.LDS_STACK}, deepest slot {int(walk.deepest.max())}")
    assert deep >= SAMPLE // 10 and walk.deepest.max() < ds.stack_capacity(st["maxDepth"])
    hit = got["geomID"] != INVALID
    if accel == isd.EAGER:
        per = isd.direct_all(rtc, inner, inst, rays)
        assert ih.equal_t_ties(per) == 0
        want = isd.merge(rays, per, inst)
        assert got.tobytes() == want.tobytes(), f"{isd.differing(got, want)} records differ from the merged direct traces"
        assert np.array_equal(occ["tfar"] == -np.inf, hit) and np.array_equal(occ["tfar"][~hit], rays["tfar"][~hit])
    else:
        none, single, want = isd.order_free_classes(rtc, inner, inst, rays)
        print(f"{accel}: {int(none.sum())} rays hit nothing, {int(single.sum())} one instance only")
        assert got[none].tobytes() == rays[none].tobytes() and got[single].tobytes() == want[single].tobytes()
        assert none.sum() >= 100 and single.sum() >= 100
        assert occ.tobytes() == isd.occluded_any(rtc, inner, inst, rays).tobytes()
    per_inst = [int((got["instID"][hit] == g).sum()) for g, _, _ in inst]
    print(f"{accel}: {int(hit.sum())} hits, per instance {per_inst}")
    assert int(hit.sum()) > 1000 and min(per_inst) > 50
    isd.release(dev, top, inner)
    # ... and with small queue shares, lanes refilled one at a time and leaves that wait for a full wave
    _knobs(monkeypatch, SMALL_SHARES)
    dev, top, inner = isd.build(rtc, accel, meshes, inst)
    g2, o2 = iq.copy(rtc, rays), iq.occ_of(rtc, rays)
    top.intersect1M(g2)
    top.occluded1M(o2)
    assert g2.tobytes() == got.tobytes() and o2.tobytes() == occ.tobytes(), "small shares differ"
    assert dev.error() == 0
    isd.release(dev, top, inner)
