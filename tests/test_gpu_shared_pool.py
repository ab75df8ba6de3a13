"""Hand-out of rays through the workgroup ray pool (csrc/trace_loop.hip.h, RayPool): every ray is traced exactly once, by one lane.

The four waves of a workgroup claim the rays of a global queue grab from one LDS word.  The bugs such a protocol can have are
hand-out bugs - a ray traced twice, never, or by two lanes at once - and a ray traced twice is invisible in closest-hit records,
so every case checks two things:
  1. the records against the oracle (`po`), not against a second run of the kernels: byte for byte where the oracle restates the
     kernel's arithmetic (the cBVH leaf mode under po.fork_arith(1), any-hit on triangles), IDs exact and t/u/v within 1e-4 on
     closest-hit triangles, exactly as tests/test_gpu_subdiv.py and tests/test_gpu_triangles.py compare;
  2. the work counters of the instrumented twin: `rays` == valid rays of the batch (all of them here), `hits` == hits stored,
     `stackSpills` == 0.
Batch sizes sit at the edges of the protocol (one ray, one lane short of / beyond a wave, a workgroup, a partial last chunk;
20 011 is no multiple of the 64 queues, of 32 or of 128), under the default chunk and under RTAMD_CHUNK=32 (128-ray workgroup grabs, claims of
at most 32).  The grid is sized to about one grab per workgroup, so in those cases a second grab happens only through stagger closure or
launch skew; test_many_grabs_per_workgroup forces six or more grabs per workgroup, so that the pool is republished while siblings are
claiming from it and the state word is contended after the first grab.
"""
import numpy as np
import pytest

from helpers import INVALID, compare_hits

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 257, 1023, 4097, 20011)
_oracle_cache = {}  # (scene, n, occluded) -> oracle records: traced once, shared by the cases, never modified


def _build(rtc, bomberman, scene):
    verts, fs, fi = bomberman
    if scene == "tri":
        dev = rtc.Device("tri_accel=bvh8.triangle4v")
        sc = rtc.Scene(dev)
        sc.add_triangles(verts, rtc.fan_triangulate(fs, fi))
    else:
        dev = rtc.Device("subdiv_accel=bvh4.compressed.leaf")
        sc = rtc.Scene(dev)
        sc.add_subdiv(verts, fs, fi)
        sc.set_levels(4, 2)
    sc.commit()
    return dev, sc


def _rays(po, bomberman, n):
    verts = bomberman[0]
    return po.make_random_rays(n, verts.min(0), verts.max(0), seed=100 + n)


def _trace(dev, sc, recs, occluded=False):
    """One call = one launch: host batches of 16 384 rays and more would be cut into pipelined chunks (Device::tunePipeMinRays), so those go
    to the GPU first and are traced in place; smaller ones are traced from host memory."""
    fn = sc.occluded1M if occluded else sc.intersect1M
    if recs.shape[0] < 16384:
        fn(recs)
        return recs
    import torch
    t = torch.from_numpy(recs.view(np.uint8).reshape(recs.shape[0], -1).copy()).cuda()
    torch.cuda.synchronize()
    fn(t)
    dev.synchronize()
    return t.cpu().numpy().reshape(-1).view(recs.dtype)


def _as_occ(rtc, rays):
    occ = rtc.aligned_rays(rays.shape[0])
    for f in occ.dtype.names:
        occ[f] = rays[f]
    return occ


def _oracle(rtc, po, bomberman, sc, scene, n, occluded=False):
    key = (scene, n, occluded)
    if key not in _oracle_cache:
        verts, fs, fi = bomberman
        want = _rays(po, bomberman, n)
        if occluded:
            want = _as_occ(rtc, want)
        if scene == "tri":
            orc = po.TriangleScene(verts, rtc.fan_triangulate(fs, fi), 0)
            (orc.occluded1M if occluded else orc.intersect1M)(want, nthreads=8)
        elif occluded:
            # the fork's any-hit is a stub that reports every blob the outer traversal reaches: checked against the oracle's own tree
            orc = po.SubdivScene(sc.accel_data(2), sc.stats()["primBytes"], 4, 2)
            orc.occluded1M(want, nthreads=8)
        else:
            # order-dependent mode: the oracle walks the product's outer BVH8, in the product's arithmetic -> byte-identical records
            orc = po.SubdivScene(sc.accel_data(2), sc.stats()["primBytes"], 4, 2, qnodes=sc.accel_data(0), root=sc.accel_root())
            with po.fork_arith(1):
                orc.intersect1M(want, nthreads=8)
        orc.free()
        want.setflags(write=False)
        _oracle_cache[key] = want
    return _oracle_cache[key]


def _check_intersect(rtc, po, bomberman, dev, sc, scene, n, what):
    want = _oracle(rtc, po, bomberman, sc, scene, n)
    got = _trace(dev, sc, _rays(po, bomberman, n))
    if scene == "tri":
        nh = compare_hits(got, want, what=what)
    else:
        assert got.tobytes() == want.tobytes(), f"{what}: records differ from the oracle (product arithmetic)"
        nh = int((got["geomID"] != INVALID).sum())
    cnt = sc.intersect1M_counted(_rays(po, bomberman, n))
    print(f"[pool] {what}: rays {cnt['rays']} of {n}, hits {cnt['hits']} of {nh}, spills {cnt['stackSpills']}, waves {cnt['waves']}")
    assert cnt["rays"] == n, (what, "rays traced", cnt["rays"], n)
    assert cnt["hits"] == nh, (what, "hits counted vs stored", cnt["hits"], nh)
    assert cnt["stackSpills"] == 0, (what, cnt["stackSpills"])
    return got


def _check_occluded(rtc, po, bomberman, dev, sc, scene, n, what):
    want = _oracle(rtc, po, bomberman, sc, scene, n, occluded=True)
    got = _trace(dev, sc, _as_occ(rtc, _rays(po, bomberman, n)), occluded=True)
    if scene == "tri":
        assert got.tobytes() == want.tobytes(), f"{what}: any-hit records differ from the oracle"
    else:
        # (different outer trees: grazing rays may differ at rounding level - the allowance of tests/test_gpu_subdiv.py; every ray
        # with a closest hit is occluded)
        diff = int(((got["tfar"] == -np.inf) != (want["tfar"] == -np.inf)).sum())
        assert diff <= max(2, n // 20000), (what, diff)
        hit = _oracle(rtc, po, bomberman, sc, scene, n)["geomID"] != INVALID
        assert np.all((got["tfar"] == -np.inf)[hit]), what
        untouched = [f for f in got.dtype.names if f != "tfar"]
        assert all(np.array_equal(got[f], want[f]) for f in untouched), what
    nocc = int((got["tfar"] == -np.inf).sum())
    cnt = sc.occluded1M_counted(_as_occ(rtc, _rays(po, bomberman, n)))
    print(f"[pool] {what}: rays {cnt['rays']} of {n}, occluded {cnt['hits']} of {nocc}, spills {cnt['stackSpills']}")
    assert cnt["rays"] == n and cnt["hits"] == nocc and cnt["stackSpills"] == 0, (what, cnt["rays"], cnt["hits"], nocc, cnt["stackSpills"])


@pytest.mark.parametrize("chunk", [None, 32])
@pytest.mark.parametrize("scene", ["cbvh.leaf", "tri"])
def test_every_ray_traced_once(rtc, po, bomberman, monkeypatch, scene, chunk):
    """cbvh.leaf goes through the two-stage leaf step, the triangle leaves do not."""
    monkeypatch.setenv("RTAMD_WG_POOL", "1")  # (unset, the library shares the pool from 16 384 rays per launch on: here at every size)
    if chunk is not None:
        monkeypatch.setenv("RTAMD_CHUNK", str(chunk))  # read by the Device constructor
    dev, sc = _build(rtc, bomberman, scene)
    for n in SIZES:
        _check_intersect(rtc, po, bomberman, dev, sc, scene, n, f"{scene} chunk {chunk} {n} rays")
    sc.release()
    dev.release()


@pytest.mark.parametrize("scene", ["cbvh.leaf", "tri"])
def test_any_hit_every_ray_traced_once(rtc, po, bomberman, monkeypatch, scene):
    """Any-hit ends rays early and changes the refill pattern."""
    monkeypatch.setenv("RTAMD_CHUNK", "32")
    monkeypatch.setenv("RTAMD_WG_POOL", "1")
    dev, sc = _build(rtc, bomberman, scene)
    for n in (4097, 20011):
        _check_occluded(rtc, po, bomberman, dev, sc, scene, n, f"{scene} occluded chunk 32 {n} rays")
    sc.release()
    dev.release()


@pytest.mark.parametrize("scene", ["cbvh.leaf", "tri"])
def test_both_knob_settings_agree(rtc, po, bomberman, monkeypatch, scene):
    """RTAMD_WG_POOL=0 (every wave grabs for itself) and =1 (workgroup pool): the same bytes, and each checked against the oracle."""
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("RTAMD_WG_POOL", knob)
        dev, sc = _build(rtc, bomberman, scene)
        out[knob] = _check_intersect(rtc, po, bomberman, dev, sc, scene, 20011, f"{scene} RTAMD_WG_POOL={knob} 20011 rays")
        sc.release()
        dev.release()
    assert out["0"].tobytes() == out["1"].tobytes()


def test_root_cull_survivor_lists_go_through_the_pool(rtc, po, bomberman, monkeypatch):
    """RTAMD_CULL=1 at a batch above Device::tuneCullMinRays (65 536): the pool hands out positions in the survivor lists."""
    monkeypatch.setenv("RTAMD_CULL", "1")
    monkeypatch.setenv("RTAMD_CHUNK", "32")
    n = 70001
    dev, sc = _build(rtc, bomberman, "cbvh.leaf")
    want = _oracle(rtc, po, bomberman, sc, "cbvh.leaf", n)
    got = _trace(dev, sc, _rays(po, bomberman, n))
    assert got.tobytes() == want.tobytes()
    nh = int((got["geomID"] != INVALID).sum())
    cnt = sc.intersect1M_counted(_rays(po, bomberman, n))
    print(f"[pool] root cull {n} rays: rays {cnt['rays']}, survivors {cnt['reserved']}, hits {cnt['hits']} of {nh}")
    assert 0 < cnt["reserved"] < n, "the pre-pass did not run"
    assert cnt["rays"] == n and cnt["hits"] == nh and cnt["stackSpills"] == 0
    sc.release()
    dev.release()


@pytest.mark.parametrize("scene", ["cbvh.leaf", "tri"])
def test_many_grabs_per_workgroup(rtc, po, bomberman, monkeypatch, scene):
    """RTAMD_CHUNK=32 and RTAMD_BLOCKS_PER_CU=1: one workgroup per CU, each global grab brings 128 rays, and 200 003 rays are more than six
    grabs for every workgroup of a 256-CU chip (more on a smaller one) - republication while siblings fetch-add, the hand-back of the state
    when the pool was refilled meanwhile, and compare-and-swap contention after the first grab all happen by construction."""
    monkeypatch.setenv("RTAMD_CHUNK", "32")
    monkeypatch.setenv("RTAMD_BLOCKS_PER_CU", "1")
    dev, sc = _build(rtc, bomberman, scene)
    _check_intersect(rtc, po, bomberman, dev, sc, scene, 200003, f"{scene} chunk 32, one workgroup per CU, 200003 rays")
    _check_occluded(rtc, po, bomberman, dev, sc, scene, 200003, f"{scene} occluded chunk 32, one workgroup per CU, 200003 rays")
    sc.release()
    dev.release()
