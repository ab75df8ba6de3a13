"""The root cull pre-pass (csrc/trace_cull.hip.h, RTAMD_CULL=1) runs on exactly the kinds whose row in csrc/accel_kinds.h allows it.

The pre-pass starts at Device::tuneCullMinRays = 65 536 rays per launch, a size no other test reaches for the record families beyond
triangles.  Each case builds the smallest scene whose root is an inner node - 64 primitives in a row, a leaf holds at most 28 - and traces
exactly 65 536 rays on a device with RTAMD_CULL=0 and on one with RTAMD_CULL=1, as a plain batch (device-resident: a host batch of that
size would be cut into pipelined chunks) and as a counted batch.  The four results are byte-identical, and the counted batch reports
survivors of the pre-pass (RTCAMDTraceCounters::reserved) exactly where the kind's row says it runs.  The kinds are not written here: a
case reads its kind from the committed scene and the expectation from rtc.accel_kind_row."""
import numpy as np
import pytest

from helpers import INVALID, fill_rays

pytestmark = pytest.mark.gpu

N, M = 64, 65536
F = np.float32
ROBUST = 4  # RTC_SCENE_FLAG_ROBUST
LINEAR = "mb_bounds=linear"
STEP = np.array([0.0, 0.25, 0.0], F)  # what every vertex moves by between the two time steps


def _corners():
    """[N, 4, 3]: the unit-spaced squares of side 0.8 in the plane z = 0, one per primitive"""
    x = np.arange(N, dtype=F)[:, None, None] * np.array([1, 0, 0], F)
    return x + np.array([[0, 0, 0], [0.8, 0, 0], [0.8, 0.8, 0], [0, 0.8, 0]], F)


def _w(p, r=0.1):
    return np.concatenate([p, np.full(p.shape[:-1] + (1,), r, F)], -1).reshape(-1, 4)


def _tri(sc, mb):
    v = _corners()[:, :3].reshape(-1, 3)
    t = np.arange(3 * N, dtype=np.uint32).reshape(-1, 3)
    return sc.add_triangles_mb([v, v + STEP], t) if mb else sc.add_triangles(v, t)


def _quad(sc, mb):
    v = _corners().reshape(-1, 3)
    q = np.arange(4 * N, dtype=np.uint32).reshape(-1, 4)
    return sc.add_quads_mb([v, v + STEP], q) if mb else sc.add_quads(v, q)


def _line(sc, mb):
    c = _corners()[:, [0, 2]]  # the diagonal of each square
    idx = np.arange(N, dtype=np.uint32) * 2
    return sc.add_lines_mb([_w(c), _w(c + STEP)], idx) if mb else sc.add_lines(_w(c), idx)


def _curve(sc, mb):
    c = _corners()  # the four corners as Bezier control points
    idx = np.arange(N, dtype=np.uint32) * 4
    return sc.add_curves_mb([_w(c), _w(c + STEP)], idx) if mb else sc.add_curves(_w(c), idx)


def _subdiv(sc, mb):
    sc.add_subdiv(_corners().reshape(-1, 3), np.full(N, 4, np.uint32), np.arange(4 * N, dtype=np.uint32))
    sc.set_levels(2, 1)


FAMILIES = {"triangles": _tri, "quads": _quad, "lines": _line, "curves": _curve}
# (id, geometry, moving, scene flags, device config): the eight record families robust and fast, the moving ones also under
# mb_bounds=linear, eager subdivision and bvh4.compressed.leaf
CASES = [(f"{name}{' mb' if mb else ''}{' linear' if cfg else ''} {'robust' if flags else 'fast'}", add, mb, flags, cfg)
         for name, add in FAMILIES.items() for mb, cfg in ((False, ""), (True, ""), (True, LINEAR)) for flags in (ROBUST, 0)]
CASES += [("subdiv eager", _subdiv, False, 0, ""), ("subdiv compressed.leaf", _subdiv, False, 0, "subdiv_accel=bvh4.compressed.leaf")]


def _rays(rtc):
    """seeded; the even rays run between two points of the scene's box (a little enlarged), the odd rays start beyond it and point away"""
    rng = np.random.RandomState(65536)
    lo, hi = np.array([-0.5, -0.5, -0.5]), np.array([N + 0.5, 1.5, 0.5])
    p1, p2 = lo + rng.rand(M, 3) * (hi - lo), lo + rng.rand(M, 3) * (hi - lo)
    org, d = p1.astype(F), (p2 - p1).astype(F)
    org[1::2] = (hi + 5.0).astype(F)
    d[1::2] = np.abs(d[1::2]) + F(0.1)
    rh = rtc.aligned_rayhits(M)
    fill_rays(rh, org, d)
    rh["time"] = rng.rand(M).astype(F)
    return rh


def _run(rtc, monkeypatch, cull, add, mb, flags, cfg, rays):
    import torch
    monkeypatch.setenv("RTAMD_CULL", cull)  # the knobs are read when a device is created
    dev = rtc.Device(cfg)
    sc = rtc.Scene(dev, flags)
    add(sc, mb)
    sc.commit()
    kind = sc.stats()["accelKind"]
    assert sc.accel_root() != INVALID and not sc.accel_root() & 0x80000000, "the root is an inner node"
    plain = torch.from_numpy(rays.view(np.uint8).reshape(M, -1).copy()).cuda()
    torch.cuda.synchronize()
    sc.intersect1M(plain)
    dev.synchronize()
    counted = rays.copy()
    cnt = sc.intersect1M_counted(counted)
    assert dev.error() == 0
    sc.release()
    dev.release()
    return kind, plain.cpu().numpy().reshape(-1).view(rays.dtype), counted, cnt


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_pre_pass_runs_where_the_kinds_row_allows_it(rtc, monkeypatch, case):
    name, add, mb, flags, cfg = case
    rays = _rays(rtc)
    kind, plain0, counted0, cnt0 = _run(rtc, monkeypatch, "0", add, mb, flags, cfg, rays)
    kind1, plain1, counted1, cnt1 = _run(rtc, monkeypatch, "1", add, mb, flags, cfg, rays)
    row = rtc.accel_kind_row(kind)
    hits = int((plain0["geomID"] != INVALID).sum())
    print(f"[launch decisions] {name}: kind {kind}, cull allowed {row['cull']}, {hits} hits, survivors {cnt0['reserved']} / {cnt1['reserved']} of {M}")
    assert kind1 == kind and row is not None
    assert 0 < hits and not (plain0["geomID"][1::2] != INVALID).any()  # the scene is hit, and never by a ray aimed away
    for what, got in (("RTAMD_CULL=0 counted", counted0), ("RTAMD_CULL=1 plain", plain1), ("RTAMD_CULL=1 counted", counted1)):
        assert got.tobytes() == plain0.tobytes(), (name, what)
    assert cnt0["rays"] == M and cnt1["rays"] == M and cnt0["hits"] == hits and cnt1["hits"] == hits
    assert cnt0["reserved"] == 0, "no pre-pass without RTAMD_CULL=1"
    assert (cnt1["reserved"] != 0) == bool(row["cull"]), (name, kind)
    if row["cull"]:
        assert cnt1["reserved"] <= M // 2, "the rays aimed away were culled"


def test_the_cases_cover_every_kind_of_their_launchers(rtc):
    """the scenes of the cases commit to distinct kinds outside any instance, and to every kind that shares a launcher with one of them"""
    kinds = []
    for name, add, mb, flags, cfg in CASES:
        dev = rtc.Device(cfg)
        sc = rtc.Scene(dev, flags)
        add(sc, mb)
        sc.commit()
        kinds.append(sc.stats()["accelKind"])
        sc.release()
        dev.release()
    rows = {k: rtc.accel_kind_row(k) for k in range(64) if rtc.accel_kind_row(k)}
    assert len(set(kinds)) == len(CASES) and all(rows[k]["inst"] == rtc.KIND_INST.index("none") for k in kinds)
    assert {k for k, r in rows.items() if r["launcher"] in {rows[j]["launcher"] for j in kinds}} == set(kinds)
