"""Shared by tests/test_host_cbvh_forms.py, tests/test_gpu_cbvh_forms.py and tools/parity_dryrun.py: the inputs of the cBVH form matrix.

Every fork mode (bvh4.compressed.box / .leaf / .grid / .full) is compiled once per compression level C = 1..5, and each of those in three
forms chosen in launch_cbvh (csrc/trace_cbvh.hip.h): the quad form (four lanes per ray), the one-ray-per-lane form in the lane skeleton
and the one-ray-per-lane form in the ray-pool skeleton (csrc/trace_pool.hip.h); every form again as closest hit / any hit, counted twin /
plain and for 16-byte aligned / other records.  The addresses inside a blob are compile-time functions of C and the mode, so the matrix
is walked on one small mesh: the first 32 faces of bomberman (52 vertices on the 2^-10 grid), 20 000 random rays through its bounding
box, and level pairs (L, C) that cover every C, L == C (one blob per patch: the outer BVH8 ends directly on whole patches) at the
shallowest, a middle and the deepest level, and 32 or 128 blobs."""
import numpy as np

import instance_subdiv_helpers as isd
from helpers import FORK_MODES, FORK_ORACLE_MODE, INVALID, ORDERED_FORK

PAIRS = [(1, 1), (2, 1), (3, 2), (3, 3), (5, 4), (5, 5), (6, 5)]  # (L, C)
MODES = FORK_MODES
FORMS = ("quad", "lane", "pool")
NRAYS = 20_000
FACES = 32
HITS_FLOOR = 2000  # below the smallest pinned hit count of tests/test_host_cbvh_forms.py (EXPECTED)
KNOBS = ("RTAMD_KERNEL", "RTAMD_CBVH_FORM")


def mesh(bomberman):
    """(verts, face sizes, face indices) of the 32-face mesh"""
    return isd.bomberman_faces(bomberman, FACES)


def blob_count(L, C):
    return FACES * 4 ** (L - C)


def make_rays(po, verts, n=NRAYS):
    """RTCRayHit records, 16-byte aligned"""
    return po.make_random_rays(n, verts.min(0), verts.max(0), seed=3, double_eval=True)


def occ_of(rtc, rays):
    """the RTCRay part (first 48 bytes) of RTCRayHit records, 16-byte aligned"""
    occ = rtc.aligned_rays(len(rays))
    for f in occ.dtype.names:
        occ[f] = rays[f]
    return occ


def set_form(monkeypatch, form):
    """the knobs that select a kernel form; they are read in the Device constructor, so call this BEFORE the device is created.
    "quad": the library's defaults (no knob set)."""
    assert form in FORMS
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if form == "lane":
        monkeypatch.setenv("RTAMD_CBVH_FORM", "lane")
        monkeypatch.setenv("RTAMD_KERNEL", "lane")
    elif form == "pool":
        monkeypatch.setenv("RTAMD_KERNEL", "pool")


def build(rtc, monkeypatch, accel, L, C, form, m, cfg=""):
    """(device, committed scene) of mesh `m` under subdiv_accel=`accel` at levels (L, C), traced by kernel form `form`;
    cfg: a prefix of the device's config string such as "gpu=none" or "service=1"."""
    set_form(monkeypatch, form)
    dev = rtc.Device((cfg + "," if cfg else "") + "subdiv_accel=" + accel)
    sc = rtc.Scene(dev)
    assert sc.add_subdiv(*m) == 0
    sc.set_levels(L, C)
    sc.commit()
    return dev, sc


def oracle(po, sc, accel, C, same_tree=None):
    """the oracle over the scene's exported blobs.  same_tree (default: for the order-dependent modes box / leaf / full): it walks the
    product's outer BVH8, so it reaches the blobs in the kernels' order; otherwise it builds a full-precision tree of its own."""
    if same_tree is None:
        same_tree = accel in ORDERED_FORK
    stride = sc.stats()["primBytes"]
    if same_tree:
        return po.SubdivScene(sc.accel_data(2), stride, FORK_ORACLE_MODE[accel], C, qnodes=sc.accel_data(0), root=sc.accel_root())
    return po.SubdivScene(sc.accel_data(2), stride, FORK_ORACLE_MODE[accel], C)


def hits_of(rays):
    return int((rays["geomID"] != INVALID).sum())


def occluded_of(occ):
    return int((occ["tfar"] == -np.inf).sum())


def differing(a, b):
    """number of records whose bytes differ"""
    size = a.dtype.itemsize
    return int((a.view(np.uint8).reshape(-1, size) != b.view(np.uint8).reshape(-1, size)).any(1).sum())


def expected(po, sc, accel, C, src):
    """(closest-hit records of the oracle in product arithmetic, the same in reference arithmetic, any-hit records of the oracle on its
    own tree) for the RTCRayHit records `src`"""
    orc = oracle(po, sc, accel, C)
    prod, ref = src.copy(), src.copy()
    with po.fork_arith(1):
        orc.intersect1M(prod, nthreads=8)
    orc.intersect1M(ref, nthreads=8)
    orc.free()
    own = oracle(po, sc, accel, C, same_tree=False)
    occ = np.zeros(len(src), dtype=[(n, src.dtype[n]) for n in src.dtype.names[:12]])
    for f in occ.dtype.names:
        occ[f] = src[f]
    own.occluded1M(occ, nthreads=8)
    own.free()
    return prod, ref, occ
