"""Invalid rays on instances of subdivision scenes, after tests/edge_rays_helpers.py and section 4 of tests/test_gpu_edge_rays.py: ten
rays of a batch of 40 000 are poisoned - NaN / infinite origin, direction, tnear, tfar, time = NaN, +inf, -3, 7, a null direction, an
inverted range (tnear > tfar) - and every OTHER record must be byte for byte that of the clean batch.  What a poisoned ray reports itself
is not checked.

Why no poisoned field can form an out-of-range index in trace_instance_subdiv.hip:
  * both node steps are those of the mesh kernels: org / dir / tnear / tfar reach slab tests only; fmaxf / fminf drop a NaN operand, so
    a NaN slab distance lets the ray enter every child at most - 7 stacked entries per level plus the exit marker, which is what the
    host reserves (7 (maxDepth + 1) + 2); a push beyond that is dropped behind a bounds check and raises the overflow word (the test
    would see dev.error() != 0), a pop beyond it returns EMPTY.  The octant only selects between words already loaded.  A ray with
    tnear > tfar or a NaN in either is skipped at the fetch (`tnear <= tfar` fails).
  * the InstanceRecord is addressed by the top-level leaf reference; time only picks InstanceStep[itime], [itime + 1] with
    itime = clamp(floor(time S), 0, S - 1), in range for every input (NaN -> 0, +inf -> S - 1), and the instance owns S + 1 steps; a
    lerped matrix that is not finite is refused by instance_world2local (the ray does not enter, nothing is pushed).
  * below an instance the leaf is addressed by the rebased leaf reference, never by a ray value.  GridCellLeaf::intersect indexes its
    40 cell words with compile-time constants; a non-finite local ray fails the edge tests.  CbvhLeaf::intersect forms the child
    index 4 * curr + 1 + k from the loop counters of the fixed-depth quadtree walk and reads its LDS tables with 3-bit fields of the
    node word; ray values enter comparisons only - the frustum test `near <= far && near1 == near1 && far1 == far1` is false for a NaN,
    the slab tests of the walk drop NaN operands like the outer ones, and a hit only writes u, v, t and the ids of the blob's header."""
import numpy as np
import pytest

import edge_rays_helpers as er
import instance_helpers as ih
import instance_quads_helpers as iq
import instance_subdiv_helpers as isd
from helpers import INVALID

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("accel", isd.FAMILIES)
def test_invalid_rays_leave_the_others_alone(rtc, bomberman, accel):
    meshes = {"m": isd.bomberman_faces(bomberman) + (3, 2)}
    inst = isd.lattice_instances(9)
    g, k, s = inst[4]
    inst[4] = (g, k, [s[0], ih.affine((45.0, 38.0, 2.0), (1.0,) * 3), ih.affine((50.0, 44.0, -1.0), (1.0,) * 3)])  # one of them moves: ray.time is read
    dev, top, inner = isd.build(rtc, accel, meshes, inst)
    assert top.stats()["accelKind"] == isd.KIND[accel]
    n = 40_000
    clean = er.with_times(isd.crossing_rays(rtc, meshes, inst, n, 91))
    want = iq.copy(rtc, clean)
    top.intersect1M(want)
    nh = int((want["geomID"] != INVALID).sum())
    print(f"invalid rays, {accel}: {nh} hits of the clean batch in {len(np.unique(want['instID'][want['geomID'] != INVALID]))} instances")
    assert nh > 1000
    bad = np.arange(100, n, 4001)  # ten rays
    assert len(bad) == 10
    fields = ["org_x", "dir_y", "tnear", "tfar", "dir_z", "org_z", "time", "time", "time", "time"]
    values = [np.nan, np.nan, np.nan, np.nan, np.inf, -np.inf, np.nan, np.inf, -3.0, 7.0]

    def poison(recs):
        for j, i in enumerate(bad):
            recs[fields[j]][i] = values[j]
        recs["dir_x"][bad[-1]] = recs["dir_y"][bad[-1]] = recs["dir_z"][bad[-1]] = 0.0  # null direction
        recs["tnear"][bad[-2]], recs["tfar"][bad[-2]] = 5.0, 1.0  # inverted range

    dirty = iq.copy(rtc, clean)
    poison(dirty)
    top.intersect1M(dirty)
    keep = np.ones(n, bool)
    keep[bad] = False
    assert dirty[keep].tobytes() == want[keep].tobytes()
    assert dirty[bad[-2]].tobytes() != want[bad[-2]].tobytes() and dirty["geomID"][bad[-2]] == INVALID and dirty["tfar"][bad[-2]] == 1.0  # skipped
    wocc = iq.occ_of(rtc, clean)
    top.occluded1M(wocc)
    occ = iq.occ_of(rtc, clean)
    poison(occ)
    top.occluded1M(occ)
    assert occ[keep].tobytes() == wocc[keep].tobytes()
    assert occ["tfar"][bad[-2]] == 1.0
    assert np.all((wocc["tfar"] == -np.inf)[want["geomID"] != INVALID])
    assert dev.error() == 0
    isd.release(dev, top, inner)
