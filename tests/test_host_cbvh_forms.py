"""CPU side of the cBVH form matrix (tests/cbvh_forms_helpers.py, tests/test_gpu_cbvh_forms.py): pins what the GPU test expects.

On a host-only device (gpu=none: builders only) and the oracle alone, per (mode, L, C):
  1. the oracle's hit count in product arithmetic (the arithmetic of the kernels: the GPU test's regression leg demands these very bytes) and the
     occluded count of the oracle on its own full-precision tree are pinned in EXPECTED; the GPU test's floor of 2000 hits lies below all of them;
  2. the classified comparison oracle(product arithmetic) vs oracle(reference arithmetic) passes with the default floors - the dry run of the
     GPU test's parity leg (the kernels are byte-identical to the first, so this IS the comparison the GPU test makes);
  3. the two arithmetics differ in the bytes of far more records than the regression leg's allowance of one: on these 20 000 rays the byte
     comparison notices a change of arithmetic in every mode (the count is pinned from below at half of what was measured);
  4. the blob count is 32 x 4^(L-C) and the blob stride is the one helpers.cbvh_layout gives for (C, mode) - the kernels take every section
     offset of a blob from C and the mode at compile time."""
import numpy as np
import pytest

import cbvh_forms_helpers as cf
from helpers import CBVH_NODES, assert_fork_classes, cbvh_header, cbvh_layout

# (mode, L, C): (hits of the oracle in product arithmetic, rays occluded on the oracle's own tree, records whose bytes differ between product
# and reference arithmetic) - measured with this file's inputs.  Every case has hundreds of differing records (the t of a hit goes through a
# division and a square root in all four modes), so none has to rely on the parity leg alone.
EXPECTED = {
    ("box", 1, 1): (2986, 3031, 815),
    ("box", 2, 1): (2571, 3666, 723),
    ("box", 3, 2): (2571, 3630, 723),
    ("box", 3, 3): (2983, 3017, 823),
    ("box", 5, 4): (2511, 3351, 714),
    ("box", 5, 5): (2677, 3002, 747),
    ("box", 6, 5): (2488, 3170, 711),
    ("leaf", 1, 1): (2980, 3031, 2739),
    ("leaf", 2, 1): (2570, 3666, 2256),
    ("leaf", 3, 2): (2570, 3630, 1217),
    ("leaf", 3, 3): (2980, 3017, 1177),
    ("leaf", 5, 4): (2511, 3351, 829),
    ("leaf", 5, 5): (2675, 3002, 948),
    ("leaf", 6, 5): (2488, 3170, 796),
    ("grid", 1, 1): (2230, 3024, 676),
    ("grid", 2, 1): (2402, 3115, 710),
    ("grid", 3, 2): (2438, 3153, 716),
    ("grid", 3, 3): (2438, 3015, 715),
    ("grid", 5, 4): (2445, 3107, 713),
    ("grid", 5, 5): (2445, 3002, 711),
    ("grid", 6, 5): (2445, 3050, 698),
    ("full", 1, 1): (2986, 3026, 819),
    ("full", 2, 1): (2571, 3606, 724),
    ("full", 3, 2): (2526, 3363, 715),
    ("full", 3, 3): (2664, 3004, 747),
    ("full", 5, 4): (2465, 3086, 703),
    ("full", 5, 5): (2512, 3000, 706),
    ("full", 6, 5): (2455, 3038, 703),
}
# The oracle's own tree is walked with the reference's rcp (hardware estimate + Newton step), whose last bit is not the same on every CPU: a ray
# that grazes a node box may flip.  The allowance is the one the GPU any-hit comparison has on these rays (max(2, nrays // 20000)).
OCCLUDED_SLACK = 2


def test_the_table_covers_the_matrix_and_the_floor():
    assert set(EXPECTED) == {(a.split(".")[-1], L, C) for a in cf.MODES for L, C in cf.PAIRS}
    assert sorted({C for _, C in cf.PAIRS}) == [1, 2, 3, 4, 5] and sum(L == C for L, C in cf.PAIRS) == 3
    assert min(h for h, _, _ in EXPECTED.values()) >= cf.HITS_FLOOR
    assert min(d for _, _, d in EXPECTED.values()) // 2 > 1  # above the regression leg's allowance (helpers.check_fork_parity)


@pytest.fixture(scope="module")
def inputs(po, bomberman):
    m = cf.mesh(bomberman)
    assert m[0].shape == (52, 3) and len(m[1]) == cf.FACES and np.array_equal(m[0] * 1024, np.round(m[0] * 1024))
    return m, cf.make_rays(po, m[0])


@pytest.mark.parametrize("L,C", cf.PAIRS)
@pytest.mark.parametrize("accel", cf.MODES)
def test_expected_side_of_the_form_matrix(rtc, po, monkeypatch, inputs, accel, L, C):
    m, src = inputs
    mode = accel.split(".")[-1]
    dev, sc = cf.build(rtc, monkeypatch, accel, L, C, "quad", m, cfg="gpu=none")
    # 4. blob count and stride
    payload, tail, stride = cbvh_layout(C, mode)
    st = sc.stats()
    blobs = sc.accel_data(2)
    assert st["primBytes"] == stride and st["primCount"] == cf.blob_count(L, C) and len(blobs) == stride * cf.blob_count(L, C)
    assert CBVH_NODES <= payload <= tail and tail + 64 <= stride < tail + 64 + 128
    B = blobs.reshape(-1, stride)
    for k in (0, len(B) - 1):
        h = cbvh_header(B[k], C, mode)
        assert h["levels"] == C and h["elems"] == (4 ** C - 1) // 3 and h["grid_width"] == 2 ** C + 1
        assert np.all(h["wlo"] <= h["whi"]) and np.isfinite(h["iproj"]).all()  # the tail is where the layout says
    # 1. the pinned counts
    prod, ref, occ = cf.expected(po, sc, accel, C, src)
    hits, occluded, ndiff = cf.hits_of(prod), cf.occluded_of(occ), cf.differing(prod, ref)
    print(f"[cbvh forms] {accel} L{L} C{C}: {hits} hits (product arithmetic), {occluded} occluded (own tree), {ndiff} records differ between the arithmetics")
    want_hits, want_occ, measured_diff = EXPECTED[(mode, L, C)]
    assert hits == want_hits
    assert abs(occluded - want_occ) <= OCCLUDED_SLACK, (occluded, want_occ)
    # every ray with a closest hit lies in a blob's bounds; untouched records of the any-hit query stay as they were
    po_hit = prod["geomID"] != 0xFFFFFFFF
    free = occ["tfar"] != -np.inf
    assert occluded >= hits - OCCLUDED_SLACK and int((po_hit & free).sum()) <= OCCLUDED_SLACK
    assert cf.occ_of(rtc, src)[free].tobytes() == occ[free].tobytes()
    # 2. dry run of the parity leg
    assert_fork_classes(prod, ref, accel, what=f"{accel} L{L} C{C} (oracle, product vs reference arithmetic)", cell=2.0 ** -L)
    # 3. the byte comparison would notice the other arithmetic
    assert ndiff >= measured_diff // 2 and ndiff > 1, (ndiff, measured_diff)
    sc.release()
    dev.release()
