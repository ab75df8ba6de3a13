"""The subdivision kernels against the surface itself: the records of rtcIntersect1M / rtcOccluded1M are held directly to the float64 brute-force tracer of
tests/cbvh_truth_helpers.py (every ray against both triangles of every cell of the kept vertex grids), not to the oracle and not through the product's blobs.

Same cases, rays and truth arrays as tests/test_host_cbvh_ray_truth.py, which pins the expected side on the oracle alone (cbvh_truth_helpers.PINNED); the brute force
runs on the host inside the test (2 to 6 s per case, once per case).  Per case and mode the default kernel form (the quad form; compressed.grid and eager: the
library's own choice) traces the 20 000 rays once:

  eager, compressed.grid   the truth's hit set and patch IDs exactly (rays whose truth hit lies within 1e-6 of a triangle's border may be set aside, at most 0.1 % of
                           the truth hits), t within 4 x the oracle's pinned largest error of that case: kernel and oracle round the same float32 expressions in
                           different orders, neither is the more exact one.  The measured maximum is printed (DESIGN.md section 9 records it).
  box, leaf, full          no true hit lost, hits more than 1e-3 behind the true surface within the host test's bound, total hits within the flip allowance (2) of the
                           host-pinned count.
  eager, any hit           rtcOccluded1M reports exactly the rays the truth hits, with the same set-aside.

The lane and pool forms, the counted twins and the unaligned-record twins need no legs here: tests/test_gpu_cbvh_forms.py demands the quad form's bytes from each."""
import numpy as np
import pytest

import cbvh_forms_helpers as cf
import cbvh_truth_helpers as th

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mesh,L,C", th.RAY_CASES)
@pytest.mark.parametrize("accel", th.RAY_MODES)
def test_kernels_against_the_surface(rtc, po, bomberman, monkeypatch, accel, mesh, L, C):
    m, src, t, pid, mg, aligned = th.ray_truth(rtc, po, bomberman, mesh, L, C)
    mode = accel.split(".")[-1]
    hits, farther, nearer, maxrel = th.PINNED[(mesh, L, C)][mode]
    truth = int(np.isfinite(t).sum())
    assert truth == th.PINNED[(mesh, L, C)]["truth"]
    dev, sc = cf.build(rtc, monkeypatch, accel, L, C, "quad", m)
    rec = rtc.aligned_rayhits(len(src))
    rec[:] = src
    sc.intersect1M(rec)
    st = th.truth_stats(rec, t, pid, mg)
    st.pop("far_rays")
    print(f"[gpu truth] {mesh} L{L} C{C} {mode}: {st}")
    assert st["aside"] <= th.MARGIN_CAP * truth
    assert st["lost"] == 0, st
    if mode in ("default", "grid"):
        assert st["added"] == 0 and st["ids"] == 0, st
        print(f"[gpu truth] {mesh} L{L} C{C} {mode}: largest relative error of t {st['maxrel']:.3g} (oracle {maxrel:.3g}, bound {4 * maxrel:.3g})")
        assert st["maxrel"] <= 4 * maxrel, (st["maxrel"], maxrel)
    else:
        assert st["farther"] <= (th.FLIPS if mesh == "bomb32" else farther + th.FLIPS), st
        assert abs(st["hits"] - hits) <= th.FLIPS, (st["hits"], hits)
    if mode == "default":
        occ = cf.occ_of(rtc, src)
        before = occ.copy()
        sc.occluded1M(occ)
        occluded = occ["tfar"] == -np.inf
        want = np.isfinite(t)
        differ = occluded != want
        aside = differ & (mg < th.MARGIN)
        print(f"[gpu truth] {mesh} L{L} C{C} any hit: {int(occluded.sum())} occluded, {int(differ.sum())} differ from the truth, {int(aside.sum())} set aside")
        assert int((differ & ~aside).sum()) == 0 and int(aside.sum()) <= th.MARGIN_CAP * truth
        assert occ[~occluded].tobytes() == before[~occluded].tobytes()
    assert dev.error() == rtc.RTC_ERROR_NONE
    sc.release()
    dev.release()
