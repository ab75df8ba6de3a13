"""Shared by the tests of motion blur on flat cubic curves (tests/test_host_curve_motion_blur.py, tests/test_gpu_curve_motion_blur.py):
the CurveMBRecord layout, the control points of a moving curve geometry at a ray time, the pinned moving hair and the truth the GPU leaf
is held to.

The truth of a moving scene is the truth of tests/curve_helpers.py on the geometry AT the ray's time: getTimeSegment (kernels/common/
geometry.h:28-34) plus lerp(p0, p1, f) = (1 - f) p0 + f p1 of the four NATIVE control points on all four components, radius included
(NativeCurves::gather with a time, scene_bezier_curves.h:138-158).  The pinned inputs are chosen so that every interpolated value is exact
in float32; at_time() computes in float64 and asserts that, so the static truth (and the static GPU kernel) can be handed the very
control points the motion-blur leaf computes.  B-spline input is converted to Bezier points PER STEP and then interpolated."""
import numpy as np

import curve_helpers as ch
from line_mb_helpers import round_robin_times, time_segment64  # noqa: F401  (re-exported)
from mb_linear_helpers import rot_y

ACCEL_CURVEMB_ROBUST, ACCEL_CURVEMB_FAST, ACCEL_CURVEMB_LINEAR_ROBUST, ACCEL_CURVEMB_LINEAR_FAST = 44, 45, 46, 47
# va[k] / vb[k] = (x, y, z, radius) of native control point k at the start / end of the record's time segment
CURVEMB_DT = np.dtype([("va", "<f4", (4, 4)), ("vb", "<f4", (4, 4)), ("geomID", "<u4"), ("primID", "<u4"), ("segment", "<u4"), ("numSegments", "<u4"),
                       ("N", "<u4"), ("pad", "<u4", 3)])
assert CURVEMB_DT.itemsize == 160


def snap16(v):
    """multiples of 2^-16 (2^-10, the grid of the moving lines, is too coarse for radii of 0.004 .. 0.012)"""
    return np.round(np.asarray(v, np.float64) * 65536.0) / 65536.0


def lerp_exact(p0, p1, f):
    """(1 - f) p0 + f p1 in float64 of float32 inputs; asserts that f, 1 - f, f * p1 and the result are exact in float32 (so is the
    kernel's fmaf(1 - f, p0, f * p1) then)"""
    assert np.float32(f) == f and np.float32(1.0 - f) == 1.0 - f
    p0, p1 = np.asarray(p0, np.float32).astype(np.float64), np.asarray(p1, np.float32).astype(np.float64)
    assert np.array_equal((f * p1).astype(np.float32).astype(np.float64), f * p1)
    v = (1.0 - f) * p0 + f * p1
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v), "at_time: the interpolated geometry is not exact in float32"
    return out


def at_time(steps, time):
    """verts4 [nv, 4] float32 of a moving BEZIER curve geometry (steps: N arrays [nv, 4] = x, y, z, radius) at `time`; exact (lerp_exact)"""
    it, f = time_segment64(time, len(steps) - 1)
    return lerp_exact(steps[it], steps[it + 1], f)


def native_steps(steps, idx, basis="bezier"):
    """the native (Bezier) control points [n, 4, 4] float32 of every time step"""
    return [ch.native(s, idx, basis) for s in steps]


def native_at_time(nat, time, exact=True):
    """the native control points [n, 4, 4] at `time` from the per-step native points: exact (asserted) or, for B-spline input whose converted
    points are not on a grid, the kernel's float32 fmaf(1 - f, p0, f * p1)"""
    it, f = time_segment64(time, len(nat) - 1)
    if exact:
        return lerp_exact(nat[it], nat[it + 1], f)
    f32 = np.float32(f)
    g = np.float32(np.float32(1) - f32)
    return ch.fma32(g, nat[it], (f32 * nat[it + 1]).astype(np.float32))


def interpolated_records(recs, time):
    """(cp [k, 4, 4] float32, take [k]): the native control points the CurveMBRecords `recs` give a ray at `time` in the kernel's float32
    arithmetic - time_segment() then fmaf(1 - f, a, f * b) - and the mask of the records that accept that time (itime == segment)"""
    S = recs["numSegments"].astype(np.float32)
    ts = (np.float32(time) * S).astype(np.float32)
    it = np.minimum(np.maximum(np.floor(ts), np.float32(0)), S - np.float32(1)).astype(np.float32)
    f = (ts - it).astype(np.float32)
    g = (np.float32(1) - f).astype(np.float32)
    take = it.astype(np.int64) == recs["segment"].astype(np.int64)
    cp = ch.fma32(g[:, None, None], recs["va"], (f[:, None, None] * recs["vb"]).astype(np.float32))
    return cp, take


def record_box_at(recs, time):
    """(lo [k, 3], hi [k, 3], take [k]) in float64: curve_helpers.tessellated_bounds of the exactly interpolated control points of every
    record, at the record's own rate N; take: the record accepts `time` (itime == segment on the geometry's own axis)"""
    lo, hi, take = np.zeros((len(recs), 3)), np.zeros((len(recs), 3)), np.zeros(len(recs), bool)
    for S in np.unique(recs["numSegments"]):
        it, f = time_segment64(time, int(S))
        for N in np.unique(recs["N"]):
            sel = (recs["numSegments"] == S) & (recs["N"] == N)
            take[sel] = recs["segment"][sel] == it
            cp = (1.0 - f) * recs["va"][sel].astype(np.float64) + f * recs["vb"][sel].astype(np.float64)
            lo[sel], hi[sel] = _bounds64(cp, int(N))
    return lo, hi, take


def _bounds64(cp, N):
    """tessellated_bounds in float64 of float64 control points (curve_helpers.tessellated_bounds rounds its input to float32 first)"""
    u = np.arange(N) / np.float64(N)
    b = [x[None, :, None] for x in ch.bezier_basis(u, np.float64)]
    p = ch.combine(b, cp[:, None, 0], cp[:, None, 1], cp[:, None, 2], cp[:, None, 3], np.float64)
    p = np.concatenate([p, cp[:, None, 3]], 1)
    r = np.abs(p[..., 3]).max(1)[:, None]
    return p[..., :3].min(1) - r, p[..., :3].max(1) + r


# ---- the pinned moving hair ----------------------------------------------------------------------------------------------------------
def hair_steps(nsteps):
    """The time steps of the pinned moving hair: curve_helpers.hair_and_rays()'s hair, step k of n rotated about y through its centre and
    translated exactly as line_mb_helpers.tuft_steps moves its tuft, radii grown linearly to 1.5 x at the last step, every coordinate and
    radius snapped to a multiple of 2^-16.  nsteps == 2: 20 degrees and 0.25 along x per step; otherwise 12 k degrees and the move
    ext * (0.1 k, 0.03 k^2, -0.05 k) of step k.  -> ([nsteps arrays [4n, 4]], first_index, org, dirs)"""
    v, idx, org, dirs = ch.hair_and_rays()
    xyz, rad = v[:, :3].astype(np.float64), v[:, 3].astype(np.float64)
    ext = xyz.max(0) - xyz.min(0)
    steps = []
    for k in range(nsteps):
        grow = 1.0 + 0.5 * k / (nsteps - 1)
        if nsteps == 2:
            p = rot_y(xyz, 20.0 * k) + np.array([0.25 * k, 0.0, 0.0])
        else:
            p = rot_y(xyz, 12.0 * k) + ext * np.array([0.1 * k, 0.03 * k * k, -0.05 * k])
        steps.append(np.concatenate([snap16(p), snap16(rad * grow)[:, None]], 1).astype(np.float32))
    return steps, idx, org, dirs


def moving_truth(nat, N, org, dirs, times, dtype=np.float64, exact=True, geom_id=0, tnear=None, tfar=None):
    """curve_helpers.closest per distinct ray time on native_at_time(nat, t), gathered into one dict over all rays; tnear / tfar [m]
    default to 0 and inf"""
    m = len(org)
    out = None
    tnear = np.zeros(m, np.float32) if tnear is None else np.asarray(tnear, np.float32)
    tfar = np.full(m, np.inf, np.float32) if tfar is None else np.asarray(tfar, np.float32)
    for t in np.unique(times):
        sel = np.nonzero(times == t)[0]
        c = ch.closest([(native_at_time(nat, t, exact), N, geom_id)], org[sel], dirs[sel], tnear[sel], tfar[sel], dtype)
        if out is None:
            out = {k: np.zeros((m,) + a.shape[1:], a.dtype) for k, a in c.items()}
        for k, a in c.items():
            out[k][sel] = a
    return out


# what hair_steps(2) / hair_steps(5) give with round_robin_times at the rates 4 and 9 (Bezier input): hits of the float64 truth, and the
# rays its two exclusion rules (near_edge | near_tie) leave out, of 2048
HAIR_MB_HITS = {(2, 4): 1164, (2, 9): 1171, (5, 4): 872, (5, 9): 890}
HAIR_MB_LEFT_OUT = {(2, 4): 4, (2, 9): 4, (5, 4): 3, (5, 9): 1}
_TRUTH = {}


def hair_mb_truth(nsteps, N, basis="bezier"):
    """the float64 truth of the pinned moving hair (as Bezier or as B-spline control points) with round-robin times; computed once per
    process and never changed.  -> dict of closest() plus "steps", "idx", "org", "dirs", "times", "nat" """
    key = (nsteps, N, basis)
    if key not in _TRUTH:
        steps, idx, org, dirs = hair_steps(nsteps)
        times = round_robin_times(len(org), nsteps)
        nat = native_steps(steps, idx, basis)
        t = moving_truth(nat, N, org, dirs, times, np.float64, exact=basis == "bezier")
        t.update(steps=steps, idx=idx, org=org, dirs=dirs, times=times, nat=nat)
        _TRUTH[key] = t
    return _TRUTH[key]
