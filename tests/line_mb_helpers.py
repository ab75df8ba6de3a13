"""Shared by the tests of motion blur on line segments (tests/test_host_line_motion_blur.py, tests/test_gpu_line_motion_blur.py): the
LineMBRecord layout, the geometry of a moving line geometry at a ray time, the pinned moving tuft and the truth the GPU leaf is held to.

The truth of a moving scene is the truth of tests/line_helpers.py on the geometry AT the ray's time: getTimeSegment (kernels/common/
geometry.h:28-34) plus lerp(p0, p1, f) = (1 - f) p0 + f p1 on all four components, radius included (linei.h:276-277).  The inputs are
chosen so that every interpolated value is exact in float32; at_time() computes in float64 and asserts that, so the static truth (and the
static GPU kernel) can be handed the very vertices the motion-blur leaf computes."""
import numpy as np

import line_helpers as lh
from mb_linear_helpers import rot_y, snap

ACCEL_LINEMB_ROBUST, ACCEL_LINEMB_FAST, ACCEL_LINEMB_LINEAR_ROBUST, ACCEL_LINEMB_LINEAR_FAST = 38, 39, 40, 41
LINEMB_DT = np.dtype([("v0a", "<f4", 3), ("r0a", "<f4"), ("v1a", "<f4", 3), ("r1a", "<f4"), ("v0b", "<f4", 3), ("r0b", "<f4"), ("v1b", "<f4", 3), ("r1b", "<f4"),
                      ("geomID", "<u4"), ("primID", "<u4"), ("segment", "<u4"), ("numSegments", "<u4")])
assert LINEMB_DT.itemsize == 80


def time_segment64(time, num_segments):
    """getTimeSegment in float64: (itime, ftime); times outside [0, 1] extrapolate the first / last segment"""
    ts = float(time) * num_segments
    it = int(min(max(np.floor(ts), 0.0), num_segments - 1.0))
    return it, ts - it


def at_time(steps, time):
    """verts4 [nv, 4] float32 of a moving line geometry (steps: N arrays [nv, 4] = x, y, z, radius) at `time`: getTimeSegment and the lerp
    of all four components in float64; asserts that every value is exact in float32 (so is the kernel's fmaf(1 - f, p0, f * p1) then)"""
    it, f = time_segment64(time, len(steps) - 1)
    assert np.float32(f) == f and np.float32(1.0 - f) == 1.0 - f
    p0, p1 = np.asarray(steps[it], np.float32).astype(np.float64), np.asarray(steps[it + 1], np.float32).astype(np.float64)
    assert np.array_equal((f * p1).astype(np.float32).astype(np.float64), f * p1)
    v = (1.0 - f) * p0 + f * p1
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v), "at_time: the interpolated geometry is not exact in float32"
    return out


def interpolated_records(recs, time):
    """The LineRecords (line_helpers.LINE_DT) the LineMBRecords `recs` produce for a ray at `time`, and the mask of the records that
    accept that time (itime == segment); the kernel's arithmetic in float32: fmaf(1 - f, p0, f * p1)"""
    out = np.zeros(len(recs), lh.LINE_DT)
    take = np.zeros(len(recs), bool)
    for i, r in enumerate(recs):
        S = np.float32(r["numSegments"])
        ts = np.float32(np.float32(time) * S)
        it = np.float32(min(max(np.floor(ts), np.float32(0)), S - np.float32(1)))
        f = np.float32(ts - it)
        g = np.float32(np.float32(1) - f)
        take[i] = int(it) == int(r["segment"])
        for a, b, o in (("v0a", "v0b", "v0"), ("r0a", "r0b", "r0"), ("v1a", "v1b", "v1"), ("r1a", "r1b", "r1")):
            out[o][i] = lh.fma32(g, r[a], (f * np.asarray(r[b], np.float32)).astype(np.float32))
    out["geomID"], out["primID"] = recs["geomID"], recs["primID"]
    return out, take


def leaf_rule_mb(recs, org, direction, time, tnear=0.0, tfar=np.inf):
    """line_helpers.leaf_rule on the records of one leaf of a motion-blur line accel: blocks are groups of four RECORDS from the leaf
    start, a record of another time segment keeps its lane and takes no part.  -> (primID, t) or (None, tfar)"""
    rec, take = interpolated_records(recs, time)
    v0 = np.concatenate([rec["v0"], rec["r0"][:, None]], 1)
    v1 = np.concatenate([rec["v1"], rec["r1"][:, None]], 1)
    best = None
    for b in range(0, len(rec), 4):
        valid, T, _, _ = lh.candidates(v0[b:b + 4], v1[b:b + 4], np.asarray([org], np.float32), np.asarray([direction], np.float32), [tnear], [tfar], np.float32)
        tt = np.where(valid[0] & take[b:b + 4], T[0], np.inf)
        k = int(tt.argmin())
        if np.isfinite(tt[k]):
            best, tfar = int(rec["primID"][b + k]), np.float32(tt[k])
    return best, tfar


def segment_box64(v0, v1):
    """LineMi::bounds in float64 of segments given as [n, 4] ends: merge(p0, p1) enlarged by max(r0, r1)"""
    v0, v1 = np.asarray(v0, np.float64), np.asarray(v1, np.float64)
    r = np.maximum(v0[:, 3], v1[:, 3])[:, None]
    return np.minimum(v0[:, :3], v1[:, :3]) - r, np.maximum(v0[:, :3], v1[:, :3]) + r


def record_box_at(recs, time):
    """(lo [k, 3], hi [k, 3], take [k]) in float64: the box of the interpolated segment with interpolated radii of every record that accepts
    `time` on the geometry's own axis (itime == segment), exact arithmetic"""
    lo, hi, take = np.zeros((len(recs), 3)), np.zeros((len(recs), 3)), np.zeros(len(recs), bool)
    for i, r in enumerate(recs):
        it, f = time_segment64(time, int(r["numSegments"]))
        take[i] = it == int(r["segment"])
        e = []
        for a, ra, b, rb in (("v0a", "r0a", "v0b", "r0b"), ("v1a", "r1a", "v1b", "r1b")):
            p0 = np.append(r[a].astype(np.float64), float(r[ra]))
            p1 = np.append(r[b].astype(np.float64), float(r[rb]))
            e.append((1.0 - f) * p0 + f * p1)
        l, h = segment_box64(e[0][None], e[1][None])
        lo[i], hi[i] = l[0], h[0]
    return lo, hi, take


# ---- the pinned moving tuft ------------------------------------------------------------------------------------------------------
def _snap4(xyz, radii):
    """coordinates and radii on multiples of 2^-10"""
    return np.concatenate([snap(xyz), snap(radii)[:, None]], 1).astype(np.float32)


def tuft_steps(nsteps):
    """The time steps of the pinned moving tuft: line_helpers.tuft_and_rays()'s tuft, step k of n rotated about y through its centre and
    translated, radii grown linearly to 1.5 x at the last step, every coordinate and radius snapped to a multiple of 2^-10.
    nsteps == 2: a 20 degree rotation and a move by 0.25 along x; otherwise a curved path: 12 k degrees and the move
    ext * (0.1 k, 0.03 k^2, -0.05 k) of step k (mb_linear_helpers.curved_steps).  -> ([nsteps arrays [2n, 4]], first_index, org, dirs)"""
    v, idx, org, dirs = lh.tuft_and_rays()
    xyz, rad = v[:, :3].astype(np.float64), v[:, 3].astype(np.float64)
    ext = xyz.max(0) - xyz.min(0)
    steps = []
    for k in range(nsteps):
        grow = 1.0 + 0.5 * k / (nsteps - 1)
        if nsteps == 2:
            p = rot_y(xyz, 20.0 * k) + np.array([0.25 * k, 0.0, 0.0])
        else:
            p = rot_y(xyz, 12.0 * k) + ext * np.array([0.1 * k, 0.03 * k * k, -0.05 * k])
        steps.append(_snap4(p, rad * grow))
    return steps, idx, org, dirs


def round_robin_times(m, nsteps):
    """ray times k / (4 S), k = 0 .. 4 S, assigned round-robin: exact in float32, and so is every ftime (a multiple of 1/4)"""
    S = nsteps - 1
    return ((np.arange(m) % (4 * S + 1)) / (4.0 * S)).astype(np.float32)


def moving_truth(steps, idx, org, dirs, times, dtype=np.float64, tnear=None, tfar=None):
    """line_helpers.closest per distinct ray time on at_time(steps, t), gathered into one dict over all rays; tnear / tfar [m] default
    to 0 and inf"""
    m = len(org)
    out = None
    tnear = np.zeros(m, np.float32) if tnear is None else np.asarray(tnear, np.float32)
    tfar = np.full(m, np.inf, np.float32) if tfar is None else np.asarray(tfar, np.float32)
    for t in np.unique(times):
        sel = np.nonzero(times == t)[0]
        v0, v1 = lh.ends(at_time(steps, t), idx)
        c = lh.closest(v0, v1, org[sel], dirs[sel], tnear[sel], tfar[sel], dtype)
        if out is None:
            out = {k: np.zeros((m,) + a.shape[1:], a.dtype) for k, a in c.items()}
        for k, a in c.items():
            out[k][sel] = a
    return out


# what tuft_steps(2) / tuft_steps(5) give with round_robin_times: hits of the float64 truth, and rays within 1e-4 of `d2 <= r2` or of a tie
TUFT_MB_HITS = {2: 3317, 5: 2778}
TUFT_MB_NEAR = {2: 1, 5: 0}
