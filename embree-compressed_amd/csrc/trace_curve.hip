// Ribbon leaves of the quantized BVH8: flat Bezier and B-spline curves (RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE / _FLAT_BSPLINE_CURVE).
// 80-byte records (CurveRecord, accel.h) fetched as five dwordx4: the four native (Bezier) control points with their radii in w, then
// geomID, primID and the tessellation rate N of the curve's geometry.  The leaf restates Ribbon1Intersector1 + intersect_ribbon
// (kernels/geometry/bezier_ribbon_intersector.h:80-201) + intersect_quad_backface_culling (quad_intersector.h:28-90):
//   ray space     line_space() of the line leaves (trace_line.hip.h) with the z row scaled by s once more (ray_space.vz *= depth_scale), so
//                 a transformed z is a ray parameter; the four control points go there, w = radius kept
//   segment j     of N runs from the curve point at float(j) / float(N) to the one at float(j + 1) / float(N): position (x, y, z, w) and
//                 derivative (x, y) by the nested madd of eval0 / eval1 / derivative0 / derivative1 (bezier_curve.h:227-268) over the
//                 float32 values of BezierBasis::eval / derivative (bezier_curve.cpp:21-40).  The reference reads those from two tables
//                 (bezier_basis0 / bezier_basis1); they are pure float32 arithmetic on float(j + dj) / float(N) and are recomputed here
//                 per lane - the same bits (docs/experiments.md has the measurement against a table).  basis1[N][j] and basis0[N][j + 1]
//                 are the same number, so the end of segment j IS the start of segment j + 1, bit for bit: the lane form carries it over
//   quad          normal n = normalize((dp.y, -dp.x, 0)), corners p -+ p.w * n; the ray is the origin along +z, so every dot with D =
//                 (0, 0, 1) is the z component of a cross product, kept in its msub form.  A zero derivative makes n, and with it both
//                 corners of that end, NaN in x and y; max(U, V) is then NaN (max(a, b) = a > b ? a : b as _mm_max_ps, and one NaN end
//                 reaches both edge functions) and the quad is not hit, as in the reference.  n.z = 0 * rsqrt is taken as 0: where it is
//                 NaN the quad is missed through x and y anyway, and p.z + w * 0 differs from p.z at most in the sign of a zero
//   culling       the reference's cylinder_culling_test (:74-78, :98) only switches lanes off before the quad test: a lane it rejects has
//                 the origin farther from the segment's axis than max(r0, r1), and the edge tests of the quad then fail for it - up to
//                 rounding, where the reference may drop a hit that the quad test alone would report.  It saves the reference the normal
//                 and the quad test when all 8 lanes are off; here those are a few dozen VALU operations per lane and the test would be
//                 one more divergent branch.  Dropped: a candidate is decided by the quad test alone (the float64 truth of the tests has
//                 no culling either)
//   self hits     t > tnear + 2 * lerp(r0, r1, u) * s
//   hit           u = ((k + U) + base) * (1 / N) for lane k of the pass starting at segment `base`, v = 2 V - 1, Ng = eval_du(u) of the
//                 WORLD control points with BezierBasis::derivative (RibbonHit, :38-49)
// Block and tie rule: the records of a leaf one after the other in stored order, each against the tfar the previous one left; inside a
// curve the segments in passes of 8 (the reference's 8-wide build), all of a pass against the tfar at pass entry, one minimum per pass,
// the lowest segment wins an equal t; a later pass or record wins an equal t (`<=` in the depth test).  Any-hit ends at the first valid
// segment.  The depth test is the reference's `T <= absDen * tfar`, not `t <= tfar`, and the tfar a hit leaves is fl(T / den): a later,
// bit-identical candidate passes exactly when absDen * fl(T / den) does not round below T (on the 40 rays of the tie test it rounds
// below for 3 of 21 hits) - otherwise the earlier one keeps the hit, here as in the reference.
// Forms: lane-per-ray and octet (child-parallel).  No ray-pool form and no service kernel: the pool skeleton is compiled for two
// waves per SIMD and would be a second kernel family to hold to the resource bounds for a leaf whose cost is arithmetic, not traversal.
// One arithmetic serves the robust and the fast accel; only the node test differs.
#include "trace_curve.hip.h"

namespace rtamd {

hipError_t launch_trace_curve(const LaunchParams& p, hipStream_t stream)
{
  if (p.roundCurves) return launch_trace_round_curve(p, stream); // the records are tubes (Scene::roundCurveAccel): trace_round_curve.hip
#ifdef CURVE_BASIS_TABLE
  static bool uploaded = false;
  if (!uploaded) {
    static float4 t[17][17][2];
    for (int n = 0; n <= 16; n++)
      for (int j = 0; j <= 16; j++) {
        const float t1 = (float)j / (float)n, t0 = 1.0f - t1;
        t[n][j][0] = make_float4(t0 * t0 * t0, 3.0f * t1 * (t0 * t0), 3.0f * (t1 * t1) * t0, t1 * t1 * t1);
        t[n][j][1] = make_float4(3.0f * -(t0 * t0), 3.0f * fmaf(-2.0f, t0 * t1, t0 * t0), 3.0f * fmaf(2.0f, t0 * t1, -(t1 * t1)), 3.0f * (t1 * t1));
      }
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(dev::curve_basis_table), t, sizeof(t));
    if (e != hipSuccess) return e;
    uploaded = true;
  }
#endif
  // one leaf; robust traversal for RTC_SCENE_FLAG_ROBUST scenes, fast traversal otherwise; lane kernel only (rt_trace.cpp launch_on never
  // asks for the ray-pool skeleton on this accel)
  return p.accel.kind == ACCEL_CURVE_ROBUST ? dev::launch_leaf<dev::CurveLeaf, true>(p, stream) : dev::launch_leaf<dev::CurveLeaf, false>(p, stream);
}

} // namespace rtamd
