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
namespace dev {

struct CurveLeaf : LeafTraits
{
  // Three waves per SIMD, the bound of the line leaves (at most 168 VGPRs): profiles/curve_kernel_resources.txt
  static constexpr int MIN_WAVES = 3;

  // Child-parallel form (trace_loop.hip.h): one record per pass - lane k of the octet tests segment base + k of the curve, every lane
  // against the tfar at pass entry; ONE 8-lane minimum, the lowest lane with that t wins and writes the hit into the row (words 0..7 =
  // t, Ng, u, v, geomID, primID; word 9 = 1).  A curve with N > 8 takes a second pass, which sees the first one's tfar.  Row word 10 is
  // the ray's index.  The loops are wave-uniform (every octet runs as many passes as the longest one; the others are masked).
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const CurveRecord* __restrict__ recs = (const CurveRecord*)P.accel.blobs;
    const uint32_t k = lid & 7u;
    const RayState r = row_ray(x);
    const LineSpace S = line_space(r);
    const uint32_t ref = __float_as_uint(x[8]);
    uint32_t first, cnt;
    leaf_range(ref, first, cnt);
    cnt = valid ? cnt : 0u;
    float tfar = r.tfar;
    for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i++) {
      const bool present = i < cnt;
      const float4* lp = (const float4*)(recs + first + (present ? i : 0u));
      const float4 V0 = lp[0], V1 = lp[1], V2 = lp[2], V3 = lp[3];
      const uint4 ids = *(const uint4*)(lp + 4); // geomID, primID, N, pad
      uint32_t N = present ? ids.z : 0u;
      const float4 w0 = to_ray_space(r, S, V0), w1 = to_ray_space(r, S, V1), w2 = to_ray_space(r, S, V2), w3 = to_ray_space(r, S, V3);
      for (uint32_t base = 0; __ballot(base < N) != 0ull; base += 8u) {
        const uint32_t j = base + k;
        const bool seg = j < N;
        if (COUNT && seg) wc.prims++;
        const RibbonEnd a = ribbon_end(w0, w1, w2, w3, j, N), b = ribbon_end(w0, w1, w2, w3, j + 1u, N);
        float t, U, V;
        bool ok = ribbon_quad_test(a, b, r.tnear, tfar, S.s, t, U, V) && seg;
        if (ok && P.exclOffsets) ok = !candidate_excluded(P, __float_as_uint(x[10]), ids.x, ids.y, t);
        const uint32_t m8 = octet_ballot(ok, lid);
        if (OCCLUDED) { // Occluded1EpilogMU: any valid segment
          if (m8 != 0u) {
            if (k == 0u) x[9] = __uint_as_float(1u);
            cnt = 0u;
            N = 0u;
          }
          continue;
        }
        const float tmin = octet_min8(ok ? t : RT_INF);
        const uint32_t w = octet_ballot(ok && t == tmin, lid);
        if (w != 0u && k == (uint32_t)__ffs(w) - 1u) { // select_min, the lowest lane wins an equal t (Intersect1EpilogMU, intersector_epilog.h:455-509)
          TriHit h;
          ribbon_hit(h, t, U, V, k, base, N, V0, V1, V2, V3);
          row_write_hit(x, h, ids.x, ids.y);
        }
        tfar = w != 0u ? tmin : tfar;
      }
    }
  }

  // Lane-per-ray form: the records one after the other, the five words of a record requested before the first use; the segments in
  // passes of 8 against the tfar at pass entry, visited in order and replacing the best one only with a smaller t, so the lowest
  // segment wins ties.  The end of a segment is carried over as the start of the next (the same bits, see the header).  The world
  // control points are read again for the Ng of a pass's winner: sixteen registers less across the segment loop.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ bool intersect(const LaunchParams& P, uint32_t ref, RayState& r, WorkCounters& wc, uint32_t rayIdx)
  {
    const CurveRecord* __restrict__ recs = (const CurveRecord*)P.accel.blobs;
    const LineSpace S = line_space(r);
    uint32_t first, count;
    leaf_range(ref, first, count);
    for (uint32_t i = 0; i < count; i++) {
      const float4* lp = (const float4*)(recs + first + i);
      float4 w0 = lp[0], w1 = lp[1], w2 = lp[2], w3 = lp[3];
      const uint4 ids = *(const uint4*)(lp + 4); // geomID, primID, N, pad
      const uint32_t N = ids.z;
      w0 = to_ray_space(r, S, w0); w1 = to_ray_space(r, S, w1); w2 = to_ray_space(r, S, w2); w3 = to_ray_space(r, S, w3);
      RibbonEnd a = ribbon_end(w0, w1, w2, w3, 0u, N);
      for (uint32_t base = 0; base < N; base += 8u) {
        const float tfarPass = r.tfar; // all segments of a pass see the tfar at pass entry
        const uint32_t nb = min(8u, N - base);
        bool found = false;
        float bt = RT_INF, bU = 0.f, bV = 0.f;
        uint32_t bk = 0;
        for (uint32_t k = 0; k < nb; k++) {
          if (COUNT) wc.prims++;
          const RibbonEnd b = ribbon_end(w0, w1, w2, w3, base + k + 1u, N);
          float t, U, V;
          bool ok = ribbon_quad_test(a, b, r.tnear, tfarPass, S.s, t, U, V);
          a = b;
          if (ok && P.exclOffsets) ok = !candidate_excluded(P, rayIdx, ids.x, ids.y, t);
          if (ok) {
            if (OCCLUDED) return true; // Occluded1EpilogMU: any valid segment
            if (!found || t < bt) { // select_min over the pass, lowest segment wins ties
              bt = t; bU = U; bV = V; bk = k;
              found = true;
            }
          }
        }
        if (found) { // Intersect1EpilogMU, intersector_epilog.h:455-509
          TriHit best;
          ribbon_hit(best, bt, bU, bV, bk, base, N, lp[0], lp[1], lp[2], lp[3]);
          commit_hit(r, best, ids.x, ids.y);
        }
      }
    }
    return false;
  }
};

} // namespace dev

hipError_t launch_trace_curve(const LaunchParams& p, hipStream_t stream)
{
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
