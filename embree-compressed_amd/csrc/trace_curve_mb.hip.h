// The motion-blur ribbon leaf (described in trace_curve_mb.hip, which launches its top-level kernels), in a header so that the HAIRMB
// form of the two-level kernel (trace_instance_hair_mb.hip) runs the same text on the local ray.
#pragma once
#include "trace_curve.hip.h"
#include "trace_mb.hip.h"

namespace rtamd {
namespace dev {

struct CurveMBLeaf : LeafTraits
{
  // Three waves per SIMD, the bound of the static leaf (at most 168 VGPRs): profiles/curve_mb_kernel_resources.txt
  static constexpr int MIN_WAVES = 3;

  // Child-parallel form (trace_loop.hip.h): CurveLeaf::octet_pass with one record per pass - lane k of the octet tests segment base + k
  // of the interpolated curve.  All lanes of an octet hold the same ray and the same record, so the time-segment test is uniform within
  // the octet: a record of another time segment gets N = 0 and runs no passes, its control points are not read.  The loops stay
  // wave-uniform (every octet runs as many passes as the longest one; the others are masked).  Row word 10 is the ray's index.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const CurveMBRecord* __restrict__ recs = (const CurveMBRecord*)P.accel.blobs;
    const uint32_t k = lid & 7u;
    const RayState r = row_ray(x);
    const LineSpace S = line_space(r);
    const uint32_t ref = __float_as_uint(x[8]);
    const uint32_t rayIdx = __float_as_uint(x[10]);
    const float time = ray_time(P, rayIdx);
    uint32_t first, cnt;
    leaf_range(ref, first, cnt);
    cnt = valid ? cnt : 0u;
    float tfar = r.tfar;
    for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i++) {
      const bool present = i < cnt;
      const float4* lp = (const float4*)(recs + first + (present ? i : 0u));
      const uint4 ids = *(const uint4*)(lp + 8); // geomID, primID, segment, numSegments
      float f;
      const bool mine = time_segment(time, ids.z, ids.w, f) && present;
      uint32_t N = 0u;
      float4 V0 = make_float4(0.f, 0.f, 0.f, 0.f), V1 = V0, V2 = V0, V3 = V0;
      if (mine) {
        N = *(const uint32_t*)(lp + 9);
        V0 = lerp_vertex4(lp[0], lp[4], f); V1 = lerp_vertex4(lp[1], lp[5], f);
        V2 = lerp_vertex4(lp[2], lp[6], f); V3 = lerp_vertex4(lp[3], lp[7], f);
      }
      const float4 w0 = to_ray_space(r, S, V0), w1 = to_ray_space(r, S, V1), w2 = to_ray_space(r, S, V2), w3 = to_ray_space(r, S, V3);
      for (uint32_t base = 0; __ballot(base < N) != 0ull; base += 8u) {
        const uint32_t j = base + k;
        const bool seg = j < N;
        if (COUNT && seg) wc.prims++;
        const RibbonEnd a = ribbon_end(w0, w1, w2, w3, j, N), b = ribbon_end(w0, w1, w2, w3, j + 1u, N);
        float t, U, V;
        bool ok = ribbon_quad_test(a, b, r.tnear, tfar, S.s, t, U, V) && seg;
        if (ok && P.exclOffsets) ok = !candidate_excluded(P, rayIdx, ids.x, ids.y, t);
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

  // Lane-per-ray form: the record loop of CurveLeaf::intersect.  Per record the id row is read first and a record of another time
  // segment is skipped before any arithmetic (N stays 0 and no pass runs; the any-hit kernels leave the iteration instead - which of
  // the two forms keeps every scalar register out of the vector lanes differs between the closest-hit and the any-hit kernels,
  // profiles/curve_mb_kernel_resources.txt).  Otherwise both ends are read and interpolated POINT BY POINT - two rows in, one point out,
  // straight into ray space - so at most eight registers of end points are live beside the sixteen of the ray-space curve.  The world
  // points of a pass's winner are read and interpolated again for its Ng, as the static leaf reads them again: the same madd on the same
  // operands gives the same bits, and sixteen registers less live across the segment loop.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ bool intersect(const LaunchParams& P, uint32_t ref, RayState& r, WorkCounters& wc, uint32_t rayIdx)
  {
    const CurveMBRecord* __restrict__ recs = (const CurveMBRecord*)P.accel.blobs;
    const float time = ray_time(P, rayIdx);
    const LineSpace S = line_space(r);
    uint32_t first, count;
    leaf_range(ref, first, count);
    for (uint32_t i = 0; i < count; i++) {
      const float4* lp = (const float4*)(recs + first + i);
      const uint4 ids = *(const uint4*)(lp + 8); // geomID, primID, segment, numSegments
      float f;
      uint32_t N = 0u; // stays 0 for another segment's record: no pass runs
      float4 w0 = make_float4(0.f, 0.f, 0.f, 0.f), w1 = w0, w2 = w0, w3 = w0;
      RibbonEnd a = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const bool mine = time_segment(time, ids.z, ids.w, f);
      if (OCCLUDED && !mine) continue; // (any hit: this form has no spilled scalar register and the block below alone two; closest hit: the reverse)
      if (mine) {
        N = *(const uint32_t*)(lp + 9);
        w0 = to_ray_space(r, S, lerp_vertex4(lp[0], lp[4], f));
        w1 = to_ray_space(r, S, lerp_vertex4(lp[1], lp[5], f));
        w2 = to_ray_space(r, S, lerp_vertex4(lp[2], lp[6], f));
        w3 = to_ray_space(r, S, lerp_vertex4(lp[3], lp[7], f));
        a = ribbon_end(w0, w1, w2, w3, 0u, N);
      }
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
          ribbon_hit(best, bt, bU, bV, bk, base, N, lerp_vertex4(lp[0], lp[4], f), lerp_vertex4(lp[1], lp[5], f), lerp_vertex4(lp[2], lp[6], f), lerp_vertex4(lp[3], lp[7], f));
          commit_hit(r, best, ids.x, ids.y);
        }
      }
    }
    return false;
  }
};

// The same leaf under time-dependent nodes (mb_bounds=linear, accel.h QNodeMB8): only the node step of trace_loop.hip.h differs.
struct CurveMBLeafLinear : CurveMBLeaf
{
  static constexpr bool NODE_MB = true;
};

} // namespace dev
} // namespace rtamd
