// Line segment leaves of the quantized BVH8: flat linear curves (RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE), Line4i.
// 48-byte records (LineRecord, accel.h) fetched as three dwordx4; every group of 4 records from the leaf start is one block with the
// reference's 4-wide SIMD semantics (LineMiIntersector1<4>, kernels/geometry/linei_intersector.h -> LineIntersector1<4>::intersect,
// line_intersector.h:64-98): all 4 tested against the tfar at block entry, one select_min, the lowest lane wins equal t
// (Intersect1EpilogM<4,4>); a later block sees the tfar the earlier one left and wins an equal t (`t <= tfar`).
// The test works in the ray's own space (Precalculations, line_intersector.h:53-58): s = rsqrt(dot(dir, dir)) and the transposed
// frame of s * dir - nine floats and s that depend on the ray only.  RayState and the octet exchange rows have no room for them and
// every other leaf shares those, so they are recomputed at each leaf visit (about 40 VALU operations, one division per rsqrt).
// One arithmetic serves the robust and the fast accel; only the node test differs.
// A ray exactly parallel to a segment's axis has d1 == 0 and takes its u from 0 * inf, as in the reference.
#include "trace_leaf.hip.h"
#include "trace_line.hip.h"

namespace rtamd {
namespace dev {

// Records requested per memory round trip inside a block of 4 in the lane-per-ray form (1, 2 or 4).
#ifndef LINE_FETCH
#define LINE_FETCH 4
#endif

struct LineLeaf : LeafTraits
{
  static constexpr uint32_t FETCH = LINE_FETCH;

  // Child-parallel form (trace_loop.hip.h): the 8 lanes of an octet test 8 consecutive records of the leaf of the ray in exchange row
  // `x`, two of the reference's blocks of 4 per pass: lanes 0-3 block A, lanes 4-7 block B, every lane against the tfar at pass entry.
  // The depth test of this leaf is `t <= tfar` on the very t that is minimised, so ONE 4-lane minimum serves both blocks: block B,
  // which has to see the tfar A left behind, has a winner exactly when its minimum over the lanes valid at pass entry is <= that tfar
  // (the other conditions of the test do not depend on tfar), and that minimum is then its winner's t.  Inside a block the lowest
  // lane wins; B wins an equal t of A.  The winning lane writes the hit into the row (words 0..7 = t, Ng, u, v, geomID, primID;
  // word 9 = 1).
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const LineRecord* __restrict__ lines = (const LineRecord*)P.accel.blobs;
    const uint32_t k = lid & 7u;
    const RayState r = row_ray(x);
    const LineSpace S = line_space(r);
    const uint32_t ref = __float_as_uint(x[8]);
    uint32_t first, cnt;
    leaf_range(ref, first, cnt);
    cnt = valid ? cnt : 0u;
    float tfar = r.tfar;
    for (uint32_t b = 0; __ballot(b < cnt) != 0ull; b += 8u) {
      const bool present = b + k < cnt;
      const float4* lp = (const float4*)(lines + first + (present ? b + k : 0u));
      const float4 V0 = lp[0], V1 = lp[1];
      const uint2 ids = *(const uint2*)(lp + 2);
      if (COUNT && present) wc.prims++;
      TriHit h;
      h.t = RT_INF;
      bool ok = line_test(r, S, V0, V1, tfar, h) && present;
      if (ok && P.exclOffsets) ok = !candidate_excluded(P, __float_as_uint(x[10]), ids.x, ids.y, h.t);
      const uint32_t m8 = octet_ballot(ok, lid);
      if (OCCLUDED) { // Occluded1EpilogM: any valid lane
        if (m8 != 0u) {
          if (k == 0u) x[9] = __uint_as_float(1u);
          cnt = 0u;
        }
        continue;
      }
      // (line_octet_winner of trace_line.hip.h is this selection; written out here because the counted twins of this leaf do not stay the
      // same instructions with the helper)
      const float tq = quad_min4(ok ? h.t : RT_INF); // the minimum of this lane's own block
      const float tqm = dpp_f32<DPP_HALF_MIRROR>(tq); // and of the other one
      const float tA = k < 4u ? tq : tqm, tB = k < 4u ? tqm : tq;
      const bool hasA = (m8 & 0x0fu) != 0u;
      const float tfarB = hasA ? tA : tfar;
      const bool hasB = (m8 & 0xf0u) != 0u && tB <= tfarB;
      const uint32_t wA = octet_ballot(ok && k < 4u && h.t == tA, lid) & 0x0fu;
      const uint32_t wB = hasB ? octet_ballot(ok && k >= 4u && h.t == tB, lid) & 0xf0u : 0u;
      const uint32_t winner = wB != 0u ? (uint32_t)__ffs(wB) - 1u : (wA != 0u ? (uint32_t)__ffs(wA) - 1u : 8u);
      if (k == winner) row_write_hit(x, h, ids.x, ids.y); // Intersect1EpilogM, intersector_epilog.h:293-305
      tfar = wB != 0u ? tB : (wA != 0u ? tA : tfar);
    }
  }

  // Lane-per-ray form: the 4 candidates of a block against the tfar at block entry; candidates are visited in lane order and replace
  // the best one only with a smaller t, so the lowest lane wins ties.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ bool intersect(const LaunchParams& P, uint32_t ref, RayState& r, WorkCounters& wc, uint32_t rayIdx)
  {
    const LineRecord* __restrict__ lines = (const LineRecord*)P.accel.blobs;
    const LineSpace S = line_space(r);
    uint32_t first, count;
    leaf_range(ref, first, count);
    for (uint32_t b = 0; b < count; b += 4) {
      const float tfarBlock = r.tfar;
      const uint32_t nb = min(4u, count - b);
      bool found = false;
      TriHit best;
      uint32_t bestPrim = 0, bestGeom = 0;
      best.t = RT_INF;
      for (uint32_t g = 0; g < nb; g += FETCH) {
        // all records of the fetch group are requested before the first one is used; slots past the leaf end re-read the last record
        float4 V0[FETCH], V1[FETCH];
        uint2 ids[FETCH];
#pragma unroll
        for (uint32_t k = 0; k < FETCH; k++) {
          const float4* lp = (const float4*)(lines + first + b + min(g + k, nb - 1u));
          V0[k] = lp[0]; V1[k] = lp[1];
          ids[k] = *(const uint2*)(lp + 2);
        }
#pragma unroll
        for (uint32_t k = 0; k < FETCH; k++) {
          if (g + k >= nb) break;
          if (COUNT) wc.prims++;
          TriHit h;
          bool ok = line_test(r, S, V0[k], V1[k], tfarBlock, h);
          if (ok && P.exclOffsets) ok = !candidate_excluded(P, rayIdx, ids[k].x, ids[k].y, h.t);
          if (ok) {
            if (OCCLUDED) return true; // Occluded1EpilogM: any valid lane
            if (!found || h.t < best.t) { // select_min over the 4 lanes, lowest lane wins ties
              best = h;
              bestGeom = ids[k].x;
              bestPrim = ids[k].y;
              found = true;
            }
          }
        }
      }
      if (found) commit_hit(r, best, bestGeom, bestPrim); // Intersect1EpilogM, intersector_epilog.h:293-305
    }
    return false;
  }
};

} // namespace dev

hipError_t launch_trace_line(const LaunchParams& p, hipStream_t stream)
{
  // one leaf; robust traversal for RTC_SCENE_FLAG_ROBUST scenes, fast traversal otherwise
  const bool robust = p.accel.kind == ACCEL_LINE_ROBUST;
  if (p.poolKernel) return robust ? dev::launch_leaf_pool<dev::LineLeaf, true>(p, stream) : dev::launch_leaf_pool<dev::LineLeaf, false>(p, stream);
  return robust ? dev::launch_leaf<dev::LineLeaf, true>(p, stream) : dev::launch_leaf<dev::LineLeaf, false>(p, stream);
}

} // namespace rtamd
