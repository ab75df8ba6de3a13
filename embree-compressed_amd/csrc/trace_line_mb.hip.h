// The motion-blur line segment leaf (described in trace_line_mb.hip, which launches its top-level kernels), in a header so that the
// HAIRMB form of the two-level kernel (trace_instance_hair_mb.hip) runs the same text on the local ray.
#pragma once
#include "trace_leaf.hip.h"
#include "trace_line.hip.h"
#include "trace_mb.hip.h"

namespace rtamd {
namespace dev {

// Records requested per memory round trip inside a block of 4 in the lane-per-ray form (1, 2 or 4).  A record is 20 dwords: two in
// flight are 40 registers, under the 48 the static leaf has in flight with four (LINE_FETCH); four would be 80.
#ifndef LINEMB_FETCH
#define LINEMB_FETCH 2
#endif

struct LineMBLeaf : LeafTraits
{
  static constexpr uint32_t FETCH = LINEMB_FETCH;

  // Child-parallel form (trace_loop.hip.h): as LineLeaf::octet_pass - the 8 lanes of an octet take 8 consecutive records = two blocks of
  // 4, line_octet_winner picks the winner.  A lane whose record belongs to another time segment takes no part.  Row word 10 is the
  // ray's index.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const LineMBRecord* __restrict__ recs = (const LineMBRecord*)P.accel.blobs;
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
    for (uint32_t b = 0; __ballot(b < cnt) != 0ull; b += 8u) {
      bool present = b + k < cnt;
      const float4* lp = (const float4*)(recs + first + (present ? b + k : 0u));
      const float4 V0a = lp[0], V1a = lp[1], V0b = lp[2], V1b = lp[3];
      const uint4 ids = *(const uint4*)(lp + 4); // geomID, primID, segment, numSegments
      float f;
      present = time_segment(time, ids.z, ids.w, f) && present;
      if (COUNT && present) wc.prims++;
      TriHit h;
      h.t = RT_INF;
      bool ok = false;
      if (present) ok = line_test(r, S, lerp_vertex4(V0a, V0b, f), lerp_vertex4(V1a, V1b, f), tfar, h);
      if (ok && P.exclOffsets) ok = !candidate_excluded(P, rayIdx, ids.x, ids.y, h.t);
      const uint32_t m8 = octet_ballot(ok, lid);
      if (OCCLUDED) { // Occluded1EpilogM: any valid lane
        if (m8 != 0u) {
          if (k == 0u) x[9] = __uint_as_float(1u);
          cnt = 0u;
        }
        continue;
      }
      float tfarNext;
      const uint32_t winner = line_octet_winner(ok, h.t, m8, k, lid, tfar, tfarNext);
      if (k == winner) row_write_hit(x, h, ids.x, ids.y); // Intersect1EpilogM, intersector_epilog.h:293-305
      tfar = tfarNext;
    }
  }

  // Lane-per-ray form: the block loop of LineLeaf::intersect; LINEMB_FETCH records are requested before the first one is used.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ bool intersect(const LaunchParams& P, uint32_t ref, RayState& r, WorkCounters& wc, uint32_t rayIdx)
  {
    const LineMBRecord* __restrict__ recs = (const LineMBRecord*)P.accel.blobs;
    const float time = ray_time(P, rayIdx);
    const LineSpace S = line_space(r);
    uint32_t first, count;
    leaf_range(ref, first, count);
    for (uint32_t b = 0; b < count; b += 4) {
      const float tfarBlock = r.tfar; // all lanes of a block see the tfar at block entry
      const uint32_t nb = min(4u, count - b);
      bool found = false;
      TriHit best;
      uint32_t bestPrim = 0, bestGeom = 0;
      best.t = RT_INF;
      for (uint32_t g = 0; g < nb; g += FETCH) {
        // slots past the leaf end re-read the last record and are skipped below
        float4 V0a[FETCH], V1a[FETCH], V0b[FETCH], V1b[FETCH];
        uint4 ids[FETCH];
#pragma unroll
        for (uint32_t k = 0; k < FETCH; k++) {
          const float4* lp = (const float4*)(recs + first + b + min(g + k, nb - 1u));
          V0a[k] = lp[0]; V1a[k] = lp[1]; V0b[k] = lp[2]; V1b[k] = lp[3];
          ids[k] = *(const uint4*)(lp + 4);
        }
#pragma unroll
        for (uint32_t k = 0; k < FETCH; k++) {
          if (g + k >= nb) break;
          float f;
          if (!time_segment(time, ids[k].z, ids[k].w, f)) continue; // another segment's record
          if (COUNT) wc.prims++;
          TriHit h;
          bool ok = line_test(r, S, lerp_vertex4(V0a[k], V0b[k], f), lerp_vertex4(V1a[k], V1b[k], f), tfarBlock, h);
          if (ok && P.exclOffsets) ok = !candidate_excluded(P, rayIdx, ids[k].x, ids[k].y, h.t);
          if (ok) {
            if (OCCLUDED) return true; // Occluded1EpilogM: any valid lane
            if (!found || h.t < best.t) { // select_min over the valid lanes, lowest lane wins ties
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

// The same leaf under time-dependent nodes (mb_bounds=linear, accel.h QNodeMB8): only the node step of trace_loop.hip.h differs.
struct LineMBLeafLinear : LineMBLeaf
{
  static constexpr bool NODE_MB = true;
};

} // namespace dev
} // namespace rtamd
