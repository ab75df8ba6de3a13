// The static triangle leaf (described in trace_tri.hip, which holds its launchers): here so that the two-level kernels
// (trace_instance_body.hip.h) run the same leaf below an instance.
#pragma once
#include "trace_leaf.hip.h"

namespace rtamd {
namespace dev {

// Records requested per memory round trip inside a block of 4 (1, 2 or 4): more hides latency, fewer saves registers.
#ifndef TRI_FETCH
#define TRI_FETCH 4
#endif

template <bool PLUECKER> struct TriLeaf : LeafTraits
{
  // Both forms stay in the lane kernel.  Measured with the lane-per-ray form dropped (127 VGPRs, four waves per SIMD): random
  // rays 18.0 -> 19.2 Grays/s in flight, 0.098 -> 0.089 ms alone, but rays that visit many full leaves lose: camera rays 11.4 ->
  // 10.8, bounce rays 10.3 -> 9.4, shadow rays 15.9 -> 13.2 Grays/s (8 lanes per ray test a 4-triangle leaf at half occupancy;
  // with 64 rays at a leaf the lane-per-ray block loop is the better use of the wave).
  static constexpr bool OCTET_ONLY = false;

  // Child-parallel form (trace_loop.hip.h): the 8 lanes of an octet test 8 consecutive records of the leaf of the ray in
  // exchange row `x`, i.e. two of the reference's blocks of 4 per pass: lanes 0-3 block A, lanes 4-7 block B.  Block
  // semantics are kept exactly: A is tested against the tfar at its entry, its minimum-t lane (lowest lane on ties) wins;
  // B's depth test `Ts <= absDen * tfar` is then evaluated with the tfar A left behind (so an equal-t hit of the later
  // block replaces the earlier one, triangle_intersector_pluecker.h:117), its winner chosen the same way.  The winning
  // lane writes the hit into the row (words 0..7 = t, Ng, u, v, geomID, primID; word 9 = 1).
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const TriRecord* __restrict__ prims = P.accel.prims;
    const uint32_t k = lid & 7u, sh = lid & 56u;
    const RayState r = row_ray(x);
    const uint32_t ref = __float_as_uint(x[8]);
    // (leaf_range and a shared exclusion scan change the instruction schedule of this leaf's kernels: written out, here and in intersect())
    const uint32_t first = ref & ((1u << TRI_START_BITS) - 1u);
    uint32_t cnt = valid ? (ref >> TRI_START_BITS) & 31u : 0u;
    float tfar = r.tfar;
    for (uint32_t b = 0; __ballot(b < cnt) != 0ull; b += 8u) {
      const bool present = b + k < cnt;
      const float4* tp = (const float4*)(prims + first + (present ? b + k : 0u));
      const float4 A = tp[0], B = tp[1], C = tp[2];
      if (COUNT && present) wc.prims++;
      TriHit h;
      h.t = RT_INF; h.Ts = 0.f; h.absDen = 0.f;
      bool ok = (PLUECKER ? pluecker(r, A, B, C, tfar, h) : moeller(r, A, B, C, tfar, h)) && present;
      if (ok && P.exclOffsets) { // filter re-trace: a candidate the host filter rejected before stays rejected
        const uint32_t rayIdx = __float_as_uint(x[10]);
        const uint32_t e1 = P.exclOffsets[rayIdx + 1];
        for (uint32_t e = P.exclOffsets[rayIdx]; e < e1; e++) {
          const uint2 q = P.exclPairs[e];
          if (q.x == __float_as_uint(A.w) && q.y == __float_as_uint(B.w)) ok = false;
        }
      }
      const uint32_t m8 = octet_ballot(ok, lid);
      if (OCCLUDED) { // Occluded1EpilogM: any valid lane
        if (m8 != 0u) {
          if (k == 0u) x[9] = __uint_as_float(1u);
          cnt = 0u;
        }
        continue;
      }
      // block A (also evaluated, unused, in the lanes of block B: the quads reduce separately)
      const float tq = quad_min4(ok ? h.t : RT_INF);
      const float tqm = dpp_f32<DPP_HALF_MIRROR>(tq);
      const float tA = k < 4u ? tq : tqm; // minimum of block A, in all 8 lanes
      const bool hasA = (m8 & 0x0fu) != 0u;
      const float tfarB = hasA ? tA : tfar;
      const bool okB = ok && k >= 4u && (h.Ts <= h.absDen * tfarB);
      const float tb = quad_min4(okB ? h.t : RT_INF);
      const float tbm = dpp_f32<DPP_HALF_MIRROR>(tb);
      const float tB = k >= 4u ? tb : tbm; // minimum of block B, in all 8 lanes
      const uint32_t wA = octet_ballot(ok && k < 4u && h.t == tA, lid) & 0x0fu;
      const uint32_t wB = octet_ballot(okB && h.t == tB, lid) & 0xf0u;
      const uint32_t winner = wB != 0u ? (uint32_t)__ffs(wB) - 1u : (wA != 0u ? (uint32_t)__ffs(wA) - 1u : 8u);
      if (k == winner) { // Intersect1EpilogM, intersector_epilog.h:293-305
        row_write_hit(x, h, __float_as_uint(A.w), __float_as_uint(B.w));
      }
      tfar = wB != 0u ? tB : (wA != 0u ? tA : tfar);
    }
  }

  // Lane-per-ray form.  FETCH records per round trip and the exclusion policy (trace_leaf.hip.h TopLevelExcl) are the top-level kernels' by
  // default; the two-level kernels (trace_instance_body.hip.h) pass their own.
  template <bool OCCLUDED, bool COUNT, uint32_t FETCH = TRI_FETCH, class Excl = TopLevelExcl>
  static __device__ __forceinline__ bool intersect(const LaunchParams& P, uint32_t ref, RayState& r, WorkCounters& wc, uint32_t rayIdx, const Excl excl = Excl())
  {
    const TriRecord* __restrict__ prims = P.accel.prims;
    uint32_t first, count;
    leaf_range(ref, first, count);
    for (uint32_t b = 0; b < count; b += 4) {
      const float tfarBlock = r.tfar; // all lanes of a block see the tfar at block entry
      const uint32_t nb = min(4u, count - b);
      bool found = false;
      TriHit best;
      uint32_t bestPrim = 0, bestGeom = 0;
      best.t = RT_INF;
      // all records of the block are requested before the first one is used (one memory round trip per block instead
      // of one per triangle); slots past the leaf end re-read the last record and are skipped below
      for (uint32_t g = 0; g < nb; g += FETCH) {
        float4 A[FETCH], B[FETCH], C[FETCH];
#pragma unroll
        for (uint32_t k = 0; k < FETCH; k++) {
          const float4* tp = (const float4*)(prims + first + b + min(g + k, nb - 1u));
          A[k] = tp[0]; B[k] = tp[1]; C[k] = tp[2];
        }
#pragma unroll
        for (uint32_t k = 0; k < FETCH; k++) {
          if (g + k >= nb) break;
          if (COUNT) wc.prims++;
          TriHit h;
          bool ok = PLUECKER ? pluecker(r, A[k], B[k], C[k], tfarBlock, h) : moeller(r, A[k], B[k], C[k], tfarBlock, h);
          if constexpr (std::is_same<Excl, TopLevelExcl>::value) {
            if (ok && P.exclOffsets) { // filter re-trace: a candidate the host filter rejected before stays rejected
              const uint32_t e1 = P.exclOffsets[rayIdx + 1];
              for (uint32_t e = P.exclOffsets[rayIdx]; e < e1; e++) {
                const uint2 q = P.exclPairs[e];
                if (q.x == __float_as_uint(A[k].w) && q.y == __float_as_uint(B[k].w)) ok = false;
              }
            }
          } else if (ok && excl(__float_as_uint(A[k].w), __float_as_uint(B[k].w), h.t)) ok = false;
          if (ok) {
            if (OCCLUDED) return true; // Occluded1EpilogM: any valid lane (no ray mask, no filter)
            // select_min over valid lanes, lowest lane wins ties (vfloat4_sse2.h:654-659)
            if (!found || h.t < best.t) {
              best = h;
              bestGeom = __float_as_uint(A[k].w);
              bestPrim = __float_as_uint(B[k].w);
              found = true;
            }
          }
        }
      }
      if (found) { // Intersect1EpilogM, intersector_epilog.h:293-305
        commit_hit(r, best, bestGeom, bestPrim);
      }
    }
    return false;
  }
};

} // namespace dev
} // namespace rtamd
