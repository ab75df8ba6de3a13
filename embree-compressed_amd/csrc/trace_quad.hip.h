// The static quad leaf (described in trace_quad.hip, which holds its launchers): here so that the two-level kernels
// (trace_instance_body.hip.h) run the same leaf below an instance.
#pragma once
#include "trace_leaf.hip.h"
#include "trace_quad_tests.hip.h"

namespace rtamd {
namespace dev {

// Records requested per memory round trip inside a block of 4 quads in the lane-per-ray form (1, 2 or 4).  Pluecker fetches two at
// a time: with four (16 dwordx4 in flight) its closest-hit lane kernel needs 32-40 bytes of scratch at the 3-waves register limit.
#ifndef QUAD_FETCH_PLUECKER
#define QUAD_FETCH_PLUECKER 2
#endif
#ifndef QUAD_FETCH_MOELLER
#define QUAD_FETCH_MOELLER 4
#endif

// Filter re-trace (candidate_excluded with the distance, trace_leaf.hip.h): both triangles of a quad carry the quad's (geomID,
// primID).  A ray through the diagonal v1-v3 hits A and B at a bit-identical t: rejecting one rejects both, where the reference
// would offer B after A.
template <bool PLUECKER> struct QuadLeaf : LeafTraits // both forms in the lane kernel, as for triangle leaves (trace_tri.hip)
{
  static __device__ __forceinline__ bool test(const RayState& r, const float4 a, const float4 b, const float4 c, float tfar, bool flip, TriHit& h)
  {
    return PLUECKER ? pluecker_quad(r, a, b, c, tfar, flip, h) : moeller_quad(r, a, b, c, tfar, flip, h);
  }

  // Child-parallel form (trace_loop.hip.h): lane k of the octet of the ray in exchange row `x` tests triangle A (k < 4) or B (k >= 4)
  // of quad b + (k & 3) - exactly one of the reference's 8-wide blocks per pass.  One 8-lane minimum; the lowest lane with that t
  // writes the hit into the row (words 0..7 = t, Ng, u, v, geomID, primID; word 9 = 1).
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const QuadRecord* __restrict__ quads = (const QuadRecord*)P.accel.blobs;
    const uint32_t k = lid & 7u, sh = lid & 56u;
    const bool isB = k >= 4u;
    const RayState r = row_ray(x);
    const uint32_t ref = __float_as_uint(x[8]);
    const uint32_t first = ref & ((1u << TRI_START_BITS) - 1u);
    uint32_t cnt = valid ? (ref >> TRI_START_BITS) & 31u : 0u;
    float tfar = r.tfar;
    for (uint32_t b = 0; __ballot(b < cnt) != 0ull; b += 4u) {
      const bool present = b + (k & 3u) < cnt;
      const float4* qp = (const float4*)(quads + first + (present ? b + (k & 3u) : 0u));
      const float4 V0 = qp[isB ? 2 : 0], V1 = qp[1], V3 = qp[3];
      // geomID lives in v0.w: lane k+4 takes it from lane k (same quad; half mirror, then xor 3 = lane k^4)
      const uint32_t geomID = dpp_u32<DPP_XOR3>(dpp_u32<DPP_HALF_MIRROR>(__float_as_uint(V0.w)));
      const uint32_t primID = __float_as_uint(V1.w);
      if (COUNT && present && !isB) wc.prims++;
      TriHit h;
      h.t = RT_INF; h.Ts = 0.f; h.absDen = 0.f;
      bool ok = test(r, V0, V1, V3, tfar, isB, h) && present;
      if (ok && P.exclOffsets) ok = !candidate_excluded(P, __float_as_uint(x[10]), isB ? geomID : __float_as_uint(V0.w), primID, h.t);
      const uint32_t m8 = (uint32_t)(__ballot(ok) >> sh) & 0xffu;
      if (OCCLUDED) { // Occluded1EpilogM: any valid lane
        if (m8 != 0u) {
          if (k == 0u) x[9] = __uint_as_float(1u);
          cnt = 0u;
        }
        continue;
      }
      const float tm = octet_min8(ok ? h.t : RT_INF);
      // (octet_ballot, row_write_hit and leaf_range change the instruction schedule of this leaf's octet form: written out)
      const uint32_t w = (uint32_t)(__ballot(ok && h.t == tm) >> sh) & 0xffu;
      const uint32_t winner = w != 0u ? (uint32_t)__ffs(w) - 1u : 8u;
      if (k == winner) { // Intersect1EpilogM, intersector_epilog.h:293-305
        x[0] = h.t; x[1] = h.ngx; x[2] = h.ngy; x[3] = h.ngz; x[4] = h.u; x[5] = h.v;
        x[6] = __uint_as_float(isB ? geomID : __float_as_uint(V0.w)); x[7] = __uint_as_float(primID);
        x[9] = __uint_as_float(1u);
      }
      tfar = w != 0u ? tm : tfar;
    }
  }

  // Lane-per-ray form: the 8 candidates of a block (A of quads 0-3 = lanes 0-3, B = lanes 4-7), all against the tfar at block
  // entry, tested quad by quad (A, B) so that a quad's registers die early; the lane number decides between equal t, so the
  // lowest lane wins ties as in the octet form.  FETCH and the exclusion policy: as for TriLeaf::intersect.
  template <bool OCCLUDED, bool COUNT, uint32_t FETCH = (PLUECKER ? QUAD_FETCH_PLUECKER : QUAD_FETCH_MOELLER), class Excl = TopLevelExcl>
  static __device__ __forceinline__ bool intersect(const LaunchParams& P, uint32_t ref, RayState& r, WorkCounters& wc, uint32_t rayIdx, const Excl excl = Excl())
  {
    const QuadRecord* __restrict__ quads = (const QuadRecord*)P.accel.blobs;
    uint32_t first, count;
    leaf_range(ref, first, count);
    for (uint32_t b = 0; b < count; b += 4) {
      const float tfarBlock = r.tfar;
      const uint32_t nb = min(4u, count - b);
      bool found = false;
      TriHit best;
      uint32_t bestLane = 8u, bestPrim = 0, bestGeom = 0;
      best.t = RT_INF;
      for (uint32_t g = 0; g < nb; g += FETCH) {
        // all records of the fetch group are requested before the first one is used; slots past the leaf end re-read the last record
        float4 V0[FETCH], V1[FETCH], V2[FETCH], V3[FETCH];
#pragma unroll
        for (uint32_t k = 0; k < FETCH; k++) {
          const float4* qp = (const float4*)(quads + first + b + min(g + k, nb - 1u));
          V0[k] = qp[0]; V1[k] = qp[1]; V2[k] = qp[2]; V3[k] = qp[3];
        }
#pragma unroll
        for (uint32_t k = 0; k < FETCH; k++) {
          if (g + k >= nb) break;
          if (COUNT) wc.prims++;
          const uint32_t gid = __float_as_uint(V0[k].w), pid = __float_as_uint(V1[k].w);
#pragma unroll
          for (uint32_t half = 0; half < 2; half++) { // A then B of this quad (lanes g+k and 4+g+k)
            TriHit h;
            bool ok = test(r, half ? V2[k] : V0[k], V1[k], V3[k], tfarBlock, half != 0u, h);
            if constexpr (std::is_same<Excl, TopLevelExcl>::value) {
              if (ok && P.exclOffsets) ok = !candidate_excluded(P, rayIdx, gid, pid, h.t);
            } else if (ok && excl(gid, pid, h.t)) ok = false;
            if (ok) {
              if (OCCLUDED) return true; // Occluded1EpilogM: any valid lane
              // select_min over the 8 lanes, lowest lane wins ties
              const uint32_t lane = half * 4u + g + k;
              if (!found || h.t < best.t || (h.t == best.t && lane < bestLane)) {
                best = h;
                bestLane = lane;
                bestGeom = gid;
                bestPrim = pid;
                found = true;
              }
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
