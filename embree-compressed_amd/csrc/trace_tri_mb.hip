// Motion-blur triangle leaves of the quantized BVH8: the triangle of a TriMBRecord (accel.h) interpolated to the ray's time, then the
// Pluecker (robust) or Moeller-Trumbore (fast) test of the static triangle leaf (trace_tri.hip) on the interpolated vertices.
// 96-byte records fetched as six dwordx4: the three vertices at both ends of ONE time segment of the mesh.
//   time segment          kernels/common/geometry.h:28-34 (getTimeSegment): ts = time * S, itime = clamp(floor(ts), 0, S - 1),
//                         ftime = ts - itime; times outside [0, 1] extrapolate the first / last segment
//   interpolation         kernels/geometry/trianglei.h:85-95, :343-364: lerp(p0, p1, f) = madd(1 - f, p0, f * p1)
//   test                  trianglev_mb_intersector.h -> Pluecker / MoellerTrumboreIntersector1::intersect(ray, v0, v1, v2)
// A record is tested only when the ray's itime equals the record's segment (checked before any arithmetic); with S = 1 that is
// every record and ftime = time exactly.  Blocks are groups of 4 RECORDS from the leaf start with the static leaf's semantics: all
// tested records of a block see the tfar at block entry, the lowest lane wins ties, a later block replaces an equal-t hit.
// The ray's time is not part of RayState or of the exchange rows (the kernels of the other leaves stay the instructions they were): the
// leaf reads it from the ray record, word 7, through the ray's index.
// Deviation: the reference's triangle4vmb leaf stores v0 and the per-segment deltas (trianglev_mb.h); here the vmb names run the
// arithmetic of triangle4imb on the same records.
#include "trace_leaf.hip.h"
#include "trace_mb.hip.h"

namespace rtamd {
namespace dev {

// Records requested per memory round trip inside a block of 4 in the lane-per-ray form (1, 2 or 4).  A record is 24 dwords: two in
// flight are the 48 registers the static leaf has in flight with four (TRI_FETCH).
#ifndef TRIMB_FETCH
#define TRIMB_FETCH 2
#endif

template <bool PLUECKER> struct TriMBLeaf : LeafTraits
{
  // the triangle (a, b, c) at the ray's time; Moeller forms its edges from the interpolated vertices (e1 = a - b, e2 = c - a) and is
  // then moeller()'s test on (a, e1, e2)
  static __device__ __forceinline__ bool test(const RayState& r, const float4 a, const float4 b, const float4 c, float tfar, TriHit& h)
  {
    if (PLUECKER) return pluecker(r, a, b, c, tfar, h);
    const float4 e1 = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, 0.0f);
    const float4 e2 = make_float4(c.x - a.x, c.y - a.y, c.z - a.z, 0.0f);
    return moeller(r, a, e1, e2, tfar, h);
  }

  // Child-parallel form (trace_loop.hip.h): as TriLeaf::octet_pass - the 8 lanes of an octet take 8 consecutive records = two blocks
  // of 4 (lanes 0-3 block A, lanes 4-7 block B, B's depth test re-evaluated with the tfar A left behind).  A lane whose record belongs
  // to another time segment takes no part.  Row word 10 is the ray's index.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const TriMBRecord* __restrict__ recs = (const TriMBRecord*)P.accel.blobs;
    const uint32_t k = lid & 7u;
    const RayState r = row_ray(x);
    const uint32_t ref = __float_as_uint(x[8]);
    const uint32_t rayIdx = __float_as_uint(x[10]);
    const float time = ray_time(P, rayIdx);
    uint32_t first, cnt;
    leaf_range(ref, first, cnt);
    cnt = valid ? cnt : 0u;
    float tfar = r.tfar;
    for (uint32_t b = 0; __ballot(b < cnt) != 0ull; b += 8u) {
      bool present = b + k < cnt;
      const float4* tp = (const float4*)(recs + first + (present ? b + k : 0u));
      const float4 A0 = tp[0], B0 = tp[1], C0 = tp[2], A1 = tp[3], B1 = tp[4], C1 = tp[5];
      const uint32_t geomID = __float_as_uint(A0.w), primID = __float_as_uint(B0.w);
      float f;
      present = time_segment(time, __float_as_uint(C0.w), __float_as_uint(A1.w), f) && present;
      if (COUNT && present) wc.prims++;
      TriHit h;
      h.t = RT_INF; h.Ts = 0.f; h.absDen = 0.f;
      bool ok = false;
      if (present) ok = test(r, lerp_vertex(A0, A1, f), lerp_vertex(B0, B1, f), lerp_vertex(C0, C1, f), tfar, h);
      if (ok && P.exclOffsets) { // filter re-trace: a candidate the host filter rejected before stays rejected
        const uint32_t e1 = P.exclOffsets[rayIdx + 1];
        for (uint32_t e = P.exclOffsets[rayIdx]; e < e1; e++) {
          const uint2 q = P.exclPairs[e];
          if (q.x == geomID && q.y == primID) ok = false;
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
        row_write_hit(x, h, geomID, primID);
      }
      tfar = wB != 0u ? tB : (wA != 0u ? tA : tfar);
    }
  }

  // Lane-per-ray form: the block loop of TriLeaf::intersect; TRIMB_FETCH records are requested before the first one is used.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ bool intersect(const LaunchParams& P, uint32_t ref, RayState& r, WorkCounters& wc, uint32_t rayIdx)
  {
    const TriMBRecord* __restrict__ recs = (const TriMBRecord*)P.accel.blobs;
    const float time = ray_time(P, rayIdx);
    uint32_t first, count;
    leaf_range(ref, first, count);
    for (uint32_t b = 0; b < count; b += 4) {
      const float tfarBlock = r.tfar; // all lanes of a block see the tfar at block entry
      const uint32_t nb = min(4u, count - b);
      bool found = false;
      TriHit best;
      uint32_t bestPrim = 0, bestGeom = 0;
      best.t = RT_INF;
      for (uint32_t g = 0; g < nb; g += TRIMB_FETCH) {
        // slots past the leaf end re-read the last record and are skipped below
        float4 A0[TRIMB_FETCH], B0[TRIMB_FETCH], C0[TRIMB_FETCH], A1[TRIMB_FETCH], B1[TRIMB_FETCH], C1[TRIMB_FETCH];
#pragma unroll
        for (uint32_t k = 0; k < TRIMB_FETCH; k++) {
          const float4* tp = (const float4*)(recs + first + b + min(g + k, nb - 1u));
          A0[k] = tp[0]; B0[k] = tp[1]; C0[k] = tp[2]; A1[k] = tp[3]; B1[k] = tp[4]; C1[k] = tp[5];
        }
#pragma unroll
        for (uint32_t k = 0; k < TRIMB_FETCH; k++) {
          if (g + k >= nb) break;
          float f;
          if (!time_segment(time, __float_as_uint(C0[k].w), __float_as_uint(A1[k].w), f)) continue; // another segment's record
          if (COUNT) wc.prims++;
          const uint32_t geomID = __float_as_uint(A0[k].w), primID = __float_as_uint(B0[k].w);
          TriHit h;
          bool ok = test(r, lerp_vertex(A0[k], A1[k], f), lerp_vertex(B0[k], B1[k], f), lerp_vertex(C0[k], C1[k], f), tfarBlock, h);
          if (ok && P.exclOffsets) { // filter re-trace: a candidate the host filter rejected before stays rejected
            const uint32_t e1 = P.exclOffsets[rayIdx + 1];
            for (uint32_t e = P.exclOffsets[rayIdx]; e < e1; e++) {
              const uint2 q = P.exclPairs[e];
              if (q.x == geomID && q.y == primID) ok = false;
            }
          }
          if (ok) {
            if (OCCLUDED) return true; // Occluded1EpilogM: any valid lane
            // select_min over valid lanes, lowest lane wins ties (vfloat4_sse2.h:654-659)
            if (!found || h.t < best.t) {
              best = h;
              bestGeom = geomID;
              bestPrim = primID;
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

// The same leaf under time-dependent nodes (mb_bounds=linear, accel.h QNodeMB8): only the node step of trace_loop.hip.h differs.
template <bool PLUECKER> struct TriMBLeafLinear : TriMBLeaf<PLUECKER>
{
  static constexpr bool NODE_MB = true;
};

} // namespace dev

hipError_t launch_trace_trimb(const LaunchParams& p, hipStream_t stream)
{
  // Pluecker <-> robust traversal, Moeller <-> fast traversal, as for the static triangles; lane kernel only (rt_trace.cpp launch_on
  // never asks for the ray-pool skeleton on this accel)
  if (p.accel.kind == ACCEL_TRIMB_LINEAR_PLUECKER) return dev::launch_leaf<dev::TriMBLeafLinear<true>, true>(p, stream);
  if (p.accel.kind == ACCEL_TRIMB_LINEAR_MOELLER) return dev::launch_leaf<dev::TriMBLeafLinear<false>, false>(p, stream);
  if (p.accel.kind == ACCEL_TRIMB_PLUECKER) return dev::launch_leaf<dev::TriMBLeaf<true>, true>(p, stream);
  return dev::launch_leaf<dev::TriMBLeaf<false>, false>(p, stream);
}

} // namespace rtamd
