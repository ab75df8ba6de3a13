// Motion-blur quad leaves of the quantized BVH8: the quad of a QuadMBRecord (accel.h) interpolated to the ray's time, then the 8-wide
// block of the static quad leaf (trace_quad.hip) on the interpolated vertices: triangle A = (v0, v1, v3), B = (v2, v1, v3), Pluecker
// (robust) or Moeller-Trumbore (fast), B's u / v mapping per variant (trace_quad_tests.hip.h).
// 128-byte records fetched as dwordx4: the four vertices at both ends of ONE time segment of the mesh.
//   time segment          kernels/common/geometry.h:28-34 (getTimeSegment), as for the motion-blur triangles (trace_mb.hip.h)
//   interpolation         kernels/geometry/quadi.h:441-457: lerp(p0, p1, f) = madd(1 - f, p0, f * p1)
//   test                  quadi_intersector.h:193-290 (QuadMiMBIntersector1Moeller / Pluecker) -> the static QuadMIntersector1 on (v0..v3)
// A record is tested only when the ray's itime equals the record's segment (checked before any arithmetic).  Blocks are groups of 4
// RECORDS from the leaf start with the static quad leaf's semantics: the 8 candidates of a block (A of records 0-3 = lanes 0-3, B =
// lanes 4-7) see the tfar at block entry, one minimum over the 8 lanes, the lowest lane wins ties (A beats B at equal t), a later block
// replaces an equal-t hit.  Records of another segment take no part but keep their lane.
// The ray's time is not part of RayState or of the exchange rows: the leaf reads it from the ray record through the ray's index.
// The id words of a record lie in the w of v1 and v3, which both triangles read: no lane needs another lane's ids.
#include "trace_leaf.hip.h"
#include "trace_mb.hip.h"
#include "trace_quad_tests.hip.h"

namespace rtamd {
namespace dev {

// Records requested per memory round trip inside a block of 4 in the lane-per-ray form (1, 2 or 4).  A record is 32 dwords: one in
// flight is what the static Pluecker quad leaf has in flight with two (QUAD_FETCH_PLUECKER); with two the closest-hit kernels need
// scratch at the 3-waves register limit (docs/experiments.md, "Motion blur of quads").
#ifndef QUADMB_FETCH
#define QUADMB_FETCH 1
#endif

// Filter re-trace: candidate_excluded with the distance, as for the static quad leaf - the two triangles of a quad share ids.
template <bool PLUECKER> struct QuadMBLeaf : LeafTraits
{
  static __device__ __forceinline__ bool test(const RayState& r, const float4 a, const float4 b, const float4 c, float tfar, bool flip, TriHit& h)
  {
    return PLUECKER ? pluecker_quad(r, a, b, c, tfar, flip, h) : moeller_quad(r, a, b, c, tfar, flip, h);
  }

  // Child-parallel form (trace_loop.hip.h): as QuadLeaf::octet_pass - lane k of the octet tests triangle A (k < 4) or B (k >= 4) of
  // record b + (k & 3), fetching its three vertices at both segment ends.  Row word 10 is the ray's index.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const QuadMBRecord* __restrict__ recs = (const QuadMBRecord*)P.accel.blobs;
    const uint32_t k = lid & 7u;
    const bool isB = k >= 4u;
    const RayState r = row_ray(x);
    const uint32_t ref = __float_as_uint(x[8]);
    const uint32_t rayIdx = __float_as_uint(x[10]);
    const float time = ray_time(P, rayIdx);
    uint32_t first, cnt;
    leaf_range(ref, first, cnt);
    cnt = valid ? cnt : 0u;
    float tfar = r.tfar;
    for (uint32_t b = 0; __ballot(b < cnt) != 0ull; b += 4u) {
      bool present = b + (k & 3u) < cnt;
      const float4* qp = (const float4*)(recs + first + (present ? b + (k & 3u) : 0u));
      const float4 P0 = qp[isB ? 2 : 0], P1 = qp[1], P3 = qp[3], Q0 = qp[isB ? 6 : 4], Q1 = qp[5], Q3 = qp[7];
      const uint32_t primID = __float_as_uint(P1.w), geomID = __float_as_uint(P3.w);
      float f;
      present = time_segment(time, __float_as_uint(Q1.w), __float_as_uint(Q3.w), f) && present;
      if (COUNT && present && !isB) wc.prims++;
      TriHit h;
      h.t = RT_INF; h.Ts = 0.f; h.absDen = 0.f;
      bool ok = false;
      if (present) ok = test(r, lerp_vertex(P0, Q0, f), lerp_vertex(P1, Q1, f), lerp_vertex(P3, Q3, f), tfar, isB, h);
      if (ok && P.exclOffsets) ok = !candidate_excluded(P, rayIdx, geomID, primID, h.t);
      const uint32_t m8 = octet_ballot(ok, lid);
      if (OCCLUDED) { // Occluded1EpilogM: any valid lane
        if (m8 != 0u) {
          if (k == 0u) x[9] = __uint_as_float(1u);
          cnt = 0u;
        }
        continue;
      }
      const float tm = octet_min8(ok ? h.t : RT_INF);
      const uint32_t w = octet_ballot(ok && h.t == tm, lid);
      const uint32_t winner = w != 0u ? (uint32_t)__ffs(w) - 1u : 8u;
      if (k == winner) { // Intersect1EpilogM, intersector_epilog.h:293-305
        row_write_hit(x, h, geomID, primID);
      }
      tfar = w != 0u ? tm : tfar;
    }
  }

  // Lane-per-ray form: the block loop of QuadLeaf::intersect; QUADMB_FETCH records are requested before the first one is used.  A
  // record is tested A then B so that its registers die early; the lane number decides between equal t.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ bool intersect(const LaunchParams& P, uint32_t ref, RayState& r, WorkCounters& wc, uint32_t rayIdx)
  {
    const QuadMBRecord* __restrict__ recs = (const QuadMBRecord*)P.accel.blobs;
    const float time = ray_time(P, rayIdx);
    uint32_t first, count;
    leaf_range(ref, first, count);
    for (uint32_t b = 0; b < count; b += 4) {
      const float tfarBlock = r.tfar; // all lanes of a block see the tfar at block entry
      const uint32_t nb = min(4u, count - b);
      bool found = false;
      TriHit best;
      uint32_t bestLane = 8u, bestPrim = 0, bestGeom = 0;
      best.t = RT_INF;
      for (uint32_t g = 0; g < nb; g += QUADMB_FETCH) {
        // slots past the leaf end re-read the last record and are skipped below
        float4 V[QUADMB_FETCH][8];
#pragma unroll
        for (uint32_t k = 0; k < QUADMB_FETCH; k++) {
          const float4* qp = (const float4*)(recs + first + b + min(g + k, nb - 1u));
#pragma unroll
          for (uint32_t j = 0; j < 8; j++) V[k][j] = qp[j];
        }
#pragma unroll
        for (uint32_t k = 0; k < QUADMB_FETCH; k++) {
          if (g + k >= nb) break;
          float f;
          if (!time_segment(time, __float_as_uint(V[k][5].w), __float_as_uint(V[k][7].w), f)) continue; // another segment's record
          if (COUNT) wc.prims++;
          const uint32_t pid = __float_as_uint(V[k][1].w), gid = __float_as_uint(V[k][3].w);
          const float4 v1 = lerp_vertex(V[k][1], V[k][5], f), v3 = lerp_vertex(V[k][3], V[k][7], f);
#pragma unroll
          for (uint32_t half = 0; half < 2; half++) { // A then B of this quad (lanes g+k and 4+g+k)
            TriHit h;
            bool ok = test(r, half ? lerp_vertex(V[k][2], V[k][6], f) : lerp_vertex(V[k][0], V[k][4], f), v1, v3, tfarBlock, half != 0u, h);
            if (ok && P.exclOffsets) ok = !candidate_excluded(P, rayIdx, gid, pid, h.t);
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

// The same leaf under time-dependent nodes (mb_bounds=linear, accel.h QNodeMB8): only the node step of trace_loop.hip.h differs.
template <bool PLUECKER> struct QuadMBLeafLinear : QuadMBLeaf<PLUECKER>
{
  static constexpr bool NODE_MB = true;
};

} // namespace dev

hipError_t launch_trace_quadmb(const LaunchParams& p, hipStream_t stream)
{
  // Pluecker <-> robust traversal, Moeller <-> fast traversal, as for the static quads; lane kernel only (rt_trace.cpp launch_on
  // never asks for the ray-pool skeleton on this accel)
  if (p.accel.kind == ACCEL_QUADMB_LINEAR_PLUECKER) return dev::launch_leaf<dev::QuadMBLeafLinear<true>, true>(p, stream);
  if (p.accel.kind == ACCEL_QUADMB_LINEAR_MOELLER) return dev::launch_leaf<dev::QuadMBLeafLinear<false>, false>(p, stream);
  if (p.accel.kind == ACCEL_QUADMB_PLUECKER) return dev::launch_leaf<dev::QuadMBLeaf<true>, true>(p, stream);
  return dev::launch_leaf<dev::QuadMBLeaf<false>, false>(p, stream);
}

} // namespace rtamd
