// What the leaf policies share (trace_tri.hip, trace_quad.hip, trace_grid.hip, trace_cbvh.hip.h): default policy traits, row load
// and hit write of the child-parallel (octet) forms, 8-lane minimum and ballot, closest-hit epilogue of the lane-per-ray forms,
// leaf-reference decode, exclusion scans of the filter re-trace, Pluecker / Moeller dispatch.  Stateless __forceinline__ helpers.
// A leaf uses a helper only where its kernels stay the same instructions as with the block written out (tools/kernel_metadata.py
// --digest); where the compiler schedules the inlined helper differently, the leaf keeps the block, with a comment.
#pragma once
#include <type_traits>
#include "trace_loop.hip.h"
#include "trace_pool.hip.h"

namespace rtamd {
namespace dev {

// Policy traits of a leaf with an 8-lane child-parallel form next to its lane-per-ray form; a leaf overrides what differs.
struct LeafTraits
{
  static constexpr bool OCTET = true;
  static constexpr bool CONST_NG = false;
  static constexpr int GROUP = 8;
  static constexpr bool HIT_IN_MEMORY = false;
  static constexpr bool OCTET_ONLY = false;
  static constexpr int MIN_WAVES = TRACE_MIN_WAVES_PER_SIMD;
  static __device__ __forceinline__ bool octet_ok(const LaunchParams&) { return true; }
  static __device__ __forceinline__ void prepare() {}
};

template <int CTRL> __device__ __forceinline__ float dpp_f32(float v) { return __uint_as_float(dpp_u32<CTRL>(__float_as_uint(v))); }

// org, tnear, dir, tfar of the ray in an exchange row (words 0..7)
__device__ __forceinline__ RayState row_ray(const float* x)
{
  RayState r;
  r.ox = x[0]; r.oy = x[1]; r.oz = x[2]; r.tnear = x[3];
  r.dx = x[4]; r.dy = x[5]; r.dz = x[6]; r.tfar = x[7];
  return r;
}

// the winning lane's hit into the row: words 0..7 = t, Ng, u, v, geomID, primID; word 9 = 1
__device__ __forceinline__ void row_write_hit(float* x, const TriHit& h, uint32_t geomID, uint32_t primID)
{
  x[0] = h.t; x[1] = h.ngx; x[2] = h.ngy; x[3] = h.ngz; x[4] = h.u; x[5] = h.v;
  x[6] = __uint_as_float(geomID); x[7] = __uint_as_float(primID);
  x[9] = __uint_as_float(1u);
}

// minimum over the 4 lanes of a quad / the 8 lanes of an octet, in all of them
__device__ __forceinline__ float quad_min4(float v)
{
  v = fminf(v, dpp_f32<DPP_XOR1>(v));
  return fminf(v, dpp_f32<DPP_XOR2>(v));
}
__device__ __forceinline__ float octet_min8(float v)
{
  v = quad_min4(v);
  return fminf(v, dpp_f32<DPP_HALF_MIRROR>(v));
}
// the predicate of the 8 lanes of this lane's octet, lane 0 in bit 0
__device__ __forceinline__ uint32_t octet_ballot(bool p, uint32_t lid) { return (uint32_t)(__ballot(p) >> (lid & 56u)) & 0xffu; }

// leaf reference of the triangle / quad leaves: first record and record count (lane-per-ray forms)
__device__ __forceinline__ void leaf_range(uint32_t ref, uint32_t& first, uint32_t& count)
{
  first = ref & ((1u << TRI_START_BITS) - 1u);
  count = (ref >> TRI_START_BITS) & 31u;
}

// Filter re-trace (row f3, LaunchParams::exclOffsets): a candidate the host filter rejected for this ray before stays rejected.
// Primitives whose triangles share (geomID, primID) - the 8 triangles of a grid cell, the two of a quad - identify a rejected
// candidate by its distance as well: the kernels are deterministic, the same triangle yields a bit-equal t on the re-trace
// (Intersect1EpilogMU offers the candidates one by one, intersector_epilog.h:488-509; here the host does, between passes).
__device__ __forceinline__ bool candidate_excluded(const LaunchParams& P, uint32_t rayIdx, uint32_t geomID, uint32_t primID, float t)
{
  const uint32_t e1 = P.exclOffsets[rayIdx + 1];
  for (uint32_t e = P.exclOffsets[rayIdx]; e < e1; e++) {
    const uint2 q = P.exclPairs[e];
    if (q.x == geomID && q.y == primID && P.exclT[e] == __float_as_uint(t)) return true;
  }
  return false;
}

// Exclusion policy of the static mesh leaves' lane-per-ray loops: callable as excl(geomID, primID, t) -> bool, true drops a candidate before
// the block's minimum selection.  This default stands for the top-level scan under P.exclOffsets and is never called: the scan stays
// written out in the loop, since through any callable 34 of the 42 kernels of trace_tri.hip compile to another schedule
struct TopLevelExcl {};

// closest-hit epilogue of the lane-per-ray forms (Intersect1EpilogM, intersector_epilog.h:293-305); `best` by value: by reference
// the leaves compile to another schedule than with the block written out
__device__ __forceinline__ void commit_hit(RayState& r, const TriHit best, uint32_t geomID, uint32_t primID)
{
  r.tfar = best.t;
  r.ngx = best.ngx; r.ngy = best.ngy; r.ngz = best.ngz;
  r.u = best.u; r.v = best.v;
  r.primID = primID; r.geomID = geomID;
  r.hit = 1u;
}

// Host side: Leaf<true> = Pluecker test <-> robust traversal, Leaf<false> = Moeller test <-> fast traversal; ray-pool or lane kernel
template <template <bool> class Leaf> inline hipError_t launch_pluecker_moeller(const LaunchParams& p, hipStream_t stream, bool pluecker)
{
  if (p.poolKernel) return pluecker ? launch_leaf_pool<Leaf<true>, true>(p, stream) : launch_leaf_pool<Leaf<false>, false>(p, stream);
  return pluecker ? launch_leaf<Leaf<true>, true>(p, stream) : launch_leaf<Leaf<false>, false>(p, stream);
}

} // namespace dev
} // namespace rtamd
