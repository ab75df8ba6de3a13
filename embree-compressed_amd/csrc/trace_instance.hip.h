// The two-level traversal kernel of trace_instance.hip (where it is described) as a template, shared with
// trace_instance_mesh_mb.hip, which instantiates its MESHMB form, trace_instance_mesh_mb_linear.hip (the NODEMB form) and
// trace_instance_top_linear.hip (the TOPMB form).
#pragma once
#include <type_traits>
#include "trace_leaf.hip.h"
#include "trace_quad_tests.hip.h"
#include "trace_mb.hip.h"
#include "trace_curve.hip.h" // (and trace_line.hip.h): the leaves of the HAIR form
#include "instance_xfm.h"

namespace rtamd {
namespace dev {

// Waves per SIMD the register allocator is asked for: 4 (<= 128 VGPRs), as the triangle kernels run; the kernels must compile without
// scratch at this bound (tools/kernel_resources.sh, docs/experiments.md "Instancing").
#ifndef TRACE_INST_MIN_WAVES
#define TRACE_INST_MIN_WAVES 4
#endif

// Records requested per memory round trip inside a block of 4.  The closest-hit Pluecker kernel carries two instance ids and the hit on
// top of the Pluecker test's temporaries: with four records in flight it needs 116 bytes of scratch at 128 VGPRs.
#ifndef TRACE_INST_FETCH
#define TRACE_INST_FETCH 2
#endif
// The QUADS instantiations carry the quad block loop (a record is four dwordx4, a block has 8 candidates) next to the triangle loop.
// Three of the four compile without scratch at 4 waves per SIMD; closest-hit Pluecker does not (76 bytes of scratch with two QuadRecords
// per round trip, 36 with one), as the static quad lane kernel's does not (trace_quad.hip): it alone is asked for 3 waves (<= 168 VGPRs).
#ifndef TRACE_INST_QUADS_MIN_WAVES_PLUECKER_CLOSEST
#define TRACE_INST_QUADS_MIN_WAVES_PLUECKER_CLOSEST 3
#endif
// QuadRecords requested per memory round trip inside a block of 4 (1 or 2)
#ifndef TRACE_INST_QUAD_FETCH
#define TRACE_INST_QUAD_FETCH 2
#endif
// MESHMB (trace_instance_mesh_mb.hip): the motion-blur leaves on top of the QUADS and XFMB forms.  Asked for the bound of the QUADS
// twin; records per memory round trip as in the top-level leaves (trace_tri_mb.hip TRIMB_FETCH, trace_quad_mb.hip QUADMB_FETCH).
#ifndef TRACE_INST_TRIMB_FETCH
#define TRACE_INST_TRIMB_FETCH 2
#endif
#ifndef TRACE_INST_QUADMB_FETCH
#define TRACE_INST_QUADMB_FETCH 1
#endif
// The closest-hit MESHMB kernels spill at the bound of their QUADS twins (Pluecker: 20 bytes of scratch at 3 waves, Moeller: 76 at 4;
// with one record per round trip in every leaf still 12 and 36): they are asked for one wave less, the any-hit kernels keep 4
// (docs/experiments.md, "Motion-blur meshes below an instance").
#ifndef TRACE_INST_MESHMB_MIN_WAVES_PLUECKER_CLOSEST
#define TRACE_INST_MESHMB_MIN_WAVES_PLUECKER_CLOSEST 2
#endif
#ifndef TRACE_INST_MESHMB_MIN_WAVES_MOELLER_CLOSEST
#define TRACE_INST_MESHMB_MIN_WAVES_MOELLER_CLOSEST 3
#endif
// NODEMB (trace_instance_mesh_mb_linear.hip): the MESHMB form with time-dependent nodes in the motion-blur trees - twelve more node words
// and the ray's time across the node step.  Each instantiation is asked for the bound of its MESHMB twin.
constexpr int inst_min_waves(bool pluecker, bool occluded, bool quads, bool xfmb, bool meshmb = false)
{
  if (meshmb && !occluded) return pluecker ? TRACE_INST_MESHMB_MIN_WAVES_PLUECKER_CLOSEST : TRACE_INST_MESHMB_MIN_WAVES_MOELLER_CLOSEST;
  return quads && pluecker && !occluded ? TRACE_INST_QUADS_MIN_WAVES_PLUECKER_CLOSEST : TRACE_INST_MIN_WAVES;
}
constexpr int inst_nodemb_min_waves(bool pluecker, bool occluded) { return inst_min_waves(pluecker, occluded, true, true, true); }
// HAIR (trace_instance_hair.hip): the MESHMB form with the line and the ribbon leaf (trace_line.hip.h, trace_curve.hip.h) beside the four
// mesh leaves.  Each instantiation is asked for the highest wave count, from its MESHMB twin's bound down to 2, at which it compiles
// without scratch and without VGPR spills (docs/experiments.md, "Hair below an instance").
#ifndef TRACE_INST_HAIR_MIN_WAVES_PLUECKER_CLOSEST
#define TRACE_INST_HAIR_MIN_WAVES_PLUECKER_CLOSEST 2
#endif
#ifndef TRACE_INST_HAIR_MIN_WAVES_MOELLER_CLOSEST
#define TRACE_INST_HAIR_MIN_WAVES_MOELLER_CLOSEST 2
#endif
#ifndef TRACE_INST_HAIR_MIN_WAVES_PLUECKER_ANY
#define TRACE_INST_HAIR_MIN_WAVES_PLUECKER_ANY 3
#endif
#ifndef TRACE_INST_HAIR_MIN_WAVES_MOELLER_ANY
#define TRACE_INST_HAIR_MIN_WAVES_MOELLER_ANY 4
#endif
constexpr int inst_hair_min_waves(bool pluecker, bool occluded)
{
  return occluded ? (pluecker ? TRACE_INST_HAIR_MIN_WAVES_PLUECKER_ANY : TRACE_INST_HAIR_MIN_WAVES_MOELLER_ANY)
                  : (pluecker ? TRACE_INST_HAIR_MIN_WAVES_PLUECKER_CLOSEST : TRACE_INST_HAIR_MIN_WAVES_MOELLER_CLOSEST);
}

// Filter re-trace below an instance (the EXCL form of the body, trace_instance_filter.hip): a candidate the host filter loop rejected for this
// ray before stays rejected.  The key is (instance geomID, geomID, primID, bits of t) for every leaf type: the kernels are deterministic,
// the same record gives the same t when the ray is traced again; t tells the two triangles of a quad apart (a ray through the diagonal
// v1-v3 hits both at one t: rejecting one rejects both) and a motion-blur record from its sibling; the instance tells apart two instances
// of one scene that give the same local ray.  For instance launches an entry of exclT is two words (trace.h).
__device__ __forceinline__ bool instance_candidate_excluded(const LaunchParams& P, uint32_t rayIdx, uint32_t inst, uint32_t geomID, uint32_t primID, float t)
{
  const uint2* __restrict__ ti = (const uint2*)P.exclT;
  const uint32_t e1 = P.exclOffsets[rayIdx + 1];
  for (uint32_t e = P.exclOffsets[rayIdx]; e < e1; e++) {
    const uint2 q = P.exclPairs[e];
    const uint2 k = ti[e];
    if (q.x == geomID && q.y == primID && k.x == __float_as_uint(t) && k.y == inst) return true;
  }
  return false;
}

template <bool PLUECKER, bool OCCLUDED, bool VEC, bool QUADS, bool XFMB>
__global__ __launch_bounds__(TRACE_BLOCK, inst_min_waves(PLUECKER, OCCLUDED, QUADS, XFMB)) void trace_instance_kernel(LaunchParams P)
{
  // the body needs in scope: P, PLUECKER, OCCLUDED, VEC, QUADS, XFMB, MESHMB, NODEMB, TOPMB, EXCL, HAIR (it asserts them)
  constexpr bool MESHMB = false, NODEMB = false, TOPMB = false; // the MESHMB form is trace_instance_mesh_mb.hip's kernel, the NODEMB form trace_instance_mesh_mb_linear.hip's
  constexpr bool EXCL = false; // the EXCL form of the filter re-traces is trace_instance_filter.hip's kernel
  constexpr bool HAIR = false; // the HAIR form (line and curve trees below an instance) is trace_instance_hair.hip's kernel
#include "trace_instance_body.hip.h"
}

// KVEC / KGEN: the instantiations for 16-byte aligned records and for any others
template <void (*KVEC)(LaunchParams), void (*KGEN)(LaunchParams)>
inline hipError_t launch_instance_pair(const LaunchParams& p, hipStream_t stream)
{
  const bool vec = (p.stride % 16 == 0) && (((uintptr_t)p.rays) % 16 == 0);
  // persistent grid = what is resident at once for this instantiation, capped by the host's bound (which sized the spill area)
  static int occVec = 0, occGen = 0;
  int& occ = vec ? occVec : occGen;
  if (occ == 0) {
    hipError_t e = vec ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, KVEC, TRACE_BLOCK, 0) : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, KGEN, TRACE_BLOCK, 0);
    if (e != hipSuccess || occ <= 0) occ = 1;
  }
  uint32_t blocks = (p.blocksPerCU ? std::min<uint32_t>(p.blocksPerCU, (uint32_t)occ) : (uint32_t)occ) * p.numCUs;
  if (blocks > p.gridBlocks) blocks = p.gridBlocks;
  if (vec) hipLaunchKernelGGL(KVEC, dim3(blocks), dim3(TRACE_BLOCK), 0, stream, p);
  else hipLaunchKernelGGL(KGEN, dim3(blocks), dim3(TRACE_BLOCK), 0, stream, p);
  return hipGetLastError();
}

template <bool PLUECKER, bool OCCLUDED, bool QUADS, bool XFMB>
inline hipError_t launch_instance_vec(const LaunchParams& p, hipStream_t stream)
{
  return launch_instance_pair<trace_instance_kernel<PLUECKER, OCCLUDED, true, QUADS, XFMB>, trace_instance_kernel<PLUECKER, OCCLUDED, false, QUADS, XFMB>>(p, stream);
}

} // namespace dev
} // namespace rtamd
