// The two-level traversal kernels, mesh and subdivision instances alike: what a form of the kernel is (InstanceForm), the waves per SIMD
// each form is asked for, the launcher of a kernel pair, and the kernel template of trace_instance.hip (where the kernel is described).
// The kernel's text is trace_instance_body.hip.h, included inside the braces of every __global__ function of the family:
//   trace_instance.hip                     trace_instance_kernel                      PLUECKER x OCCLUDED x QUADS x XFMB
//   trace_instance_mesh_mb.hip             trace_instance_mesh_mb_kernel              MESHMB
//   trace_instance_mesh_mb_linear.hip      trace_instance_mesh_mb_linear_kernel       NODEMB
//   trace_instance_top_linear.hip          trace_instance_top_linear[_filter]_kernel  TOPMB (and its EXCL form)
//   trace_instance_filter.hip              trace_instance_filter_kernel               EXCL
//   trace_instance_hair.hip                trace_instance_hair_kernel                 HAIR
//   trace_instance_hair_mb.hip             trace_instance_hair_mb_kernel              HAIRMB
//   trace_instance_subdiv.hip              trace_instance_subdiv_kernel               SUBDIV (through trace_instance_subdiv.hip.h)
//   trace_instance_subdiv_top_linear.hip   trace_instance_subdiv_top_linear_kernel    SUBDIV, TOPMB
// One unit per kernel template so that the instantiations compile beside each other.
#pragma once
#include <type_traits>
#include "trace_leaf.hip.h"
#include "trace_tri.hip.h" // the leaves of the mesh family
#include "trace_quad.hip.h"
#include "trace_mb.hip.h"
#include "trace_curve.hip.h" // (and trace_line.hip.h): the leaves of the HAIR form
#include "trace_curve_mb.hip.h" // the leaves of the HAIRMB form
#include "trace_line_mb.hip.h"
#include "instance_xfm.h"

namespace rtamd {
namespace dev {

// A form of the two-level kernel: the compile-time constants of trace_instance_body.hip.h, which describes each where it uses it.  A
// kernel builds its form from its template parameters and names what it turns on; the body, included with `FORM` in scope, unpacks it.
// A new constant is a member here, with its default, and the kernels that set it.
struct InstanceForm
{
  bool PLUECKER = false; // Pluecker test and robust traversal / Moeller test and fast traversal (mesh family)
  bool OCCLUDED = false; // any hit / closest hit
  bool VEC = false;      // ray records are 16-byte aligned
  bool QUADS = false;    // an instanced scene may hold a quad tree
  bool XFMB = false;     // an instance may have transform time steps
  bool MESHMB = false;   // an instanced scene holds up to four trees, two of them of motion-blur meshes
  bool NODEMB = false;   // some trees are made of time-dependent nodes: the node step interpolates the planes at the ray's time
  bool TOPMB = false;    // NODEMB, and the top-level tree is one of them
  bool EXCL = false;     // the exclusion scan of the filter re-traces
  bool HAIR = false;     // MESHMB, and a curve and a line tree behind the four mesh trees
  bool HAIRMB = false;   // HAIR, and a motion-blur curve and a motion-blur line tree: eight trees per instanced scene
  bool SUBDIV = false;   // the subdivision family: an instanced scene is one tree whose leaves are the kernel's `Leaf`
  bool GRID = false;     // SUBDIV: that leaf is the eager accel's GridCellLeaf (a wave bound depends on it)
};

// The `Leaf` of the mesh family's kernels, kept only as the type the body's SUBDIV text names: the mesh section calls TriLeaf and QuadLeaf
// (trace_tri.hip.h, trace_quad.hip.h) by the lane's tree and holds the two motion-blur block loops; this is never called.
struct MeshLeaves : LeafTraits
{
  template <bool OCCLUDED, bool COUNT> static __device__ __forceinline__ bool intersect(const LaunchParams&, uint32_t, RayState&, WorkCounters&, uint32_t) { return false; }
};

// Waves per SIMD the register allocator is asked for: 4 (<= 128 VGPRs), as the triangle kernels run; the kernels must compile without
// scratch at their bound (tools/kernel_resources.sh, docs/experiments.md "Instancing").  The exceptions are in instance_min_waves below.
#ifndef TRACE_INST_MIN_WAVES
#define TRACE_INST_MIN_WAVES 4
#endif

// Records requested per memory round trip inside a block of 4.  The closest-hit Pluecker kernel carries two instance ids and the hit on
// top of the Pluecker test's temporaries: with four records in flight it needs 116 bytes of scratch at 128 VGPRs.
#ifndef TRACE_INST_FETCH
#define TRACE_INST_FETCH 2
#endif
// QuadRecords requested per memory round trip inside a block of 4 (1 or 2)
#ifndef TRACE_INST_QUAD_FETCH
#define TRACE_INST_QUAD_FETCH 2
#endif
// MESHMB: records per memory round trip as in the top-level leaves (trace_tri_mb.hip TRIMB_FETCH, trace_quad_mb.hip QUADMB_FETCH).
#ifndef TRACE_INST_TRIMB_FETCH
#define TRACE_INST_TRIMB_FETCH 2
#endif
#ifndef TRACE_INST_QUADMB_FETCH
#define TRACE_INST_QUADMB_FETCH 1
#endif

#ifndef TRACE_INST_QUADS_MIN_WAVES_PLUECKER_CLOSEST
#define TRACE_INST_QUADS_MIN_WAVES_PLUECKER_CLOSEST 3
#endif
#ifndef TRACE_INST_MESHMB_MIN_WAVES_PLUECKER_CLOSEST
#define TRACE_INST_MESHMB_MIN_WAVES_PLUECKER_CLOSEST 2
#endif
#ifndef TRACE_INST_MESHMB_MIN_WAVES_MOELLER_CLOSEST
#define TRACE_INST_MESHMB_MIN_WAVES_MOELLER_CLOSEST 3
#endif
#ifndef TRACE_INST_FILTER_MIN_WAVES_TRI_PLUECKER
#define TRACE_INST_FILTER_MIN_WAVES_TRI_PLUECKER 3
#endif
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
#ifndef TRACE_INST_HAIRMB_MIN_WAVES_PLUECKER_CLOSEST
#define TRACE_INST_HAIRMB_MIN_WAVES_PLUECKER_CLOSEST 2
#endif
#ifndef TRACE_INST_HAIRMB_MIN_WAVES_MOELLER_CLOSEST
#define TRACE_INST_HAIRMB_MIN_WAVES_MOELLER_CLOSEST 2
#endif
#ifndef TRACE_INST_HAIRMB_MIN_WAVES_PLUECKER_ANY
#define TRACE_INST_HAIRMB_MIN_WAVES_PLUECKER_ANY 3
#endif
#ifndef TRACE_INST_HAIRMB_MIN_WAVES_MOELLER_ANY
#define TRACE_INST_HAIRMB_MIN_WAVES_MOELLER_ANY 3
#endif

// The wave bound of a form; `leafWaves` is Leaf::MIN_WAVES in the subdivision family.  Every exception, first match wins:
constexpr int instance_min_waves(InstanceForm f, int leafWaves = TRACE_INST_MIN_WAVES)
{
  // SUBDIV: the bound of the same leaf's top-level lane kernel (3, cBVH from C = 4 on 2), at which the cBVH kernels compile without
  // scratch.  The eager closest-hit kernel needs 36 bytes of scratch at 3 waves (168 VGPRs) where its twin has none - the lane kernel
  // tests cells 8 lanes per ray and does not hold GridCellLeaf::intersect with its 40 cell words at all; the ray-pool kernel, which does,
  // takes 186 VGPRs: one wave less (docs/experiments.md, "Subdivision meshes below an instance").  TOPMB: the swept twin's bound
  if (f.SUBDIV) return f.GRID && !f.OCCLUDED ? leafWaves - 1 : leafWaves;
  // HAIRMB: the motion-blur line and ribbon leaves beside the six of the HAIR form.  The highest wave count, from the HAIR twin's bound
  // down to 2, at which the kernel compiles without scratch and without VGPR spills (docs/experiments.md, "Moving hair below an instance")
  if (f.HAIRMB)
    return f.OCCLUDED ? (f.PLUECKER ? TRACE_INST_HAIRMB_MIN_WAVES_PLUECKER_ANY : TRACE_INST_HAIRMB_MIN_WAVES_MOELLER_ANY)
                      : (f.PLUECKER ? TRACE_INST_HAIRMB_MIN_WAVES_PLUECKER_CLOSEST : TRACE_INST_HAIRMB_MIN_WAVES_MOELLER_CLOSEST);
  // HAIR: the line and the ribbon leaf beside the four mesh leaves.  The highest wave count, from the MESHMB twin's bound down to 2, at
  // which the kernel compiles without scratch and without VGPR spills (docs/experiments.md, "Hair below an instance")
  if (f.HAIR)
    return f.OCCLUDED ? (f.PLUECKER ? TRACE_INST_HAIR_MIN_WAVES_PLUECKER_ANY : TRACE_INST_HAIR_MIN_WAVES_MOELLER_ANY)
                      : (f.PLUECKER ? TRACE_INST_HAIR_MIN_WAVES_PLUECKER_CLOSEST : TRACE_INST_HAIR_MIN_WAVES_MOELLER_CLOSEST);
  // EXCL: the bound of the unfiltered closest-hit twin wherever the kernel compiles without scratch there - all forms but one.  The
  // Pluecker triangle-only forms (kinds 14 and 18) are at 128 VGPRs without the scan and spill 12 bytes with it: one wave less
  if (f.EXCL && f.PLUECKER && !f.QUADS && !f.MESHMB) return TRACE_INST_FILTER_MIN_WAVES_TRI_PLUECKER;
  // MESHMB, and with it NODEMB and TOPMB, each at the bound of its MESHMB twin: the closest-hit kernels spill at the bound of their
  // QUADS twins (Pluecker: 20 bytes of scratch at 3 waves, Moeller: 76 at 4; with one record per round trip in every leaf still 12 and
  // 36) and are asked for one wave less, the any-hit kernels keep 4 (docs/experiments.md, "Motion-blur meshes below an instance")
  if (f.MESHMB && !f.OCCLUDED) return f.PLUECKER ? TRACE_INST_MESHMB_MIN_WAVES_PLUECKER_CLOSEST : TRACE_INST_MESHMB_MIN_WAVES_MOELLER_CLOSEST;
  // QUADS: the quad block loop (a record is four dwordx4, a block has 8 candidates) next to the triangle loop.  Three of the four
  // instantiations compile without scratch at 4 waves; closest-hit Pluecker does not (76 bytes of scratch with two QuadRecords per
  // round trip, 36 with one), as the static quad lane kernel's does not (trace_quad.hip): it alone is asked for 3 waves (<= 168 VGPRs)
  if (f.QUADS && f.PLUECKER && !f.OCCLUDED) return TRACE_INST_QUADS_MIN_WAVES_PLUECKER_CLOSEST;
  return TRACE_INST_MIN_WAVES;
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

constexpr InstanceForm instance_form(bool pluecker, bool occluded, bool vec, bool quads, bool xfmb)
{
  InstanceForm f;
  f.PLUECKER = pluecker; f.OCCLUDED = occluded; f.VEC = vec; f.QUADS = quads; f.XFMB = xfmb;
  return f;
}
// the MESHMB form, from which the NODEMB, TOPMB, HAIR and (through HAIR) HAIRMB forms start: always the general layout, quads and instance steps allowed
constexpr InstanceForm instance_mesh_mb_form(bool pluecker, bool occluded, bool vec)
{
  InstanceForm f = instance_form(pluecker, occluded, vec, true, true);
  f.MESHMB = true;
  return f;
}

// the HAIR form: the general layout over swept boxes; no exclusion scan in the hair leaves, filters beside instanced hair are refused.
// Here and not in trace_instance_hair.hip because the HAIRMB form (trace_instance_hair_mb.hip) starts from it.
constexpr InstanceForm instance_hair_form(bool pluecker, bool occluded, bool vec)
{
  InstanceForm f = instance_mesh_mb_form(pluecker, occluded, vec);
  f.HAIR = true;
  return f;
}

template <bool Pluecker, bool Occluded, bool Vec, bool Quads, bool Xfmb>
__global__ __launch_bounds__(TRACE_BLOCK, instance_min_waves(instance_form(Pluecker, Occluded, Vec, Quads, Xfmb))) void trace_instance_kernel(LaunchParams P)
{
  // the body needs in scope: P, FORM and Leaf
  constexpr InstanceForm FORM = instance_form(Pluecker, Occluded, Vec, Quads, Xfmb);
  using Leaf = MeshLeaves;
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
