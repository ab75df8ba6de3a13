// Subdivision meshes below an instance (accel kinds ACCEL_INSTSUBDIV_GRID / ACCEL_INSTSUBDIV_CBVH_LEAF, Scene::instSubdivAccel): a sibling
// of the two-level kernel of trace_instance.hip, whose machinery it restates - the 64 work queues with chunked grabs, the
// stack[entry][lane] LDS layout with its HBM overflow columns and the `overflow` word, the QNode8 step in the reference's child order,
// the entry into an instance (through instance_world2local for a moving one), the exit marker and the re-read of the world ray, the
// leafBatch / nodeWork rule - with the two one-ray-per-lane subdivision leaves below an instance instead of the mesh block loops:
//   GridCellLeaf::intersect (trace_grid.hip.h)                   eager accel: the 8 Pluecker triangles of a 3x3-vertex cell
//   CbvhLeaf<MODE_LEAF, C, false>::intersect (trace_cbvh.hip.h)  bvh4.compressed.leaf: the walk of one cBVH blob, C = 1..5
// A sibling and not a seventh constant of trace_instance_body.hip.h: that text is held to the instruction streams of its 40
// instantiations.  What differs from it:
//   - always the robust traversal (TravRay<true>) on both levels, as the subdivision accels run at top level (launch_leaf<Leaf, true>);
//   - every instantiation takes instances with transform time steps (the XFMB path);
//   - an instanced scene has one tree: no pending-tree markers, one state bit for "inside";
//   - a leaf below an instance calls Leaf::intersect<OCCLUDED, false> on the LOCAL ray.  `blobs` starts with the InstanceRecords and
//     InstanceSteps; the leaf blobs follow from a multiple of the blob stride on and the leaf references are rebased (accel.h), so the
//     leaf's own addressing, P.accel.blobs + index * stride, finds them.  A closest hit keeps the instanced scene's geomID / primID and
//     its u, v; Ng is what the leaf produces (the eager cell's local-space Ng, or the fork's dummy (1, 0, 0), written at store time
//     like the lane kernel's CONST_NG leaves); t is common to both spaces; instID is the instance's geomID
//     (instance_intersector.cpp:51-62).  Any-hit: an eager hit ends the ray; for compressed.leaf the fork's occluded() stub
//     (compressed.h:754-756) applies to the local ray - a blob whose exact bounds pass the robust slab test reports occluded.
// Leaf::prepare() runs once per kernel (the cBVH decode tables in LDS).  No octet / quad form, no ray-pool form, no root cull pre-pass,
// no service kernel, no instrumented twin.  24 kernels: 6 leaves x closest / any hit x 16-byte aligned records / others.
// The kernel's text is trace_instance_subdiv_body.hip.h, included below with TOPMB = false; trace_instance_subdiv_top_linear.hip includes
// it with TOPMB = true for a top-level tree of time-dependent nodes (kinds ACCEL_INSTSUBDIV_TOP_LINEAR_*, inst_subdiv_bounds=linear).
#include "trace_instance_subdiv.hip.h"

namespace rtamd {
namespace dev {

template <typename Leaf, bool OCCLUDED, bool VEC>
__global__ __launch_bounds__(TRACE_BLOCK, (inst_subdiv_min_waves<Leaf, OCCLUDED>())) void trace_instance_subdiv_kernel(LaunchParams P)
{
  constexpr bool TOPMB = false; // the TOPMB form (a top-level tree of time-dependent nodes) is trace_instance_subdiv_top_linear.hip's kernel
#include "trace_instance_subdiv_body.hip.h"
}

template <typename Leaf, bool OCCLUDED>
inline hipError_t launch_instance_subdiv_vec(const LaunchParams& p, hipStream_t stream)
{
  const bool vec = (p.stride % 16 == 0) && (((uintptr_t)p.rays) % 16 == 0);
  // persistent grid = what is resident at once for this instantiation, capped by the host's bound (which sized the spill area)
  static int occVec = 0, occGen = 0;
  int& occ = vec ? occVec : occGen;
  if (occ == 0) {
    hipError_t e = vec ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, trace_instance_subdiv_kernel<Leaf, OCCLUDED, true>, TRACE_BLOCK, 0)
                       : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, trace_instance_subdiv_kernel<Leaf, OCCLUDED, false>, TRACE_BLOCK, 0);
    if (e != hipSuccess || occ <= 0) occ = 1;
  }
  uint32_t blocks = (p.blocksPerCU ? std::min<uint32_t>(p.blocksPerCU, (uint32_t)occ) : (uint32_t)occ) * p.numCUs;
  if (blocks > p.gridBlocks) blocks = p.gridBlocks;
  if (vec) hipLaunchKernelGGL((trace_instance_subdiv_kernel<Leaf, OCCLUDED, true>), dim3(blocks), dim3(TRACE_BLOCK), 0, stream, p);
  else hipLaunchKernelGGL((trace_instance_subdiv_kernel<Leaf, OCCLUDED, false>), dim3(blocks), dim3(TRACE_BLOCK), 0, stream, p);
  return hipGetLastError();
}

template <typename Leaf> inline hipError_t launch_instance_subdiv(const LaunchParams& p, hipStream_t stream)
{
  return p.occluded ? launch_instance_subdiv_vec<Leaf, true>(p, stream) : launch_instance_subdiv_vec<Leaf, false>(p, stream);
}

} // namespace dev

hipError_t launch_trace_instance_subdiv(const LaunchParams& p, hipStream_t stream)
{
  if (p.counters) return hipErrorInvalidValue; // no instrumented twin (rt_trace.cpp refuses counted batches on scenes with instances)
  switch (p.accel.kind) {
  case ACCEL_INSTSUBDIV_GRID: return dev::launch_instance_subdiv<dev::GridCellLeaf>(p, stream);
  case ACCEL_INSTSUBDIV_CBVH_LEAF:
    switch (p.cbvhLevels) { // one kernel per compression level C = 1..5 of the instanced scenes
    case 1: return dev::launch_instance_subdiv<dev::CbvhLeaf<dev::MODE_LEAF, 1, false>>(p, stream);
    case 2: return dev::launch_instance_subdiv<dev::CbvhLeaf<dev::MODE_LEAF, 2, false>>(p, stream);
    case 3: return dev::launch_instance_subdiv<dev::CbvhLeaf<dev::MODE_LEAF, 3, false>>(p, stream);
    case 4: return dev::launch_instance_subdiv<dev::CbvhLeaf<dev::MODE_LEAF, 4, false>>(p, stream);
    case 5: return dev::launch_instance_subdiv<dev::CbvhLeaf<dev::MODE_LEAF, 5, false>>(p, stream);
    default: return hipErrorInvalidValue;
    }
  default: return hipErrorInvalidValue;
  }
}

} // namespace rtamd
