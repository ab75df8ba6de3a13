// Subdivision meshes below an instance (accel kinds ACCEL_INSTSUBDIV_GRID / ACCEL_INSTSUBDIV_CBVH_LEAF, Scene::instSubdivAccel): the
// SUBDIV form of the two-level kernel of trace_instance.hip.  The walk is that kernel's text (trace_instance_body.hip.h) - the 64 work
// queues with chunked grabs, the stack[entry][lane] LDS layout with its HBM overflow columns and the `overflow` word, the QNode8 step in
// the reference's child order, the entry into an instance (through instance_world2local for a moving one), the exit marker and the
// re-read of the world ray, the leafBatch / nodeWork rule - with the two one-ray-per-lane subdivision leaves below an instance instead
// of the mesh block loops:
//   GridCellLeaf::intersect (trace_grid.hip.h)                   eager accel: the 8 Pluecker triangles of a 3x3-vertex cell
//   CbvhLeaf<MODE_LEAF, C, false>::intersect (trace_cbvh.hip.h)  bvh4.compressed.leaf: the walk of one cBVH blob, C = 1..5
// What differs from the mesh forms:
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
// trace_instance_subdiv_top_linear.hip holds the TOPMB form for a top-level tree of time-dependent nodes (kinds
// ACCEL_INSTSUBDIV_TOP_LINEAR_*, inst_subdiv_bounds=linear).
#include "trace_instance_subdiv.hip.h"

namespace rtamd {
namespace dev {

template <typename Leaf, bool Occluded, bool Vec>
__global__ __launch_bounds__(TRACE_BLOCK, instance_min_waves(instance_subdiv_form<Leaf>(Occluded, Vec, false), Leaf::MIN_WAVES)) void trace_instance_subdiv_kernel(LaunchParams P)
{
  constexpr InstanceForm FORM = instance_subdiv_form<Leaf>(Occluded, Vec, false);
#include "trace_instance_body.hip.h"
}

template <typename Leaf> inline hipError_t launch_instance_subdiv(const LaunchParams& p, hipStream_t stream)
{
  return p.occluded ? launch_instance_pair<trace_instance_subdiv_kernel<Leaf, true, true>, trace_instance_subdiv_kernel<Leaf, true, false>>(p, stream)
                    : launch_instance_pair<trace_instance_subdiv_kernel<Leaf, false, true>, trace_instance_subdiv_kernel<Leaf, false, false>>(p, stream);
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
