// Moving subdivision instances under time-dependent top-level boxes (accel kinds ACCEL_INSTSUBDIV_TOP_LINEAR_GRID / _CBVH_LEAF,
// inst_subdiv_bounds=linear): the TOPMB form of the subdivision two-level kernel of trace_instance_subdiv.hip - instance entry, the two
// subdivision leaves, ranking, stacking, the HBM overflow path, the exit marker and the re-read of the world ray are its text
// (trace_instance_body.hip.h) - with one change in which lanes read a time-dependent node.  The node buffer has two sections
// (accel.h InstanceRecord): the instanced scenes' BVH8s as QNode8s from its start and, from a multiple of 144 bytes on, the top-level
// tree as QNodeMB8s, referenced in 144-byte units.  A lane outside an instance loads the nine dwordx4 of a QNodeMB8 and interpolates
// every plane between the node's two blocks at the ray's time, clamped to [0, 1] when the lane took its ray (NaN: 0); a lane inside an
// instance loads a QNode8 and gets the planes of the swept form, bit for bit, through the same timed formula over two equal blocks.  So a
// ray enters a moving instance - and pays for the interpolated transform, its inverse and the instanced tree - only where the
// instance's box is at the ray's time.  No EXCL form: filters stay refused on subdivision instances.
// 24 kernels: 6 leaves x closest / any hit x 16-byte aligned records / others.
#include "trace_instance_subdiv.hip.h"

namespace rtamd {
namespace dev {

// each instantiation is asked for the wave bound of its swept twin (profiles/instance_subdiv_top_linear_kernel_resources.txt)
template <typename Leaf, bool Occluded, bool Vec>
__global__ __launch_bounds__(TRACE_BLOCK, instance_min_waves(instance_subdiv_form<Leaf>(Occluded, Vec, true), Leaf::MIN_WAVES)) void trace_instance_subdiv_top_linear_kernel(LaunchParams P)
{
  constexpr InstanceForm FORM = instance_subdiv_form<Leaf>(Occluded, Vec, true);
#include "trace_instance_body.hip.h"
}

template <typename Leaf> inline hipError_t launch_instance_subdiv_top_linear(const LaunchParams& p, hipStream_t stream)
{
  return p.occluded ? launch_instance_pair<trace_instance_subdiv_top_linear_kernel<Leaf, true, true>, trace_instance_subdiv_top_linear_kernel<Leaf, true, false>>(p, stream)
                    : launch_instance_pair<trace_instance_subdiv_top_linear_kernel<Leaf, false, true>, trace_instance_subdiv_top_linear_kernel<Leaf, false, false>>(p, stream);
}

} // namespace dev

hipError_t launch_trace_instance_subdiv_top_linear(const LaunchParams& p, hipStream_t stream)
{
  if (p.counters) return hipErrorInvalidValue; // no instrumented twin (rt_trace.cpp refuses counted batches on scenes with instances)
  switch (p.accel.kind) {
  case ACCEL_INSTSUBDIV_TOP_LINEAR_GRID: return dev::launch_instance_subdiv_top_linear<dev::GridCellLeaf>(p, stream);
  case ACCEL_INSTSUBDIV_TOP_LINEAR_CBVH_LEAF:
    switch (p.cbvhLevels) { // one kernel per compression level C = 1..5 of the instanced scenes
    case 1: return dev::launch_instance_subdiv_top_linear<dev::CbvhLeaf<dev::MODE_LEAF, 1, false>>(p, stream);
    case 2: return dev::launch_instance_subdiv_top_linear<dev::CbvhLeaf<dev::MODE_LEAF, 2, false>>(p, stream);
    case 3: return dev::launch_instance_subdiv_top_linear<dev::CbvhLeaf<dev::MODE_LEAF, 3, false>>(p, stream);
    case 4: return dev::launch_instance_subdiv_top_linear<dev::CbvhLeaf<dev::MODE_LEAF, 4, false>>(p, stream);
    case 5: return dev::launch_instance_subdiv_top_linear<dev::CbvhLeaf<dev::MODE_LEAF, 5, false>>(p, stream);
    default: return hipErrorInvalidValue;
    }
  default: return hipErrorInvalidValue;
  }
}

} // namespace rtamd
