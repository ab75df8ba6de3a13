// Motion-blur meshes below an instance over time-dependent node boxes (accel kinds ACCEL_INSTMESHMB_LINEAR_PLUECKER / _MOELLER,
// inst_mb_bounds=linear): the NODEMB form of the two-level kernel, which is the MESHMB form of trace_instance_mesh_mb.hip - layout of
// `blobs` and `prims`, tree markers, instance entry, leaves, ranking, stacking and the overflow path are its text - with one change in
// the inner node step.  The node buffer has two sections (accel.h InstanceRecord): QNode8s for the top-level tree and the static trees
// of the instanced scenes, and behind them, from a multiple of 144 bytes on, the QNodeMB8s of the scenes' motion-blur trees, whose
// references index the buffer in 144-byte units.  The lanes of a wave are in different trees, so each lane picks its form of the step by
// the tree it is in: inside an instance, in a tree whose code has bit 1 set (INST_TREE_TRIMB, INST_TREE_QUADMB), it loads the nine
// dwordx4 of a QNodeMB8 and interpolates every plane between the node's two blocks at the ray's time, clamped to [0, 1] when the lane
// took its ray (the same value in world and local space; a NaN becomes 0) - the formula of accel.h QNodeMB8 and of trace_loop.hip.h's
// plane(), whose containment argument therefore carries over; everywhere else it loads the six dwordx4 of a QNode8 and gets the planes
// the other forms get, bit for bit, through the same timed formula over two equal blocks (trace_instance_body.hip.h).
#include "trace_instance.hip.h"

namespace rtamd {
namespace dev {

constexpr InstanceForm instance_mesh_mb_linear_form(bool pluecker, bool occluded, bool vec)
{
  InstanceForm f = instance_mesh_mb_form(pluecker, occluded, vec);
  f.NODEMB = true;
  return f;
}

// each instantiation is asked for the wave bound of its MESHMB twin
template <bool Pluecker, bool Occluded, bool Vec>
__global__ __launch_bounds__(TRACE_BLOCK, instance_min_waves(instance_mesh_mb_linear_form(Pluecker, Occluded, Vec))) void trace_instance_mesh_mb_linear_kernel(LaunchParams P)
{
  constexpr InstanceForm FORM = instance_mesh_mb_linear_form(Pluecker, Occluded, Vec);
  using Leaf = MeshLeaves;
#include "trace_instance_body.hip.h"
}

template <bool PLUECKER, bool OCCLUDED>
inline hipError_t launch_instance_mesh_mb_linear_vec(const LaunchParams& p, hipStream_t stream)
{
  return launch_instance_pair<trace_instance_mesh_mb_linear_kernel<PLUECKER, OCCLUDED, true>, trace_instance_mesh_mb_linear_kernel<PLUECKER, OCCLUDED, false>>(p, stream);
}

} // namespace dev

hipError_t launch_trace_instance_mesh_mb_linear(const LaunchParams& p, hipStream_t stream)
{
  if (p.counters) return hipErrorInvalidValue; // no instrumented twin (rt_trace.cpp refuses counted batches on scenes with instances)
  if (p.exclOffsets) return launch_trace_instance_filter(p, stream); // a re-trace of the host filter loop: the EXCL form (trace_instance_filter.hip)
  switch (p.accel.kind) {
  case ACCEL_INSTMESHMB_LINEAR_PLUECKER: return p.occluded ? dev::launch_instance_mesh_mb_linear_vec<true, true>(p, stream) : dev::launch_instance_mesh_mb_linear_vec<true, false>(p, stream);
  case ACCEL_INSTMESHMB_LINEAR_MOELLER: return p.occluded ? dev::launch_instance_mesh_mb_linear_vec<false, true>(p, stream) : dev::launch_instance_mesh_mb_linear_vec<false, false>(p, stream);
  default: return hipErrorInvalidValue;
  }
}

} // namespace rtamd
