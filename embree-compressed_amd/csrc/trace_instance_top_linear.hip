// Moving instances under time-dependent top-level boxes (accel kinds ACCEL_INSTTOP_LINEAR_PLUECKER / _MOELLER, inst_bounds=linear): the
// TOPMB form of the two-level kernel, which is the NODEMB form of trace_instance_mesh_mb_linear.hip - the general layout of `blobs` and
// `prims`, tree markers, instance entry, leaves, ranking, stacking and the overflow path are its text - with one change in which lanes
// read a time-dependent node.  The node buffer has the two sections of the kinds 30 / 31 (accel.h InstanceRecord): QNode8s for the
// static trees of the instanced scenes, and behind them, from a multiple of 144 bytes on, QNodeMB8s - here the top-level tree first,
// then the scenes' motion-blur trees, all referenced in 144-byte units.  A lane that is outside an instance (in the top-level tree) or
// in a motion-blur tree loads the nine dwordx4 of a QNodeMB8 and interpolates every plane between the node's two blocks at the ray's
// time, clamped to [0, 1] when the lane took its ray; a lane in a static tree of an instanced scene loads a QNode8 and gets the planes
// every other form gets, bit for bit, through the same timed formula over two equal blocks (trace_instance_body.hip.h).  So a ray enters
// a moving instance - and pays for the interpolated transform, its inverse and the instanced tree - only where the instance's box is at
// the ray's time, not wherever it is at some time of the shutter.
// The EXCL form for the re-traces of the host filter loop (inst_filters=1, trace_instance_filter.hip) lives here too.
#include "trace_instance.hip.h"

namespace rtamd {
namespace dev {

constexpr InstanceForm instance_top_linear_form(bool pluecker, bool occluded, bool vec, bool excl)
{
  InstanceForm f = instance_mesh_mb_form(pluecker, occluded, vec);
  f.NODEMB = f.TOPMB = true;
  f.EXCL = excl;
  return f;
}

// each instantiation is asked for the wave bound of its NODEMB twin
template <bool Pluecker, bool Occluded, bool Vec>
__global__ __launch_bounds__(TRACE_BLOCK, instance_min_waves(instance_top_linear_form(Pluecker, Occluded, Vec, false))) void trace_instance_top_linear_kernel(LaunchParams P)
{
  constexpr InstanceForm FORM = instance_top_linear_form(Pluecker, Occluded, Vec, false);
  using Leaf = MeshLeaves;
#include "trace_instance_body.hip.h"
}

// the filter loop runs closest-hit launches only: the bound of the closest-hit kernel above
template <bool Pluecker, bool Vec>
__global__ __launch_bounds__(TRACE_BLOCK, instance_min_waves(instance_top_linear_form(Pluecker, false, Vec, true))) void trace_instance_top_linear_filter_kernel(LaunchParams P)
{
  constexpr InstanceForm FORM = instance_top_linear_form(Pluecker, false, Vec, true);
  using Leaf = MeshLeaves;
#include "trace_instance_body.hip.h"
}

template <bool PLUECKER, bool OCCLUDED>
inline hipError_t launch_instance_top_linear_vec(const LaunchParams& p, hipStream_t stream)
{
  return launch_instance_pair<trace_instance_top_linear_kernel<PLUECKER, OCCLUDED, true>, trace_instance_top_linear_kernel<PLUECKER, OCCLUDED, false>>(p, stream);
}

template <bool PLUECKER>
inline hipError_t launch_instance_top_linear_filter_vec(const LaunchParams& p, hipStream_t stream)
{
  return launch_instance_pair<trace_instance_top_linear_filter_kernel<PLUECKER, true>, trace_instance_top_linear_filter_kernel<PLUECKER, false>>(p, stream);
}

} // namespace dev

hipError_t launch_trace_instance_top_linear(const LaunchParams& p, hipStream_t stream)
{
  if (p.counters) return hipErrorInvalidValue; // no instrumented twin (rt_trace.cpp refuses counted batches on scenes with instances)
  const bool pluecker = p.accel.kind == ACCEL_INSTTOP_LINEAR_PLUECKER;
  if (!pluecker && p.accel.kind != ACCEL_INSTTOP_LINEAR_MOELLER) return hipErrorInvalidValue;
  if (p.exclOffsets) { // a re-trace of the host filter loop: a list, its two-word keys, and a closest-hit launch
    if (p.occluded || !p.exclPairs || !p.exclT) return hipErrorInvalidValue;
    return pluecker ? dev::launch_instance_top_linear_filter_vec<true>(p, stream) : dev::launch_instance_top_linear_filter_vec<false>(p, stream);
  }
  if (pluecker) return p.occluded ? dev::launch_instance_top_linear_vec<true, true>(p, stream) : dev::launch_instance_top_linear_vec<true, false>(p, stream);
  return p.occluded ? dev::launch_instance_top_linear_vec<false, true>(p, stream) : dev::launch_instance_top_linear_vec<false, false>(p, stream);
}

} // namespace rtamd
