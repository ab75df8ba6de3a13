// Triangle leaves of the quantized BVH8: Triangle4v / Pluecker (robust) and Triangle4 / Moeller (fast).
// 48-byte records fetched as three dwordx4; every group of 4 records from the leaf start is one block with the
// reference's 4-wide SIMD semantics.
//   block loop            kernels/geometry/intersector_iterators.h:32-36 (ArrayIntersector1)
//   epilog / tie rules    kernels/geometry/intersector_epilog.h:226-307 (closest), :388-450 (any hit)
#include "trace_leaf.hip.h"
#include "trace_tri.hip.h"
#include "trace_service.hip.h"
#include "trace_cull.hip.h"

namespace rtamd {

hipError_t launch_cull(const LaunchParams& p, hipStream_t stream)
{
  // every subdivision accel, Triangle4v and the Pluecker quads traverse robustly, Triangle4 and the Moeller quads with the fast test
  // (same choice as the traversal kernels: the kind's row, accel_kinds.h)
  if (kind_row(p.accel.kind).robust) return p.occluded ? dev::launch_cull_vec<true, true>(p, stream) : dev::launch_cull_vec<true, false>(p, stream);
  return p.occluded ? dev::launch_cull_vec<false, true>(p, stream) : dev::launch_cull_vec<false, false>(p, stream);
}

hipError_t launch_service_tri(const ServiceParams& s, hipStream_t stream)
{
  if (s.base.accel.kind == ACCEL_TRI_PLUECKER) return dev::launch_service_kernel<dev::TriLeaf<true>, true>(s, stream);
  return dev::launch_service_kernel<dev::TriLeaf<false>, false>(s, stream);
}

hipError_t launch_trace_tri(const LaunchParams& p, hipStream_t stream)
{
  // Triangle4v <-> robust traversal, Triangle4 <-> fast traversal (bvh_intersector1_bvh8.cpp:27-29)
  return dev::launch_pluecker_moeller<dev::TriLeaf>(p, stream, p.accel.kind == ACCEL_TRI_PLUECKER);
}

} // namespace rtamd
