// Eager subdivision path on gfx950: the trace and service kernels of GridCellLeaf (trace_grid.hip.h), a translation unit of their own.
#include "trace_grid.hip.h"

namespace rtamd {

hipError_t launch_service_grid(const ServiceParams& s, hipStream_t stream) { return dev::launch_service_kernel<dev::GridCellLeaf, true>(s, stream); }

hipError_t launch_trace_grid(const LaunchParams& p, hipStream_t stream)
{
  if (p.poolKernel) return dev::launch_leaf_pool<dev::GridCellLeaf, true>(p, stream);
  return dev::launch_leaf<dev::GridCellLeaf, true>(p, stream);
}

} // namespace rtamd
