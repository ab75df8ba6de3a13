// Fork path, subdiv_accel=bvh4.compressed.full: the trace and service kernels of CbvhLeaf<MODE_FULL> (trace_cbvh.hip.h), a translation unit of their own.
#include "trace_cbvh.hip.h"

namespace rtamd {

hipError_t launch_trace_cbvh_full(const LaunchParams& p, hipStream_t stream) { return dev::launch_cbvh<dev::MODE_FULL>(p, stream); }
hipError_t launch_service_cbvh_full(const ServiceParams& s, hipStream_t stream) { return dev::launch_service_cbvh<dev::MODE_FULL>(s, stream); }

} // namespace rtamd
