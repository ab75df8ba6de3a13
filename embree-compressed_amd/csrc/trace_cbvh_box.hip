// Fork path, subdiv_accel=bvh4.compressed.box: the trace and service kernels of CbvhLeaf<MODE_BOX> (trace_cbvh.hip.h), a translation unit of their own.
#include "trace_cbvh.hip.h"

namespace rtamd {

hipError_t launch_trace_cbvh_box(const LaunchParams& p, hipStream_t stream) { return dev::launch_cbvh<dev::MODE_BOX>(p, stream); }
hipError_t launch_service_cbvh_box(const ServiceParams& s, hipStream_t stream) { return dev::launch_service_cbvh<dev::MODE_BOX>(s, stream); }

} // namespace rtamd
