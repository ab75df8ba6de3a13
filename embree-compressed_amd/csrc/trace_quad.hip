// Quad leaves of the quantized BVH8: Quad4v with Pluecker (robust) or Moeller-Trumbore (fast) arithmetic.
// 64-byte records (QuadRecord, accel.h) fetched as four dwordx4; every group of 4 records from the leaf start is one block of the
// reference's AVX form, which tests the 4 quads as ONE 8-wide block of triangles:
//   lanes 0-3 = triangle A (v0, v1, v3) of quads 0-3, lanes 4-7 = triangle B (v2, v1, v3) of quads 0-3
//   (quad_intersector_pluecker.h:264-299, quad_intersector_moeller.h:251-290), all 8 tested against the tfar at block entry,
//   one select_min over the 8 lanes (Intersect1EpilogM<8,8,filter>): the lowest lane wins ties, so A beats B at equal t.
// Hits on a B triangle report the quad's parametrisation and the negated triangle normal; the u / v mapping differs per variant:
//   Pluecker  u = 1 - v_tri, v = 1 - u_tri after the division (QuadHitPlueckerM::finalize, the AVX branch, pluecker.h:45-66)
//   Moeller   U' = absDen - V, V' = absDen - U before the division by absDen (quad_intersector_moeller.h:268-282)
#include "trace_leaf.hip.h"
#include "trace_quad.hip.h"
#include "trace_service.hip.h"

namespace rtamd {

hipError_t launch_service_quad(const ServiceParams& s, hipStream_t stream)
{
  if (s.base.accel.kind == ACCEL_QUAD_PLUECKER) return dev::launch_service_kernel<dev::QuadLeaf<true>, true>(s, stream);
  return dev::launch_service_kernel<dev::QuadLeaf<false>, false>(s, stream);
}

hipError_t launch_trace_quad(const LaunchParams& p, hipStream_t stream)
{
  // Quad4v: Pluecker <-> robust traversal, Moeller <-> fast traversal (bvh_intersector1_bvh8.cpp:37-39)
  return dev::launch_pluecker_moeller<dev::QuadLeaf>(p, stream, p.accel.kind == ACCEL_QUAD_PLUECKER);
}

} // namespace rtamd
