// world2local(time) of an instance with time steps: ONE definition, compiled as the same text by the host (rtcore_api.cpp
// rtcamdGetGeometryWorld2Local, rt_scene.cpp) and by the kernel (trace_instance.hip, XFMB).  It uses no other helper of the project.
// The reference computes world2local = rcp(lerp(local2world[itime], local2world[itime + 1], ftime)) per ray (scene_instance.h:58-63,
// instance_intersector.cpp:51-56; lerp: math.h madd(1 - f, a, f * b); rcp of an AffineSpace3f: affinespace.h:91,145; inverse of a
// LinearSpace3f = adjoint / det: linearspace3.h:57-63).  Deviation: the reference multiplies by its approximate SSE rcp(det); this
// is the IEEE quotient 1.0f / det, so parity with reference arithmetic is a tolerance, not bit equality.
// Every fused operation is written as fmaf (the build is -ffp-contract=off on both sides), every other operation is one IEEE fp32
// operation: host and device agree in every bit.
// Matrices are 12 floats, the columns vx, vy, vz, p of an AffineSpace3f (InstanceRecord::world2local, InstanceStep::local2world).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTAMD_XFM_FN __host__ __device__ inline
#else
#define RTAMD_XFM_FN inline
#endif

namespace rtamd {

// time -> (itime, ftime) over S = steps - 1 segments, as accel.h / trace_mb.hip.h time_segment: ts = time * S,
// itime = clamp(floor(ts), 0, S - 1), ftime = ts - itime
RTAMD_XFM_FN uint32_t instance_time_segment(float time, uint32_t numSegments, float& f)
{
  const float S = (float)numSegments;
  const float ts = time * S;
  const float itimef = fminf(fmaxf(floorf(ts), 0.0f), S - 1.0f);
  f = ts - itimef;
  return (uint32_t)(int)itimef;
}

// M = lerp(A, B, f): madd(1 - f, A[k], f * B[k]) for the 12 entries
RTAMD_XFM_FN void instance_lerp(const float* A, const float* B, float f, float* M)
{
  const float g = 1.0f - f;
  for (int k = 0; k < 12; k++) M[k] = fmaf(g, A[k], f * B[k]);
}

// out = inverse(M) for the affine map M.  false: det == 0, or a result that is not finite - `out` is then not to be used.
RTAMD_XFM_FN bool instance_invert(const float* M, float* out)
{
  const float vxx = M[0], vxy = M[1], vxz = M[2], vyx = M[3], vyy = M[4], vyz = M[5], vzx = M[6], vzy = M[7], vzz = M[8];
  const float px = M[9], py = M[10], pz = M[11];
  // cross(a, b) = (msub(a.y, b.z, a.z * b.y), msub(a.z, b.x, a.x * b.z), msub(a.x, b.y, a.y * b.x))
  const float c0x = fmaf(vyy, vzz, -(vyz * vzy)), c0y = fmaf(vyz, vzx, -(vyx * vzz)), c0z = fmaf(vyx, vzy, -(vyy * vzx)); // cross(vy, vz)
  const float c1x = fmaf(vzy, vxz, -(vzz * vxy)), c1y = fmaf(vzz, vxx, -(vzx * vxz)), c1z = fmaf(vzx, vxy, -(vzy * vxx)); // cross(vz, vx)
  const float c2x = fmaf(vxy, vyz, -(vxz * vyy)), c2y = fmaf(vxz, vyx, -(vxx * vyz)), c2z = fmaf(vxx, vyy, -(vxy * vyx)); // cross(vx, vy)
  const float det = fmaf(vxx, c0x, fmaf(vxy, c0y, vxz * c0z));
  const float r = 1.0f / det;
  out[0] = c0x * r; out[1] = c1x * r; out[2] = c2x * r; // vx' = (c0.x, c1.x, c2.x) * r
  out[3] = c0y * r; out[4] = c1y * r; out[5] = c2y * r; // vy'
  out[6] = c0z * r; out[7] = c1z * r; out[8] = c2z * r; // vz'
  // p' = -xfmVector(inverse linear part, p) = -(madd(p.x, vx', madd(p.y, vy', p.z * vz')))
  out[9] = -fmaf(px, out[0], fmaf(py, out[3], pz * out[6]));
  out[10] = -fmaf(px, out[1], fmaf(py, out[4], pz * out[7]));
  out[11] = -fmaf(px, out[2], fmaf(py, out[5], pz * out[8]));
  bool ok = det != 0.0f;
  for (int k = 0; k < 12; k++) ok = ok && (fabsf(out[k]) < INFINITY); // finite: neither NaN nor an infinity
  return ok;
}

// world2local at ftime `f` between the steps A and B (local2world each): inverse(lerp(A, B, f))
RTAMD_XFM_FN bool instance_world2local(const float* A, const float* B, float f, float* out)
{
  float M[12];
  instance_lerp(A, B, f, M);
  return instance_invert(M, out);
}

} // namespace rtamd
