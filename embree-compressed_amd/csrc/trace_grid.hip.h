// Eager subdivision path on gfx950: grid-cell leaves of the quantized BVH8.
//   GridCellLeaf   one 3x3-vertex cell = 8 Pluecker triangles with patch-uv mapping
//                  (kernels/geometry/grid_soa_intersector1.h:44-117, Gather3x3 grid_soa.h:198-245, MapUV :137-156,
//                   decodeUV :248-257, Intersect1EpilogMU intersector_epilog.h:460-530)
// The fork path (cBVH blobs) is trace_cbvh.hip.h.  A header so that trace_instance_subdiv.hip can run the same leaf below an instance;
// the kernels of the eager accel itself are instantiated by trace_grid.hip.
#pragma once
#include "trace_leaf.hip.h"
#include "trace_service.hip.h"

namespace rtamd {
namespace dev {

struct RelV
{
  float x, y, z;
};

// Pluecker on vertices already relative to the ray origin; returns un-mapped barycentrics.
__device__ __forceinline__ bool pluecker_rel(const RayState& r, const RelV a, const RelV b, const RelV c, float tfarBlock, TriHit& h)
{
  const float e0x = c.x - a.x, e0y = c.y - a.y, e0z = c.z - a.z;
  const float e1x = a.x - b.x, e1y = a.y - b.y, e1z = a.z - b.z;
  const float e2x = b.x - c.x, e2y = b.y - c.y, e2z = b.z - c.z;
  float sx = c.x + a.x, sy = c.y + a.y, sz = c.z + a.z;
  const float U = dot3(msub(e0y, sz, e0z * sy), msub(e0z, sx, e0x * sz), msub(e0x, sy, e0y * sx), r.dx, r.dy, r.dz);
  sx = a.x + b.x; sy = a.y + b.y; sz = a.z + b.z;
  const float V = dot3(msub(e1y, sz, e1z * sy), msub(e1z, sx, e1x * sz), msub(e1x, sy, e1y * sx), r.dx, r.dy, r.dz);
  sx = b.x + c.x; sy = b.y + c.y; sz = b.z + c.z;
  const float W = dot3(msub(e2y, sz, e2z * sy), msub(e2z, sx, e2x * sz), msub(e2x, sy, e2y * sx), r.dx, r.dy, r.dz);
  const float minUVW = fminf(fminf(U, V), W);
  const float maxUVW = fmaxf(fmaxf(U, V), W);
  if (!((minUVW >= 0.0f) | (maxUVW <= 0.0f))) return false;
  const float ab_x = e0z * e1y, ab_y = e0x * e1z, ab_z = e0y * e1x;
  const float bc_x = e1z * e2y, bc_y = e1x * e2z, bc_z = e1y * e2x;
  const float cab_x = msub(e0y, e1z, ab_x), cab_y = msub(e0z, e1x, ab_y), cab_z = msub(e0x, e1y, ab_z);
  const float cbc_x = msub(e1y, e2z, bc_x), cbc_y = msub(e1z, e2x, bc_y), cbc_z = msub(e1x, e2y, bc_z);
  const float ngx = fabsf(ab_x) < fabsf(bc_x) ? cab_x : cbc_x;
  const float ngy = fabsf(ab_y) < fabsf(bc_y) ? cab_y : cbc_y;
  const float ngz = fabsf(ab_z) < fabsf(bc_z) ? cab_z : cbc_z;
  const float dn = dot3(ngx, ngy, ngz, r.dx, r.dy, r.dz);
  const float den = dn + dn;
  const float absDen = fabsf(den);
  const uint32_t sgnDen = __float_as_uint(den) & 0x80000000u;
  const float tn = dot3(a.x, a.y, a.z, ngx, ngy, ngz);
  const float T = tn + tn;
  const float Ts = xorf(T, sgnDen);
  if (!(absDen * r.tnear < Ts)) return false;
  if (!(Ts <= absDen * tfarBlock)) return false;
  if (!(den != 0.0f)) return false;
  const float rcpDen = 1.0f / den;
  h.t = T * rcpDen;
  const float UVW = U + V + W;
  const float rcpUVW = fabsf(UVW) < 1e-18f ? 0.0f : 1.0f / UVW;
  h.u = U * rcpUVW;
  h.v = V * rcpUVW;
  h.ngx = ngx; h.ngy = ngy; h.ngz = ngz;
  return true;
}

struct GridCellLeaf : LeafTraits
{
  static constexpr bool OCTET_ONLY = true; // lane kernel: cells are always tested 8 lanes per ray (intersect() below serves the ray-pool kernel)

  // Child-parallel form (trace_loop.hip.h): lane 8g+k tests triangle k of the cell of the ray in exchange row `x`
  // (words 0..7 = org, tnear, dir, tfar; word 8 = leaf ref).  Same vertex differences, same Pluecker test against the tfar
  // at cell entry, same winner (minimum t, lowest triangle on ties, select_min vfloat4_sse2.h:654-659) as intersect()
  // below; the winning lane maps uv and writes the hit into the row (words 0..7 = t, Ng, u, v, geomID, primID; word 9 = 1).
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const uint32_t k = lid & 7u;
    const RayState r = row_ray(x);
    const uint32_t idx = __float_as_uint(x[8]) & 0x7FFFFFFFu;
    const float* gp = (const float*)(P.accel.blobs + (size_t)idx * sizeof(GridCell));
    // Gather3x3 lane -> vertex indices (grid_soa.h:218-223), one nibble per triangle
    const uint32_t i0 = (0x74634130u >> (4u * k)) & 15u, i1 = (0x55442211u >> (4u * k)) & 15u, i2 = (0x87765443u >> (4u * k)) & 15u;
    const RelV a = RelV{gp[i0] - r.ox, gp[9u + i0] - r.oy, gp[18u + i0] - r.oz};
    const RelV b = RelV{gp[i1] - r.ox, gp[9u + i1] - r.oy, gp[18u + i1] - r.oz};
    const RelV c = RelV{gp[i2] - r.ox, gp[9u + i2] - r.oy, gp[18u + i2] - r.oz};
    TriHit h;
    h.t = RT_INF;
    bool ok = pluecker_rel(r, a, b, c, r.tfar, h) && valid;
    if (ok && P.exclOffsets) ok = !candidate_excluded(P, __float_as_uint(x[10]), __float_as_uint(gp[36]), __float_as_uint(gp[37]), h.t);
    // (octet_ballot, row_write_hit and commit_hit change the instruction schedule of this leaf's kernels: written out, here and in intersect())
    const uint32_t mask8 = (uint32_t)(__ballot(ok) >> (lid & 56u)) & 0xffu;
    if (COUNT && valid && k == 0u) {
      wc.prims++;
      wc.inner += (OCCLUDED && mask8) ? (unsigned long long)__ffs(mask8) : 8ull; // the lane-per-ray any-hit loop stops at the first valid triangle
    }
    if (OCCLUDED) {
      if (valid && k == 0u && mask8 != 0u) x[9] = __uint_as_float(1u);
      return;
    }
    const float tmin = octet_min8(ok ? h.t : RT_INF);
    const uint32_t win8 = (uint32_t)(__ballot(ok && h.t == tmin) >> (lid & 56u)) & 0xffu;
    if (ok && win8 != 0u && k == (uint32_t)__ffs(win8) - 1u) {
      // MapUV (grid_soa.h:148-155): uv = u*uv1 + v*uv2 + (1-u-v)*uv0 on the 16-bit decoded vertex uvs
      const uint32_t w0 = __float_as_uint(gp[27u + i0]), w1 = __float_as_uint(gp[27u + i1]), w2 = __float_as_uint(gp[27u + i2]);
      const float s = 8.0f / 0x10000;
      const float u0 = (float)(w0 & 0xffffu) * s, v0 = (float)(w0 >> 16) * s;
      const float u1 = (float)(w1 & 0xffffu) * s, v1 = (float)(w1 >> 16) * s;
      const float u2 = (float)(w2 & 0xffffu) * s, v2 = (float)(w2 >> 16) * s;
      const float bu = h.u, bv = h.v;
      const float bw = (1.0f - bu) - bv;
      x[0] = h.t; x[1] = h.ngx; x[2] = h.ngy; x[3] = h.ngz;
      x[4] = (bu * u1 + bv * u2) + bw * u0;
      x[5] = (bu * v1 + bv * v2) + bw * v0;
      x[6] = gp[36];
      x[7] = gp[37];
      x[9] = __uint_as_float(1u);
    }
  }

  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ bool intersect(const LaunchParams& P, uint32_t ref, RayState& r, WorkCounters& wc, uint32_t rayIdx)
  {
    const uint32_t idx = ref & 0x7FFFFFFFu;
    const float4* gp = (const float4*)(P.accel.blobs + (size_t)idx * sizeof(GridCell));
    float f[40];
#pragma unroll
    for (int k = 0; k < 10; k++) {
      const float4 q = gp[k];
      f[4 * k] = q.x; f[4 * k + 1] = q.y; f[4 * k + 2] = q.z; f[4 * k + 3] = q.w;
    }
    if (COUNT) wc.prims++;
    // f[0..8] px, f[9..17] py, f[18..26] pz, f[27..35] packed uv, f[36] geomID, f[37] primID
    RelV p[9];
#pragma unroll
    for (int k = 0; k < 9; k++) p[k] = RelV{f[k] - r.ox, f[9 + k] - r.oy, f[18 + k] - r.oz};
    // Gather3x3 lane -> (v0,v1,v2) vertex indices r*3+c (grid_soa.h:218-223)
    constexpr int T0[8] = {0, 3, 1, 4, 3, 6, 4, 7};
    constexpr int T1[8] = {1, 1, 2, 2, 4, 4, 5, 5};
    constexpr int T2[8] = {3, 4, 4, 5, 6, 7, 7, 8};
    const float tfarBlock = r.tfar;
    bool found = false;
    TriHit best;
    best.t = RT_INF;
    int bestLane = 0;
#pragma unroll
    for (int l = 0; l < 8; l++) {
      if (COUNT) wc.inner++;
      TriHit h;
      if (pluecker_rel(r, p[T0[l]], p[T1[l]], p[T2[l]], tfarBlock, h)) {
        if (P.exclOffsets && candidate_excluded(P, rayIdx, __float_as_uint(f[36]), __float_as_uint(f[37]), h.t)) continue;
        if (OCCLUDED) return true;
        if (!found || h.t < best.t) { // select_min: lowest lane among equal minima
          best = h;
          bestLane = l;
          found = true;
        }
      }
    }
    if (found) {
      // MapUV (grid_soa.h:148-155): uv = u*uv1 + v*uv2 + (1-u-v)*uv0 on the 16-bit decoded vertex uvs
      uint32_t w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
      for (int l = 0; l < 8; l++)
        if (l == bestLane) {
          w0 = __float_as_uint(f[27 + T0[l]]);
          w1 = __float_as_uint(f[27 + T1[l]]);
          w2 = __float_as_uint(f[27 + T2[l]]);
        }
      const float s = 8.0f / 0x10000;
      const float u0 = (float)(w0 & 0xffffu) * s, v0 = (float)(w0 >> 16) * s;
      const float u1 = (float)(w1 & 0xffffu) * s, v1 = (float)(w1 >> 16) * s;
      const float u2 = (float)(w2 & 0xffffu) * s, v2 = (float)(w2 >> 16) * s;
      const float bu = best.u, bv = best.v;
      const float bw = (1.0f - bu) - bv;
      r.u = (bu * u1 + bv * u2) + bw * u0;
      r.v = (bu * v1 + bv * v2) + bw * v0;
      r.tfar = best.t;
      r.ngx = best.ngx; r.ngy = best.ngy; r.ngz = best.ngz;
      r.geomID = __float_as_uint(f[36]);
      r.primID = __float_as_uint(f[37]);
      r.hit = 1u;
    }
    return false;
  }
};

} // namespace dev
} // namespace rtamd
