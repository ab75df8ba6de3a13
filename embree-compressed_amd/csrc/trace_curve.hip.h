// What the ribbon leaves share (trace_curve.hip, trace_curve_mb.hip): the Bezier basis, the ray space of the control points, the corners
// of a ribbon quad, the quad test and the hit of the winning segment - the arithmetic described in the header of trace_curve.hip.
// Stateless __forceinline__ helpers, under the rule of trace_leaf.hip.h: a leaf uses a helper only where its kernels stay the same
// instructions as with the helper in its own unit (tools/kernel_metadata.py --digest).
#pragma once
#include "trace_leaf.hip.h"
#include "trace_line.hip.h"

namespace rtamd {
namespace dev {

// One end of a ribbon quad in ray space: the lower (p + w n) and upper (p - w n) corner; both have the curve point's z
struct RibbonEnd
{
  float lx, ly, ux, uy, z, w;
};

// BezierBasis::eval / derivative at u (bezier_curve.h:27-49), the products in the reference's order
__device__ __forceinline__ void bezier_eval(float u, float& b0, float& b1, float& b2, float& b3)
{
  const float t1 = u, t0 = 1.0f - t1;
  b0 = t0 * t0 * t0;
  b1 = 3.0f * t1 * (t0 * t0);
  b2 = 3.0f * (t1 * t1) * t0;
  b3 = t1 * t1 * t1;
}
__device__ __forceinline__ void bezier_derivative(float u, float& d0, float& d1, float& d2, float& d3)
{
  const float t1 = u, t0 = 1.0f - t1;
  d0 = 3.0f * -(t0 * t0);
  d1 = 3.0f * madd(-2.0f, t0 * t1, t0 * t0);
  d2 = 3.0f * msub(+2.0f, t0 * t1, t1 * t1);
  d3 = 3.0f * (t1 * t1);
}
__device__ __forceinline__ float bezier_combine(float c0, float c1, float c2, float c3, float a, float b, float c, float d)
{
  return madd(c0, a, madd(c1, b, madd(c2, c, c3 * d)));
}

// xfmVector(ray_space, v - org) with w = radius kept; the z row is N * s (ray_space.vz *= depth_scale)
__device__ __forceinline__ float4 to_ray_space(const RayState& r, const LineSpace& S, const float4 V)
{
  const float ax = V.x - r.ox, ay = V.y - r.oy, az = V.z - r.oz;
  return make_float4(dot3(ax, ay, az, S.dxx, S.dxy, S.dxz), dot3(ax, ay, az, S.dyx, S.dyy, S.dyz), dot3(ax, ay, az, S.nx * S.s, S.ny * S.s, S.nz * S.s), V.w);
}

// -DCURVE_BASIS_TABLE: the basis from a table in device memory, [N][j] = BezierBasis::eval and derivative at float(j) / float(N), as the
// reference's bezier_basis0 / bezier_basis1 - built on the host with the same float32 arithmetic and uploaded before the first launch.
// A build for the measurement in docs/experiments.md only (one device, the upload synchronises); the results are the same bits.
#ifdef CURVE_BASIS_TABLE
__device__ float4 curve_basis_table[17][17][2];
#endif

// The corners of the ribbon at curve parameter float(j) / float(N) of the ray-space curve w0 .. w3
__device__ __forceinline__ RibbonEnd ribbon_end(const float4 w0, const float4 w1, const float4 w2, const float4 w3, uint32_t j, uint32_t N)
{
  float c0, c1, c2, c3, d0, d1, d2, d3;
#ifdef CURVE_BASIS_TABLE
  const float4 tc = curve_basis_table[min(N, 16u)][min(j, 16u)][0], td = curve_basis_table[min(N, 16u)][min(j, 16u)][1];
  c0 = tc.x; c1 = tc.y; c2 = tc.z; c3 = tc.w;
  d0 = td.x; d1 = td.y; d2 = td.z; d3 = td.w;
#else
  const float u = (float)j / (float)N;
  bezier_eval(u, c0, c1, c2, c3);
  bezier_derivative(u, d0, d1, d2, d3);
#endif
  const float px = bezier_combine(c0, c1, c2, c3, w0.x, w1.x, w2.x, w3.x);
  const float py = bezier_combine(c0, c1, c2, c3, w0.y, w1.y, w2.y, w3.y);
  const float dx = bezier_combine(d0, d1, d2, d3, w0.x, w1.x, w2.x, w3.x);
  const float dy = bezier_combine(d0, d1, d2, d3, w0.y, w1.y, w2.y, w3.y);
  RibbonEnd e;
  e.z = bezier_combine(c0, c1, c2, c3, w0.z, w1.z, w2.z, w3.z);
  e.w = bezier_combine(c0, c1, c2, c3, w0.w, w1.w, w2.w, w3.w);
  // n = (dy, -dx, 0), nn = n * rsqrt(dot(n, n)) with dot = madd(n.x, n.x, madd(n.y, n.y, n.z * n.z))
  const float nx = dy, ny = -dx;
  const float rs = 1.0f / sqrtf(madd(nx, nx, madd(ny, ny, 0.0f)));
  const float nnx = nx * rs, nny = ny * rs;
  e.lx = madd(e.w, nnx, px); e.ly = madd(e.w, nny, py);   // lp = madd(p.w, nn, p)
  e.ux = madd(-e.w, nnx, px); e.uy = madd(-e.w, nny, py); // up = nmadd(p.w, nn, p)
  return e;
}

// intersect_quad_backface_culling on the quad (lp0, lp1, up1, up0) = (va, vb, vc, vd) with the ray at the origin along +z, then the
// self-intersection test of intersect_ribbon.  U, V: the quad's own coordinates (the caller turns them into the hit's u, v).
__device__ __forceinline__ bool ribbon_quad_test(const RibbonEnd& a, const RibbonEnd& b, float tnear, float tfar, float s, float& t, float& U, float& V)
{
  // edb = vb - vd, WW = dot(cross(vd, edb), D)
  const float edbx = b.lx - a.ux, edby = b.ly - a.uy;
  const float WW = msub(a.ux, edby, a.uy * edbx);
  const bool first = WW <= 0.0f; // triangle (va, vb, vd), else (vc, vd, vb)
  const float v0x = first ? a.lx : b.ux, v0y = first ? a.ly : b.uy, v0z = first ? a.z : b.z;
  const float v1x = first ? b.lx : a.ux, v1y = first ? b.ly : a.uy, v1z = first ? b.z : a.z;
  const float v2x = first ? a.ux : b.lx, v2y = first ? a.uy : b.ly, v2z = first ? a.z : b.z;
  const float e0x = v2x - v0x, e0y = v2y - v0y, e0z = v2z - v0z;
  const float e1x = v0x - v1x, e1y = v0y - v1y, e1z = v0z - v1z;
  const float Ue = msub(v0x, e0y, v0y * e0x); // dot(cross(v0, e0), D)
  const float Ve = msub(v1x, e1y, v1y * e1x); // dot(cross(v1, e1), D)
  const float m = Ue > Ve ? Ue : Ve;          // max(U, V) as _mm_max_ps: NaN in either operand gives the second
  bool valid = m <= 0.0f;
  // Ng = cross(e1, e0), den = dot(Ng, D)
  const float ngx = msub(e1y, e0z, e1z * e0y), ngy = msub(e1z, e0x, e1x * e0z), den = msub(e1x, e0y, e1y * e0x);
  const float absDen = fabsf(den);
  const uint32_t sgnDen = __float_as_uint(den) & 0x80000000u;
  const float T = dot3(v0x, v0y, v0z, ngx, ngy, den);
  const float Ts = xorf(T, sgnDen);
  valid &= (absDen * tnear < Ts) & (Ts <= absDen * tfar) & (den != 0.0f);
  const float rcpDen = 1.0f / den;
  t = T * rcpDen;
  const float u = Ue * rcpDen, v = Ve * rcpDen;
  U = first ? u : 1.0f - u;
  V = first ? v : 1.0f - v;
  // ignore self intersections: r = lerp(p0.w, p1.w, u) = madd(1 - u, p0.w, u * p1.w)
  const float rad = madd(1.0f - U, a.w, U * b.w);
  valid &= t > tnear + 2.0f * rad * s;
  return valid;
}

// RibbonHit::finalize and Ng of the winning segment: lane k of the pass that starts at segment `base`
__device__ __forceinline__ void ribbon_hit(TriHit& h, float t, float U, float V, uint32_t k, uint32_t base, uint32_t N, const float4 V0, const float4 V1, const float4 V2,
                                           const float4 V3)
{
  h.t = t;
  h.u = (((float)k + U) + (float)base) * (1.0f / (float)N);
  h.v = madd(2.0f, V, -1.0f);
  float d0, d1, d2, d3;
  bezier_derivative(h.u, d0, d1, d2, d3);
  h.ngx = bezier_combine(d0, d1, d2, d3, V0.x, V1.x, V2.x, V3.x);
  h.ngy = bezier_combine(d0, d1, d2, d3, V0.y, V1.y, V2.y, V3.y);
  h.ngz = bezier_combine(d0, d1, d2, d3, V0.z, V1.z, V2.z, V3.z);
}

// The static ribbon leaf (described in trace_curve.hip, which holds its launcher): here so that the hair form of the two-level kernel
// (trace_instance_hair.hip) runs the same leaf below an instance.
struct CurveLeaf : LeafTraits
{
  // Three waves per SIMD, the bound of the line leaves (at most 168 VGPRs): profiles/curve_kernel_resources.txt
  static constexpr int MIN_WAVES = 3;

  // Child-parallel form (trace_loop.hip.h): one record per pass - lane k of the octet tests segment base + k of the curve, every lane
  // against the tfar at pass entry; ONE 8-lane minimum, the lowest lane with that t wins and writes the hit into the row (words 0..7 =
  // t, Ng, u, v, geomID, primID; word 9 = 1).  A curve with N > 8 takes a second pass, which sees the first one's tfar.  Row word 10 is
  // the ray's index.  The loops are wave-uniform (every octet runs as many passes as the longest one; the others are masked).
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const CurveRecord* __restrict__ recs = (const CurveRecord*)P.accel.blobs;
    const uint32_t k = lid & 7u;
    const RayState r = row_ray(x);
    const LineSpace S = line_space(r);
    const uint32_t ref = __float_as_uint(x[8]);
    uint32_t first, cnt;
    leaf_range(ref, first, cnt);
    cnt = valid ? cnt : 0u;
    float tfar = r.tfar;
    for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i++) {
      const bool present = i < cnt;
      const float4* lp = (const float4*)(recs + first + (present ? i : 0u));
      const float4 V0 = lp[0], V1 = lp[1], V2 = lp[2], V3 = lp[3];
      const uint4 ids = *(const uint4*)(lp + 4); // geomID, primID, N, pad
      uint32_t N = present ? ids.z : 0u;
      const float4 w0 = to_ray_space(r, S, V0), w1 = to_ray_space(r, S, V1), w2 = to_ray_space(r, S, V2), w3 = to_ray_space(r, S, V3);
      for (uint32_t base = 0; __ballot(base < N) != 0ull; base += 8u) {
        const uint32_t j = base + k;
        const bool seg = j < N;
        if (COUNT && seg) wc.prims++;
        const RibbonEnd a = ribbon_end(w0, w1, w2, w3, j, N), b = ribbon_end(w0, w1, w2, w3, j + 1u, N);
        float t, U, V;
        bool ok = ribbon_quad_test(a, b, r.tnear, tfar, S.s, t, U, V) && seg;
        if (ok && P.exclOffsets) ok = !candidate_excluded(P, __float_as_uint(x[10]), ids.x, ids.y, t);
        const uint32_t m8 = octet_ballot(ok, lid);
        if (OCCLUDED) { // Occluded1EpilogMU: any valid segment
          if (m8 != 0u) {
            if (k == 0u) x[9] = __uint_as_float(1u);
            cnt = 0u;
            N = 0u;
          }
          continue;
        }
        const float tmin = octet_min8(ok ? t : RT_INF);
        const uint32_t w = octet_ballot(ok && t == tmin, lid);
        if (w != 0u && k == (uint32_t)__ffs(w) - 1u) { // select_min, the lowest lane wins an equal t (Intersect1EpilogMU, intersector_epilog.h:455-509)
          TriHit h;
          ribbon_hit(h, t, U, V, k, base, N, V0, V1, V2, V3);
          row_write_hit(x, h, ids.x, ids.y);
        }
        tfar = w != 0u ? tmin : tfar;
      }
    }
  }

  // Lane-per-ray form: the records one after the other, the five words of a record requested before the first use; the segments in
  // passes of 8 against the tfar at pass entry, visited in order and replacing the best one only with a smaller t, so the lowest
  // segment wins ties.  The end of a segment is carried over as the start of the next (the same bits, see the header).  The world
  // control points are read again for the Ng of a pass's winner: sixteen registers less across the segment loop.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ bool intersect(const LaunchParams& P, uint32_t ref, RayState& r, WorkCounters& wc, uint32_t rayIdx)
  {
    const CurveRecord* __restrict__ recs = (const CurveRecord*)P.accel.blobs;
    const LineSpace S = line_space(r);
    uint32_t first, count;
    leaf_range(ref, first, count);
    for (uint32_t i = 0; i < count; i++) {
      const float4* lp = (const float4*)(recs + first + i);
      float4 w0 = lp[0], w1 = lp[1], w2 = lp[2], w3 = lp[3];
      const uint4 ids = *(const uint4*)(lp + 4); // geomID, primID, N, pad
      const uint32_t N = ids.z;
      w0 = to_ray_space(r, S, w0); w1 = to_ray_space(r, S, w1); w2 = to_ray_space(r, S, w2); w3 = to_ray_space(r, S, w3);
      RibbonEnd a = ribbon_end(w0, w1, w2, w3, 0u, N);
      for (uint32_t base = 0; base < N; base += 8u) {
        const float tfarPass = r.tfar; // all segments of a pass see the tfar at pass entry
        const uint32_t nb = min(8u, N - base);
        bool found = false;
        float bt = RT_INF, bU = 0.f, bV = 0.f;
        uint32_t bk = 0;
        for (uint32_t k = 0; k < nb; k++) {
          if (COUNT) wc.prims++;
          const RibbonEnd b = ribbon_end(w0, w1, w2, w3, base + k + 1u, N);
          float t, U, V;
          bool ok = ribbon_quad_test(a, b, r.tnear, tfarPass, S.s, t, U, V);
          a = b;
          if (ok && P.exclOffsets) ok = !candidate_excluded(P, rayIdx, ids.x, ids.y, t);
          if (ok) {
            if (OCCLUDED) return true; // Occluded1EpilogMU: any valid segment
            if (!found || t < bt) { // select_min over the pass, lowest segment wins ties
              bt = t; bU = U; bV = V; bk = k;
              found = true;
            }
          }
        }
        if (found) { // Intersect1EpilogMU, intersector_epilog.h:455-509
          TriHit best;
          ribbon_hit(best, bt, bU, bV, bk, base, N, lp[0], lp[1], lp[2], lp[3]);
          commit_hit(r, best, ids.x, ids.y);
        }
      }
    }
    return false;
  }
};

} // namespace dev
} // namespace rtamd
