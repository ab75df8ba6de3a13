// What the line segment leaves share (trace_line.hip, trace_line_mb.hip): the ray's own space and the test of one segment
// (LineIntersector1<4>::intersect, kernels/geometry/line_intersector.h:53-98).  Stateless __forceinline__ helpers, under the rule of
// trace_leaf.hip.h: a leaf uses a helper only where its kernels stay the same instructions as with the helper in its own unit
// (tools/kernel_metadata.py --digest).
#pragma once
#include "trace_leaf.hip.h"

namespace rtamd {
namespace dev {

// ray_space = frame(s * dir).transposed() (common/math/linearspace3.h:126-133) as its three rows, and the depth scale s
struct LineSpace
{
  float dxx, dxy, dxz; // dx
  float dyx, dyy, dyz; // dy
  float nx, ny, nz;    // N = s * dir
  float s;
};

// Vec3fa dot (vec3fa.h:289: dpps), normalize = a * rsqrt(dot(a, a)), cross = msub(a0, b0, a1 * b1) shuffled (vec3fa.h:298-305);
// rsqrt is 1 / sqrt, both correctly rounded
__device__ __forceinline__ float dot3_plain(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

__device__ __forceinline__ LineSpace line_space(const RayState& r)
{
  LineSpace S;
  S.s = 1.0f / sqrtf(dot3_plain(r.dx, r.dy, r.dz, r.dx, r.dy, r.dz));
  S.nx = S.s * r.dx; S.ny = S.s * r.dy; S.nz = S.s * r.dz;
  // dx0 = (0, N.z, -N.y), dx1 = (-N.z, 0, N.x): the longer one, normalized
  const float l0 = dot3_plain(0.0f, S.nz, -S.ny, 0.0f, S.nz, -S.ny);
  const float l1 = dot3_plain(-S.nz, 0.0f, S.nx, -S.nz, 0.0f, S.nx);
  const bool first = l0 > l1;
  const float ax = first ? 0.0f : -S.nz, ay = first ? S.nz : 0.0f, az = first ? -S.ny : S.nx;
  const float ra = 1.0f / sqrtf(dot3_plain(ax, ay, az, ax, ay, az));
  S.dxx = ax * ra; S.dxy = ay * ra; S.dxz = az * ra;
  // dy = normalize(cross(N, dx))
  const float cx = msub(S.ny, S.dxz, S.nz * S.dxy), cy = msub(S.nz, S.dxx, S.nx * S.dxz), cz = msub(S.nx, S.dxy, S.ny * S.dxx);
  const float rc = 1.0f / sqrtf(dot3_plain(cx, cy, cz, cx, cy, cz));
  S.dyx = cx * rc; S.dyy = cy * rc; S.dyz = cz * rc;
  return S;
}

// LineIntersector1::intersect on one record: V0 = (v0.xyz, r0), V1 = (v1.xyz, r1).  xfmVector(ray_space, a) = madd(a.x, vx, madd(a.y, vy,
// a.z * vz)) with the transposed frame's columns, i.e. per component dot3(a, row) in the order of vec3.h:193.
__device__ __forceinline__ bool line_test(const RayState& r, const LineSpace& S, const float4 V0, const float4 V1, float tfarBlock, TriHit& h)
{
  const float a0x = V0.x - r.ox, a0y = V0.y - r.oy, a0z = V0.z - r.oz;
  const float a1x = V1.x - r.ox, a1y = V1.y - r.oy, a1z = V1.z - r.oz;
  const float p0x = dot3(a0x, a0y, a0z, S.dxx, S.dxy, S.dxz), p0y = dot3(a0x, a0y, a0z, S.dyx, S.dyy, S.dyz), p0z = dot3(a0x, a0y, a0z, S.nx, S.ny, S.nz);
  const float p1x = dot3(a1x, a1y, a1z, S.dxx, S.dxy, S.dxz), p1y = dot3(a1x, a1y, a1z, S.dyx, S.dyy, S.dyz), p1z = dot3(a1x, a1y, a1z, S.nx, S.ny, S.nz);
  // approximative intersection with cone
  const float vx = p1x - p0x, vy = p1y - p0y, vz = p1z - p0z, vw = V1.w - V0.w;
  const float wx = -p0x, wy = -p0y;
  const float d0 = madd(wx, vx, wy * vy);
  const float d1 = madd(vx, vx, vy * vy);
  const float u = fminf(fmaxf(d0 * (1.0f / d1), 0.0f), 1.0f);
  const float px = madd(u, vx, p0x), py = madd(u, vy, p0y), pz = madd(u, vz, p0z), pw = madd(u, vw, V0.w);
  const float t = pz * S.s;
  const float d2 = madd(px, px, py * py);
  const float r2 = pw * pw;
  h.t = t;
  if (!((d2 <= r2) & (r.tnear < t) & (t <= tfarBlock))) return false;
  if (!(t > r.tnear + 2.0f * pw * S.s)) return false; // ignore self intersections
  // ignore denormalized segments
  const float Tx = V1.x - V0.x, Ty = V1.y - V0.y, Tz = V1.z - V0.z;
  if (!((Tx != 0.0f) | (Ty != 0.0f) | (Tz != 0.0f))) return false;
  h.u = u; h.v = 0.0f;
  h.ngx = Tx; h.ngy = Ty; h.ngz = Tz;
  return true;
}

// The selection of an octet pass over two blocks of 4 line records (lanes 0-3 block A, lanes 4-7 block B), as LineLeaf::octet_pass
// writes it out (its counted twins do not stay the same instructions with this helper, so only the motion-blur leaf calls it).  The depth test of these leaves is `t <= tfar` on the very t that is minimised, so ONE 4-lane minimum serves both
// blocks: block B, which has to see the tfar A left behind, has a winner exactly when its minimum over the lanes valid at pass entry is
// <= that tfar (the other conditions of the test do not depend on tfar), and that minimum is then its winner's t.  Inside a block the
// lowest lane wins; B wins an equal t of A.  Returns the winning lane (8: none); tfarNext is the tfar the pass leaves behind.
__device__ __forceinline__ uint32_t line_octet_winner(bool ok, float t, uint32_t m8, uint32_t k, uint32_t lid, float tfar, float& tfarNext)
{
  const float tq = quad_min4(ok ? t : RT_INF); // the minimum of this lane's own block
  const float tqm = dpp_f32<DPP_HALF_MIRROR>(tq); // and of the other one
  const float tA = k < 4u ? tq : tqm, tB = k < 4u ? tqm : tq;
  const bool hasA = (m8 & 0x0fu) != 0u;
  const float tfarB = hasA ? tA : tfar;
  const bool hasB = (m8 & 0xf0u) != 0u && tB <= tfarB;
  const uint32_t wA = octet_ballot(ok && k < 4u && t == tA, lid) & 0x0fu;
  const uint32_t wB = hasB ? octet_ballot(ok && k >= 4u && t == tB, lid) & 0xf0u : 0u;
  tfarNext = wB != 0u ? tB : (wA != 0u ? tA : tfar);
  return wB != 0u ? (uint32_t)__ffs(wB) - 1u : (wA != 0u ? (uint32_t)__ffs(wA) - 1u : 8u);
}

// The static line leaf (described in trace_line.hip, which holds its launcher): here so that the hair form of the two-level kernel
// (trace_instance_hair.hip) runs the same leaf below an instance.
// Records requested per memory round trip inside a block of 4 in the lane-per-ray form (1, 2 or 4).
#ifndef LINE_FETCH
#define LINE_FETCH 4
#endif

struct LineLeaf : LeafTraits
{
  static constexpr uint32_t FETCH = LINE_FETCH;

  // Child-parallel form (trace_loop.hip.h): the 8 lanes of an octet test 8 consecutive records of the leaf of the ray in exchange row
  // `x`, two of the reference's blocks of 4 per pass: lanes 0-3 block A, lanes 4-7 block B, every lane against the tfar at pass entry.
  // The depth test of this leaf is `t <= tfar` on the very t that is minimised, so ONE 4-lane minimum serves both blocks: block B,
  // which has to see the tfar A left behind, has a winner exactly when its minimum over the lanes valid at pass entry is <= that tfar
  // (the other conditions of the test do not depend on tfar), and that minimum is then its winner's t.  Inside a block the lowest
  // lane wins; B wins an equal t of A.  The winning lane writes the hit into the row (words 0..7 = t, Ng, u, v, geomID, primID;
  // word 9 = 1).
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const LineRecord* __restrict__ lines = (const LineRecord*)P.accel.blobs;
    const uint32_t k = lid & 7u;
    const RayState r = row_ray(x);
    const LineSpace S = line_space(r);
    const uint32_t ref = __float_as_uint(x[8]);
    uint32_t first, cnt;
    leaf_range(ref, first, cnt);
    cnt = valid ? cnt : 0u;
    float tfar = r.tfar;
    for (uint32_t b = 0; __ballot(b < cnt) != 0ull; b += 8u) {
      const bool present = b + k < cnt;
      const float4* lp = (const float4*)(lines + first + (present ? b + k : 0u));
      const float4 V0 = lp[0], V1 = lp[1];
      const uint2 ids = *(const uint2*)(lp + 2);
      if (COUNT && present) wc.prims++;
      TriHit h;
      h.t = RT_INF;
      bool ok = line_test(r, S, V0, V1, tfar, h) && present;
      if (ok && P.exclOffsets) ok = !candidate_excluded(P, __float_as_uint(x[10]), ids.x, ids.y, h.t);
      const uint32_t m8 = octet_ballot(ok, lid);
      if (OCCLUDED) { // Occluded1EpilogM: any valid lane
        if (m8 != 0u) {
          if (k == 0u) x[9] = __uint_as_float(1u);
          cnt = 0u;
        }
        continue;
      }
      // (line_octet_winner of trace_line.hip.h is this selection; written out here because the counted twins of this leaf do not stay the
      // same instructions with the helper)
      const float tq = quad_min4(ok ? h.t : RT_INF); // the minimum of this lane's own block
      const float tqm = dpp_f32<DPP_HALF_MIRROR>(tq); // and of the other one
      const float tA = k < 4u ? tq : tqm, tB = k < 4u ? tqm : tq;
      const bool hasA = (m8 & 0x0fu) != 0u;
      const float tfarB = hasA ? tA : tfar;
      const bool hasB = (m8 & 0xf0u) != 0u && tB <= tfarB;
      const uint32_t wA = octet_ballot(ok && k < 4u && h.t == tA, lid) & 0x0fu;
      const uint32_t wB = hasB ? octet_ballot(ok && k >= 4u && h.t == tB, lid) & 0xf0u : 0u;
      const uint32_t winner = wB != 0u ? (uint32_t)__ffs(wB) - 1u : (wA != 0u ? (uint32_t)__ffs(wA) - 1u : 8u);
      if (k == winner) row_write_hit(x, h, ids.x, ids.y); // Intersect1EpilogM, intersector_epilog.h:293-305
      tfar = wB != 0u ? tB : (wA != 0u ? tA : tfar);
    }
  }

  // Lane-per-ray form: the 4 candidates of a block against the tfar at block entry; candidates are visited in lane order and replace
  // the best one only with a smaller t, so the lowest lane wins ties.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ bool intersect(const LaunchParams& P, uint32_t ref, RayState& r, WorkCounters& wc, uint32_t rayIdx)
  {
    const LineRecord* __restrict__ lines = (const LineRecord*)P.accel.blobs;
    const LineSpace S = line_space(r);
    uint32_t first, count;
    leaf_range(ref, first, count);
    for (uint32_t b = 0; b < count; b += 4) {
      const float tfarBlock = r.tfar;
      const uint32_t nb = min(4u, count - b);
      bool found = false;
      TriHit best;
      uint32_t bestPrim = 0, bestGeom = 0;
      best.t = RT_INF;
      for (uint32_t g = 0; g < nb; g += FETCH) {
        // all records of the fetch group are requested before the first one is used; slots past the leaf end re-read the last record
        float4 V0[FETCH], V1[FETCH];
        uint2 ids[FETCH];
#pragma unroll
        for (uint32_t k = 0; k < FETCH; k++) {
          const float4* lp = (const float4*)(lines + first + b + min(g + k, nb - 1u));
          V0[k] = lp[0]; V1[k] = lp[1];
          ids[k] = *(const uint2*)(lp + 2);
        }
#pragma unroll
        for (uint32_t k = 0; k < FETCH; k++) {
          if (g + k >= nb) break;
          if (COUNT) wc.prims++;
          TriHit h;
          bool ok = line_test(r, S, V0[k], V1[k], tfarBlock, h);
          if (ok && P.exclOffsets) ok = !candidate_excluded(P, rayIdx, ids[k].x, ids[k].y, h.t);
          if (ok) {
            if (OCCLUDED) return true; // Occluded1EpilogM: any valid lane
            if (!found || h.t < best.t) { // select_min over the 4 lanes, lowest lane wins ties
              best = h;
              bestGeom = ids[k].x;
              bestPrim = ids[k].y;
              found = true;
            }
          }
        }
      }
      if (found) commit_hit(r, best, bestGeom, bestPrim); // Intersect1EpilogM, intersector_epilog.h:293-305
    }
    return false;
  }
};

} // namespace dev
} // namespace rtamd
