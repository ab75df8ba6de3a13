// Single-level instancing (RTC_GEOMETRY_TYPE_INSTANCE, one time step): a two-level traversal kernel of its own, one ray per lane.
// The accel (accel.h InstanceRecord, rt_scene.cpp build_instance_accel) is ONE node array: a top-level BVH8 over the instances' world
// bounds with one instance per leaf, and behind it the triangle trees of the instanced scenes, rebased, over one TriRecord array.
// Per ray:
//   1. the top-level tree is traversed in world space (the loop of bvh_intersector1.cpp:40-126 / :128-209, as trace_loop.hip.h);
//   2. at an instance leaf the ray enters the instance (instance_intersector.cpp:51-59): org' = xfmPoint(world2local, org)
//      (affinespace.h:110), dir' = xfmVector(world2local, dir) (linearspace3.h:169), tnear and tfar unchanged - t is common to both
//      spaces; the node-test constants are re-derived from the local ray, an exit marker (REF_INST_EXIT) goes on the stack and the
//      traversal continues at the instanced scene's root with the same stack;
//   3. triangle leaves below are the block loop of TriLeaf::intersect (trace_tri.hip) restated: all records of a block of 4 see the tfar
//      at block entry, the lowest lane wins ties, a later block replaces an equal t.  A hit keeps the instanced scene's geomID / primID and
//      Ng, u, v as computed in LOCAL space (the reference does not transform Ng), and the instance's geomID as instID
//      (instance_intersector.cpp:57), whatever the context's instID[0] holds;
//   4. popping the marker restores the world-space ray (read again through the ray's index) and its node-test constants
//      (instance_intersector.cpp:61-62).
// What a world-space entry below the marker was stacked with - its entry distance - is compared with the ray's tfar as ever: t is common.
// From the shared headers: LaunchParams, the 64 work queues with chunked grabs, the stack[entry][lane] LDS layout with its HBM overflow
// columns and the `overflow` word, TravRay, the QNode8 decode and slab test with the reference's child order, pluecker / moeller /
// commit_hit, load_ray / store_hit.  No octet form, no ray-pool form, no root cull pre-pass, no service kernel, no instrumented twin
// (rt_trace.cpp launch_on, rt_service.cpp; counted batches on scenes with instances are refused).
//
// QUADS (accel kinds ACCEL_INST_PLUECKER / ACCEL_INST_MOELLER): an instanced scene may hold a quad tree next to, or instead of, its
// triangle tree.  Inside an instance the local ray traverses the triangle tree completely and then the quad tree, against the tfar the
// triangles left (the instanced scene's AccelN, scene.cpp:650-654) - so a quad at a bit-identical t replaces the triangle:
//   2'. entering an instance whose record has a quad root stacks a second marker (REF_INST_QUADS, the quad root in the entry's
//       distance word) above the exit marker and continues at the triangle root; without a triangle tree it starts in the quad tree;
//   3'. popping that marker sets the lane's ST_QUADS bit and continues at the quad root; with the bit set a leaf is the block loop of
//       QuadLeaf::intersect (trace_quad.hip) restated over pluecker_quad / moeller_quad: 8 candidates per block of 4 records (A =
//       (v0, v1, v3) in lanes 0-3, B = (v2, v1, v3) in lanes 4-7), all against the tfar at block entry, one minimum, the lowest lane
//       wins ties, a later block replaces an equal t.  The QuadRecords lie behind the InstanceRecords in `blobs`, one 64-byte array;
//   4'. the exit marker clears the bit.
//
// XFMB (accel kinds ACCEL_INSTMB_*): instances may have time steps (instance motion blur, scene_instance.h:58-63,
// instance_intersector.cpp:51-56).  Entering an instance whose record names InstanceSteps (pad[1] != 0) the lane reads its ray's time
// through the ray's index, loads the two steps around it and computes world2local = inverse(lerp(step[itime], step[itime + 1], ftime))
// with the function the host exports (instance_xfm.h), in place of the record's matrix; everything after that - the transform of org
// and dir, the markers, the trees, leaving - is the static form.  A singular interpolated transform (det == 0 or a matrix that is
// not finite) is not entered: the lane pops instead and pushes nothing, where the reference would trace NaNs.  An instance with one
// time step in such a scene (pad[1] == 0) is entered through its record.
#include "trace_leaf.hip.h"
#include "trace_quad_tests.hip.h"
#include "trace_mb.hip.h"
#include "instance_xfm.h"

namespace rtamd {
namespace dev {

// Waves per SIMD the register allocator is asked for: 4 (<= 128 VGPRs), as the triangle kernels run; the kernels must compile without
// scratch at this bound (tools/kernel_resources.sh, docs/experiments.md "Instancing").
#ifndef TRACE_INST_MIN_WAVES
#define TRACE_INST_MIN_WAVES 4
#endif

// Records requested per memory round trip inside a block of 4.  The closest-hit Pluecker kernel carries two instance ids and the hit on
// top of the Pluecker test's temporaries: with four records in flight it needs 116 bytes of scratch at 128 VGPRs.
#ifndef TRACE_INST_FETCH
#define TRACE_INST_FETCH 2
#endif
// The QUADS instantiations carry the quad block loop (a record is four dwordx4, a block has 8 candidates) next to the triangle loop.
// Three of the four compile without scratch at 4 waves per SIMD; closest-hit Pluecker does not (76 bytes of scratch with two QuadRecords
// per round trip, 36 with one), as the static quad lane kernel's does not (trace_quad.hip): it alone is asked for 3 waves (<= 168 VGPRs).
#ifndef TRACE_INST_QUADS_MIN_WAVES_PLUECKER_CLOSEST
#define TRACE_INST_QUADS_MIN_WAVES_PLUECKER_CLOSEST 3
#endif
// QuadRecords requested per memory round trip inside a block of 4 (1 or 2)
#ifndef TRACE_INST_QUAD_FETCH
#define TRACE_INST_QUAD_FETCH 2
#endif
constexpr int inst_min_waves(bool pluecker, bool occluded, bool quads, bool xfmb)
{
  return quads && pluecker && !occluded ? TRACE_INST_QUADS_MIN_WAVES_PLUECKER_CLOSEST : TRACE_INST_MIN_WAVES;
}

template <bool PLUECKER, bool OCCLUDED, bool VEC, bool QUADS, bool XFMB>
__global__ __launch_bounds__(TRACE_BLOCK, inst_min_waves(PLUECKER, OCCLUDED, QUADS, XFMB)) void trace_instance_kernel(LaunchParams P)
{
  constexpr uint32_t FETCH = TRACE_INST_FETCH;
  constexpr uint32_t QFETCH = TRACE_INST_QUAD_FETCH;
  constexpr bool ROBUST = PLUECKER; // Pluecker <-> robust traversal, Moeller <-> fast traversal, on both levels
  __shared__ uint2 ldsStack[TRACE_LDS_STACK + 1][TRACE_BLOCK]; // + one scratch row for the branch-free pushes
  const uint32_t tid = threadIdx.x;
  const uint32_t gthread = blockIdx.x * TRACE_BLOCK + tid;
  auto spill_col = [&]() -> uint2* { // see trace_loop.hip.h: formed where it is used, from an opaque copy of the thread index
    uint32_t g = gthread;
    asm volatile("" : "+v"(g));
    return (uint2*)P.spill + (size_t)g * P.spillDepth;
  };
  const QNode8* __restrict__ nodes = P.accel.nodes;
  const TriRecord* __restrict__ prims = P.accel.prims;
  const InstanceRecord* __restrict__ insts = (const InstanceRecord*)P.accel.blobs;
  uint32_t* __restrict__ queues = P.queues;

  // work queues: queue q owns the rays [q * perQ, (q + 1) * perQ); a wave starts at its home queue (trace_loop.hip.h)
  const uint32_t perQ = (P.count + (uint32_t)TRACE_QUEUES - 1u) / (uint32_t)TRACE_QUEUES;
  const uint32_t laneId = lane_rank(~0ull);
  auto queue_len = [&](uint32_t q) -> uint32_t {
    const uint32_t lo = min(q * perQ, P.count);
    return min(lo + perQ, P.count) - lo;
  };
  uint32_t qCur = (blockIdx.x * (TRACE_BLOCK / 64) + (tid >> 6)) & (uint32_t)(TRACE_QUEUES - 1); // wave-uniform
  uint32_t poolNext = 0, poolEnd = 0; // wave-uniform: rays [poolNext, poolEnd) belong to this wave
  bool exhausted = P.accel.root == REF_EMPTY;

  RayState r;
  TravRay<ROBUST> tr;
  float travFar = 0.f;
  uint32_t sp = 0, cur = REF_EMPTY, rayIdx = 0;
  uint32_t curInst = 0xFFFFFFFFu, hitInst = 0xFFFFFFFFu; // geomID of the instance being traversed / of the hit's instance
  // lane state bits (vector register, see RayState::hit): the lane owns a ray, its next event is a pop, it is inside an instance,
  // it is in the instanced scene's quad tree (QUADS only)
  enum : uint32_t { ST_ACTIVE = 1u, ST_POP = 2u, ST_INSIDE = 4u, ST_QUADS = 8u };
  uint32_t st = 0u;
  r.hit = 0u;

  auto push = [&](uint32_t ref, uint32_t dist, uint32_t slot) {
    if (slot < (uint32_t)TRACE_LDS_STACK) ldsStack[slot][tid] = make_uint2(ref, dist);
    else {
      if (slot - TRACE_LDS_STACK < P.spillDepth) spill_col()[slot - TRACE_LDS_STACK] = make_uint2(ref, dist);
      else __hip_atomic_store(P.overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); // entry dropped: the host raises an error
    }
  };
  auto pop_spill = [&](uint32_t slot) -> uint2 {
    if (!(slot - TRACE_LDS_STACK < P.spillDepth)) return make_uint2(REF_EMPTY, 0x7f800000u);
    const uint32_t* e = (const uint32_t*)(spill_col() + (slot - TRACE_LDS_STACK));
    return make_uint2(__builtin_nontemporal_load(e), __builtin_nontemporal_load(e + 1));
  };

  for (;;) {
    // ---- refill idle lanes (trace_loop.hip.h) -----------------------------------------------------------------------
    const uint64_t idleMask = __ballot(!(st & ST_ACTIVE));
    if (idleMask != 0ull && !exhausted && (__popcll(idleMask) >= (int)P.refillBatch || idleMask == ~0ull)) {
      if (poolNext == poolEnd) { // take a new chunk (one lane does the atomic, the result is wave-uniform)
        for (;;) {
          const uint32_t qLo = qCur * perQ;
          const uint32_t qLen = queue_len(qCur);
          uint32_t base = 0xFFFFFFFFu;
          if (laneId == 0u) base = atomicAdd(&queues[qCur * QUEUE_STRIDE], P.rayChunk);
          base = __builtin_amdgcn_readfirstlane(base);
          if (base < qLen) {
            poolNext = qLo + base;
            poolEnd = min(poolNext + P.rayChunk, qLo + qLen);
            break;
          }
          // drained: lane l reads head l, the ballot marks the queues that still have rays, take the next one cyclically after qCur
          const uint32_t head = __hip_atomic_load(&queues[laneId * QUEUE_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const uint64_t live = __ballot(laneId < (uint32_t)TRACE_QUEUES && head < queue_len(laneId));
          if (live == 0ull) { exhausted = true; break; }
          const uint64_t rot = (live >> qCur) | (qCur ? (live << (64u - qCur)) : 0ull); // bit k = queue (qCur+k)&63
          qCur = (qCur + (uint32_t)__builtin_ctzll(rot)) & (uint32_t)(TRACE_QUEUES - 1);
        }
      }
      if (poolNext != poolEnd) {
        const uint32_t mine = poolNext + lane_rank(idleMask);
        if (!(st & ST_ACTIVE) && mine < poolEnd) {
          rayIdx = mine;
          load_ray<VEC>((const char*)P.rays + (size_t)rayIdx * P.stride, r);
          r.hit = 0u;
          // rays with tnear > tfar are skipped (bvh_intersector_stream_filters.cpp:156); occluded: already-occluded rays return early
          // (bvh_intersector1.cpp:132-134)
          bool ok = r.tnear <= r.tfar;
          if (OCCLUDED) ok = ok && !(r.tfar < 0.0f);
          if (ok) {
            tr.init(r);
            travFar = fmaxf(r.tfar, 0.0f); // tray.tfar
            sp = 0;
            cur = P.accel.root;
            st = ST_ACTIVE;
          }
        }
        poolNext = min(poolNext + (uint32_t)__popcll(idleMask), poolEnd);
      }
    }
    if (__ballot((st & ST_ACTIVE) != 0u) == 0ull) {
      if (exhausted) break;
      continue;
    }

    // ---- inner node step: the lane-per-ray step of trace_loop.hip.h, on either level ---------------------------------
    if (!(st & ST_POP) && (st & ST_ACTIVE) && !(cur & REF_LEAF)) {
      const uint4* np = (const uint4*)(nodes + cur);
      const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3], n4 = np[4], n5 = np[5];
      const float ox = __uint_as_float(n0.x), oy = __uint_as_float(n0.y), oz = __uint_as_float(n0.z);
      const float sx = __uint_as_float((n0.w & 0xffu) << 23);
      const float sy = __uint_as_float(((n0.w >> 8) & 0xffu) << 23);
      const float sz = __uint_as_float(((n0.w >> 16) & 0xffu) << 23);
      // near / far plane bytes per axis: words .x,.y = lower[0..7], .z,.w = upper[0..7]
      const bool ngx = tr.negx(), ngy = tr.negy(), ngz = tr.negz();
      const uint32_t nx0 = ngx ? n3.z : n3.x, nx1 = ngx ? n3.w : n3.y;
      const uint32_t fx0 = ngx ? n3.x : n3.z, fx1 = ngx ? n3.y : n3.w;
      const uint32_t ny0 = ngy ? n4.z : n4.x, ny1 = ngy ? n4.w : n4.y;
      const uint32_t fy0 = ngy ? n4.x : n4.z, fy1 = ngy ? n4.y : n4.w;
      const uint32_t nz0 = ngz ? n5.z : n5.x, nz1 = ngz ? n5.w : n5.y;
      const uint32_t fz0 = ngz ? n5.x : n5.z, fz1 = ngz ? n5.y : n5.w;
      const uint32_t cref[8] = {n1.x, n1.y, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w};

      uint32_t dist[8];
      uint32_t mask = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int kk = k & 3;
        const float npx = madd(q2f(k < 4 ? nx0 : nx1, kk), sx, ox);
        const float npy = madd(q2f(k < 4 ? ny0 : ny1, kk), sy, oy);
        const float npz = madd(q2f(k < 4 ? nz0 : nz1, kk), sz, oz);
        const float fpx = madd(q2f(k < 4 ? fx0 : fx1, kk), sx, ox);
        const float fpy = madd(q2f(k < 4 ? fy0 : fy1, kk), sy, oy);
        const float fpz = madd(q2f(k < 4 ? fz0 : fz1, kk), sz, oz);
        const float tN = fmaxf(tr.nearT(npx, npy, npz), tr.tnear);
        const float tF = fminf(tr.farT(fpx, fpy, fpz), travFar);
        const bool h = (tN <= tF) & (cref[k] != REF_EMPTY);
        // non-hit: distinct sentinels above every distance and below 2^31 (the ranking takes the sign of 32-bit differences)
        dist[k] = h ? __float_as_uint(tN) : (0x7FFFFFF8u + (uint32_t)k);
        mask |= h ? (1u << k) : 0u;
      }
      const int nhit = __popc(mask);
      if (nhit == 0) st |= ST_POP;
      else if (nhit == 1) {
        const int k = __ffs(mask) - 1;
        uint32_t c = cref[0];
#pragma unroll
        for (int j = 1; j < 8; j++) c = (k == j) ? cref[j] : c;
        cur = c;
      } else {
        // rank[k] = number of hit children visited before child k; rank 0 is entered now, the others are stacked in pop order
        uint32_t rank[8];
        if (OCCLUDED) {
          // traverseAnyHit (bvh_traverser1.h:638-666): descend into the highest-index hit child, stack the rest in ascending order
#pragma unroll
          for (int k = 0; k < 8; k++) rank[k] = (uint32_t)__popc(mask >> (k + 1));
        } else {
          // traverseClosestHit: ascending uint(tNear), equal distances -> higher child index first (bvh_traverser1.h:590-591,
          // stack_item.h:39-80); exactly four hit children with a tie: the 5-comparator network (trace_common.hip.h)
#pragma unroll
          for (int k = 0; k < 8; k++) rank[k] = (uint32_t)(7 - k);
#pragma unroll
          for (int a = 0; a < 8; a++) {
#pragma unroll
            for (int b = a + 1; b < 8; b++) {
              const uint32_t aFirst = (dist[a] - dist[b]) >> 31; // tie -> 0 -> b (higher index) first
              rank[b] += aFirst;
              rank[a] -= aFirst;
            }
          }
          if (__ballot(nhit == 4) != 0ull) {
            bool tie = false; // non-hit children carry distinct sentinels, so any equality is a tie between hit children
#pragma unroll
            for (int a = 0; a < 8; a++)
#pragma unroll
              for (int b = a + 1; b < 8; b++) tie |= dist[a] == dist[b];
            if (nhit == 4 && tie) rank4_by_network(mask, dist, rank);
          }
        }
        const uint32_t top = sp + (uint32_t)nhit - 1u;
        uint32_t next = REF_EMPTY;
        if (top <= (uint32_t)TRACE_LDS_STACK) {
          // common case, branch-free: every entry lands in LDS; children that are not stacked write to the scratch row
#pragma unroll
          for (int k = 0; k < 8; k++) {
            const bool h = (mask >> k) & 1u;
            const bool stacked = h && rank[k] != 0u;
            next = (h && rank[k] == 0u) ? cref[k] : next;
            ldsStack[stacked ? top - rank[k] : (uint32_t)TRACE_LDS_STACK][tid] = make_uint2(cref[k], dist[k]);
          }
        } else {
#pragma unroll
          for (int k = 0; k < 8; k++) {
            if (mask & (1u << k)) {
              if (rank[k] == 0u) next = cref[k];
              else push(cref[k], dist[k], top - rank[k]);
            }
          }
        }
        sp = top;
        cur = next;
      }
    }

    // ---- instance leaf: the ray enters the instance (no waiting: four loads, twelve FMAs, three divisions) -------------
    if (st == ST_ACTIVE && (cur & REF_LEAF)) {
      const float4* ip = (const float4*)(insts + (cur & ((1u << TRI_START_BITS) - 1u)));
      float4 q0 = ip[0], q1 = ip[1], q2 = ip[2]; // vx.xyz vy.x | vy.yz vz.xy | vz.z p.xyz
      const uint4 q3 = ((const uint4*)ip)[3];    // geomID, root, quad root, (S << 24) | firstStep
      bool enter = true;
      if (XFMB) {
        if (q3.w != 0u) { // a moving instance: world2local at the ray's time replaces the record's (instance_xfm.h)
          float f;
          const uint32_t itime = instance_time_segment(ray_time(P, rayIdx), q3.w >> 24, f);
          const float4* sp4 = (const float4*)(insts + (q3.w & 0xFFFFFFu) + itime); // InstanceStep[itime], [itime + 1]: 64 bytes each
          const float4 a0 = sp4[0], a1 = sp4[1], a2 = sp4[2], b0 = sp4[4], b1 = sp4[5], b2 = sp4[6];
          const float A[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
          const float B[12] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w};
          float W[12];
          enter = instance_world2local(A, B, f, W);
          q0 = make_float4(W[0], W[1], W[2], W[3]);
          q1 = make_float4(W[4], W[5], W[6], W[7]);
          q2 = make_float4(W[8], W[9], W[10], W[11]);
        }
      }
      if (XFMB && !enter) st |= ST_POP; // singular interpolated transform: the ray does not enter, nothing is pushed
      else {
      const float wox = r.ox, woy = r.oy, woz = r.oz, wdx = r.dx, wdy = r.dy, wdz = r.dz;
      // xfmPoint (affinespace.h:110): madd(p.x, vx, madd(p.y, vy, madd(p.z, vz, p)))
      r.ox = madd(wox, q0.x, madd(woy, q0.w, madd(woz, q1.z, q2.y)));
      r.oy = madd(wox, q0.y, madd(woy, q1.x, madd(woz, q1.w, q2.z)));
      r.oz = madd(wox, q0.z, madd(woy, q1.y, madd(woz, q2.x, q2.w)));
      // xfmVector (linearspace3.h:169): madd(v.x, vx, madd(v.y, vy, v.z * vz))
      r.dx = madd(wdx, q0.x, madd(wdy, q0.w, wdz * q1.z));
      r.dy = madd(wdx, q0.y, madd(wdy, q1.x, wdz * q1.w));
      r.dz = madd(wdx, q0.z, madd(wdy, q1.y, wdz * q2.x));
      tr.init(r); // tnear, tfar and travFar stay: t is common to both spaces
      push(REF_INST_EXIT, 0u, sp);
      sp++;
      curInst = q3.x;
      cur = q3.y;
      st = ST_ACTIVE | ST_INSIDE;
      if (QUADS) { // q3.z: the quad root (InstanceRecord::pad[0]), REF_EMPTY without quads; q3.y is REF_EMPTY without triangles
        if (q3.z != REF_EMPTY) {
          if (cur != REF_EMPTY) { // triangles first: the quad tree waits on the stack, its root in the distance word
            push(REF_INST_QUADS, q3.z, sp);
            sp++;
          } else {
            cur = q3.z;
            st |= ST_QUADS;
          }
        } else if (cur == REF_EMPTY) st |= ST_POP; // neither tree (the builder leaves such instances out)
      }
      }
    }

    // ---- triangle / quad leaf inside an instance: run when enough lanes wait at one, or when nobody has node work -------
    const bool atLeaf = (QUADS ? st & ~ST_QUADS : st) == (ST_ACTIVE | ST_INSIDE) && (cur & REF_LEAF);
    const uint64_t leafMask = __ballot(atLeaf);
    if (leafMask != 0ull) {
      const bool nodeWork = __ballot((st & ST_ACTIVE) && !(st & ST_POP) && !(cur & REF_LEAF)) != 0ull;
      if (((uint32_t)__popcll(leafMask) >= P.leafBatch || !nodeWork) && atLeaf) {
        uint32_t first, count;
        leaf_range(cur, first, count);
        bool occl = false;
        if (QUADS && (st & ST_QUADS)) {
          // the block loop of QuadLeaf::intersect (trace_quad.hip; quad_intersector_pluecker.h:264-299, quad_intersector_moeller.h:251-290)
          const QuadRecord* __restrict__ quads = (const QuadRecord*)P.accel.blobs; // behind the InstanceRecords: the leaf references are rebased
          for (uint32_t b = 0; b < count && !occl; b += 4) {
            const float tfarBlock = r.tfar; // all 8 candidates of a block see the tfar at block entry
            const uint32_t nb = min(4u, count - b);
            bool found = false;
            TriHit best;
            uint32_t bestLane = 8u, bestPrim = 0, bestGeom = 0;
            best.t = RT_INF;
            // QFETCH records are requested before the first one is used; slots past the leaf end re-read the last record and are skipped below
            for (uint32_t g = 0; g < nb && !occl; g += QFETCH) {
              float4 V0[QFETCH], V1[QFETCH], V2[QFETCH], V3[QFETCH];
#pragma unroll
              for (uint32_t k = 0; k < QFETCH; k++) {
                const float4* qp = (const float4*)(quads + first + b + min(g + k, nb - 1u));
                V0[k] = qp[0]; V1[k] = qp[1]; V2[k] = qp[2]; V3[k] = qp[3];
              }
#pragma unroll
              for (uint32_t k = 0; k < QFETCH; k++) {
                if (g + k >= nb || occl) break;
                const uint32_t gid = __float_as_uint(V0[k].w), pid = __float_as_uint(V1[k].w);
#pragma unroll
                for (uint32_t half = 0; half < 2; half++) { // A then B of this quad (lanes g+k and 4+g+k)
                  TriHit h;
                  const bool ok = PLUECKER ? pluecker_quad(r, half ? V2[k] : V0[k], V1[k], V3[k], tfarBlock, half != 0u, h)
                                           : moeller_quad(r, half ? V2[k] : V0[k], V1[k], V3[k], tfarBlock, half != 0u, h);
                  if (ok) {
                    if (OCCLUDED) { occl = true; break; } // Occluded1EpilogM: any valid lane
                    // select_min over the 8 lanes, lowest lane wins ties
                    const uint32_t lane = half * 4u + g + k;
                    if (!found || h.t < best.t || (h.t == best.t && lane < bestLane)) {
                      best = h;
                      bestLane = lane;
                      bestGeom = gid;
                      bestPrim = pid;
                      found = true;
                    }
                  }
                }
              }
            }
            if (found) { // Intersect1EpilogM, intersector_epilog.h:293-305; instID: instance_intersector.cpp:57
              commit_hit(r, best, bestGeom, bestPrim);
              hitInst = curInst;
            }
          }
        } else {
          // the block loop of TriLeaf::intersect (trace_tri.hip; intersector_iterators.h:32-36, epilog intersector_epilog.h:226-307 / :388-450)
          for (uint32_t b = 0; b < count && !occl; b += 4) {
            const float tfarBlock = r.tfar; // all records of a block see the tfar at block entry
            const uint32_t nb = min(4u, count - b);
            bool found = false;
            TriHit best;
            uint32_t bestPrim = 0, bestGeom = 0;
            best.t = RT_INF;
            // FETCH records are requested before the first one is used; slots past the leaf end re-read the last record and are skipped below
            for (uint32_t g = 0; g < nb && !occl; g += FETCH) {
              float4 A[FETCH], B[FETCH], C[FETCH];
#pragma unroll
              for (uint32_t k = 0; k < FETCH; k++) {
                const float4* tp = (const float4*)(prims + first + b + min(g + k, nb - 1u));
                A[k] = tp[0]; B[k] = tp[1]; C[k] = tp[2];
              }
#pragma unroll
              for (uint32_t k = 0; k < FETCH; k++) {
                if (g + k >= nb) break;
                TriHit h;
                const bool ok = PLUECKER ? pluecker(r, A[k], B[k], C[k], tfarBlock, h) : moeller(r, A[k], B[k], C[k], tfarBlock, h);
                if (ok) {
                  if (OCCLUDED) { occl = true; break; } // Occluded1EpilogM: any valid lane
                  // select_min over valid lanes, lowest lane wins ties (vfloat4_sse2.h:654-659)
                  if (!found || h.t < best.t) {
                    best = h;
                    bestGeom = __float_as_uint(A[k].w);
                    bestPrim = __float_as_uint(B[k].w);
                    found = true;
                  }
                }
              }
            }
            if (found) { // Intersect1EpilogM, intersector_epilog.h:293-305; instID: instance_intersector.cpp:57
              commit_hit(r, best, bestGeom, bestPrim);
              hitInst = curInst;
            }
          }
        }
        if (OCCLUDED && occl) {
          r.tfar = -RT_INF; // bvh_intersector1.cpp:198-201
          r.hit = 1u;
          sp = 0;           // any hit found: terminate this ray
        }
        travFar = OCCLUDED ? travFar : r.tfar; // tray.tfar = ray.tfar (bvh_intersector1.cpp:117)
        st |= ST_POP;
      }
    }

    // ---- pop ------------------------------------------------------------------------------------------------------------
    if ((st & (ST_ACTIVE | ST_POP)) == (ST_ACTIVE | ST_POP)) {
      bool finished = false;
      for (;;) {
        if (sp == 0) { finished = true; break; }
        sp--;
        uint2 e;
        if (sp < (uint32_t)TRACE_LDS_STACK) e = ldsStack[sp][tid];
        else e = pop_spill(sp);
        if (e.x == REF_EMPTY) continue; // entry lost to an exhausted spill area
        if (e.x == REF_INST_EXIT) {     // the ray leaves the instance (instance_intersector.cpp:61-62); checked before the distance cull
          // the world-space ray is read again through the ray's index (org and dir are never written): six registers less across the
          // loop, which keeps the closest-hit Pluecker kernel free of scratch at 128 VGPRs
          RayState w;
          load_ray<VEC>((const char*)P.rays + (size_t)rayIdx * P.stride, w);
          r.ox = w.ox; r.oy = w.oy; r.oz = w.oz;
          r.dx = w.dx; r.dy = w.dy; r.dz = w.dz;
          tr.init(r);
          st &= QUADS ? ~(ST_INSIDE | ST_QUADS) : ~ST_INSIDE;
          continue;
        }
        if (QUADS && e.x == REF_INST_QUADS) { // the triangle tree is done: on to the instanced scene's quad tree; before the distance cull
          st |= ST_QUADS;
          cur = e.y;
          break;
        }
        if (!OCCLUDED && __uint_as_float(e.y) > r.tfar) continue; // bvh_intersector1.cpp:86
        cur = e.x;
        break;
      }
      st &= ~ST_POP;
      if (finished) {
        if (r.hit) {
          char* rp = (char*)P.rays + (size_t)rayIdx * P.stride;
          if (OCCLUDED) ((float*)rp)[8] = r.tfar;
          else store_hit<VEC>(rp, r, hitInst);
        }
        st = 0u;
      }
    }
  }
}

template <bool PLUECKER, bool OCCLUDED, bool QUADS, bool XFMB>
inline hipError_t launch_instance_vec(const LaunchParams& p, hipStream_t stream)
{
  const bool vec = (p.stride % 16 == 0) && (((uintptr_t)p.rays) % 16 == 0);
  // persistent grid = what is resident at once for this instantiation, capped by the host's bound (which sized the spill area)
  static int occVec = 0, occGen = 0;
  int& occ = vec ? occVec : occGen;
  if (occ == 0) {
    hipError_t e = vec ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, trace_instance_kernel<PLUECKER, OCCLUDED, true, QUADS, XFMB>, TRACE_BLOCK, 0)
                       : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, trace_instance_kernel<PLUECKER, OCCLUDED, false, QUADS, XFMB>, TRACE_BLOCK, 0);
    if (e != hipSuccess || occ <= 0) occ = 1;
  }
  uint32_t blocks = (p.blocksPerCU ? std::min<uint32_t>(p.blocksPerCU, (uint32_t)occ) : (uint32_t)occ) * p.numCUs;
  if (blocks > p.gridBlocks) blocks = p.gridBlocks;
  if (vec) hipLaunchKernelGGL((trace_instance_kernel<PLUECKER, OCCLUDED, true, QUADS, XFMB>), dim3(blocks), dim3(TRACE_BLOCK), 0, stream, p);
  else hipLaunchKernelGGL((trace_instance_kernel<PLUECKER, OCCLUDED, false, QUADS, XFMB>), dim3(blocks), dim3(TRACE_BLOCK), 0, stream, p);
  return hipGetLastError();
}

} // namespace dev

hipError_t launch_trace_instance(const LaunchParams& p, hipStream_t stream)
{
  if (p.counters) return hipErrorInvalidValue; // no instrumented twin (rt_trace.cpp refuses counted batches on scenes with instances)
  switch (p.accel.kind) {
  case ACCEL_INST_TRI_PLUECKER: return p.occluded ? dev::launch_instance_vec<true, true, false, false>(p, stream) : dev::launch_instance_vec<true, false, false, false>(p, stream);
  case ACCEL_INST_TRI_MOELLER: return p.occluded ? dev::launch_instance_vec<false, true, false, false>(p, stream) : dev::launch_instance_vec<false, false, false, false>(p, stream);
  case ACCEL_INST_PLUECKER: return p.occluded ? dev::launch_instance_vec<true, true, true, false>(p, stream) : dev::launch_instance_vec<true, false, true, false>(p, stream);
  case ACCEL_INST_MOELLER: return p.occluded ? dev::launch_instance_vec<false, true, true, false>(p, stream) : dev::launch_instance_vec<false, false, true, false>(p, stream);
  case ACCEL_INSTMB_TRI_PLUECKER: return p.occluded ? dev::launch_instance_vec<true, true, false, true>(p, stream) : dev::launch_instance_vec<true, false, false, true>(p, stream);
  case ACCEL_INSTMB_TRI_MOELLER: return p.occluded ? dev::launch_instance_vec<false, true, false, true>(p, stream) : dev::launch_instance_vec<false, false, false, true>(p, stream);
  case ACCEL_INSTMB_PLUECKER: return p.occluded ? dev::launch_instance_vec<true, true, true, true>(p, stream) : dev::launch_instance_vec<true, false, true, true>(p, stream);
  case ACCEL_INSTMB_MOELLER: return p.occluded ? dev::launch_instance_vec<false, true, true, true>(p, stream) : dev::launch_instance_vec<false, false, true, true>(p, stream);
  default: return hipErrorInvalidValue;
  }
}

} // namespace rtamd
