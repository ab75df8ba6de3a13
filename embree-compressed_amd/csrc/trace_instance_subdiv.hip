// Subdivision meshes below an instance (accel kinds ACCEL_INSTSUBDIV_GRID / ACCEL_INSTSUBDIV_CBVH_LEAF, Scene::instSubdivAccel): a sibling
// of the two-level kernel of trace_instance.hip, whose machinery it restates - the 64 work queues with chunked grabs, the
// stack[entry][lane] LDS layout with its HBM overflow columns and the `overflow` word, the QNode8 step in the reference's child order,
// the entry into an instance (through instance_world2local for a moving one), the exit marker and the re-read of the world ray, the
// leafBatch / nodeWork rule - with the two one-ray-per-lane subdivision leaves below an instance instead of the mesh block loops:
//   GridCellLeaf::intersect (trace_grid.hip.h)                   eager accel: the 8 Pluecker triangles of a 3x3-vertex cell
//   CbvhLeaf<MODE_LEAF, C, false>::intersect (trace_cbvh.hip.h)  bvh4.compressed.leaf: the walk of one cBVH blob, C = 1..5
// A sibling and not a seventh constant of trace_instance_body.hip.h: that text is held to the instruction streams of its 40
// instantiations.  What differs from it:
//   - always the robust traversal (TravRay<true>) on both levels, as the subdivision accels run at top level (launch_leaf<Leaf, true>);
//   - every instantiation takes instances with transform time steps (the XFMB path);
//   - an instanced scene has one tree: no pending-tree markers, one state bit for "inside";
//   - a leaf below an instance calls Leaf::intersect<OCCLUDED, false> on the LOCAL ray.  `blobs` starts with the InstanceRecords and
//     InstanceSteps; the leaf blobs follow from a multiple of the blob stride on and the leaf references are rebased (accel.h), so the
//     leaf's own addressing, P.accel.blobs + index * stride, finds them.  A closest hit keeps the instanced scene's geomID / primID and
//     its u, v; Ng is what the leaf produces (the eager cell's local-space Ng, or the fork's dummy (1, 0, 0), written at store time
//     like the lane kernel's CONST_NG leaves); t is common to both spaces; instID is the instance's geomID
//     (instance_intersector.cpp:51-62).  Any-hit: an eager hit ends the ray; for compressed.leaf the fork's occluded() stub
//     (compressed.h:754-756) applies to the local ray - a blob whose exact bounds pass the robust slab test reports occluded.
// Leaf::prepare() runs once per kernel (the cBVH decode tables in LDS).  No octet / quad form, no ray-pool form, no root cull pre-pass,
// no service kernel, no instrumented twin.  24 kernels: 6 leaves x closest / any hit x 16-byte aligned records / others.
#include "trace_grid.hip.h"
#include "trace_cbvh.hip.h"
#include "trace_mb.hip.h"
#include "instance_xfm.h"

namespace rtamd {
namespace dev {

// Waves per SIMD the register allocator is asked for: the bound of the same leaf's top-level lane kernel (Leaf::MIN_WAVES: 3, cBVH from
// C = 4 on 2), one wave less for a closest-hit kernel that spills more than that twin (tools/kernel_resources.sh; the table is in
// docs/experiments.md, "Subdivision meshes below an instance").  The cBVH kernels compile without scratch at their twins' bounds.  The
// eager closest-hit kernel needs 36 bytes of scratch at 3 waves (168 VGPRs) where its twin has none - the lane kernel tests cells 8
// lanes per ray and does not hold GridCellLeaf::intersect with its 40 cell words at all; the ray-pool kernel, which does, takes 186
// VGPRs: 2 waves.
template <typename Leaf> struct inst_subdiv_waves
{
  static constexpr int closest = Leaf::MIN_WAVES, any = Leaf::MIN_WAVES;
};
template <> struct inst_subdiv_waves<GridCellLeaf>
{
  static constexpr int closest = GridCellLeaf::MIN_WAVES - 1, any = GridCellLeaf::MIN_WAVES;
};
template <typename Leaf, bool OCCLUDED> constexpr int inst_subdiv_min_waves() { return OCCLUDED ? inst_subdiv_waves<Leaf>::any : inst_subdiv_waves<Leaf>::closest; }

template <typename Leaf, bool OCCLUDED, bool VEC>
__global__ __launch_bounds__(TRACE_BLOCK, (inst_subdiv_min_waves<Leaf, OCCLUDED>())) void trace_instance_subdiv_kernel(LaunchParams P)
{
  __shared__ uint2 ldsStack[TRACE_LDS_STACK + 1][TRACE_BLOCK]; // + one scratch row for the branch-free pushes
  Leaf::prepare();
  const uint32_t tid = threadIdx.x;
  const uint32_t gthread = blockIdx.x * TRACE_BLOCK + tid;
  auto spill_col = [&]() -> uint2* { // see trace_loop.hip.h: formed where it is used, from an opaque copy of the thread index
    uint32_t g = gthread;
    asm volatile("" : "+v"(g));
    return (uint2*)P.spill + (size_t)g * P.spillDepth;
  };
  const QNode8* __restrict__ nodes = P.accel.nodes;
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
  TravRay<true> tr;
  WorkCounters wc; // the leaves' counting argument: never counted here
  float travFar = 0.f;
  uint32_t sp = 0, cur = REF_EMPTY, rayIdx = 0;
  uint32_t curInst = 0xFFFFFFFFu, hitInst = 0xFFFFFFFFu; // geomID of the instance being traversed / of the hit's instance
  // lane state bits (vector register, see RayState::hit): the lane owns a ray, its next event is a pop, it is inside an instance
  enum : uint32_t { ST_ACTIVE = 1u, ST_POP = 2u, ST_INSIDE = 4u };
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
          if (laneId == 0u) base = atomicAdd(&queues[qCur * TRACE_QUEUE_STRIDE], P.rayChunk);
          base = __builtin_amdgcn_readfirstlane(base);
          if (base < qLen) {
            poolNext = qLo + base;
            poolEnd = min(poolNext + P.rayChunk, qLo + qLen);
            break;
          }
          // drained: lane l reads head l, the ballot marks the queues that still have rays, take the next one cyclically after qCur
          const uint32_t head = __hip_atomic_load(&queues[laneId * TRACE_QUEUE_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
      const uint4 q3 = ((const uint4*)ip)[3];    // geomID, root, 0, (S << 24) | firstStep
      bool enter = true;
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
      if (!enter) st |= ST_POP; // singular interpolated transform: the ray does not enter, nothing is pushed
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
        if (cur == REF_EMPTY) st |= ST_POP; // no tree (the builder leaves such instances out)
      }
    }

    // ---- subdivision leaf inside an instance: run when enough lanes wait at one, or when nobody has node work -------------
    const bool atLeaf = st == (ST_ACTIVE | ST_INSIDE) && (cur & REF_LEAF);
    const uint64_t leafMask = __ballot(atLeaf);
    if (leafMask != 0ull) {
      const bool nodeWork = __ballot((st & ST_ACTIVE) && !(st & ST_POP) && !(cur & REF_LEAF)) != 0ull;
      if (((uint32_t)__popcll(leafMask) >= P.leafBatch || !nodeWork) && atLeaf) {
        // the leaf sets r.hit when IT finds a hit: cleared around the call so that such a hit takes the instance's id, whatever
        // its t (a hit at the t of the hit so far replaces it, as in the leaf's top-level kernel)
        const uint32_t had = r.hit;
        r.hit = 0u;
        if (Leaf::template intersect<OCCLUDED, false>(P, cur, r, wc, rayIdx)) {
          r.tfar = -RT_INF; // bvh_intersector1.cpp:198-201
          r.hit = 1u;
          sp = 0;           // any hit found: terminate this ray
        }
        if (!OCCLUDED && r.hit) hitInst = curInst; // instID: instance_intersector.cpp:57
        r.hit |= had;
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
          // the world-space ray is read again through the ray's index (org and dir are never written): six registers less across the loop
          RayState w;
          load_ray<VEC>((const char*)P.rays + (size_t)rayIdx * P.stride, w);
          r.ox = w.ox; r.oy = w.oy; r.oz = w.oz;
          r.dx = w.dx; r.dy = w.dy; r.dz = w.dz;
          tr.init(r);
          st &= ~ST_INSIDE;
          continue;
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
          else {
            if constexpr (Leaf::CONST_NG) { // the fork's dummy normal is not kept across the loop (trace_loop.hip.h)
              float one = 1.f, zero = 0.f;
              asm volatile("" : "+v"(one), "+v"(zero));
              r.ngx = one; r.ngy = zero; r.ngz = zero;
            }
            store_hit<VEC>(rp, r, hitInst);
          }
        }
        st = 0u;
      }
    }
  }
}

template <typename Leaf, bool OCCLUDED>
inline hipError_t launch_instance_subdiv_vec(const LaunchParams& p, hipStream_t stream)
{
  const bool vec = (p.stride % 16 == 0) && (((uintptr_t)p.rays) % 16 == 0);
  // persistent grid = what is resident at once for this instantiation, capped by the host's bound (which sized the spill area)
  static int occVec = 0, occGen = 0;
  int& occ = vec ? occVec : occGen;
  if (occ == 0) {
    hipError_t e = vec ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, trace_instance_subdiv_kernel<Leaf, OCCLUDED, true>, TRACE_BLOCK, 0)
                       : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, trace_instance_subdiv_kernel<Leaf, OCCLUDED, false>, TRACE_BLOCK, 0);
    if (e != hipSuccess || occ <= 0) occ = 1;
  }
  uint32_t blocks = (p.blocksPerCU ? std::min<uint32_t>(p.blocksPerCU, (uint32_t)occ) : (uint32_t)occ) * p.numCUs;
  if (blocks > p.gridBlocks) blocks = p.gridBlocks;
  if (vec) hipLaunchKernelGGL((trace_instance_subdiv_kernel<Leaf, OCCLUDED, true>), dim3(blocks), dim3(TRACE_BLOCK), 0, stream, p);
  else hipLaunchKernelGGL((trace_instance_subdiv_kernel<Leaf, OCCLUDED, false>), dim3(blocks), dim3(TRACE_BLOCK), 0, stream, p);
  return hipGetLastError();
}

template <typename Leaf> inline hipError_t launch_instance_subdiv(const LaunchParams& p, hipStream_t stream)
{
  return p.occluded ? launch_instance_subdiv_vec<Leaf, true>(p, stream) : launch_instance_subdiv_vec<Leaf, false>(p, stream);
}

} // namespace dev

hipError_t launch_trace_instance_subdiv(const LaunchParams& p, hipStream_t stream)
{
  if (p.counters) return hipErrorInvalidValue; // no instrumented twin (rt_trace.cpp refuses counted batches on scenes with instances)
  switch (p.accel.kind) {
  case ACCEL_INSTSUBDIV_GRID: return dev::launch_instance_subdiv<dev::GridCellLeaf>(p, stream);
  case ACCEL_INSTSUBDIV_CBVH_LEAF:
    switch (p.cbvhLevels) { // one kernel per compression level C = 1..5 of the instanced scenes
    case 1: return dev::launch_instance_subdiv<dev::CbvhLeaf<dev::MODE_LEAF, 1, false>>(p, stream);
    case 2: return dev::launch_instance_subdiv<dev::CbvhLeaf<dev::MODE_LEAF, 2, false>>(p, stream);
    case 3: return dev::launch_instance_subdiv<dev::CbvhLeaf<dev::MODE_LEAF, 3, false>>(p, stream);
    case 4: return dev::launch_instance_subdiv<dev::CbvhLeaf<dev::MODE_LEAF, 4, false>>(p, stream);
    case 5: return dev::launch_instance_subdiv<dev::CbvhLeaf<dev::MODE_LEAF, 5, false>>(p, stream);
    default: return hipErrorInvalidValue;
    }
  default: return hipErrorInvalidValue;
  }
}

} // namespace rtamd
