// The body of the two-level traversal kernels, as text: it is included inside the braces of a __global__ function that has the launch
// parameters `P`, the kernel's form `FORM` (trace_instance.hip.h InstanceForm) and its leaf type `Leaf` in scope - a subdivision leaf
// (trace_instance_subdiv.hip.h) or MeshLeaves.  The units that include it are listed in trace_instance.hip.h; trace_instance.hip describes
// the mesh family, trace_instance_subdiv.hip the subdivision family.  The walk - setup, refill, node step, ranking, push, instance entry,
// pop, exit marker, store - is one text for both; they part in the leaf section, and in a few places marked SUBDIV.
// Text and not a function called from the kernels: through a function the compiler schedules the loads of the launch parameters
// differently, and the instruction streams of the instantiations are held to what they were (tools/kernel_metadata.py --digest,
// docs/experiments.md).  No include guard: one inclusion per kernel.  Everything else the text uses comes from the headers
// trace_instance.hip.h includes and from the TRACE_INST_* macros it defines; the text declares only locals of its own and ends with the
// traversal loop.
  static_assert(std::is_same<decltype(P), LaunchParams>::value, "trace_instance_body.hip.h: `LaunchParams P` must be the kernel's parameter");
  constexpr bool PLUECKER = FORM.PLUECKER, OCCLUDED = FORM.OCCLUDED, VEC = FORM.VEC, QUADS = FORM.QUADS, XFMB = FORM.XFMB, MESHMB = FORM.MESHMB;
  constexpr bool NODEMB = FORM.NODEMB, TOPMB = FORM.TOPMB, EXCL = FORM.EXCL, HAIR = FORM.HAIR, HAIRMB = FORM.HAIRMB, SUBDIV = FORM.SUBDIV;
  constexpr uint32_t FETCH = TRACE_INST_FETCH;
  constexpr uint32_t QFETCH = TRACE_INST_QUAD_FETCH;
  constexpr uint32_t TMFETCH = TRACE_INST_TRIMB_FETCH;
  constexpr uint32_t QMFETCH = TRACE_INST_QUADMB_FETCH;
  static_assert(!MESHMB || (QUADS && XFMB), "the MESHMB form carries the general layout: quads and instance steps");
  static_assert(!NODEMB || MESHMB || SUBDIV, "the NODEMB form of the mesh family is the MESHMB form over time-dependent nodes in the motion-blur trees");
  static_assert(!TOPMB || NODEMB, "the TOPMB form is the NODEMB form over a top-level tree of time-dependent nodes");
  // SUBDIV (trace_instance_subdiv.hip): an instanced scene is one tree - no pending-tree markers, no tree code in the lane state - over
  // swept boxes, its leaves are Leaf::intersect on the local ray, every instance may have time steps, and the traversal is the robust
  // one on both levels, as the subdivision accels run at top level.  Time-dependent nodes only at top level: NODEMB with TOPMB.
  static_assert(!SUBDIV || (XFMB && !PLUECKER && !QUADS && !MESHMB && !EXCL && !HAIR && NODEMB == TOPMB), "the SUBDIV forms: instance steps, one swept tree per scene, TOPMB or not");
  // EXCL (trace_instance_filter.hip, the re-traces of the host filter loop): in every leaf loop a candidate that passed its test is dropped
  // before the block's minimum selection when the ray's exclusion list names it - (curInst, geomID, primID, bits of t), instance_candidate_excluded
  // in trace_instance.hip.h.  P.exclOffsets is set for every launch of such a kernel and indexed by the ray's index in the batch.
  static_assert(!EXCL || !OCCLUDED, "the filter loop runs closest-hit launches only");
  // HAIR (trace_instance_hair.hip): an instanced scene may hold a curve and a line tree behind its four mesh trees (accel.h
  // InstanceSceneRecord); their leaves are CurveLeaf::intersect / LineLeaf::intersect on the local ray.  The swept MESHMB form only, and
  // no exclusion scan: filters beside instanced hair are refused at commit and at the call.
  static_assert(!HAIR || (MESHMB && !NODEMB && !TOPMB && !EXCL), "the HAIR form is the MESHMB form over swept boxes, without the exclusion scan");
  // HAIRMB (trace_instance_hair_mb.hip): the HAIR form with a motion-blur curve and a motion-blur line tree per scene, eight trees in all;
  // their leaves are CurveMBLeaf::intersect / LineMBLeaf::intersect (trace_curve_mb.hip.h, trace_line_mb.hip.h) on the local ray, their
  // nodes swept QNode8s like every node of the form
  static_assert(!HAIRMB || HAIR, "the HAIRMB form is the HAIR form with two more trees");
  constexpr bool ROBUST = SUBDIV || PLUECKER; // Pluecker <-> robust traversal, Moeller <-> fast traversal, on both levels
  __shared__ uint2 ldsStack[TRACE_LDS_STACK + 1][TRACE_BLOCK]; // + one scratch row for the branch-free pushes
  Leaf::prepare(); // SUBDIV: once per kernel (the cBVH decode tables in LDS); nothing for the others
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
  float nodeTime = 0.f; // NODEMB: the ray's time, clamped to [0, 1] (a NaN becomes 0), as in trace_loop.hip.h
  uint32_t sp = 0, cur = REF_EMPTY, rayIdx = 0;
  uint32_t curInst = 0xFFFFFFFFu, hitInst = 0xFFFFFFFFu; // geomID of the instance being traversed / of the hit's instance
  // lane state bits (vector register, see RayState::hit): the lane owns a ray, its next event is a pop, it is inside an instance,
  // it is in the instanced scene's quad tree (QUADS only).  MESHMB: two bits, the code of the tree it is in (accel.h INST_TREE_*);
  // HAIR: three, for the codes of the curve and the line tree.  SUBDIV: the first three bits only
  enum : uint32_t { ST_ACTIVE = 1u, ST_POP = 2u, ST_INSIDE = 4u, ST_QUADS = 8u, ST_TREE_SHIFT = 3u, ST_TREE = (HAIR ? 7u : 3u) << ST_TREE_SHIFT };
  static_assert((INST_TREE_QUAD << ST_TREE_SHIFT) == ST_QUADS, "the quad tree's code is the ST_QUADS bit");
  // NODEMB: bit 1 of the code says that the tree's nodes are QNodeMB8s; the bits are clear outside an instance
  enum : uint32_t { ST_TREE_MB = 2u << ST_TREE_SHIFT };
  static_assert(!(INST_TREE_TRI & 2u) && !(INST_TREE_QUAD & 2u) && (INST_TREE_TRIMB & 2u) && (INST_TREE_QUADMB & 2u), "bit 1 of a tree's code: a motion-blur tree");
  static_assert(!(INST_TREE_CURVE & 2u) && !(INST_TREE_LINE & 2u) && INST_TREE_CURVE < 8u && INST_TREE_LINE < 8u, "the hair trees' codes: three bits, bit 1 clear");
  static_assert((INST_TREE_CURVEMB & 2u) != 0u && (INST_TREE_LINEMB & 2u) != 0u && INST_TREE_CURVEMB < 8u && INST_TREE_LINEMB < 8u, "the moving-hair trees' codes: three bits, bit 1 set");
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
            if (NODEMB) nodeTime = fminf(fmaxf(ray_time(P, rayIdx), 0.0f), 1.0f);
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
      // NODEMB: the lane's tree says which node type `cur` names - a QNodeMB8 of the buffer indexed in 144-byte units while the lane is in
      // a motion-blur tree of an instanced scene, a QNode8 everywhere else (top level, static trees).  TOPMB (kinds ACCEL_INSTTOP_LINEAR_*):
      // the top-level tree is made of QNodeMB8s too - a lane outside an instance reads one, and enters a moving instance only where its
      // box is at the ray's time.  SUBDIV has no tree codes: with TOPMB a QNodeMB8 outside an instance, a QNode8 inside one
      const bool mbNode = NODEMB && ((MESHMB && (st & ST_TREE_MB) != 0u) || (TOPMB && !(st & ST_INSIDE)));
      const uint4* np = mbNode ? (const uint4*)((const QNodeMB8*)nodes + cur) : (const uint4*)(nodes + cur);
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
      if (!NODEMB) { // the loop of the other forms as it stands (shared with the NODEMB form through a lambda it left their instruction streams changed)
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
      } else {
        // NODEMB: every plane interpolated between the node's two plane blocks at nodeTime, by the formula of accel.h QNodeMB8 and of
        // trace_loop.hip.h's plane().  A lane at a QNode8 takes its only block for both: fmaf(t, q - q, q) = q for the finite t, the
        // planes of the other forms bit for bit, and all lanes of the wave run one instruction stream (a branch around the timed decode
        // was measured slower and spills at these wave bounds: docs/experiments.md "Linear node bounds below an instance")
        uint4 n6 = n3, n7 = n4, n8 = n5;
        if (mbNode) { n6 = np[6]; n7 = np[7]; n8 = np[8]; }
        const uint32_t rnx0 = ngx ? n6.z : n6.x, rnx1 = ngx ? n6.w : n6.y;
        const uint32_t rfx0 = ngx ? n6.x : n6.z, rfx1 = ngx ? n6.y : n6.w;
        const uint32_t rny0 = ngy ? n7.z : n7.x, rny1 = ngy ? n7.w : n7.y;
        const uint32_t rfy0 = ngy ? n7.x : n7.z, rfy1 = ngy ? n7.y : n7.w;
        const uint32_t rnz0 = ngz ? n8.z : n8.x, rnz1 = ngz ? n8.w : n8.y;
        const uint32_t rfz0 = ngz ? n8.x : n8.z, rfz1 = ngz ? n8.y : n8.w;
        auto plane = [&](uint32_t w0, uint32_t w1, int kk, float s, float o) -> float {
          return madd(madd(nodeTime, q2f(w1, kk) - q2f(w0, kk), q2f(w0, kk)), s, o);
        };
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int kk = k & 3;
          const float npx = plane(k < 4 ? nx0 : nx1, k < 4 ? rnx0 : rnx1, kk, sx, ox);
          const float npy = plane(k < 4 ? ny0 : ny1, k < 4 ? rny0 : rny1, kk, sy, oy);
          const float npz = plane(k < 4 ? nz0 : nz1, k < 4 ? rnz0 : rnz1, kk, sz, oz);
          const float fpx = plane(k < 4 ? fx0 : fx1, k < 4 ? rfx0 : rfx1, kk, sx, ox);
          const float fpy = plane(k < 4 ? fy0 : fy1, k < 4 ? rfy0 : rfy1, kk, sy, oy);
          const float fpz = plane(k < 4 ? fz0 : fz1, k < 4 ? rfz0 : rfz1, kk, sz, oz);
          const float tN = fmaxf(tr.nearT(npx, npy, npz), tr.tnear);
          const float tF = fminf(tr.farT(fpx, fpy, fpz), travFar);
          const bool h = (tN <= tF) & (cref[k] != REF_EMPTY);
          dist[k] = h ? __float_as_uint(tN) : (0x7FFFFFF8u + (uint32_t)k); // sentinels as above
          mask |= h ? (1u << k) : 0u;
        }
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
      if (MESHMB) {
        // q3.y names the scene's InstanceSceneRecord: its four roots in visiting order (triangles, motion-blur triangles, quads,
        // motion-blur quads).  Walking them backwards, every tree that has one before it is stacked as a marker with its root in the
        // distance word; the lane starts in the first tree the scene has.
        // HAIR: six roots - the curve and the line root lead the record's second dwordx4 and are visited last, curves before lines
        // HAIRMB: eight - all four words of that dwordx4, visited in Scene's slot order (curves, motion-blur curves, lines, motion-blur
        // lines), which is not the word order (curve, line, motion-blur curve, motion-blur line)
        const uint4 sr = ((const uint4*)(insts + q3.y))[0];
        constexpr int TREES = HAIRMB ? 8 : HAIR ? 6 : 4;
        uint32_t roots[TREES] = {sr.x, sr.y, sr.z, sr.w};
        uint32_t codes[TREES] = {INST_TREE_TRI, INST_TREE_TRIMB, INST_TREE_QUAD, INST_TREE_QUADMB};
        if constexpr (HAIRMB) {
          const uint4 sh = ((const uint4*)(insts + q3.y))[1];
          roots[4] = sh.x; roots[5] = sh.z; roots[6] = sh.y; roots[7] = sh.w;
          codes[4] = INST_TREE_CURVE; codes[5] = INST_TREE_CURVEMB; codes[6] = INST_TREE_LINE; codes[7] = INST_TREE_LINEMB;
        } else if (HAIR) {
          const uint4 sh = ((const uint4*)(insts + q3.y))[1];
          roots[TREES - 2] = sh.x; roots[TREES - 1] = sh.y;
          codes[TREES - 2] = INST_TREE_CURVE; codes[TREES - 1] = INST_TREE_LINE;
        }
        uint32_t nextRoot = REF_EMPTY, nextCode = 0u;
#pragma unroll
        for (int i = TREES - 1; i >= 0; i--) {
          if (roots[i] != REF_EMPTY) {
            if (nextRoot != REF_EMPTY) {
              push(REF_INST_TREE(nextCode), nextRoot, sp);
              sp++;
            }
            nextRoot = roots[i];
            nextCode = codes[i];
          }
        }
        cur = nextRoot;
        st |= nextCode << ST_TREE_SHIFT;
        if (cur == REF_EMPTY) st |= ST_POP; // no tree (the builder leaves such instances out)
      } else if (QUADS) { // q3.z: the quad root (InstanceRecord::pad[0]), REF_EMPTY without quads; q3.y is REF_EMPTY without triangles
        if (q3.z != REF_EMPTY) {
          if (cur != REF_EMPTY) { // triangles first: the quad tree waits on the stack, its root in the distance word
            push(REF_INST_QUADS, q3.z, sp);
            sp++;
          } else {
            cur = q3.z;
            st |= ST_QUADS;
          }
        } else if (cur == REF_EMPTY) st |= ST_POP; // neither tree (the builder leaves such instances out)
      } else if (SUBDIV) {
        if (cur == REF_EMPTY) st |= ST_POP; // no tree (the builder leaves such instances out)
      }
      }
    }

    // ---- leaf inside an instance: run when enough lanes wait at one, or when nobody has node work ----------------------
    const bool atLeaf = (MESHMB ? st & ~ST_TREE : QUADS ? st & ~ST_QUADS : st) == (ST_ACTIVE | ST_INSIDE) && (cur & REF_LEAF);
    const uint64_t leafMask = __ballot(atLeaf);
    if (leafMask != 0ull) {
      const bool nodeWork = __ballot((st & ST_ACTIVE) && !(st & ST_POP) && !(cur & REF_LEAF)) != 0ull;
      if (((uint32_t)__popcll(leafMask) >= P.leafBatch || !nodeWork) && atLeaf) {
        uint32_t first, count;
        leaf_range(cur, first, count);
        bool occl = false;
        if (SUBDIV) {
          // the subdivision family's leaf.  It sets r.hit when IT finds a hit: cleared around the call so that such a hit takes the
          // instance's id, whatever its t (a hit at the t of the hit so far replaces it, as in the leaf's top-level kernel).  It ends an
          // occluded ray itself and not through `occl` like the HAIR branch below, whose statement order moves 12 of these kernels' digests
          WorkCounters wc; // the leaf's counting argument: never counted here.  Declared where it is used, here and below: one declaration
                           // at function level changes the instruction streams of the mesh family's closest-hit kernels
          const uint32_t had = r.hit;
          r.hit = 0u;
          if (Leaf::template intersect<OCCLUDED, false>(P, cur, r, wc, rayIdx)) {
            r.tfar = -RT_INF; // bvh_intersector1.cpp:198-201
            r.hit = 1u;
            sp = 0;           // any hit found: terminate this ray
          }
          if (!OCCLUDED && r.hit) hitInst = curInst; // instID: instance_intersector.cpp:57
          r.hit |= had;
        } else if (HAIR && ((st & ST_TREE) == (INST_TREE_CURVE << ST_TREE_SHIFT) || (st & ST_TREE) == (INST_TREE_LINE << ST_TREE_SHIFT) ||
                            (HAIRMB && ((st & ST_TREE) == (INST_TREE_CURVEMB << ST_TREE_SHIFT) || (st & ST_TREE) == (INST_TREE_LINEMB << ST_TREE_SHIFT))))) {
          // the leaves of the top-level curve and line accels (trace_curve.hip.h, trace_line.hip.h) on the LOCAL ray: the ray's own space
          // depends on the length of the local direction, as in the reference, which hands the local ray to the instanced scene's
          // intersectors unchanged.  The leaf references are rebased so that `blobs` is ONE array of CurveRecords / LineRecords, which is how
          // the two leaves index it.  r.hit is cleared around the call: a hit the leaf commits - also one at a t equal to the hit of an
          // earlier instance - is this instance's.  HAIRMB: the same for the two motion-blur leaves, which read the ray's time through the
          // ray's index (ray_time: the same value in world and local space) and index `blobs` as one array of CurveMBRecords / LineMBRecords
          WorkCounters wc;
          const uint32_t had = r.hit;
          r.hit = 0u;
          if ((st & ST_TREE) == (INST_TREE_CURVE << ST_TREE_SHIFT)) occl = CurveLeaf::intersect<OCCLUDED, false>(P, cur, r, wc, rayIdx);
          else if (HAIRMB && (st & ST_TREE) == (INST_TREE_CURVEMB << ST_TREE_SHIFT)) occl = CurveMBLeaf::intersect<OCCLUDED, false>(P, cur, r, wc, rayIdx);
          else if (HAIRMB && (st & ST_TREE) == (INST_TREE_LINEMB << ST_TREE_SHIFT)) occl = LineMBLeaf::intersect<OCCLUDED, false>(P, cur, r, wc, rayIdx);
          else occl = LineLeaf::intersect<OCCLUDED, false>(P, cur, r, wc, rayIdx);
          if (r.hit) hitInst = curInst; // instID: instance_intersector.cpp:57
          r.hit |= had;
        } else if (MESHMB && (st & ST_TREE) == (INST_TREE_TRIMB << ST_TREE_SHIFT)) {
          // the block loop of TriMBLeaf::intersect (trace_tri_mb.hip), written out and not called like the static leaves below: with all four
          // leaves called, moving two-step triangles below instances trace 3.5 to 3.8 % slower (Pluecker) and 1.2 to 1.5 % (Moeller); with this
          // loop alone written out the any-hit Moeller HAIR kernels spill 2 VGPRs; with the quad one too nothing spills and the rates are
          // the parent's (docs/experiments.md, "Mesh leaves below an instance").  A record is tested only when its segment is the ray's itime, on the
          // vertices interpolated to the ray's time; Moeller forms its edges from them (e1 = a - b, e2 = c - a)
          const TriMBRecord* __restrict__ mrecs = (const TriMBRecord*)P.accel.blobs; // the leaf references are rebased to the section's start
          const float time = ray_time(P, rayIdx); // the same value in world and local space
          for (uint32_t b = 0; b < count && !occl; b += 4) {
            const float tfarBlock = r.tfar; // all records of a block see the tfar at block entry
            const uint32_t nb = min(4u, count - b);
            bool found = false;
            TriHit best;
            uint32_t bestPrim = 0, bestGeom = 0;
            best.t = RT_INF;
            for (uint32_t g = 0; g < nb && !occl; g += TMFETCH) {
              // slots past the leaf end re-read the last record and are skipped below
              float4 A0[TMFETCH], B0[TMFETCH], C0[TMFETCH], A1[TMFETCH], B1[TMFETCH], C1[TMFETCH];
#pragma unroll
              for (uint32_t k = 0; k < TMFETCH; k++) {
                const float4* tp = (const float4*)(mrecs + first + b + min(g + k, nb - 1u));
                A0[k] = tp[0]; B0[k] = tp[1]; C0[k] = tp[2]; A1[k] = tp[3]; B1[k] = tp[4]; C1[k] = tp[5];
              }
#pragma unroll
              for (uint32_t k = 0; k < TMFETCH; k++) {
                if (g + k >= nb) break;
                float f;
                if (!time_segment(time, __float_as_uint(C0[k].w), __float_as_uint(A1[k].w), f)) continue; // another segment's record
                const float4 a = lerp_vertex(A0[k], A1[k], f), bb = lerp_vertex(B0[k], B1[k], f), c = lerp_vertex(C0[k], C1[k], f);
                TriHit h;
                bool ok;
                if (PLUECKER) ok = pluecker(r, a, bb, c, tfarBlock, h);
                else ok = moeller(r, a, make_float4(a.x - bb.x, a.y - bb.y, a.z - bb.z, 0.0f), make_float4(c.x - a.x, c.y - a.y, c.z - a.z, 0.0f), tfarBlock, h);
                if (EXCL) ok = ok && !instance_candidate_excluded(P, rayIdx, curInst, __float_as_uint(A0[k].w), __float_as_uint(B0[k].w), h.t);
                if (ok) {
                  if (OCCLUDED) { occl = true; break; } // Occluded1EpilogM: any valid lane
                  if (!found || h.t < best.t) { // select_min over valid lanes, lowest lane wins ties
                    best = h;
                    bestGeom = __float_as_uint(A0[k].w);
                    bestPrim = __float_as_uint(B0[k].w);
                    found = true;
                  }
                }
              }
            }
            if (found) { // Intersect1EpilogM; instID: instance_intersector.cpp:57
              commit_hit(r, best, bestGeom, bestPrim);
              hitInst = curInst;
            }
          }
        } else if (MESHMB && (st & ST_TREE) == (INST_TREE_QUADMB << ST_TREE_SHIFT)) {
          // the block loop of QuadMBLeaf::intersect (trace_quad_mb.hip), written out for the reason given above: 8 candidates per block of 4 records (A = (v0, v1, v3) in lanes
          // 0-3, B = (v2, v1, v3) in lanes 4-7) on the interpolated vertices; records of another segment take no part but keep their lane
          const QuadMBRecord* __restrict__ mrecs = (const QuadMBRecord*)P.accel.blobs; // the leaf references are rebased to the section's start
          const float time = ray_time(P, rayIdx);
          for (uint32_t b = 0; b < count && !occl; b += 4) {
            const float tfarBlock = r.tfar; // all 8 candidates of a block see the tfar at block entry
            const uint32_t nb = min(4u, count - b);
            bool found = false;
            TriHit best;
            uint32_t bestLane = 8u, bestPrim = 0, bestGeom = 0;
            best.t = RT_INF;
            for (uint32_t g = 0; g < nb && !occl; g += QMFETCH) {
              float4 V[QMFETCH][8];
#pragma unroll
              for (uint32_t k = 0; k < QMFETCH; k++) {
                const float4* qp = (const float4*)(mrecs + first + b + min(g + k, nb - 1u));
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) V[k][j] = qp[j];
              }
#pragma unroll
              for (uint32_t k = 0; k < QMFETCH; k++) {
                if (g + k >= nb || occl) break;
                float f;
                if (!time_segment(time, __float_as_uint(V[k][5].w), __float_as_uint(V[k][7].w), f)) continue; // another segment's record
                const uint32_t pid = __float_as_uint(V[k][1].w), gid = __float_as_uint(V[k][3].w);
                const float4 v1 = lerp_vertex(V[k][1], V[k][5], f), v3 = lerp_vertex(V[k][3], V[k][7], f);
#pragma unroll
                for (uint32_t half = 0; half < 2; half++) { // A then B of this quad (lanes g+k and 4+g+k)
                  const float4 v02 = half ? lerp_vertex(V[k][2], V[k][6], f) : lerp_vertex(V[k][0], V[k][4], f);
                  TriHit h;
                  bool ok = PLUECKER ? pluecker_quad(r, v02, v1, v3, tfarBlock, half != 0u, h) : moeller_quad(r, v02, v1, v3, tfarBlock, half != 0u, h);
                  if (EXCL) ok = ok && !instance_candidate_excluded(P, rayIdx, curInst, gid, pid, h.t);
                  if (ok) {
                    if (OCCLUDED) { occl = true; break; } // Occluded1EpilogM: any valid lane
                    const uint32_t lane = half * 4u + g + k; // select_min over the 8 lanes, lowest lane wins ties
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
            if (found) { // Intersect1EpilogM; instID: instance_intersector.cpp:57
              commit_hit(r, best, bestGeom, bestPrim);
              hitInst = curInst;
            }
          }
        } else if (QUADS) {
          // the leaves of the top-level static mesh accels (trace_tri.hip.h, trace_quad.hip.h) on the local ray, with this kernel's fetch
          // widths and, in the EXCL form, its exclusion scan; `blobs` is ONE array of QuadRecords (rebased references).  r.hit as above
          WorkCounters wc;
          const uint32_t had = r.hit;
          r.hit = 0u;
          const auto excl = [&](uint32_t geomID, uint32_t primID, float t) -> bool { return EXCL && instance_candidate_excluded(P, rayIdx, curInst, geomID, primID, t); };
          if (MESHMB ? (st & ST_TREE) == ST_QUADS : (st & ST_QUADS) != 0u) occl = QuadLeaf<PLUECKER>::template intersect<OCCLUDED, false, QFETCH>(P, cur, r, wc, rayIdx, excl);
          else occl = TriLeaf<PLUECKER>::template intersect<OCCLUDED, false, FETCH>(P, cur, r, wc, rayIdx, excl);
          if (r.hit) hitInst = curInst; // instID: instance_intersector.cpp:57
          r.hit |= had;
        } else {
          // QUADS = false: the block loop of TriLeaf::intersect (trace_tri.hip.h; intersector_iterators.h:32-36, epilog intersector_epilog.h:
          // 226-307 / :388-450) written out.  Through the call above these forms' closest-hit Pluecker kernels, at 128 VGPRs, spill 2 where
          // they have none, in twelve shapes of the call site; with this loop in the other forms too, Moeller QUADS and HAIR kernels spill
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
                bool ok = PLUECKER ? pluecker(r, A[k], B[k], C[k], tfarBlock, h) : moeller(r, A[k], B[k], C[k], tfarBlock, h);
                if (EXCL) ok = ok && !instance_candidate_excluded(P, rayIdx, curInst, __float_as_uint(A[k].w), __float_as_uint(B[k].w), h.t);
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
          st &= MESHMB ? ~(ST_INSIDE | ST_TREE) : QUADS ? ~(ST_INSIDE | ST_QUADS) : ~ST_INSIDE;
          continue;
        }
        if (MESHMB) {
          if (e.x - REF_INST_TREE(1u) < (HAIRMB ? 7u : HAIR ? 5u : 3u)) { // the tree before is done: on to the pending tree whose marker this is; before the distance cull
            st = (st & ~ST_TREE) | ((e.x & (HAIR ? 7u : 3u)) << ST_TREE_SHIFT);
            cur = e.y;
            break;
          }
        } else if (QUADS && e.x == REF_INST_QUADS) { // the triangle tree is done: on to the instanced scene's quad tree; before the distance cull
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
          else {
            if constexpr (SUBDIV && Leaf::CONST_NG) { // the fork's dummy normal is not kept across the loop (trace_loop.hip.h)
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
