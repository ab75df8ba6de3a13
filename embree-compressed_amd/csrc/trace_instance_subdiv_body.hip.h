// The body of the subdivision two-level kernel (trace_instance_subdiv.hip, where it is described; trace_instance_subdiv_top_linear.hip),
// as text: it is included inside the braces of a __global__ function template that has the launch parameters `P`, the leaf type `Leaf` and
// the compile-time constants OCCLUDED, VEC and TOPMB in scope.  Text and not a function called from the kernels, as
// trace_instance_body.hip.h is and for its reason: the instruction streams of the 24 instantiations of trace_instance_subdiv.hip are held
// to what they were (tools/kernel_metadata.py --digest, docs/experiments.md).  No include guard: one inclusion per kernel.
// TOPMB (kinds ACCEL_INSTSUBDIV_TOP_LINEAR_*): the top-level tree is made of QNodeMB8s in the second section of the node buffer, indexed
// in 144-byte units; a lane outside an instance reads one and interpolates every plane at the ray's time, a lane inside an instance
// reads a QNode8 as in the other form.  Everything else is one text.
  static_assert(std::is_same<decltype(P), LaunchParams>::value, "trace_instance_subdiv_body.hip.h: `LaunchParams P` must be the kernel's parameter");
  static_assert(std::is_same<typename std::remove_const<decltype(OCCLUDED)>::type, bool>::value && std::is_same<typename std::remove_const<decltype(VEC)>::type, bool>::value &&
                    std::is_same<typename std::remove_const<decltype(TOPMB)>::type, bool>::value,
                "trace_instance_subdiv_body.hip.h: OCCLUDED, VEC and TOPMB must be bool constants in scope");
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
  float nodeTime = 0.f; // TOPMB: the ray's time clamped to [0, 1] (NaN: 0), at which the top-level planes are taken
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
            if (TOPMB) nodeTime = fminf(fmaxf(ray_time(P, rayIdx), 0.0f), 1.0f);
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
      // TOPMB: where the lane is says which node type `cur` names - a QNodeMB8 of the buffer indexed in 144-byte units outside an instance
      // (the top-level tree), a QNode8 inside one (the instanced scenes' trees)
      const bool mbNode = TOPMB && !(st & ST_INSIDE);
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
      if (!TOPMB) { // the loop of the swept form as it stands
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
        // TOPMB: every plane interpolated between the node's two plane blocks at nodeTime, by the formula of accel.h QNodeMB8 and of the
        // NODEMB form of trace_instance_body.hip.h.  A lane at a QNode8 (inside an instance) takes its only block for both ends:
        // fmaf(t, q - q, q) = q for the finite t, the planes of the swept form bit for bit, and all lanes of the wave run one instruction
        // stream (below mesh instances a branch around the timed decode was measured slower: docs/experiments.md "Linear node bounds below
        // an instance")
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
