// Batches with filter callbacks: the host filter loop over exclusion-list re-traces.
#include "rt_trace.h"
#include "rt_excl_list.h"

namespace rtamd {

// ---- filter callbacks (row f3) -----------------------------------------------------------------------------------------
// Filter functions are host function pointers (intersector_epilog.h:251-291, filter.h:27-130): the device cannot call
// them.  Two-phase scheme: the kernel finds the closest candidate of every ray; the host runs the geometry's filter and
// then the context filter on it with the reference's argument protocol (ray.tfar = candidate distance, N = 1); an
// accepted candidate is the ray's result; a rejected one is put on the ray's exclusion list and the ray is traced again
// (only those rays, compacted), the kernel skipping listed candidates, until every ray has an accepted hit or none.
// For pure accept/reject filters this is the reference's result: rejected candidates never shorten the ray there either,
// so the closest accepted candidate wins.  The callbacks see the candidates of a ray in order of distance instead of
// traversal order, each at most once.  Occlusion filters run the same loop on closest candidates (any accepted candidate
// = occluded).
// Subdivision geometry (round 2):
//  * eager grid cells (GridSOAIntersector1 -> Intersect1EpilogMU / Occluded1EpilogMU, grid_soa_intersector1.h:61,83,
//    intersector_epilog.h:460-600: every triangle of a patch is offered to the filter on its own, with the PATCH's geomID / primID):
//    a candidate is identified by (geomID, primID, bits of t) - kernels are deterministic, the same triangle gives the same t
//    when the ray is traced again.  Two triangles of one patch hit at a bit-identical distance (a ray through their shared edge)
//    are rejected together, where the reference would offer both.
//  * quads (QuadMvIntersector1*<4,true>, filter = true) offer each triangle with the QUAD's geomID / primID: identified like grid cells
//    by (geomID, primID, bits of t); a ray through the diagonal v1-v3 hits both triangles at one t, and rejecting one rejects both.
//  * line segments (LineMiIntersector1<4,4,true>) offer one candidate per segment: identified by (geomID, primID) and, as the shared scan
//    compares it too, the bits of t.  Line segments with time steps (LineMiMBIntersector1) likewise, in a list of their own.
//  * flat Bezier / B-spline curves (Ribbon1Intersector1 with Intersect1EpilogMU) offer one candidate per ribbon quad, all with the curve's
//    geomID / primID: identified by (geomID, primID, bits of t), in a list of their own.
//  * the fork's compressed modes never call a filter: CompressedBVHIntersector1::intersect writes the hit itself and occluded()
//    is a stub (compressed.h:454-756, no runIntersectionFilter1 anywhere in compressed*.h).  Hits on such an accel are accepted
//    without a callback, geometry and context filter alike; for any-hit queries the stub pass runs first, unfiltered.
// Meshes below an instance (device config inst_filters=1; without it such filters are refused at commit / at the call and a hit on an
// instance is accepted as it is):
//  * a hit with hit.instID[0] != the context's value lies below the instance s->geometries[hit.instID[0]]; its geometry is
//    instScene->geometries[hit.geomID].  The callbacks run in the reference's order (instance_intersector.cpp:51-62 traces the instanced
//    scene with context->instID[0] = the instance, so the geometry's filter and then the context filter run down there): the instanced
//    geometry's intersect / occluded filter with THAT geometry's user pointer, then the context filter if the lane is still valid.  Both
//    get the caller's own context object (applications derive from RTCIntersectContext) with instID[0] = the instance's geomID for the
//    duration of the callbacks.
//  * a candidate is (instance geomID, geomID, primID, bits of t) for every leaf type - a list of its own (Scene::INST) whose flattened
//    entries carry two words, t and the instance (trace.h); the re-trace of the instance accel runs the EXCL form of the two-level
//    kernel (trace_instance_filter.hip).  t tells a quad's two triangles apart (the diagonal: as above) and a motion-blur record from
//    its sibling; the instance tells two instances of one scene under one transform apart.
//  * instances of subdivision scenes (Scene::instSubdivAccel): no filter can be set below them and a context filter is refused on such a
//    top scene, so their hits stay accepted without a callback.
static const unsigned FILTER_MAX_ROUNDS = 256;

// The candidates the callbacks rejected on one accel, and their flattened form for the active rays of a round (rt_excl_list.h), with the upload.
struct ExclList : ExclListHost
{
  static_assert(sizeof(Pair) == sizeof(uint2), "ExclListHost::Pair is a device uint2");
  // into deviceBytes() bytes at D; an empty list is not uploaded and its launch gets no exclusion pointers
  LaunchExtras upload(char* D, hipStream_t stream) const
  {
    LaunchExtras x;
    if (pairs.empty()) return x;
    char* dPairs = D + a16(offBytes());
    char* dT = dPairs + a16(pairBytes());
    HIP_CHECK(hipMemcpyAsync(D, off.data(), offBytes(), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(dPairs, pairs.data(), pairBytes(), hipMemcpyHostToDevice, stream));
    if (!tbits.empty()) HIP_CHECK(hipMemcpyAsync(dT, tbits.data(), tBytes(), hipMemcpyHostToDevice, stream));
    x.exclOffsets = (const uint32_t*)D;
    x.exclPairs = (const uint2*)dPairs;
    x.exclT = tbits.empty() ? nullptr : (const uint32_t*)dT;
    return x;
  }
};

void trace_filtered(Scene* s, void* rays, uint32_t M, size_t byteStride, bool occluded, const RTCIntersectContext* callerCtx)
{
  Device* dev = s->device;
  RTCIntersectContext localCtx;
  // the callbacks get the caller's own context object (applications derive from RTCIntersectContext: a copy would lose their fields); the
  // only word written through it is instID[0] around the callbacks of a hit below an instance, put back before the call returns
  RTCIntersectContext* ctx = const_cast<RTCIntersectContext*>(callerCtx);
  if (!ctx) { memset(&localCtx, 0, sizeof(localCtx)); localCtx.instID[0] = RTC_INVALID_GEOMETRY_ID; ctx = &localCtx; }
  const uint32_t instID = ctx->instID[0];
  const uint32_t recIn = occluded ? (uint32_t)sizeof(RTCRay) : (uint32_t)sizeof(RTCRayHit);
  const bool forkAccel = s->subdivAccel.traceable() && s->subdivAccel.kind != ACCEL_GRIDSOA; // no filter calls on these (see above)
  std::lock_guard<std::mutex> lock(dev->launchMutex);
  // the host filter loop runs on the first shard (its rounds are latency bound, not throughput bound)
  Device::GpuShard& sh = dev->primary();
  sh.use();

  // the caller's records, on the host
  const bool devPtr = is_device_pointer(rays);
  const size_t span = (size_t)(M - 1) * byteStride + recIn;
  std::vector<char> mirror;
  char* src = (char*)rays;
  if (devPtr) {
    mirror.resize(span);
    HIP_CHECK(hipMemcpyAsync(mirror.data(), rays, span, hipMemcpyDeviceToHost, sh.stream));
    HIP_CHECK(hipStreamSynchronize(sh.stream));
    src = mirror.data();
  }
  std::vector<RTCRayHit> W(M);
  std::vector<uint32_t> act;
  act.reserve(M);
  for (uint32_t i = 0; i < M; i++) {
    memcpy(&W[i].ray, src + (size_t)i * byteStride, sizeof(RTCRay));
    if (occluded) {
      memset(&W[i].hit, 0, sizeof(RTCHit));
      W[i].hit.geomID = W[i].hit.primID = W[i].hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
    } else
      memcpy(&W[i].hit, src + (size_t)i * byteStride + sizeof(RTCRay), sizeof(RTCHit));
    if (W[i].ray.tnear <= W[i].ray.tfar && !(occluded && W[i].ray.tfar < 0.0f)) act.push_back(i);
  }
  if (occluded && forkAccel && !act.empty()) {
    // the stub any-hit pass of the fork's accel, unfiltered; the filter loop below then only sees the triangle accel
    const uint32_t K = (uint32_t)act.size();
    const size_t bytes = (size_t)K * sizeof(RTCRay);
    sh.ensureStaging(bytes);
    RTCRay* h = (RTCRay*)sh.stageHost;
    for (uint32_t k = 0; k < K; k++) h[k] = W[act[k]].ray;
    HIP_CHECK(hipMemcpyAsync(sh.stageDev, h, bytes, hipMemcpyHostToDevice, sh.stream));
    launch_on(s, s->subdivAccel, 0, Batch{sh.stageDev, K, (uint32_t)sizeof(RTCRay), true, false, instID, nullptr});
    HIP_CHECK(hipMemcpyAsync(h, sh.stageDev, bytes, hipMemcpyDeviceToHost, sh.stream));
    HIP_CHECK(hipStreamSynchronize(sh.stream));
    std::vector<uint32_t> rest;
    for (uint32_t k = 0; k < K; k++) {
      if (h[k].tfar < 0.0f) W[act[k]].ray.tfar = -std::numeric_limits<float>::infinity();
      else rest.push_back(act[k]);
    }
    act.swap(rest);
  }
  ExclList excl[Scene::NUM_ACCELS];
  for (ExclList& e : excl) e.perRay.resize(M);
  for (const SlotRow& r : SCENE_SLOTS) { excl[r.slot].keyedByT = r.keyedByT; excl[r.slot].withInst = r.withInst; } // why each list is keyed as it is: SCENE_SLOTS
  std::vector<uint32_t> next;
  void* dExcl = nullptr;
  size_t dExclBytes = 0;
  auto freeExcl = [&]() { if (dExcl) hipFree(dExcl); dExcl = nullptr; };
  try {
    for (unsigned round = 0; !act.empty() && round < FILTER_MAX_ROUNDS; round++) {
      const uint32_t K = (uint32_t)act.size();
      const size_t bytes = (size_t)K * sizeof(RTCRayHit);
      sh.ensureStaging(bytes);
      RTCRayHit* h = (RTCRayHit*)sh.stageHost;
      for (uint32_t k = 0; k < K; k++) h[k] = W[act[k]];
      size_t need = 0, listed = 0;
      for (ExclList& e : excl) {
        e.flatten(act);
        need += e.deviceBytes();
        listed += e.pairs.size();
      }
      LaunchExtras extras[Scene::NUM_ACCELS];
      if (listed) {
        if (need > dExclBytes) {
          HIP_CHECK(hipStreamSynchronize(sh.stream));
          freeExcl();
          dExclBytes = need * 2;
          HIP_CHECK(hipMalloc(&dExcl, dExclBytes));
        }
        char* D = (char*)dExcl;
        for (size_t i = 0; i < Scene::NUM_ACCELS; i++) {
          extras[i] = excl[i].upload(D, sh.stream);
          D += excl[i].deviceBytes();
        }
      }
      HIP_CHECK(hipMemcpyAsync(sh.stageDev, h, bytes, hipMemcpyHostToDevice, sh.stream));
      // (any-hit queries on a fork accel: its stub pass above was the subdivision launch)
      trace_accels(s, 0, Batch{sh.stageDev, K, (uint32_t)sizeof(RTCRayHit), false, false, instID, nullptr}, extras, occluded && forkAccel ? &s->subdivAccel : nullptr);
      HIP_CHECK(hipMemcpyAsync(h, sh.stageDev, bytes, hipMemcpyDeviceToHost, sh.stream));
      HIP_CHECK(hipStreamSynchronize(sh.stream));
      next.clear();
      for (uint32_t k = 0; k < K; k++) {
        const uint32_t i = act[k];
        const RTCRayHit& got = h[k];
        const bool found = got.hit.geomID != RTC_INVALID_GEOMETRY_ID &&
                           (got.ray.tfar != W[i].ray.tfar || got.hit.primID != W[i].hit.primID || got.hit.geomID != W[i].hit.geomID);
        if (!found) continue; // miss: the caller's record stays as it is
        // a hit inside an instance names a geometry of the INSTANCED scene and carries the instance's geomID in instID, every other hit
        // the context's value.  Without inst_filters=1 no filter applies to it (geometry filters inside instanced scenes are refused at
        // commit, context filters on scenes with instances at the call): accepted as it is.  With the key, a hit below a MESH instance is
        // resolved through the instance to the instanced scene's geometry, whose filter and user pointer the callbacks get; hits below an
        // instance of a subdivision scene stay unfiltered (no filter can be set there, and the call refuses a context filter).
        const bool onInstance = s->hasInstances() && got.hit.instID[0] != instID;
        Geometry* geo = !onInstance && got.hit.geomID < s->geometries.size() ? s->geometries[got.hit.geomID] : nullptr;
        bool belowMeshInstance = false;
        if (onInstance && dev->inst_filters && got.hit.instID[0] < s->geometries.size()) {
          const Geometry* inst = s->geometries[got.hit.instID[0]];
          const Scene* o = inst && inst->type == RTC_GEOMETRY_TYPE_INSTANCE ? inst->instScene : nullptr;
          Geometry* og = o && got.hit.geomID < o->geometries.size() ? o->geometries[got.hit.geomID] : nullptr;
          if (og && (og->type == RTC_GEOMETRY_TYPE_TRIANGLE || og->type == RTC_GEOMETRY_TYPE_QUAD)) {
            geo = og;
            belowMeshInstance = true;
          }
        }
        const bool onSubdiv = geo && geo->type == RTC_GEOMETRY_TYPE_SUBDIVISION;
        const bool unfiltered = onSubdiv && forkAccel;
        RTCFilterFunctionN fn = geo && !unfiltered ? (occluded ? geo->occludedFilter : geo->intersectFilter) : nullptr;
        RTCFilterFunctionN cfn = unfiltered || (onInstance && !belowMeshInstance) ? nullptr : ctx->filter;
        bool accepted = true;
        RTCRayHit cand = W[i];
        cand.ray.tfar = got.ray.tfar; // filter.h / intersector_epilog.h:277-279: the callback sees tfar = candidate distance
        RTCHit hit = got.hit;
        if (fn || cfn) {
          int mask = -1;
          RTCFilterFunctionNArguments a;
          a.valid = &mask;
          a.geometryUserPtr = geo ? geo->userPtr : nullptr;
          a.context = ctx;
          a.ray = (RTCRayN*)&cand.ray;
          a.hit = (RTCHitN*)&hit;
          a.N = 1;
          // below an instance the context names the instance while the callbacks run (instance_intersector.cpp:57-60).  The reference
          // writes -1 back, which is what a top-level call held there; here the caller's value is put back, so that the hits of later
          // rounds that are not on an instance (hit.instID = the context's value) stay right whatever the caller passed.
          if (belowMeshInstance) ctx->instID[0] = got.hit.instID[0];
          if (fn) fn(&a);
          if (mask != 0 && cfn) cfn(&a);
          if (belowMeshInstance) ctx->instID[0] = instID;
          accepted = mask != 0;
        }
        if (accepted) {
          if (occluded) W[i].ray.tfar = -std::numeric_limits<float>::infinity();
          else { W[i].ray = cand.ray; W[i].hit = hit; } // copyHitToRay
        } else {
          uint32_t tb;
          memcpy(&tb, &got.ray.tfar, 4);
          const size_t list = belowMeshInstance ? Scene::INST : (geo ? slot_of(geo) : Scene::TRI); // (a hit on no geometry of this scene: the triangles' list, as ever)
          excl[list].perRay[i].push_back(ExclList::Rejected{got.hit.geomID, got.hit.primID, tb, got.hit.instID[0]});
          next.push_back(i);
        }
      }
      act.swap(next);
    }
  } catch (...) {
    freeExcl();
    throw;
  }
  freeExcl();
  // outputs: tfar, and the hit for rtcIntersect
  scatter_outputs(src, byteStride, W.data(), (uint32_t)sizeof(RTCRayHit), M, occluded);
  if (devPtr) {
    HIP_CHECK(hipMemcpyAsync(rays, mirror.data(), span, hipMemcpyHostToDevice, sh.stream));
    HIP_CHECK(hipStreamSynchronize(sh.stream));
  }
}

} // namespace rtamd
