// Small host-pointer calls: the persistent service kernel and the call combiner behind rtcIntersect1 / rtcOccluded1 and short 1M streams
// (SURVEY.md section 8 row f2).
#include "rt_trace.h"
#include <chrono>

namespace rtamd {

// ---- persistent consumer for small calls (row f2) -------------------------------------------------------------
// See trace_service.hip.h.  One resident kernel per RTCDevice, for the accel kind of the first scene that makes a small call; a caller owns
// one slot of the ring for the duration of its call (threads are dealt slots round-robin; two threads that share a slot take turns).
struct Device::Service
{
  static const uint32_t SLOTS = 64;          // wavefronts of the service kernel = calls in flight
  static const uint32_t SPILL_DEPTH = 512;   // HBM stack overflow entries per lane the service can offer (scenes that need more keep the combiner)
  uint32_t kind = 0, levels = 0;
  hipStream_t stream = nullptr;
  ServiceSlot* slotsHost = nullptr;
  ServiceSlot* slotsDev = nullptr;
  uint32_t* stopHost = nullptr;
  uint32_t* stopDev = nullptr;
  uint32_t* activityDev = nullptr;
  void* spillDev = nullptr;
  LaunchParams base;
  std::atomic<uint32_t> slotLock[SLOTS];
  uint32_t slotSeq[SLOTS];
  std::atomic<uint32_t> nextSlot{0};
  std::atomic<uint64_t> lastSubmitNs{0};
  std::atomic<uint64_t> starts{0};
  bool failed = false;
};

// every live service, so that a process that exits without releasing its RTCDevice still stops the resident kernels BEFORE the runtime tears
// down the host-mapped ring they poll (a kernel reading freed host memory faults the GPU)
static std::mutex g_serviceRegistryMutex;
static std::vector<Device::Service*> g_serviceRegistry;
static void service_stop_all_at_exit()
{
  std::lock_guard<std::mutex> g(g_serviceRegistryMutex);
  for (Device::Service* sv : g_serviceRegistry) {
    if (sv->stopHost) __atomic_store_n(sv->stopHost, 1u, __ATOMIC_RELEASE);
    if (sv->stream) (void)hipStreamSynchronize(sv->stream);
  }
  g_serviceRegistry.clear();
}
static void service_register(Device::Service* sv)
{
  std::lock_guard<std::mutex> g(g_serviceRegistryMutex);
  static bool hooked = false;
  if (!hooked) { atexit(service_stop_all_at_exit); hooked = true; }
  g_serviceRegistry.push_back(sv);
}
static void service_unregister(Device::Service* sv)
{
  std::lock_guard<std::mutex> g(g_serviceRegistryMutex);
  g_serviceRegistry.erase(std::remove(g_serviceRegistry.begin(), g_serviceRegistry.end(), sv), g_serviceRegistry.end());
}

static uint64_t now_ns() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void service_destroy(Device* dev)
{
  Device::Service* sv = dev->service;
  if (!sv) return;
  dev->service = nullptr;
  service_unregister(sv);
  if (dev->gpu >= 0) (void)hipSetDevice(dev->gpu);
  if (sv->stopHost) __atomic_store_n(sv->stopHost, 1u, __ATOMIC_RELEASE);
  if (sv->stream) { (void)hipStreamSynchronize(sv->stream); (void)hipStreamDestroy(sv->stream); }
  if (sv->slotsHost) (void)hipHostFree(sv->slotsHost);
  if (sv->stopHost) (void)hipHostFree(sv->stopHost);
  if (sv->activityDev) (void)hipFree(sv->activityDev);
  if (sv->spillDev) (void)hipFree(sv->spillDev);
  delete sv;
}

// Stop the service kernel and wait for it (it restarts on demand): before the library allocates or frees device memory, which synchronises
// the whole device and would otherwise wait for the resident kernel's idle exit.  Jobs in flight are finished first; a job that arrives in
// between is served after the restart its caller triggers.
void service_quiesce(Device* dev)
{
  if (!dev->service) return;
  std::lock_guard<std::mutex> g(dev->serviceMutex);
  Device::Service* sv = dev->service;
  if (!sv || sv->failed || !sv->stream) return;
  if (dev->gpu >= 0) (void)hipSetDevice(dev->gpu);
  __atomic_store_n(sv->stopHost, 1u, __ATOMIC_RELEASE);
  (void)hipStreamSynchronize(sv->stream);
  __atomic_store_n(sv->stopHost, 0u, __ATOMIC_RELEASE);
}

// (re)start the service kernel if it is not running; serviceMutex held
static void service_start_locked(Device* dev, Device::Service* sv)
{
  const hipError_t q = hipStreamQuery(sv->stream);
  if (q == hipErrorNotReady) { (void)hipGetLastError(); return; } // running
  if (q != hipSuccess) HIP_CHECK(q);
  ServiceParams sp;
  sp.base = sv->base;
  sp.slots = sv->slotsDev;
  sp.numSlots = Device::Service::SLOTS;
  sp.idlePolls = 16384u; // ~30 ms without a single job: the kernel leaves the GPU to itself
  sp.stop = sv->stopDev;
  sp.activity = sv->activityDev;
  HIP_CHECK(launch_service(sp, sv->stream));
  sv->starts++;
}

// Trace a call of up to 64 rays through the service.  false: not applicable (the caller falls back to the combiner).
static bool service_trace(Scene* s, char* rays, uint32_t M, size_t byteStride, bool occluded, uint32_t instID)
{
  Device* dev = s->device;
  if (!dev->tuneService || dev->gpu < 0 || dev->shards.size() != 1 || M > (uint32_t)SERVICE_SLOT_RAYS) return false;
  const Accel* only = nullptr;
  for (const Accel* a : s->accels())
    if (a->traceable()) { if (only) return false; only = a; } // several accels (AccelN): the general path
  if (!only) return false;
  const Accel& A = *only;
  const KindRow& K = kind_row(A.kind);
  if (!K.serve) return false; // no service kernel for this kind (accel_kinds.h): the combiner traces these calls with the batch kernels
  const uint32_t worst = 7u * (A.maxDepth + 1u) + 2u;
  const uint32_t need = worst > (uint32_t)TRACE_LDS_STACK ? worst - TRACE_LDS_STACK : 0u;
  if (need > Device::Service::SPILL_DEPTH) return false;
  Device::GpuShard& sh = dev->primary();
  Device::Service* sv = dev->service;
  if (!sv) {
    std::lock_guard<std::mutex> g(dev->serviceMutex);
    if (!dev->service) {
      sh.use();
      std::unique_ptr<Device::Service> n(new Device::Service);
      n->kind = A.kind;
      n->levels = s->compressionLevel;
      for (uint32_t i = 0; i < Device::Service::SLOTS; i++) { n->slotLock[i].store(0u); n->slotSeq[i] = 0u; }
      LaunchParams& p = n->base;
      memset(&p, 0, sizeof(p));
      p.accel = A.desc(0);
      p.cbvhLevels = s->compressionLevel;
      p.numCUs = (uint32_t)sh.numCUs;
      p.rayChunk = (uint32_t)SERVICE_SLOT_RAYS;
      p.leafBatch = dev->tuneLeafBatch;
      p.refillBatch = dev->tuneRefillBatch;
      p.octMax = dev->tuneOctMax;
      p.walkBatch = dev->tuneWalkBatch;
      p.octSteps = dev->tuneOctSteps;
      p.octLeaf = dev->tuneOctLeaf != 0xFFFFFFFFu ? dev->tuneOctLeaf : (uint32_t)K.octLeaf;
      p.overflow = sh.overflowDev;
      p.spillDepth = Device::Service::SPILL_DEPTH;
      p.gridBlocks = Device::Service::SLOTS / (TRACE_BLOCK / 64);
      try {
        HIP_CHECK(hipStreamCreateWithFlags(&n->stream, hipStreamNonBlocking));
        HIP_CHECK(hipHostMalloc((void**)&n->slotsHost, sizeof(ServiceSlot) * Device::Service::SLOTS, hipHostMallocMapped));
        memset(n->slotsHost, 0, sizeof(ServiceSlot) * Device::Service::SLOTS);
        HIP_CHECK(hipHostGetDevicePointer((void**)&n->slotsDev, n->slotsHost, 0));
        HIP_CHECK(hipHostMalloc((void**)&n->stopHost, 128, hipHostMallocMapped));
        memset(n->stopHost, 0, 128);
        HIP_CHECK(hipHostGetDevicePointer((void**)&n->stopDev, n->stopHost, 0));
        HIP_CHECK(hipMalloc((void**)&n->activityDev, 128));
        HIP_CHECK(hipMemset(n->activityDev, 0, 128));
        HIP_CHECK(hipMalloc(&n->spillDev, (size_t)Device::Service::SLOTS * 64u * Device::Service::SPILL_DEPTH * 8u + 16u));
        p.spill = n->spillDev;
        service_register(n.get());
        service_start_locked(dev, n.get());
      } catch (...) { // no service kernel for this accel kind / level, or out of memory: the combiner serves the calls
        n->failed = true;
        (void)hipGetLastError();
      }
      dev->service = n.release();
    }
    sv = dev->service;
  }
  if (sv->failed || sv->kind != A.kind || (sv->levels != s->compressionLevel && !K.levelFree)) return false;

  // a slot: threads are dealt slots round-robin once; a shared slot is taken in turns
  static thread_local uint32_t mySlot = 0xFFFFFFFFu;
  static thread_local const Device::Service* mySlotOf = nullptr;
  if (mySlotOf != sv) { mySlot = sv->nextSlot.fetch_add(1u) % Device::Service::SLOTS; mySlotOf = sv; }
  unsigned spins = 0;
  for (;;) {
    uint32_t expect = 0u;
    if (sv->slotLock[mySlot].compare_exchange_weak(expect, 1u, std::memory_order_acquire)) break;
    if ((++spins & 255u) == 0u) std::this_thread::yield();
  }
  struct Unlock { std::atomic<uint32_t>& l; ~Unlock() { l.store(0u, std::memory_order_release); } } unlock{sv->slotLock[mySlot]};

  const uint64_t t0 = now_ns();
  if (t0 - sv->lastSubmitNs.load(std::memory_order_relaxed) > 10000000ull) { // quiet for 10 ms: the kernel may have left, look before the job goes in
    std::lock_guard<std::mutex> g(dev->serviceMutex);
    sh.use();
    service_start_locked(dev, sv);
  }
  sv->lastSubmitNs.store(t0, std::memory_order_relaxed);
  ServiceSlot& slot = sv->slotsHost[mySlot];
  const uint32_t rec = occluded ? (uint32_t)sizeof(RTCRay) : (uint32_t)sizeof(RTCRayHit);
  gather_records(slot.rays, rays, M, byteStride, rec);
  if (M == 1u) { // the ray itself rides in the polled header line (trace_service.hip.h)
    memcpy(slot.ray0, rays, 28);
    memcpy(slot.ray0 + 7, rays + 32, 4);
  }
  slot.count = M;
  slot.occluded = occluded ? 1u : 0u;
  slot.instID = instID;
  slot.spillDepth = need;
  slot.accel = A.desc(0);
  const uint32_t seq = ++sv->slotSeq[mySlot];
  __atomic_store_n(&slot.seq2, seq, __ATOMIC_RELEASE);
  __atomic_store_n(&slot.seq, seq, __ATOMIC_RELEASE);
  spins = 0;
  uint64_t lastCheck = t0;
  while (__atomic_load_n(&slot.done, __ATOMIC_ACQUIRE) != seq) {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
    if ((++spins & 127u) == 0u) std::this_thread::yield(); // more callers than cores: let the others put their jobs in
    if ((spins & 4095u) == 0u) {
      const uint64_t t = now_ns();
      if (t - lastCheck > 2000000ull) { // 2 ms without an answer: has the kernel left (idle exit raced with this job)?  restart it
        std::lock_guard<std::mutex> g(dev->serviceMutex);
        sh.use();
        service_start_locked(dev, sv);
        lastCheck = t;
      }
      if (t - t0 > 5000000000ull) RT_THROW(RTC_ERROR_UNKNOWN, "the small-call service kernel does not answer");
    }
  }
  scatter_outputs(rays, byteStride, slot.rays, rec, M, occluded);
  dev->statServiceCalls++;
  return true;
}

// ---- call combiner (row f2) -----------------------------------------------------------------------------------------
// The reference answers rtcIntersect1 in ~1 us on the calling core; here a call costs a staging copy, a kernel launch
// and a synchronisation (~60 us) whatever its size.  Harness threads of an embree application call concurrently
// (SURVEY.md section 8b "Threading"), so the calls that arrive while a launch is in flight are traced together by the
// next leader: T calling threads then see ~T rays per launch instead of one.  Results are those of independent calls
// (a stream is M independent single-ray calls); no timer, no extra thread, no CPU traversal.
static void combine_process(Device* dev, std::vector<Device::SmallCall*>& batch)
{
  // group by (scene, kind, instID); each group becomes one contiguous batch
  std::vector<char> done(batch.size(), 0);
  for (size_t i = 0; i < batch.size(); i++) {
    if (done[i]) continue;
    Device::SmallCall* a = batch[i];
    std::vector<Device::SmallCall*> group;
    size_t total = 0;
    for (size_t j = i; j < batch.size(); j++) {
      Device::SmallCall* b = batch[j];
      if (!done[j] && b->scene == a->scene && b->occluded == a->occluded && b->instID == a->instID) {
        done[j] = 1;
        group.push_back(b);
        total += b->M;
      }
    }
    const uint32_t rec = a->occluded ? (uint32_t)sizeof(RTCRay) : (uint32_t)sizeof(RTCRayHit);
    try {
      std::vector<char> tmp(total * rec + 16);
      char* base = (char*)(((uintptr_t)tmp.data() + 15) & ~(uintptr_t)15);
      size_t k = 0;
      for (Device::SmallCall* c : group) {
        gather_records(base + k * rec, c->base, c->M, c->stride, rec);
        k += c->M;
      }
      RTCIntersectContext ctx;
      memset(&ctx, 0, sizeof(ctx));
      ctx.instID[0] = a->instID;
      trace_batch(a->scene, base, (uint32_t)total, rec, a->occluded, &ctx, nullptr);
      k = 0;
      for (Device::SmallCall* c : group) {
        scatter_outputs(c->base, c->stride, base + k * rec, rec, c->M, c->occluded);
        k += c->M;
      }
      dev->statCombinedBatches++;
    } catch (const rtc_error& e) {
      for (Device::SmallCall* c : group) { c->error = e.code; c->message = e.msg; }
    } catch (const std::exception& e) {
      for (Device::SmallCall* c : group) { c->error = RTC_ERROR_UNKNOWN; c->message = e.what(); }
    }
  }
}

void trace_call(Scene* s, void* rays, uint32_t M, size_t byteStride, bool occluded, const RTCIntersectContext* ctx)
{
  Device* dev = s->device;
  if (M == 0 || M > COMBINE_MAX_RAYS || (ctx && ctx->filter) || s->triIntersectFilter || s->triOccludedFilter || s->subdivFilter || s->instIntersectFilter || s->instOccludedFilter || s->modified || (((uintptr_t)rays) & 3) ||
      byteStride > 0xFFFFFFFFull || is_device_pointer(rays)) {
    trace_batch(s, rays, M, byteStride, occluded, ctx, nullptr); // large, device-resident, or about to raise its own error
    return;
  }
  if (service_trace(s, (char*)rays, M, byteStride, occluded, ctx ? ctx->instID[0] : RTC_INVALID_GEOMETRY_ID)) return;
  Device::SmallCall call;
  call.scene = s;
  call.base = (char*)rays;
  call.M = M;
  call.stride = byteStride;
  call.occluded = occluded;
  call.instID = ctx ? ctx->instID[0] : RTC_INVALID_GEOMETRY_ID;
  std::unique_lock<std::mutex> lk(dev->combMutex);
  dev->combPending.push_back(&call);
  dev->statCombinedCalls++; // counted once the call is pending (the held-leader test waits on this count)
  while (!call.done) {
    if (!dev->combBusy) { // become the leader for everything that is pending now (own call included)
      dev->combBusy = true;
      while (dev->combHold.load(std::memory_order_acquire)) { // test hook (rtcamdDebugHoldCombiner): the leader waits, the others queue up behind it
        lk.unlock();
        std::this_thread::yield();
        lk.lock();
      }
      std::vector<Device::SmallCall*> batch;
      batch.swap(dev->combPending);
      lk.unlock();
      combine_process(dev, batch);
      lk.lock();
      for (Device::SmallCall* c : batch) c->done = true;
      dev->combBusy = false;
      dev->combCv.notify_all();
    } else
      dev->combCv.wait(lk);
  }
  lk.unlock();
  if (call.error != RTC_ERROR_NONE) throw rtc_error(call.error, call.message);
}

} // namespace rtamd
