// Batch front-end of the hot path: host/device pointer handling, staging, kernel launches.
// Replaces RayStreamFilter::filterAOS (kernels/bvh/bvh_intersector_stream_filters.cpp:24-165) and the
// per-ray dispatch through Accel::Intersectors (kernels/common/accel.h:264-267).
#include "rt_trace.h"
#include <chrono>

namespace rtamd {

uint32_t trace_grid_blocks(uint32_t count, int numCUs, uint32_t rayChunk)
{
  // upper bound of the resident set: 20 waves per CU; a wave takes `rayChunk` rays per queue grab
  const uint32_t resident = (uint32_t)numCUs * 5u * (256u / TRACE_BLOCK);
  const uint32_t perBlock = std::max(1u, rayChunk) * (TRACE_BLOCK / 64u);
  const uint32_t need = (count + perBlock - 1) / perBlock;
  return need < resident ? (need ? need : 1u) : resident;
}

// Rays a wave takes from a work queue per grab.  Large batches: Device::tuneChunk (256: one atomic per 256 rays keeps the queue heads
// cold).  Batches that cannot give every resident wavefront (16 per CU) such a share are cut finer, down to 32 rays per wave, so that a
// mid-size batch - a 16 k .. 128 k chunk of the host pipeline, a test batch, a combined group of small calls - spreads over the whole chip
// instead of count / 256 wavefronts (round 3 finding, profiles/r03_deep_subset_probe.txt: 1000 rays ran on FOUR wavefronts).
// With other batches in flight the coarse share wins again from ~100 k rays on (every wavefront pays its deepest ray's iterations, the chip
// is issue bound: fewer, fuller wavefronts per batch), so launch_on switches back to tuneChunk there.  Measured round 3, cbvh.leaf, kernel
// alone / four batches in flight, fine vs 256-ray chunks (profiles/r03_chunk_ab.txt): 4 k rays 43 vs 105 us / 222 vs 105 Mrays/s, 16 k 46 vs
// 89 us / 779 vs 525, 64 k 61 vs 98 us / 1.90 vs 1.84 Grays/s, 128 k 73 vs 98 us / 2.97 vs 3.52, 250 k 104 vs 107 us / 4.8 vs 5.7, 500 k 0 % / -7 %.
static uint32_t ray_chunk_for(const Device* dev, uint32_t M, int numCUs)
{
  if (dev->tuneChunkFixed) return dev->tuneChunk;
  // the share that gives every resident wavefront exactly ONE grab: a queue owns ceil(M / TRACE_QUEUES) rays and serves waves / TRACE_QUEUES wavefronts.
  // (1 M rays on 4096 wavefronts: 245, not 256 - 64 grabs per queue instead of 61 full ones and a rest of 9 rays; a wave that needs a second grab late
  // doubles its life: 240 rays per grab cost +5 %, 245 gain 1.2 % over 256, profiles/r03_chunk_busy_ab.txt)
  const uint32_t waves = (uint32_t)numCUs * 16u;
  const uint32_t perQ = (M + (uint32_t)TRACE_QUEUES - 1u) / (uint32_t)TRACE_QUEUES;
  const uint32_t grabs = std::max(1u, waves / (uint32_t)TRACE_QUEUES);
  const uint32_t share = (perQ + grabs - 1u) / grabs;
  return std::min(dev->tuneChunk, std::max(32u, share));
}

int pointer_device(const void* p)
{
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) {
    (void)hipGetLastError(); // plain (unregistered) host memory
    return -1;
  }
  return (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged) ? attr.device : -1;
}

void launch_on(Scene* s, const Accel& A, size_t si, const Batch& b, const LaunchExtras& x)
{
  Device* dev = s->device;
  Device::GpuShard& sh = *dev->shards[si];
  if (!A.traceable()) return;
  const uint32_t M = b.count;
  LaunchParams p;
  p.accel = A.desc(si);
  p.rays = b.rays;
  p.count = M;
  p.stride = b.stride;
  p.instID = b.instID;
  p.occluded = b.occluded ? 1u : 0u;
  p.rayChunk = ray_chunk_for(dev, M, sh.numCUs);
  p.gridBlocks = trace_grid_blocks(M, sh.numCUs, p.rayChunk);
  // Ray-pool skeleton for very large batches - where it still pays.  Since the two-stage blob visits and the batched leaf passes of round 3 the lane
  // kernel is the faster one at EVERY size for grid cells and the cBVH box / leaf / full modes (4 M rays, one stream: cbvh.leaf 12.0 vs 10.2 Grays/s,
  // eager 6 M 14.5 vs 10.7); the pool keeps triangles (6 M: 16.8 vs 14.8) and the cBVH grid mode (11.0 vs 8.3).  profiles/r03_lane_pool_ab.txt
  // (quad leaves stay on the lane kernel unless RTAMD_KERNEL=pool: not measured)
  const KindRow& K = kind_row(A.kind); // which kinds have a pool form, and why the others have none: accel_kinds.h
  p.poolKernel = !K.pool ? 0u : (dev->tunePoolKernel == 2u ? (K.poolPays && M >= dev->tunePoolMinRays ? 1u : 0u) : dev->tunePoolKernel);
  // worst-case stack: 7 siblings per level plus the entry being expanded.  The overflow area is sized for it, so a push
  // can only be dropped if the tree is deeper than the builder reported; the kernels then raise `overflow` (below).
  const uint32_t worst = 7u * (A.maxDepth + 1u) + 2u;
  size_t spillBytes;
  if (p.poolKernel) { // one overflow column per ray slot of every resident wavefront
    p.gridBlocks = (uint32_t)sh.numCUs * TRACE_POOL_BLOCKS_PER_CU;
    p.spillDepth = worst > (uint32_t)TRACE_POOL_STACK ? worst - TRACE_POOL_STACK : 0u;
    spillBytes = (size_t)p.gridBlocks * (TRACE_POOL_BLOCK / 64) * TRACE_POOL_SLOTS * (size_t)p.spillDepth * 8u + 16u;
  } else {
    p.spillDepth = worst > (uint32_t)TRACE_LDS_STACK ? worst - TRACE_LDS_STACK : 0u;
    // development aid (env RTAMD_INST_SPILL_MAX, two-level kernels only): fewer overflow entries than the depth asks for, to exercise the
    // documented failure - a push beyond the area is dropped behind its bounds check, the kernel raises `overflow`, the call RTC_ERROR_UNKNOWN
    if (K.inst != INST_NONE) p.spillDepth = std::min(p.spillDepth, dev->tuneInstSpillMax);
    spillBytes = (size_t)p.gridBlocks * TRACE_BLOCK * (size_t)p.spillDepth * 8u + 16u;
  }
  p.counters = x.counters;
  p.instHair = A.instHair; // line and curve trees below the instances: 1 the HAIR form of the two-level kernel, 2 (moving ones among them) the HAIRMB form
  p.roundCurves = A.roundCurves; // the kinds 42 / 43 on Scene::roundCurveAccel: the tube leaf
  p.cbvhLevels = A.cbvhLevels ? A.cbvhLevels : s->compressionLevel; // (instanced cBVH blobs, kinds 25 / 35, carry the level of the scenes they come from)
  // cBVH blob walk: quad form (four lanes per ray, two-stage visits) or one ray per lane.  Coherent batches (RTC_INTERSECT_CONTEXT_FLAG_COHERENT,
  // e.g. the primary rays of viewer_stream_device.cpp:305) keep most lanes at blobs at once; since the two-stage visits the quad form is the faster
  // one for them too when the batch has the chip (1920x1080 camera rays alone: 0.630 vs 0.768 ms), the lane form still wins with several batches
  // in flight (6.8 vs 6.2 Grays/s) - decided below, once the launch context says how many others are running.  RTAMD_CBVH_FORM=quad|lane overrides.
  p.cbvhLaneForm = dev->tuneCbvhForm == 2u ? 0u : dev->tuneCbvhForm;
  p.numCUs = (uint32_t)sh.numCUs;
  p.leafBatch = dev->tuneLeafBatch;
  p.refillBatch = dev->tuneRefillBatch;
  p.octMax = dev->tuneOctMax;
  p.walkBatch = dev->tuneWalkBatch;
  p.inlineRay = 0u;
  p.wgPool = dev->tuneWgPool == 2u ? (M >= dev->tuneWgPoolMinRays ? 1u : 0u) : dev->tuneWgPool; // small batches: see rt_objects.h
  p.octSteps = dev->tuneOctSteps;
  // waiting rays from which the child-parallel leaf phase runs: triangle leaves 16, grid cells 24 (measured optima), cBVH blobs
  // (quad form, 16 rays per pass) 16
  p.octLeaf = dev->tuneOctLeaf != 0xFFFFFFFFu ? dev->tuneOctLeaf : (uint32_t)K.octLeaf;
  p.exclOffsets = x.exclOffsets;
  p.exclPairs = x.exclPairs;
  p.exclT = x.exclT;
  p.overflow = sh.overflowDev;
  static const bool timeline = getenv("RTAMD_TIMELINE") != nullptr; // development aid, see trace.h
  p.timeline = (timeline && !x.counters) ? (unsigned long long*)sh.countersDev : nullptr;
  // {context, queue heads, launch, event} as one unit: concurrent callers on device-resident batches must not pick the same
  // context (its event still reads "finished" until the new launch has recorded it).  The stream is read once.
  std::lock_guard<std::mutex> seq(sh.seqMutex);
  const hipStream_t stream = b.stream ? b.stream : sh.stream;
  unsigned busyOther = 0;
  Device::LaunchCtx& ctx = sh.acquireLaunchCtx(spillBytes, &busyOther, stream);
  p.spill = ctx.spill;
  if (dev->tuneCbvhForm == 2u && b.coherent && busyOther >= 2u) p.cbvhLaneForm = 1u;
  // A batch alone on the chip is fastest with two workgroups per CU; when two or more batches are running on other
  // streams a leaner grid is better: every wave pays its deepest ray's iterations, so fewer waves per batch waste fewer
  // instructions (measured: 11.2 -> 12.0 Grays/s with four batches in flight; alone 0.174 -> 0.237 ms, hence adaptive).
  // (The grid-cell kernel, whose leaves are always tested 8 lanes per ray, needs 118 VGPRs: four waves per SIMD fit, and a batch
  // alone on the chip is 10 % faster with four workgroups per CU; 0.169 -> 0.151 ms.)
  const bool octOnly = K.octOnly == OCT_ALWAYS || (K.octOnly == OCT_QUAD_FORM && !p.cbvhLaneForm); // four waves per SIMD
  const uint32_t aloneBlocks = octOnly ? dev->tuneAloneBlocksOct : 2u;
  // with that fourth wave slot two workgroups per CU per batch are also the better grid in flight (eager, 40 steps: random rays
  // 13.3 -> 13.8 Grays/s, shadow rays 9.3 -> 9.8, camera rays 7.1 -> 7.7)
  const uint32_t busyBlocks = octOnly ? dev->tuneBusyBlocksOct : 1u;
  p.blocksPerCU = (dev->tuneBlocksAuto ? (busyOther >= 2u ? busyBlocks : (busyOther == 1u ? 2u : aloneBlocks)) : dev->tuneBlocksPerCU) * (256u / TRACE_BLOCK); // knob unit: 4 waves
  // With two or more other batches running, fewer and fuller wavefronts still (up to tuneChunkBusy = 512 rays per grab) as long as the batch
  // keeps half of the chip's wavefront slots busy: 1 M rays 12.8 -> 13.05 Grays/s, eager 14.2 -> 14.7, triangles 18.3 -> 18.9; a flat 512
  // loses 16-19 % at 131 k - 250 k rays (profiles/r03_chunk_busy_ab.txt)
  uint32_t busyChunk = dev->tuneChunk;
  if (busyOther >= 2u) busyChunk = std::min(std::max(dev->tuneChunk, (M / ((uint32_t)sh.numCUs * 8u)) & ~63u), std::max(dev->tuneChunk, dev->tuneChunkBusy));
  if (busyOther >= 1u && M >= 100000u && !dev->tuneChunkFixed && p.rayChunk < busyChunk && !p.poolKernel) {
    p.rayChunk = busyChunk; // in flight: coarse shares (see ray_chunk_for); the grid only shrinks, the overflow area was sized for the larger one
    p.gridBlocks = trace_grid_blocks(M, sh.numCUs, p.rayChunk);
  }
  p.queues = (uint32_t*)ctx.queues;
  // Root cull pre-pass (trace_cull.hip.h): large batches on the lane kernel whose root is an inner node.  Filter re-traces
  // (exclusion lists) are small and skip it.
  p.survivors = nullptr;
  // (only on the kinds whose row allows it, accel_kinds.h)
  if (dev->tuneCull && K.cull && !p.poolKernel && !x.exclOffsets && M >= dev->tuneCullMinRays && !(A.root & REF_LEAF)) {
    const size_t need = ((size_t)(M + TRACE_QUEUES - 1) / TRACE_QUEUES) * TRACE_QUEUES * 4u;
    if (need > ctx.survivorsBytes) { // first batch of this size on this context (an allocation synchronises the device)
      HIP_CHECK(hipStreamSynchronize(stream));
      if (ctx.survivors) HIP_CHECK(hipFree(ctx.survivors));
      ctx.survivors = nullptr;
      ctx.survivorsBytes = 0;
      HIP_CHECK(hipMalloc(&ctx.survivors, need + need / 4));
      ctx.survivorsBytes = need + need / 4;
    }
    p.survivors = (uint32_t*)ctx.survivors;
  }
  HIP_CHECK(hipMemsetAsync(ctx.queues, 0, TRACE_QUEUES * TRACE_QUEUE_STRIDE * 4, stream)); // heads, survivor counts, valid-ray counts
  if (p.timeline) HIP_CHECK(hipMemsetAsync(p.timeline, 0, (size_t)WAVE_LOG_CAPACITY * 64, stream));
  if (p.survivors) HIP_CHECK(launch_cull(p, stream));
  HIP_CHECK(launch_trace(p, stream));
  if (x.cullCountsOut && p.survivors) HIP_CHECK(hipMemcpyAsync(x.cullCountsOut, ctx.queues, TRACE_QUEUES * TRACE_QUEUE_STRIDE * 4, hipMemcpyDeviceToHost, stream));
  else if (x.cullCountsOut) memset(x.cullCountsOut, 0, TRACE_QUEUES * TRACE_QUEUE_STRIDE * 4);
  HIP_CHECK(hipEventRecord(ctx.done, stream));
  dev->statLaunches++;
}

void trace_accels(Scene* s, size_t si, const Batch& b, const LaunchExtras* extras, const Accel* skip)
{
  const auto accels = s->accels();
  for (size_t i = 0; i < accels.size(); i++)
    if (accels[i] != skip) launch_on(s, *accels[i], si, b, extras ? extras[i] : LaunchExtras());
}

// Counted batches: every wavefront of the instrumented twin stores one WaveRecord.  Each traceable accel, in trace order, gets the next
// slice of the wave log at dLog and of the host cull words; returns the slices in use.
static size_t counted_extras(Scene* s, WaveRecord* dLog, uint32_t* cullWords, LaunchExtras* extras)
{
  size_t n = 0;
  const auto accels = s->accels();
  for (size_t i = 0; i < accels.size(); i++) {
    if (!accels[i]->traceable()) continue;
    extras[i].counters = dLog + n * WAVE_LOG_CAPACITY;
    extras[i].cullCountsOut = cullWords + n * (size_t)TRACE_QUEUES * TRACE_QUEUE_STRIDE;
    n++;
  }
  return n;
}

// ---- large host-pointer batches: chunked pipeline ---------------------------------------------------------------------------
// The callers of the drop-in API pass HOST records (viewer_stream_device.cpp:288-341).  One such batch used to be: memcpy into
// pinned memory, H2D, traversal, D2H, scatter - one after the other, the copies on one host thread (~0.1 Grays/s; the traversal is
// 1-2 % of that).  Here the range of every shard is cut into chunks of Device::tunePipeChunk rays; chunk k is gathered into pinned
// memory by the host pool while chunks k-1 and k-2 are on the GPU (upload, traversal, download on two alternating internal streams:
// PCIe is full duplex), and chunk k-2 is scattered back when its event has fired.  The results are those of the unpipelined path:
// a stream is M independent rays (tests/test_gpu_host_pipeline.py compares the two byte for byte).
static void trace_host_pipelined(Scene* s, char* rays, uint32_t M, size_t byteStride, bool occluded, uint32_t instID, bool coherent, uint32_t rec)
{
  Device* dev = s->device;
  const size_t G = M < 2u * dev->shards.size() ? 1 : dev->shards.size();
  // chunk size by batch size (tools/pcie_probe.py and a sweep of 16 k .. 200 k rays on MI355X: 32 k rays in 16 k chunks 0.29 ms against 0.41 ms
  // unpipelined, 64 k in 32 k chunks 0.41 / 0.70 ms, 128 k 0.69 / 1.20 ms, 200 k 0.99 / 1.79 ms, 1 M in 128 k chunks 2.84 / 9.4 ms)
  const uint32_t CH = dev->tunePipeChunk ? dev->tunePipeChunk : (M < 49152u ? 16384u : (M < 300000u ? 32768u : (M < 600000u ? 65536u : 131072u)));
  const unsigned LAG = 2;
  if (dev->hostPool.threads.empty()) {
    const unsigned hw = std::max(2u, std::thread::hardware_concurrency());
    const unsigned want = dev->tuneHostThreads ? dev->tuneHostThreads : std::min(8u, hw / 2u);
    if (want > 1) dev->hostPool.start(want - 1); // the calling thread is the last worker
  }
  const size_t workers = dev->hostPool.threads.size() + 1;
  struct Lane { Device::GpuShard* sh; size_t g; uint32_t lo, n, chunks; };
  std::vector<Lane> lanes;
  uint32_t maxChunks = 0;
  for (size_t g = 0; g < G; g++) {
    Lane L;
    L.sh = dev->shards[g].get();
    L.g = g;
    L.lo = (uint32_t)((uint64_t)M * g / G);
    L.n = (uint32_t)((uint64_t)M * (g + 1) / G) - L.lo;
    if (L.n == 0) continue;
    L.chunks = (L.n + CH - 1) / CH;
    maxChunks = std::max(maxChunks, L.chunks);
    L.sh->use();
    L.sh->ensureStaging((size_t)L.n * rec);
    // the two internal streams exist from the first pipelined batch on: created with the device they took hardware queues away from
    // the caller's streams (measured: four device-resident batches in flight on four streams fell from 11.4 to 9.3 Grays/s, at most
    // three kernels overlapped)
    for (hipStream_t& ps : L.sh->pipeStream)
      if (!ps) HIP_CHECK(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
    while (L.sh->pipeEvents.size() < L.chunks) {
      hipEvent_t e;
      HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      L.sh->pipeEvents.push_back(e);
    }
    lanes.push_back(L);
  }
  // rays [a, b) of a lane, split over the workers
  auto for_parts = [&](uint32_t a, uint32_t b, const std::function<void(uint32_t, uint32_t)>& body) {
    const uint32_t n = b - a;
    const size_t parts = std::min<size_t>(workers, std::max<uint32_t>(1u, n / 4096u));
    dev->hostPool.run(parts, [&](size_t p) { body(a + (uint32_t)((uint64_t)n * p / parts), a + (uint32_t)((uint64_t)n * (p + 1) / parts)); });
  };
  struct Hot { Device::HostPool& p; Hot(Device::HostPool& q) : p(q) { p.begin(); } ~Hot() { p.end(); } } hot(dev->hostPool); // helpers poll for the duration of the call
  // RTAMD_PIPE_TRACE=1: where the calling thread's time goes (gather / enqueue / waiting for a chunk's event / scatter), per call
  static const bool pipeTrace = getenv("RTAMD_PIPE_TRACE") != nullptr;
  double tGather = 0, tEnq = 0, tWait = 0, tScatter = 0;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  for (uint32_t k = 0; k < maxChunks + LAG; k++) {
    for (Lane& L : lanes) {
      if (k >= L.chunks) continue;
      const double t0 = pipeTrace ? now() : 0.0;
      const uint32_t a = k * CH, b = std::min(L.n, a + CH);
      char* h = (char*)L.sh->stageHost;
      const char* src = rays + (size_t)L.lo * byteStride;
      for_parts(a, b, [&](uint32_t x, uint32_t y) { gather_records(h + (size_t)x * rec, src + (size_t)x * byteStride, y - x, byteStride, rec); });
      const double t1 = pipeTrace ? now() : 0.0;
      L.sh->use();
      const hipStream_t st = L.sh->pipeStream[k & 1u];
      char* d = (char*)L.sh->stageDev + (size_t)a * rec;
      const size_t bytes = (size_t)(b - a) * rec;
      HIP_CHECK(hipMemcpyAsync(d, h + (size_t)a * rec, bytes, hipMemcpyHostToDevice, st));
      trace_accels(s, L.g, Batch{d, b - a, rec, occluded, coherent, instID, st});
      HIP_CHECK(hipMemcpyAsync(h + (size_t)a * rec, d, bytes, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipEventRecord(L.sh->pipeEvents[k], st));
      if (pipeTrace) { const double t2 = now(); tGather += t1 - t0; tEnq += t2 - t1; }
    }
    if (k < LAG) continue;
    const uint32_t j = k - LAG;
    for (Lane& L : lanes) {
      if (j >= L.chunks) continue;
      L.sh->use();
      const double t0 = pipeTrace ? now() : 0.0;
      HIP_CHECK(hipEventSynchronize(L.sh->pipeEvents[j]));
      const double t1 = pipeTrace ? now() : 0.0;
      const uint32_t a = j * CH, b = std::min(L.n, a + CH);
      const char* h = (const char*)L.sh->stageHost;
      char* dst0 = rays + (size_t)L.lo * byteStride;
      for_parts(a, b, [&](uint32_t x, uint32_t y) { scatter_outputs(dst0 + (size_t)x * byteStride, byteStride, h + (size_t)x * rec, rec, y - x, occluded, true); });
      if (pipeTrace) { const double t2 = now(); tWait += t1 - t0; tScatter += t2 - t1; }
    }
  }
  if (pipeTrace) fprintf(stderr, "embree3-amd: pipelined host batch of %u rays: gather %.2f ms, enqueue %.2f ms, waiting for events %.2f ms, scatter %.2f ms (%zu host threads, %u chunks)\n", M, tGather, tEnq, tWait, tScatter, workers, maxChunks);
  for (Lane& L : lanes) L.sh->checkOverflow();
}

void trace_batch(Scene* s, void* rays, uint32_t M, size_t byteStride, bool occluded, const RTCIntersectContext* ctx,
                 TraceCounters* countersOut)
{
  Device* dev = s->device;
  if (s->modified) RT_THROW(RTC_ERROR_INVALID_OPERATION, "scene got not committed"); // scene.cpp:25,54
  if (M == 0) return;
  if (s->hasInstances()) { // refused before anything touches the GPU
    // inst_filters=1: taken when all instances are mesh instances (the two-level kernel of subdivision instances has no exclusion scan)
    if (ctx && ctx->filter && (!dev->inst_filters || s->instSubdivAccel.traceable()))
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "RTCIntersectContext::filter is not supported on a scene with instances");
    // inst_hair=1: the hair form of the two-level kernel has no exclusion scan (the commit has refused geometry filters below such a scene)
    if (ctx && ctx->filter && s->instAccel.instHair)
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "inst_hair=1: RTCIntersectContext::filter is not supported on a scene with instanced line segments or flat curves");
    if (countersOut) RT_THROW(RTC_ERROR_INVALID_OPERATION, "counted batches are not supported on a scene with instances");
  }
  dev->useDevice();
  if (byteStride > 0xFFFFFFFFull) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "byteStride too large");
  if (((uintptr_t)rays) & 3) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "ray not aligned to 4 bytes"); // rtcore.cpp:413
  // (geometry filters on subdivision meshes are called on the eager accel only: the fork's intersector never calls one, see trace_filtered)
  const bool subdivFilters = s->subdivFilter && s->subdivAccel.kind == ACCEL_GRIDSOA;
  // (instIntersectFilter / instOccludedFilter: filters below mesh instances, set only under inst_filters=1)
  const bool instFilters = occluded ? s->instOccludedFilter : s->instIntersectFilter;
  const bool lineFilters = occluded ? s->lineOccludedFilter : s->lineIntersectFilter; // static and moving line geometries, flat cubic curves
  if (!countersOut && ((ctx && ctx->filter) || subdivFilters || instFilters || lineFilters || (occluded ? s->triOccludedFilter : s->triIntersectFilter))) {
    trace_filtered(s, rays, M, byteStride, occluded, ctx);
    return;
  }
  const uint32_t instID = ctx ? ctx->instID[0] : RTC_INVALID_GEOMETRY_ID;
  const bool coherent = ctx && (ctx->flags & RTC_INTERSECT_CONTEXT_FLAG_COHERENT);
  const uint32_t rec = occluded ? (uint32_t)sizeof(RTCRay) : (uint32_t)sizeof(RTCRayHit);

  // instrumented twin (counted_extras).  Counted batches run on ONE shard (the first, or the one the device pointer lives on) and one at a time.
  std::unique_lock<std::mutex> countLock(dev->launchMutex, std::defer_lock);
  LaunchExtras counted[Scene::NUM_ACCELS];
  WaveRecord* dLog = nullptr;
  size_t logBytes = 0, countShard = 0;
  std::vector<uint32_t> cullWords; // counted batches: the queue words of every launch
  if (countersOut) cullWords.assign(Scene::NUM_ACCELS * (size_t)TRACE_QUEUES * TRACE_QUEUE_STRIDE, 0u);
  auto beginCounted = [&](size_t shard) { // hand out the slices of the shard's wave log and clear those in use (an empty scene: one)
    Device::GpuShard& sh = *dev->shards[shard];
    countShard = shard;
    dLog = (WaveRecord*)sh.countersDev;
    logBytes = std::max<size_t>(1, counted_extras(s, dLog, cullWords.data(), counted)) * WAVE_LOG_CAPACITY * sizeof(WaveRecord);
    HIP_CHECK(hipMemsetAsync(dLog, 0, logBytes, sh.stream));
  };

  const int ptrDev = pointer_device(rays);
  if (ptrDev >= 0) {
    // device-resident stream: trace in place on the GPU the records live on, stream-ordered, no host synchronisation
    size_t si = dev->shards.size();
    for (size_t i = 0; i < dev->shards.size() && si == dev->shards.size(); i++)
      if (dev->shards[i]->ordinal == ptrDev) si = i;
    if (si == dev->shards.size()) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "the ray buffer lives on a GPU this RTCDevice does not use (gpu= / gpus=)");
    Device::GpuShard& sh = *dev->shards[si];
    sh.use();
    sh.checkOverflow(); // report of an earlier asynchronous batch
    if (countersOut) {
      countLock.lock();
      beginCounted(si);
    }
    trace_accels(s, si, Batch{rays, M, (uint32_t)byteStride, occluded, coherent, instID, nullptr}, countersOut ? counted : nullptr);
  } else {
    // Host records: staged through pinned memory.  With several shards the M rays are split into contiguous ranges
    // [g*M/G, (g+1)*M/G), one per shard: H2D, traversal and D2H of the ranges run concurrently on the shards' own streams
    // and write disjoint slices of the caller's buffer (no exchange step, no collective).
    if (!countLock.owns_lock()) countLock.lock();
    if (!countersOut && M >= dev->tunePipeMinRays) {
      trace_host_pipelined(s, (char*)rays, M, byteStride, occluded, instID, coherent, rec);
      return;
    }
    const size_t G = (countersOut || M < 2u * dev->shards.size()) ? 1 : dev->shards.size();
    std::vector<uint32_t> lo(G + 1);
    for (size_t g = 0; g <= G; g++) lo[g] = (uint32_t)((uint64_t)M * g / G);
    for (size_t g = 0; g < G; g++) {
      Device::GpuShard& sh = *dev->shards[g];
      const uint32_t n = lo[g + 1] - lo[g];
      if (n == 0) continue;
      sh.use();
      const size_t bytes = (size_t)n * rec;
      sh.ensureStaging(bytes);
      char* h = (char*)sh.stageHost;
      const char* src = (const char*)rays + (size_t)lo[g] * byteStride;
      gather_records(h, src, n, byteStride, rec);
      // Small batches (single rays and the combiner's groups, row f2): the kernels read and write the pinned staging buffer in place
      // over PCIe - two copies and their DMA latency less per call; a few KB of rays cost nothing over the bus.
      void* dRays = sh.stageDev;
      const bool zeroCopy = !countersOut && n <= dev->tuneZeroCopyMax;
      if (zeroCopy) HIP_CHECK(hipHostGetDevicePointer(&dRays, h, 0));
      else HIP_CHECK(hipMemcpyAsync(sh.stageDev, h, bytes, hipMemcpyHostToDevice, sh.stream));
      if (countersOut) beginCounted(g);
      trace_accels(s, g, Batch{dRays, n, rec, occluded, coherent, instID, nullptr}, countersOut ? counted : nullptr);
      if (!zeroCopy) HIP_CHECK(hipMemcpyAsync(h, sh.stageDev, bytes, hipMemcpyDeviceToHost, sh.stream));
    }
    for (size_t g = 0; g < G; g++) {
      Device::GpuShard& sh = *dev->shards[g];
      const uint32_t n = lo[g + 1] - lo[g];
      if (n == 0) continue;
      sh.use();
      HIP_CHECK(hipStreamSynchronize(sh.stream));
      scatter_outputs((char*)rays + (size_t)lo[g] * byteStride, byteStride, sh.stageHost, rec, n, occluded);
    }
    for (size_t g = 0; g < G; g++) dev->shards[g]->checkOverflow();
  }

  if (countersOut) {
    std::vector<WaveRecord> log(logBytes / sizeof(WaveRecord));
    Device::GpuShard& csh = *dev->shards[countShard];
    csh.use();
    HIP_CHECK(hipMemcpyAsync(log.data(), dLog, logBytes, hipMemcpyDeviceToHost, csh.stream));
    HIP_CHECK(hipStreamSynchronize(csh.stream));
    csh.checkOverflow();
    TraceCounters& c = *countersOut;
    memset(&c, 0, sizeof(c));
    unsigned long long first = ~0ull;
    for (const WaveRecord& w : log)
      if (w.valid) first = std::min(first, w.start);
    c.startInv = ~first;
    for (const WaveRecord& w : log) {
      if (!w.valid) continue;
      c.rays += w.rays; c.nodeVisits += w.nodes; c.leafVisits += w.leaves; c.primTests += w.prims;
      c.innerVisits += w.inner; c.hits += w.hits; c.stackSpills += w.spills;
      c.cyclesFetch += w.cyclesFetch; c.cyclesNode += w.cyclesNode; c.cyclesLeaf += w.cyclesLeaf; c.cyclesPop += w.cyclesPop;
      c.cyclesTotal += w.cyclesTotal;
      c.iterations += w.iterations; c.leafPhases += w.leafPhases; c.waves += 1; c.activeLaneIters += w.laneIters;
      c.maxRaySteps = std::max(c.maxRaySteps, w.maxRaySteps);
      c.drainTicksSum += w.end - w.lastGrab;
      c.drainTicksMax = std::max(c.drainTicksMax, w.end - w.lastGrab);
      c.waveEndHist[std::min<unsigned long long>((w.end - first) / 400ull, 63ull)] += 1; // 4 us buckets of 10 ns ticks
      c.waveIterHist[std::min<unsigned long long>(w.iterations / 2ull, 63ull)] += 1;
    }
    // root cull pre-pass: it visited the root once for every valid ray; the traversal kernel saw (and counted) the survivors only
    for (size_t l = 0; l < Scene::NUM_ACCELS; l++) {
      unsigned long long survivors = 0, valid = 0;
      for (int q = 0; q < TRACE_QUEUES; q++) {
        survivors += cullWords[(l * TRACE_QUEUES + q) * TRACE_QUEUE_STRIDE + 1];
        valid += cullWords[(l * TRACE_QUEUES + q) * TRACE_QUEUE_STRIDE + 2];
      }
      if (valid) {
        c.rays += valid - survivors;
        c.nodeVisits += valid;
        c.reserved += survivors; // rays that survived the root cull (reported as `cullSurvivors` by the Python binding)
      }
    }
  }
}

void trace_pointers(Scene* s, void** ptrs, uint32_t M, bool occluded, const RTCIntersectContext* ctx)
{
  // rtcIntersect1Mp / rtcOccluded1Mp: gather the pointed-to records into one batch (filterAOP, filters.cpp:167-)
  const uint32_t rec = occluded ? (uint32_t)sizeof(RTCRay) : (uint32_t)sizeof(RTCRayHit);
  std::vector<char> tmp((size_t)M * rec + 16);
  char* base = (char*)(((uintptr_t)tmp.data() + 15) & ~(uintptr_t)15);
  for (uint32_t i = 0; i < M; i++) memcpy(base + (size_t)i * rec, ptrs[i], rec);
  trace_batch(s, base, M, rec, occluded, ctx, nullptr);
  for (uint32_t i = 0; i < M; i++) scatter_outputs(ptrs[i], 0, base + (size_t)i * rec, rec, 1, occluded);
}

} // namespace rtamd
