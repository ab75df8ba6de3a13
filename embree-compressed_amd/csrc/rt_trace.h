// Batch front-end of the hot path: rt_trace.cpp (launches, staged / pipelined / device-resident batches), rt_filter.cpp (host filter
// loop), rt_service.cpp (persistent small-call service, call combiner).
#pragma once
#include "rt_objects.h"
#include "trace.h"

namespace rtamd {

// Trace M records starting at `rays` (host or device memory) with the given byte stride.
// countersOut != nullptr selects the instrumented kernels and implies a host synchronisation.
void trace_batch(Scene* s, void* rays, uint32_t M, size_t byteStride, bool occluded, const RTCIntersectContext* ctx,
                 TraceCounters* countersOut);
void trace_pointers(Scene* s, void** ptrs, uint32_t M, bool occluded, const RTCIntersectContext* ctx);
// Entry for the rtcIntersect1/1M, rtcOccluded1/1M API calls: small host-pointer calls go through the call combiner
// (SURVEY.md section 8 row f2), everything else straight to trace_batch.  (rt_service.cpp)
void trace_call(Scene* s, void* rays, uint32_t M, size_t byteStride, bool occluded, const RTCIntersectContext* ctx);
// persistent consumer for calls of up to 64 rays (rt_service.cpp, trace_service.hip.h)
void service_destroy(Device* dev);
void service_quiesce(Device* dev);
static const uint32_t COMBINE_MAX_RAYS = 1024; // host-pointer calls up to this size are combined

// ---- shared by rt_trace.cpp, rt_filter.cpp and rt_service.cpp ---------------------------------------------------------------
// One batch as a launch sees it: `count` records, `stride` bytes apart, at `rays` (memory the shard's GPU can reach).
struct Batch
{
  void* rays;
  uint32_t count, stride;
  bool occluded, coherent;
  uint32_t instID;
  hipStream_t stream; // nullptr: the shard's stream
};

// What one accel's launch gets on top of the batch; everything optional.
struct LaunchExtras
{
  WaveRecord* counters = nullptr; // counted batches: this launch's slice of the wave log (selects the instrumented kernels)
  // counted batches: host buffer of TRACE_QUEUES * TRACE_QUEUE_STRIDE words that receives the launch's queue words after the kernels
  // (word 1 of a queue = rays that survived the root cull pre-pass, word 2 = valid rays the pre-pass tested)
  uint32_t* cullCountsOut = nullptr;
  // filter re-traces: candidates to skip, pairs [offsets[k], offsets[k + 1]) for ray k; tbits where the accel keys candidates by t
  const uint32_t* exclOffsets = nullptr;
  const uint2* exclPairs = nullptr;
  const uint32_t* exclT = nullptr;
};

// One traversal launch of `A` over the batch on shard `si`.  The calling thread's current HIP device must be the shard's (GpuShard::use()).
void launch_on(Scene* s, const Accel& A, size_t si, const Batch& b, const LaunchExtras& x = LaunchExtras());
// The launches of a batch: every accel of the scene in trace order.  extras: one entry per accel (Scene::TRI / QUAD / SUBDIV) or nullptr;
// `skip`: an accel that gets no launch.
void trace_accels(Scene* s, size_t si, const Batch& b, const LaunchExtras* extras = nullptr, const Accel* skip = nullptr);
// rt_filter.cpp: batches of scenes / contexts with filter callbacks
void trace_filtered(Scene* s, void* rays, uint32_t M, size_t byteStride, bool occluded, const RTCIntersectContext* ctx);

// -1: plain host memory; otherwise the HIP ordinal the allocation lives on
int pointer_device(const void* p);
inline bool is_device_pointer(const void* p) { return pointer_device(p) >= 0; }

// n records of `rec` bytes, srcStride bytes apart, packed into dst
inline void gather_records(void* dst, const void* src, size_t n, size_t srcStride, uint32_t rec)
{
  if (srcStride == rec) { memcpy(dst, src, n * rec); return; }
  for (size_t i = 0; i < n; i++) memcpy((char*)dst + i * rec, (const char*)src + i * srcStride, rec);
}

// The outputs of n traced records (`rec` bytes apart at src) into the caller's: only tfar (byte 32) and, for rtcIntersect, the hit
// record (bytes 48..79) are outputs.  onlyChanged (large host batches): a miss leaves a record untouched, and most incoherent rays miss;
// a record whose outputs came back unchanged is not written (reading the caller's cache line is cheaper than dirtying it: 1 M random
// rays 1.5 -> ~0.9 ms of scatter)
inline void scatter_outputs(void* dst, size_t dstStride, const void* src, uint32_t rec, size_t n, bool occluded, bool onlyChanged = false)
{
  for (size_t i = 0; i < n; i++) {
    char* d = (char*)dst + i * dstStride;
    const char* r = (const char*)src + i * rec;
    if (!onlyChanged || memcmp(d + 32, r + 32, 4) != 0) memcpy(d + 32, r + 32, 4);
    if (!occluded && (!onlyChanged || memcmp(d + 48, r + 48, 32) != 0)) memcpy(d + 48, r + 48, 32);
  }
}

} // namespace rtamd
