/*
 * MI355X extensions to the embree3 contract.  These are additions, not replacements: the reference has
 * no counterpart because it has no device, no stream and no batch boundary.  They exist so that a caller
 * who already owns device-resident ray buffers (bench.py, a wavefront renderer) can run the hot path
 * without host staging and can time / inspect it.
 *
 * Everything here is plain C ABI: opaque handles from rtcore.h, void* for HIP handles, sized structs.
 */
#ifndef EMBREE3_AMD_RTCORE_AMD_H
#define EMBREE3_AMD_RTCORE_AMD_H

#include "rtcore.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* HIP stream (hipStream_t as void*) on which the device enqueues uploads and traversal kernels.
 * rtcIntersect1M/rtcOccluded1M on DEVICE pointers are stream-ordered on it and return without a host
 * sync; on HOST pointers they synchronise before returning (embree semantics). */
RTC_API void* rtcamdGetDeviceStream(RTCDevice device);
/* Use a caller-owned stream (e.g. the framework's current stream) instead of the library's own.
 * May be changed between calls: batches enqueued on DIFFERENT streams are independent and run concurrently (the
 * library keeps its per-launch scratch - work-queue heads, stack overflow area - in a ring of launch contexts).
 * A renderer that keeps 2-4 batches in flight this way hides the drain of one batch (a few deep rays) under the
 * start of the next; on MI355X that is worth ~1.5x in rays/s for 1 M-ray batches.  Order between batches on
 * different streams is the caller's business (HIP events), as for any other stream work. */
RTC_API void rtcamdSetDeviceStream(RTCDevice device, void* hipStream);
/* Block until everything enqueued on the device's stream has completed. */
RTC_API void rtcamdSynchronizeDevice(RTCDevice device);
/* HIP device ordinal the RTCDevice was created on (config key "gpu="). */
RTC_API int rtcamdGetDeviceOrdinal(RTCDevice device);

/* World-to-local transform of an RTC_GEOMETRY_TYPE_INSTANCE geometry at `time`, in `format` (one of the three transform
 * formats of rtcSetGeometryTransform): exactly the matrix the traversal applies to a ray with that ray.time when it enters
 * the instance.  Hits inside an instance carry Ng in the instance's LOCAL space; a world-space normal is the transposed
 * linear part of this matrix applied to Ng.  With one time step it is the inverse of the transform set; with more it is
 * inverse(lerp(step[itime], step[itime + 1], ftime)), where rtcGetGeometryTransform(time) returns the lerp itself.
 * A singular transform gives an all-zero matrix (such an instance is not entered).  Errors: RTC_ERROR_INVALID_ARGUMENT for a
 * null handle or pointer or a format that is no transform format, RTC_ERROR_INVALID_OPERATION for a geometry that is no
 * instance. */
RTC_API void rtcamdGetGeometryWorld2Local(RTCGeometry geometry, float time, enum RTCFormat format, void* xfm);

/* Extra readable properties for rtcGetDeviceProperty (cast to enum RTCDeviceProperty; the values lie inside that
 * enum's range and above every value the reference defines): counters of the call
 * combiner.  Host-pointer calls of up to 1024 rays (rtcIntersect1, rtcOccluded1, short 1M streams) issued
 * concurrently by several threads are traced together: the calls that arrive while a launch is in flight form the
 * next batch.  Results are those of independent calls.  (The reference answers such a call on the calling core.) */
enum RTCAMDDeviceProperty
{
  RTCAMD_DEVICE_PROPERTY_TRACE_LAUNCHES = 240,     /* traversal kernel launches so far */
  RTCAMD_DEVICE_PROPERTY_COMBINED_CALLS = 241,     /* API calls that went through the combiner */
  RTCAMD_DEVICE_PROPERTY_COMBINED_BATCHES = 242, /* batches formed out of them */
  RTCAMD_DEVICE_PROPERTY_SERVICE_CALLS = 243     /* API calls answered by the persistent small-call kernel (config key service=1) */
};

/* Layout facts of a committed scene's device acceleration structure; sizes in bytes.
 * Replaces what the reference prints with verbose=2 (kernels/bvh/bvh_statistics.cpp). */
struct RTCAMDSceneStats
{
  size_t byteSize;          /* sizeof(struct RTCAMDSceneStats), set by the caller */
  unsigned int accelKind;   /* 0 none, 1 bvh8.triangle4v (Pluecker), 2 bvh8.triangle4 (Moeller),
                               3 cbvh.box, 4 cbvh.leaf, 5 cbvh.grid, 6 gridsoa (eager), 7 cbvh.full,
                               8 quads (Pluecker), 9 quads (Moeller),
                               10 / 11 motion blur triangles (Pluecker / Moeller), 12 / 13 motion blur quads, 14..25 instance accels,
                               26 / 27 motion blur triangles and 28 / 29 motion blur quads over time-dependent node boxes
                               (device config mb_bounds=linear; nodeBytes is 144 there),
                               30 / 31 the instance accels 22 / 23 over such scenes (device config inst_mb_bounds=linear, default swept:
                               without it a top scene over a scene of the kinds 26..29 is refused at commit); nodeCount / nodeBytes
                               describe their 96-byte nodes (top-level tree, static trees), the instanced scenes' 144-byte nodes follow
                               in the same buffer from a multiple of 144 bytes on: rtcamdGetAccelData(scene, 0) returns all of it,
                               (scene, 3) two words - how many there are and the index of the first one in 144-byte units,
                               32 / 33 the mesh instance accel of a scene with at least one moving instance under the device config
                               inst_bounds=linear (default swept): the top-level tree itself is made of 144-byte time-dependent nodes
                               and leads the second section of that buffer, so a ray enters a moving instance only where it is at
                               the ray's time; nodeCount / nodeBytes describe the 96-byte nodes of the instanced scenes' static trees,
                               34 / 35 the subdivision instance accels 24 / 25 of a scene with at least one moving subdivision instance
                               under the device config inst_subdiv_bounds=linear (default swept; independent of inst_bounds): the
                               instanced scenes' 96-byte nodes lead the buffer (nodeCount / nodeBytes), the top-level tree of 144-byte
                               time-dependent nodes follows from a multiple of 144 bytes on; rtcamdGetAccelData(scene, 3) returns four
                               words - leaf blobs, index of the first blob, 144-byte nodes, index of the first one in 144-byte units,
                               36 / 37 line segments (robust / fast traversal; 48-byte records),
                               38 / 39 motion blur line segments (robust / fast traversal; 80-byte records, one per segment and time
                               segment), 40 / 41 the same over time-dependent node boxes (mb_bounds=linear; nodeBytes is 144 there),
                               42 / 43 flat Bezier and B-spline curves (robust / fast traversal; 80-byte records: the four Bezier
                               control points with their radii, geomID, primID and the tessellation rate of the curve's geometry),
                               44 / 45 motion blur flat Bezier and B-spline curves (device config hair_accel_mb=default | bvh4.bezier1imb |
                               bvh8.bezier1imb, all the one BVH8; robust / fast traversal; 160-byte records, one per curve and time
                               segment: the four Bezier control points with their radii at both ends of the segment, then geomID,
                               primID, segment, numSegments and the tessellation rate), 46 / 47 the same over time-dependent node boxes
                               (mb_bounds=linear; nodeBytes is 144 there) */
  unsigned int branching;   /* 8 */
  size_t nodeCount;         /* quantized BVH8 nodes */
  size_t nodeBytes;         /* bytes per node record (96; 144 in the kinds 26..29, 40 / 41 and 46 / 47) */
  size_t primCount;         /* triangles, quads, or cBVH / GridSOA leaves */
  size_t primBytes;         /* bytes per triangle record (48), per quad record (64) or mean bytes per subdiv leaf blob */
  size_t leafCount;         /* BVH8 leaves */
  size_t totalBytes;        /* resident HBM bytes of the accel */
  unsigned int maxDepth;
  unsigned int reserved;
};
RTC_API void rtcamdGetSceneStats(RTCScene scene, struct RTCAMDSceneStats* stats);

/* Per-batch traversal work counters, produced by an instrumented twin of the intersect kernel (same
 * code path; every wavefront stores one record, folded on the host).  The batch is traced exactly like rtcIntersect1M does.  Used to price the
 * algorithmic bytes per ray, B = 84 + nodes*nodeBytes + prims*primBytes; the
 * reference's counterpart is the EMBREE_STAT_COUNTERS build (kernels/common/stat.h:21-33). */
struct RTCAMDTraceCounters
{
  unsigned long long rays;        /* valid rays traced */
  unsigned long long nodeVisits;  /* BVH8 node records fetched */
  unsigned long long leafVisits;  /* BVH8 leaves entered */
  unsigned long long primTests;   /* triangle records fetched / cBVH or grid leaves entered */
  unsigned long long innerVisits; /* cBVH-internal 4-byte nodes decoded / GridSOA cells tested */
  unsigned long long hits;        /* rays that report a hit */
  unsigned long long stackSpills; /* pushes that overflowed the LDS stack into the HBM spill area */
  unsigned long long reserved;    /* rays that survived the root cull pre-pass (0: the pre-pass did not run); `rays` and `nodeVisits`
                                     include the rays / root visits of the pre-pass */
  /* shader-clock cycles summed over wavefronts, per phase of the traversal loop (the phases are wave-uniform):
     ray fetch, inner-node step, leaf step, pop/finish, and the whole loop.  Diagnostic: where a batch spends time. */
  unsigned long long cyclesFetch, cyclesNode, cyclesLeaf, cyclesPop, cyclesTotal;
  unsigned long long iterations, leafPhases, waves; /* loop iterations, iterations that ran the leaf phase, waves */
  /* wave timeline (100 MHz s_memrealtime): lanes with a ray summed over iterations (/(64*iterations) = occupancy of the
     loop), ~(earliest wave start), and two per-wave histograms: end time since the earliest start in 4 us buckets,
     and iterations per wave in buckets of 2.  Diagnostic: how long the drain of a batch is. */
  unsigned long long activeLaneIters, startInv;
  /* longest single ray in loop iterations (node steps + leaf steps + waiting), and the drain of the waves: time from a
     wave's last successful work-queue grab to its end, summed over waves / maximum (10 ns ticks) */
  unsigned long long maxRaySteps, drainTicksSum, drainTicksMax;
  unsigned long long waveEndHist[64], waveIterHist[64];
};
RTC_API void rtcamdIntersect1MCounted(RTCScene scene, struct RTCIntersectContext* context, struct RTCRayHit* rayhit,
                                      unsigned int M, size_t byteStride, struct RTCAMDTraceCounters* counters);

/* The same for an any-hit batch (rtcOccluded1M semantics). */
RTC_API void rtcamdOccluded1MCounted(RTCScene scene, struct RTCIntersectContext* context, struct RTCRay* ray, unsigned int M,
                                     size_t byteStride, struct RTCAMDTraceCounters* counters);

/* Read-only views of the host copy of the committed accel (valid until the next commit / release).
 * Test infrastructure: lets an external checker walk the exact structure the kernels traverse.
 * kind: 0 = BVH8 nodes, 1 = primitive records, 2 = subdiv leaf blobs, 3 = blob offset table; 16 + these: the same arrays of the
 * scene's subdivision instance accel (instances of scenes that hold subdivision meshes), whatever else the scene holds. */
RTC_API const void* rtcamdGetAccelData(RTCScene scene, unsigned int kind, size_t* byteSize);
/* Test hook: the encoder's restatement of the fork's leaf quantiser (quantTris<4>::setZ / estimateExtent,
 * kernels/geometry/compressed_leaf.h:193-251) on caller-supplied inputs: box = lower xyz, upper xyz of the parent box,
 * v = the four corner vertices (12 floats).  Lets tests compare it with the reference header compiled in oracle/_ref. */
/* development aid: raw wave log of the last launch (csrc/trace.h `timeline`, csrc/accel.h WaveRecord) */
RTC_API size_t rtcamdDebugReadWaveLog(RTCDevice device, void* out, size_t bytes);
/* test hook: hold (1) / release (0) the leader of the small-call combiner */
RTC_API void rtcamdDebugHoldCombiner(RTCDevice device, int hold);
RTC_API void rtcamdDebugCbvhLeafCodec(const float* box, const float* v, float extent, unsigned char* bytesOut, float* extentEstimate);
/* Test hook: runs `jobs` parallel jobs of `parts` parts each through the device's pool of staging threads (the pool behind the
 * chunked pipeline of large host-pointer batches; `threads` helpers are started if fewer exist), in `cycles` begin / end cycles,
 * and returns the number of parts that ran exactly once with the right index.  Works on a gpu=none device: CPU-side coverage of the pool. */
RTC_API unsigned long long rtcamdDebugHostPoolSelfTest(RTCDevice device, unsigned int threads, unsigned int cycles, unsigned int jobs, unsigned int parts);
/* Test hook: what the library knows about an accel kind (RTCAMDSceneStats::accelKind; the table of csrc/accel_kinds.h) as one word - the
 * bit layout is documented at the definition - and all ones for a value that is no accel kind. */
RTC_API unsigned int rtcamdDebugAccelKindRow(unsigned int kind);
/* Root reference of the BVH8 (encoding documented in DESIGN.md / csrc/accel.h). */
RTC_API unsigned int rtcamdGetAccelRoot(RTCScene scene);
/* The geometry filter functions the scene's last commit saw - what routes a batch through the host filter loop: on its own enabled
 * triangle / quad meshes (intersect, occluded), on its subdivision meshes (either), and - device config inst_filters=1 only - on the
 * enabled meshes of the scenes of its placed mesh instances (intersect, occluded). */
enum RTCAMDSceneFilterFlags
{
  RTCAMD_SCENE_FILTER_MESH_INTERSECT = 1,
  RTCAMD_SCENE_FILTER_MESH_OCCLUDED = 2,
  RTCAMD_SCENE_FILTER_SUBDIV = 4,
  RTCAMD_SCENE_FILTER_INSTANCED_INTERSECT = 8,
  RTCAMD_SCENE_FILTER_INSTANCED_OCCLUDED = 16
};
RTC_API unsigned int rtcamdGetSceneFilterFlags(RTCScene scene);

#if defined(__cplusplus)
}
#endif
#endif
