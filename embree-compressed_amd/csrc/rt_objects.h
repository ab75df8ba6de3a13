// Host object model behind the opaque embree3 handles: Device, Buffer, Geometry, Scene.
// Mirrors the roles of kernels/common/{device,state,buffer,geometry,scene_triangle_mesh,scene_subdiv_mesh,scene}.*
// of the reference, reduced to what the traversal hot path and its builders need.
#pragma once
#include <map>
#include <memory>
#include <array>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <unordered_map>

#include "accel_kinds.h"
#include "rt_common.h"

namespace rtamd {

struct Scene;

// ---------------------------------------------------------------------------------------------------
// Device: config string, error state, HIP device + stream, staging buffers.
// ---------------------------------------------------------------------------------------------------
struct Device : RefCounted
{
  // config (reference: State::parse, kernels/common/state.cpp:241-430)
  std::string tri_accel = "default";
  std::string subdiv_accel = "default";
  std::string quad_accel = "default";
  std::string tri_accel_mb = "default"; // triangle meshes with more than one time step
  std::string quad_accel_mb = "default"; // quad meshes with more than one time step
  std::string mb_bounds = "swept"; // node boxes of the motion-blur mesh accels: "swept" (one box over the whole shutter, QNode8) or "linear" (time-dependent, QNodeMB8)
  std::string inst_mb_bounds = "swept"; // node boxes of motion-blur trees below an instance: "swept" (scenes built under mb_bounds=linear are refused below an instance) or "linear" (such scenes keep their QNodeMB8s, kinds ACCEL_INSTMESHMB_LINEAR_*)
  std::string inst_bounds = "swept"; // top-level boxes of moving instances: "swept" (the union over the instance's time steps, QNode8) or "linear" (time-dependent, a top-level tree of QNodeMB8s, kinds ACCEL_INSTTOP_LINEAR_*)
  std::string inst_subdiv_bounds = "swept"; // top-level boxes of moving subdivision instances (Scene::instSubdivAccel): "swept" (QNode8, kinds 24 / 25) or "linear" (a top-level tree of QNodeMB8s, kinds ACCEL_INSTSUBDIV_TOP_LINEAR_*)
  bool inst_filters = false; // "inst_filters=1": filter functions run on hits below mesh instances (geometry filters inside instanced mesh scenes, RTCIntersectContext::filter on scenes with mesh instances); 0, the default: both are refused as before
  bool inst_hair = false; // "inst_hair=1": an instanced scene may hold static line segments and flat curves, alone or beside its triangle and quad meshes (the HAIR form of the two-level kernel, trace_instance_hair.hip); 0, the default: refused as before
  bool inst_hair_mb = false; // "inst_hair_mb=1", beside inst_hair=1: the line segments and flat curves of an instanced scene may have time steps (the HAIRMB form of the two-level kernel, trace_instance_hair_mb.hip); 0, the default: refused as before
  bool round_curves = false; // "round_curves=1": RTC_GEOMETRY_TYPE_ROUND_BEZIER_CURVE / _ROUND_BSPLINE_CURVE are taken (static, top level only) and traced by the tube leaf (trace_round_curve.hip) from Scene::roundCurveAccel; 0, the default: refused at rtcNewGeometry as before
  std::string line_accel = "default"; // flat linear curves: default / bvh8.line4i / bvh4.line4i, all the one BVH8 over LineRecords (build_line_accel raises for any other at commit)
  std::string line_accel_mb = "default"; // flat linear curves with time steps: default / bvh8.line4imb / bvh4.line4imb, all the one BVH8 over LineMBRecords (build_linemb_accel raises for any other at commit)
  bool lineAccelMBNamed = false; // "line_accel_mb=" given (a host-only device builds the motion-blur line accel only then, lines_mb_enabled())
  std::string hair_accel = "default"; // flat Bezier and B-spline curves: the names of Scene::createHairAccel (default, bvh4.bezier1v, bvh4.bezier1i, bvh4obb.bezier1v, bvh4obb.bezier1i, bvh8obb.bezier1v, bvh8obb.bezier1i), all the one BVH8 over CurveRecords - oriented-box nodes are not built (build_curve_accel raises for any other name at commit)
  std::string hair_accel_mb = "default"; // flat Bezier and B-spline curves with time steps: the names of Scene::createHairMBAccel (default, bvh4.bezier1imb, bvh8.bezier1imb), all the one BVH8 over CurveMBRecords - oriented-box nodes are not built (build_curvemb_accel raises for any other name at commit)
  bool hairAccelMBNamed = false; // "hair_accel_mb=" given (a host-only device builds the motion-blur curve accel only then, curves_mb_enabled())
  bool hairAccelNamed = false; // "hair_accel=" given (a host-only device takes the flat cubic curve types only then, curves_enabled())
  std::string inst_accel = "default"; // instances: "default" is the only name (build_instance_accel, rt_instance_build.cpp, raises for any other at commit)
  bool instAccelNamed = false; // "inst_accel=" given (a host-only device takes quad meshes inside an instanced scene only then, inst_quads_enabled())
  bool quadAccelMBNamed = false; // "quad_accel_mb=" given (a host-only device builds the motion-blur quad accel only then, quads_mb_enabled())
  bool triAccelMBNamed = false; // "tri_accel_mb=" given (with inst_accel=: a host-only device takes motion-blur meshes inside an instanced scene, inst_mesh_motion_enabled())
  bool quadAccelNamed = false; // "quad_accel=" given (a host-only device takes quad geometry only then, quads_enabled())
  bool subdivAccelNamed = false; // "subdiv_accel=" given (with inst_accel=: a host-only device takes instances of subdivision scenes, inst_subdiv_enabled())
  int verbose = 0;
  int gpu = 0;            // HIP device ordinal ("gpu=" key; falls back to env RTAMD_GPU, LOCAL_RANK is NOT read here)
  int numThreads = 0;     // accepted, used only for host-side builders
  int benchmark = 0;
  int keepGrids = 0;      // "keep_grids=1": keep the tessellated vertex grids for inspection (tests)

  // error state (reference: Device::process_error device.cpp:258-286, getDeviceErrorCode :250-256)
  std::mutex errMutex;
  std::unordered_map<uint64_t, RTCError> threadErrors; // per calling thread, first error wins
  RTCErrorFunction errorFn = nullptr;
  void* errorFnUser = nullptr;
  RTCMemoryMonitorFunction memFn = nullptr;
  void* memFnUser = nullptr;

  // HIP state.  One GpuShard per GPU the device traces on ("gpu=<ordinal>" -> one shard; "gpus=0-7" / "gpus=0:2:5" ->
  // several: the accel is replicated on every shard at commit and one host-pointer rtcIntersect1M / rtcOccluded1M call is
  // split into contiguous ray ranges, one per shard, each with its own stream and staging buffers and a disjoint D2H into
  // the caller's records - SURVEY.md section 8e; no collective).  The same ordinal may be listed twice ("gpus=0:0"): two
  // logical shards on one GPU, which is how the sharded path is tested on a one-GPU box.
  struct LaunchCtx
  {
    void* queues = nullptr;  // TRACE_QUEUES heads, one 128-byte line each
    void* spill = nullptr;
    size_t spillBytes = 0;
    void* survivors = nullptr; // root cull pre-pass: per-queue survivor lists (4 bytes per ray of the largest batch so far)
    size_t survivorsBytes = 0;
    hipEvent_t done = nullptr;
    bool used = false;
    hipStream_t stream = nullptr; // stream of the launch that last used this context
  };
  static const int NUM_LAUNCH_CTX = 8;
  struct GpuShard
  {
    int ordinal = 0;
    int numCUs = 256;
    hipStream_t stream = nullptr;
    bool ownsStream = false;
    // staging (host-pointer path): pinned host mirror + device batch, grown on demand
    void* stageHost = nullptr;
    void* stageDev = nullptr;
    size_t stageBytes = 0;
    // pipelined host-pointer batches (rt_trace.cpp trace_host_pipelined): chunks alternate between two internal streams, so that
    // the upload of one chunk runs under the traversal and the download of the previous one (PCIe is full duplex); one event per chunk
    hipStream_t pipeStream[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> pipeEvents;
    // Per-launch scratch (work-queue heads + LDS-stack overflow area).  A ring of contexts, so that batches enqueued on
    // DIFFERENT streams (rtcamdSetDeviceStream between calls) can be in flight together: the drain of one batch - a few
    // deep rays keeping waves alive - then overlaps the start of the next.  A context is reused only after the kernel
    // that last used it has finished (stream-side wait on its event, no host block).
    LaunchCtx launchCtx[NUM_LAUNCH_CTX];
    unsigned nextCtx = 0;
    // serialises {pick a launch context, zero its queue heads, launch, record its event}: rtcIntersect1M / rtcOccluded1M on
    // device-resident batches are callable from several threads at once, like the reference's (rtcore.cpp:403-432)
    std::mutex seqMutex;
    void* countersDev = nullptr; // wave log of the instrumented twin (one counted batch at a time, under launchMutex)
    // One word of host-mapped pinned memory the kernels set when a traversal-stack entry had to be dropped (the overflow
    // area is sized from the tree depth, so this cannot happen for a tree the builder made; if it ever does, the call
    // raises RTC_ERROR_UNKNOWN instead of silently missing a subtree).
    uint32_t* overflowHost = nullptr;
    uint32_t* overflowDev = nullptr;
    void use() const;
    void ensureStaging(size_t bytes);
    // picks the next context, makes `stream` wait for its previous user; *busyOther = OTHER streams with unfinished launches.
    // Call with seqMutex held.
    LaunchCtx& acquireLaunchCtx(size_t spillBytesNeeded, unsigned* busyOther = nullptr, hipStream_t onStream = nullptr);
    void checkOverflow(); // throws RTC_ERROR_UNKNOWN (and clears the flag) when a kernel reported a dropped stack entry
  };
  std::vector<std::unique_ptr<GpuShard>> shards; // empty for gpu=none
  std::vector<int> gpuList;                      // "gpus=" ordinals in the order given
  GpuShard& primary() { return *shards[0]; }
  std::mutex launchMutex; // serialises host-pointer batches (they share the staging buffers) and counted batches

  // Host threads for the staging copies of large host-pointer batches (gather of the caller's records into pinned memory, scatter of
  // tfar + hit back): one thread moves ~10 GB/s, PCIe 5 x16 ~55 GB/s each way.  Started with the first such batch; the caller works too.
  struct HostPool
  {
    // While a pipelined batch is running (`hot`) the helpers spin on `ticket` instead of sleeping: a part of a chunk is ~100 us of
    // copying, a condition-variable wake-up costs 20-50 us.  ticket = (job generation << 32) | next part: a helper that is late for
    // a job sees another generation and takes nothing.
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cv;
    std::atomic<bool> stop{false}, hot{false};
    std::atomic<uint64_t> ticket{0};
    std::atomic<size_t> done{0};
    std::atomic<const std::function<void(size_t)>*> job{nullptr}; // (a helper that is late may read these while the next job is being
    std::atomic<size_t> nParts{0};                                 //  set up: its generation check then fails and it takes nothing)
    void start(unsigned n);
    void begin();                                                  // helpers start polling
    void end();                                                    // helpers go back to sleep
    void run(size_t parts, const std::function<void(size_t)>& f); // f(0..parts-1), returns when all are done; the caller works too
    bool take(uint64_t gen, size_t n, size_t& i);
    ~HostPool();
  };
  HostPool hostPool;
  uint32_t tuneZeroCopyMax = 512;      // env RTAMD_ZEROCOPY_MAX: host batches up to this many rays are traced in place in pinned host memory (0 = never)
  uint32_t tuneHostThreads = 0;        // env RTAMD_HOST_THREADS (0: min(8, hardware threads / 2))
  uint32_t tunePipeMinRays = 16384;    // env RTAMD_PIPE_MIN: host-pointer batches from this size on are pipelined in chunks
  uint32_t tunePipeChunk = 0;          // env RTAMD_PIPE_CHUNK: rays per chunk; 0 = by batch size (rt_trace.cpp, measured optima)

  // Call combiner for small host-pointer calls (rtcIntersect1 / rtcOccluded1 / short 1M streams from many threads):
  // whoever finds the device idle becomes the leader and traces everything that is pending - its own call and the
  // calls that queued up behind the previous launch - as ONE batch; the others sleep until their record is done.
  struct SmallCall
  {
    struct Scene* scene;
    char* base;
    uint32_t M;
    size_t stride;
    bool occluded;
    uint32_t instID;
    bool done = false;
    RTCError error = RTC_ERROR_NONE;
    std::string message;
  };
  // Persistent consumer for calls of up to 64 rays (trace_service.hip.h, rt_service.cpp service_trace): env RTAMD_SERVICE / config key service=1
  struct Service;
  Service* service = nullptr;
  std::mutex serviceMutex; // creation / restart of the service kernel
  uint32_t tuneService = 0;
  std::mutex combMutex;
  std::condition_variable combCv;
  std::vector<SmallCall*> combPending;
  bool combBusy = false;
  std::atomic<bool> combHold{false}; // test hook: rtcamdDebugHoldCombiner
  std::atomic<uint64_t> statLaunches{0};      // traversal kernel launches
  std::atomic<uint64_t> statServiceCalls{0};  // calls answered by the persistent service kernel
  std::atomic<uint64_t> statCombinedCalls{0}; // calls that went through the combiner
  std::atomic<uint64_t> statCombinedBatches{0}; // batches the combiner formed out of them
  uint32_t tuneRefillBatch = 8; // env RTAMD_REFILL_BATCH
  uint32_t tuneOctLeaf = 0xFFFFFFFFu; // auto: 16 for triangle leaves, 24 for grid cells (measured optima);    // env RTAMD_OCT_LEAF (trace_loop.hip.h, octet leaf step; leaves that have one)
  uint32_t tuneOctSteps = 2;    // env RTAMD_OCT_STEPS
  uint32_t tuneCbvhForm = 2;    // env RTAMD_CBVH_FORM: 0 quad form, 1 one ray per lane, 2 by the context's coherent flag (rt_trace.cpp)
  // env RTAMD_CULL=1: root cull pre-pass in front of the lane kernel (trace_cull.hip.h).  OFF by default: measured on MI355X
  // (profiles/r02_cull_ab.txt) it removes 17 % of the wave instructions of a 1 M-ray batch (40.8 M -> 6.0 M + 27.8 M) but the
  // traversal kernel, fed with survivors only, takes longer (158 -> 24 + 181 us alone) and four batches in flight gain nothing
  // (cbvh.leaf +0.7 %, triangles +5 %, eager -12 %): the kernels are bound by dependent latency at three waves per SIMD, not by
  // instruction issue.
  uint32_t tuneCull = 0;
  uint32_t tuneCullMinRays = 65536; // batches below this size go straight to the traversal kernel (the extra launch costs ~5 us)
  uint32_t tuneAloneBlocksOct = 4; // env RTAMD_ALONE_BLOCKS: workgroups per CU of a batch alone on the chip, octet-only leaf kernels
  uint32_t tuneBusyBlocksOct = 2;  // env RTAMD_BUSY_BLOCKS: the same with two or more batches running on other streams
  uint32_t tuneWalkBatch = 16;  // env RTAMD_WALK_BATCH (trace_loop.hip.h, two-stage blob visits: rays parked after the frustum test before a walk pass runs;
                                // 16 = one full pass of quads; measured 8..32, profiles/r03_two_stage_ab.txt)
  uint32_t tuneOctMax = 16;     // env RTAMD_OCT_MAX (trace_loop.hip.h, octet node step), clamped to the build's TRACE_OCT_MAX in the kernel
  // kernel tuning knobs (env RTAMD_CHUNK / RTAMD_LEAF_BATCH / RTAMD_BLOCKS_PER_CU).  Measured on MI355X, 1 M-ray batches:
  // alone on the chip every setting within chunk 128-256, leaf batch 24-40, 2-3 workgroups per CU is within +-4 %; with
  // four batches in flight 256 / 32 / 2 is +15-20 % over 128 / 24 / 3 (each kernel leaves the third wave slot of a SIMD
  // to the other batches, and takes its rays in fewer, larger grabs).
  uint32_t tuneChunk = 256, tuneLeafBatch = 32, tuneBlocksPerCU = 2;
  uint32_t tuneChunkBusy = 512; // env RTAMD_CHUNK_BUSY: upper bound of the chunk of a large batch launched while two or more others run (rt_trace.cpp launch_on)
  // env RTAMD_WG_POOL=0|1: workgroup ray pool of the lane kernel (trace_loop.hip.h RayPool); 0 = every wave grabs for itself, 1 = always shared,
  // unset (2) = shared from tuneWgPoolMinRays rays per launch on.  Measured on MI355X, cbvh.leaf, four batches in flight, parent -> pool
  // (profiles/r04_wg_pool_ab.txt): 1 M rays 13.08 -> 13.65 Grays/s, 128 k 3.45 -> 3.77, 64 k 2.02 -> 2.83, 16 k 0.83 -> 0.89, but 4 k 215 -> 173 Mrays/s:
  // 32 workgroups whose four waves wait for one grab instead of grabbing side by side.
  uint32_t tuneWgPool = 2;
  uint32_t tuneInstSpillMax = 0xFFFFFFFFu; // env RTAMD_INST_SPILL_MAX (tests): upper bound of the overflow entries per lane of a two-level launch (rt_trace.cpp launch_on)
  uint32_t tuneWgPoolMinRays = 16384;
  bool tuneChunkFixed = false; // RTAMD_CHUNK given: every batch uses exactly that chunk (otherwise small batches are cut finer, rt_trace.cpp ray_chunk_for)
  // traversal skeleton: 0 lane-per-ray (trace_loop.hip.h), 1 ray pool (trace_pool.hip.h), 2 by batch size: the pool kernel's
  // steady state is 14 % faster, its drain slower - it wins from ~2.5 M rays per launch on (env RTAMD_KERNEL=lane|pool|auto)
  uint32_t tunePoolKernel = 2;
  uint32_t tunePoolMinRays = 2500000;

  explicit Device(const char* cfg);
  ~Device() override;

  void parse(const std::string& cfg);
  void setError(RTCError code, const char* msg);
  RTCError takeError();
  void useDevice() const; // hipSetDevice(first shard) for the calling thread; throws on a gpu=none device
  void synchronize();     // all shards' streams; raises a pending stack-overflow report
  // Quad meshes are traced by the GPU kernels (trace_quad.hip): every device with a GPU takes them.  A host-only device (gpu=none) keeps
  // the geometry set of the host object model as it was - RTC_GEOMETRY_TYPE_QUAD raises INVALID_OPERATION there, as in a build without
  // the feature - unless its config names a quad accel (quad_accel=... or quad_accel_mb=...), which builds quad scenes for inspection.
  bool quads_enabled() const { return gpu >= 0 || quadAccelNamed || quadAccelMBNamed; }
  // Quad meshes with time steps follow the same rule with their own key: a host-only device whose config does not name quad_accel_mb=
  // raises INVALID_OPERATION at commit for them, as before the motion-blur quad accel existed.
  bool quads_mb_enabled() const { return gpu >= 0 || quadAccelMBNamed; }
  // Line segments with time steps, the same rule with the key line_accel_mb=: a host-only device without it raises "motion blur of line
  // segments is not supported" at commit, as before the motion-blur line accel existed.
  bool lines_mb_enabled() const { return gpu >= 0 || lineAccelMBNamed; }
  // Flat Bezier and B-spline curves, the same rule with the key hair_accel=: a host-only device without it refuses the two types at
  // rtcNewGeometry ("RTC_GEOMETRY_TYPE_*_CURVE not supported"), as before the curve accel existed.
  bool curves_enabled() const { return gpu >= 0 || hairAccelNamed; }
  // Round Bezier and B-spline curves (round_curves=1): every device that has the key, host-only ones included.  With them and the flat
  // types all five curve types are taken, which is what RTC_DEVICE_PROPERTY_CURVE_GEOMETRY_SUPPORTED speaks for.
  bool round_curves_enabled() const { return round_curves; }
  bool all_curve_types_enabled() const { return round_curves && curves_enabled(); }
  // Flat cubic curves with time steps, the rule of lines_mb_enabled() with the key hair_accel_mb=: a host-only device without it raises
  // "motion blur of flat Bezier and B-spline curves is not supported" at commit, as before the motion-blur curve accel existed.
  bool curves_mb_enabled() const { return gpu >= 0 || hairAccelMBNamed; }
  // Quad meshes inside an instanced scene, the same rule with the key inst_accel=: a host-only device without it refuses them at the top
  // scene's commit, as before the instance accel took quads.
  bool inst_quads_enabled() const { return gpu >= 0 || instAccelNamed; }
  // Instances with more than one time step, the same rule: a host-only device whose config does not name inst_accel= refuses them at
  // commit, as before the instance accel took them.
  bool inst_motion_enabled() const { return gpu >= 0 || instAccelNamed; }
  // Time-dependent top-level boxes (inst_bounds=linear) concern moving instances only: a host-only device honours the key where it takes
  // such instances at all.
  bool inst_top_linear_enabled() const { return inst_bounds == "linear" && inst_motion_enabled(); }
  // Triangle and quad meshes with time steps inside an instanced scene: a host-only device takes them only when its config names
  // inst_accel= and at least one of tri_accel_mb= / quad_accel_mb=; under any other config it refuses them as before.
  bool inst_mesh_motion_enabled() const { return gpu >= 0 || (instAccelNamed && (triAccelMBNamed || quadAccelMBNamed)); }
  // Instances of scenes that hold subdivision meshes: a host-only device takes them only when its config names inst_accel= and
  // subdiv_accel=; under any other config it refuses them as before.
  bool inst_subdiv_enabled() const { return gpu >= 0 || (instAccelNamed && subdivAccelNamed); }
  // Line segments and flat curves inside an instanced scene (inst_hair=1): a host-only device honours the key only when its config names
  // inst_accel=, and for the flat cubic curves hair_accel= as well; under any other config it refuses them as before.
  bool inst_hair_lines_enabled() const { return inst_hair && (gpu >= 0 || instAccelNamed); }
  bool inst_hair_curves_enabled() const { return inst_hair && (gpu >= 0 || (instAccelNamed && hairAccelNamed)); }
  // The same with time steps (inst_hair_mb=1, which acts only where inst_hair=1 acts): a host-only device honours the key only when its
  // config also names the motion-blur accel of the type, line_accel_mb= / hair_accel_mb=, as it builds those accels only then.
  bool inst_hair_mb_lines_enabled() const { return inst_hair_mb && inst_hair_lines_enabled() && lines_mb_enabled(); }
  bool inst_hair_mb_curves_enabled() const { return inst_hair_mb && inst_hair_curves_enabled() && curves_mb_enabled(); }
  // Time-dependent top-level boxes above moving subdivision instances (inst_subdiv_bounds=linear, independent of inst_bounds): a host-only
  // device honours the key where it takes moving subdivision instances at all.
  bool inst_subdiv_top_linear_enabled() const { return inst_subdiv_bounds == "linear" && inst_subdiv_enabled() && inst_motion_enabled(); }
  bool tuneBlocksAuto = true; // no RTAMD_BLOCKS_PER_CU given: 2 workgroups per CU, 1 when >= 2 batches run on other streams
  void memoryMonitor(ssize_t bytes, bool post);
};

// thread-local error slot used when no device exists yet (rtcNewDevice failure; device.cpp:262-263)
RTCError& thread_error();

// ---------------------------------------------------------------------------------------------------
// Buffer: owned or shared (borrowed) byte range.
// ---------------------------------------------------------------------------------------------------
struct Buffer : RefCounted
{
  Device* device;
  char* ptr = nullptr;
  size_t bytes = 0;
  bool shared = false;
  Buffer(Device* d, size_t n, void* sharedPtr);
  ~Buffer() override;
};

// A typed view into a Buffer as bound to a geometry slot (reference: RawBufferView, kernels/common/buffer.h).
struct BufferView
{
  Buffer* buf = nullptr;
  RTCFormat format = RTC_FORMAT_UNDEFINED;
  size_t offset = 0, stride = 0, count = 0;
  bool modified = true;
  const char* at(size_t i) const { return buf->ptr + offset + i * stride; }
  bool valid() const { return buf != nullptr; }
  void set(Buffer* b, RTCFormat f, size_t off, size_t str, size_t n);
  void clear();
};

// ---------------------------------------------------------------------------------------------------
// Geometry
// ---------------------------------------------------------------------------------------------------
struct Geometry : RefCounted
{
  Device* device;
  RTCGeometryType type;
  bool enabled = true;
  bool committed = false;
  unsigned mask = 0xFFFFFFFFu;
  unsigned timeSteps = 1;
  RTCBuildQuality quality = RTC_BUILD_QUALITY_MEDIUM;
  void* userPtr = nullptr;
  RTCFilterFunctionN intersectFilter = nullptr;
  RTCFilterFunctionN occludedFilter = nullptr;
  RTCDisplacementFunctionN displacement = nullptr;
  float tessellationRate = 2.0f;
  unsigned vertexAttribCount = 0;
  unsigned topologyCount = 1;
  std::vector<RTCSubdivisionMode> subdivMode{RTC_SUBDIVISION_MODE_SMOOTH_BOUNDARY};

  // buffer slots, keyed by (type, slot)
  std::map<std::pair<int, unsigned>, BufferView> views;

  // face-varying data: topology (= index buffer slot) used by each vertex attribute slot (default 0)
  std::vector<unsigned> attribTopology;
  // rtcInterpolate on subdivision meshes: refined buffers, built on first use, dropped by rtcCommitGeometry
  std::shared_ptr<void> interpCache;
  std::mutex interpMutex;

  // RTC_GEOMETRY_TYPE_INSTANCE (reference: Instance, kernels/common/scene_instance.h): the instanced scene (retained) and the
  // local-to-world transform of every time step as the columns vx, vy, vz, p of an AffineSpace3f (identity by default); an instance
  // keeps `timeSteps` of them (setInstanceTimeSteps: Instance::setNumTimeSteps, scene_instance.cpp:50-67)
  typedef std::array<float, 12> Xfm;
  static constexpr Xfm identityXfm = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
  Scene* instScene = nullptr;
  std::vector<Xfm> local2world{identityXfm};
  void setInstancedScene(Scene* s);
  void setInstanceTimeSteps(unsigned n) { local2world.resize(n, identityXfm); } // existing steps are kept, new ones are the identity
  // local-to-world at `time`: lerp(local2world[itime], local2world[itime + 1], ftime); the step itself with one time step
  void local2worldAt(float time, float* out) const;
  // the matrix the instance kernel uses for a ray at `time` (csrc/instance_xfm.h); with one time step the record's world2local of the
  // static path (invert_affine).  false: singular - `out` is all zero then
  bool world2localAt(float time, float* out) const;

  Geometry(Device* d, RTCGeometryType t);
  ~Geometry() override;

  // (view, vertex and segment are defined here: the builders of other files read every primitive through them)
  BufferView* view(RTCBufferType t, unsigned slot)
  {
    auto it = views.find({(int)t, slot});
    return it == views.end() ? nullptr : &it->second;
  }
  const BufferView* view(RTCBufferType t, unsigned slot) const
  {
    auto it = views.find({(int)t, slot});
    return it == views.end() ? nullptr : &it->second;
  }
  void bind(RTCBufferType t, unsigned slot, RTCFormat f, Buffer* b, size_t off, size_t stride, size_t count);

  // triangle mesh accessors (reference: TriangleMesh, kernels/common/scene_triangle_mesh.h)
  size_t numTriangles() const;
  size_t numVertices() const;
  void triangle(size_t i, unsigned idx[3]) const;
  V3 vertex(size_t i, unsigned slot = 0) const // slot = time step
  {
    const float* p = (const float*)view(RTC_BUFFER_TYPE_VERTEX, slot)->at(i);
    return V3(p[0], p[1], p[2]);
  }
  bool validTriangle(size_t i, unsigned slot = 0) const;
  // quad mesh accessors (reference: QuadMesh, kernels/common/scene_quad_mesh.h)
  size_t numQuads() const { return numTriangles(); } // index buffer records (UINT4 for quads)
  void quad(size_t i, unsigned idx[4]) const;
  bool validQuad(size_t i, unsigned slot = 0) const;
  // flat linear curve accessors (reference: LineSegments, kernels/common/scene_line_segments.h): segment i runs from vertex
  // index[i] to vertex index[i] + 1; vertices are (x, y, z, radius)
  size_t numSegments() const { return numTriangles(); } // index buffer records (UINT)
  unsigned segment(size_t i) const { return *(const unsigned*)view(RTC_BUFFER_TYPE_INDEX, 0)->at(i); }
  bool validSegment(size_t i, unsigned slot = 0) const; // LineSegments::valid(i, itime): against the vertex buffer of time step `slot`
  // flat cubic curve accessors (reference: NativeCurves, kernels/common/scene_bezier_curves.h): curve i uses the vertices index[i] ..
  // index[i] + 3 = (x, y, z, radius), control points of the geometry's own basis
  bool isFlatCubicCurve() const { return type == RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE || type == RTC_GEOMETRY_TYPE_FLAT_BSPLINE_CURVE; }
  // round cubic curves (round_curves=1): the buffers and the native control points of the flat cubic types, swept tubes instead of ribbons
  bool isRoundCurve() const { return type == RTC_GEOMETRY_TYPE_ROUND_BEZIER_CURVE || type == RTC_GEOMETRY_TYPE_ROUND_BSPLINE_CURVE; }
  bool isCubicCurve() const { return isFlatCubicCurve() || isRoundCurve(); }
  bool isBSplineCurve() const { return type == RTC_GEOMETRY_TYPE_FLAT_BSPLINE_CURVE || type == RTC_GEOMETRY_TYPE_ROUND_BSPLINE_CURVE; }
  size_t numCurves() const { return numTriangles(); } // index buffer records (UINT)
  bool validCurve(size_t i, unsigned slot = 0) const; // NativeCurves::valid (scene_bezier_curves.h:193-218) at one time step: against the vertex buffer of `slot`
  unsigned curveRate() const;                         // NativeCurves::setTessellationRate: clamp((int)rate, 1, 16)
  void nativeCurve(size_t i, float out[16], unsigned slot = 0) const; // the four Bezier control points of curve i at time step `slot` (B-spline input converted in float32)
};

// ---------------------------------------------------------------------------------------------------
// Scene
// ---------------------------------------------------------------------------------------------------
// One device accel: host mirror (for tests / stats) + HBM arrays.
struct Accel
{
  std::vector<QNode8> nodes;
  std::vector<QNodeMB8> nodesMB; // the kinds ACCEL_*MB_LINEAR_* (mb_bounds=linear): their time-dependent nodes, `nodes` is empty then;
                                 // the kinds ACCEL_INSTMESHMB_LINEAR_* / ACCEL_INSTTOP_LINEAR_* / ACCEL_INSTSUBDIV_TOP_LINEAR_*: the second section of the node array, behind `nodes`
  std::vector<uint8_t> nodeImage; // the kinds ACCEL_INSTMESHMB_LINEAR_* / ACCEL_INSTTOP_LINEAR_* / ACCEL_INSTSUBDIV_TOP_LINEAR_*: `nodes` | zero padding to a multiple of 144 bytes | `nodesMB`, as uploaded
  std::vector<TriRecord> prims;
  std::vector<uint8_t> blobs;
  std::vector<uint32_t> blobOffsets;
  uint32_t root = REF_EMPTY;
  uint32_t kind = ACCEL_NONE;
  uint32_t robust = 0;
  uint32_t maxDepth = 0;
  uint32_t blobStride = 0;
  uint32_t instHair = 0;   // kinds ACCEL_INSTMESHMB_*: 1 = an instanced scene has a curve or a line tree (inst_hair=1; accel.h InstanceSceneRecord), 2 = one has a motion-blur curve or line tree as well (inst_hair_mb=1) -> LaunchParams::instHair
  uint32_t roundCurves = 0; // kinds ACCEL_CURVE_*: 1 = the records are round curves (Scene::roundCurveAccel): launch_trace_curve diverts to launch_trace_round_curve -> LaunchParams::roundCurves
  uint32_t cbvhLevels = 0; // ACCEL_INSTSUBDIV_CBVH_LEAF / ACCEL_INSTSUBDIV_TOP_LINEAR_CBVH_LEAF: the compression level C of the instanced scenes' blobs (0: the scene's own level applies)
  size_t leafCount = 0;
  // device copies, one set per shard of the device (replicated accel)
  struct DevCopy
  {
    void* dNodes = nullptr;
    void* dPrims = nullptr;
    void* dBlobs = nullptr;
    void* dBlobOffsets = nullptr;
  };
  std::vector<DevCopy> dev;
  std::vector<int> devOrdinals; // ordinal each copy lives on (for freeDevice)
  AccelDesc desc(size_t shard = 0) const;
  // the node array whichever of the two it is: what is counted and - see nodeImage*() - uploaded and handed out for inspection.  The kinds
  // ACCEL_INSTMESHMB_LINEAR_* / ACCEL_INSTTOP_LINEAR_* / ACCEL_INSTSUBDIV_TOP_LINEAR_* hold both: these three describe their QNode8 section
  // (static trees, and in the kinds 30 / 31 the top-level tree), the QNodeMB8 section is described by the accel's two blobOffsets words
  // (the kinds 34 / 35: its words 2 and 3)
  // (nodesAreMB: the instance builder asks it of the triangle and quad motion-blur accels of an instanced scene only; a scene with a
  // motion-blur line or curve accel is refused below an instance before it gets there unless inst_hair_mb=1 takes it, which asks the same of
  // those two and refuses QNodeMB8s; the static ones hold QNode8s)
  bool nodesAreMB() const { return kind_row(kind).nodes == NODES_MB8; }
  bool twoSections() const { return kind_row(kind).nodes == NODES_TWO_SECTION; }
  size_t nodeCount() const { return nodesAreMB() ? nodesMB.size() : nodes.size(); }
  size_t nodeStride() const { return nodesAreMB() ? sizeof(QNodeMB8) : sizeof(QNode8); }
  const void* nodeData() const { return nodesAreMB() ? (const void*)nodesMB.data() : (const void*)nodes.data(); }
  // the bytes of the device's node buffer
  size_t nodeImageBytes() const { return twoSections() ? nodeImage.size() : nodeCount() * nodeStride(); }
  const void* nodeImageData() const { return twoSections() ? (const void*)nodeImage.data() : nodeData(); }
  bool traceable() const { return kind != ACCEL_NONE && root != REF_EMPTY; } // a launch on anything else returns before it touches the GPU
  size_t deviceBytes() const;
  void upload(Device* dev);
  void freeDevice();
  void clear();
};

struct Scene : RefCounted
{
  Device* device;
  std::vector<Geometry*> geometries; // index = geomID, nullptr = free slot
  RTCSceneFlags flags = RTC_SCENE_FLAG_NONE;
  RTCBuildQuality quality = RTC_BUILD_QUALITY_MEDIUM;
  unsigned subdivisionLevel = 6; // fork defaults, kernels/common/scene.cpp:41-42
  unsigned compressionLevel = 3;
  RTCProgressMonitorFunction progressFn = nullptr;
  void* progressUser = nullptr;
  bool modified = true; // "scene got not committed" until the first commit (scene.cpp:25,54)
  // filter callbacks present at commit time (Scene::hasGeometryFilterFunction, scene.h): they route a batch through the
  // host filter loop of rt_filter.cpp (the tri* flags cover quad meshes too)
  bool triIntersectFilter = false, triOccludedFilter = false, subdivFilter = false;
  bool lineIntersectFilter = false, lineOccludedFilter = false; // the same for flat linear and flat cubic curves (reported with the meshes' flags)
  // the same for what lies below this scene's mesh instances (inst_filters=1; build_instance_accel, at this scene's commit): an enabled
  // geometry with an intersect / occluded filter in the scene of a placed instance
  bool instIntersectFilter = false, instOccludedFilter = false;
  std::mutex buildMutex;
  Box3 bounds;

  std::vector<uint8_t> debugGrids; // keep_grids=1: per patch {geomID,primID,n} + x[],y[],z[] of the (n+1)^2 grid

  Accel triAccel;    // triangles with one time step
  Accel triMBAccel;  // triangles with several time steps (TriMBRecord[] in `blobs`); traced after the static triangles, before the quads (scene.cpp:650-654)
  Accel quadAccel;   // quads with one time step (QuadRecord[] in `blobs`); traced after the triangles, before the motion-blur quads
  Accel quadMBAccel; // quads with several time steps (QuadMBRecord[] in `blobs`); traced after the static quads, before the subdivision patches
  Accel subdivAccel; // subdivision patches (cBVH / GridSOA leaves)
  Accel curveAccel;  // flat Bezier and B-spline curves (CurveRecord[] in `blobs`); traced after the subdivision patches and before the line segments (scene.cpp:654-658: createSubdivAccel, createHairAccel, createLineAccel)
  Accel curveMBAccel; // flat Bezier and B-spline curves with several time steps (CurveMBRecord[] in `blobs`); traced right after the static curves (scene.cpp:370-441: createHairAccel, createHairMBAccel)
  Accel lineAccel;   // flat linear curves (LineRecord[] in `blobs`); traced after the subdivision patches, before the instances (scene.cpp:650-663)
  Accel lineMBAccel; // flat linear curves with several time steps (LineMBRecord[] in `blobs`); traced right after the static lines (scene.cpp: createLineAccel, createLineMBAccel)
  Accel instAccel;   // instances (InstanceRecord[] in `blobs`, the instanced scenes' triangle and quad trees behind the top-level tree); traced last (scene.cpp:661-665)
  Accel roundCurveAccel; // round Bezier and B-spline curves (round_curves=1; CurveRecord[] with N = 0 in `blobs`, kinds ACCEL_CURVE_* with Accel::roundCurves); traced last
  Accel instSubdivAccel; // instances of scenes that hold subdivision meshes only (InstanceRecord[] and the instanced scenes' leaf blobs in `blobs`, their BVH8s behind the top-level tree); traced after the mesh instances
  // the accel slots in trace order (one row each in SCENE_SLOTS below); they index whatever a path keeps per accel
  enum { TRI = 0, TRIMB = 1, QUAD = 2, QUADMB = 3, SUBDIV = 4, CURVE = 5, CURVEMB = 6, LINE = 7, LINEMB = 8, INST = 9, INSTSUBDIV = 10, ROUND = 11, NUM_ACCELS = 12 };
  std::array<Accel*, NUM_ACCELS> accels();
  bool hasInstances() const { return instAccel.kind != ACCEL_NONE || instSubdivAccel.kind != ACCEL_NONE; }
  // records the layout of instAccel placed in `blobs` behind the InstanceRecords, as build_instance_accel counted them (host only: the
  // verbose line of commit prints them)
  struct InstanceCounts { size_t quads = 0, steps = 0, triMB = 0, quadMB = 0, curves = 0, lines = 0, curveMB = 0, lineMB = 0; };
  InstanceCounts instCounts;

  explicit Scene(Device* d);
  ~Scene() override;

  unsigned attach(Geometry* g);
  void attachByID(Geometry* g, unsigned id);
  void detach(unsigned id);
  Geometry* get(unsigned id) const;
  void commit();
  bool isRobust() const { return (flags & RTC_SCENE_FLAG_ROBUST) != 0; }
};

// affine maps as the columns vx, vy, vz, p (rt_scene.cpp): the inverse, false for a singular map; xfmPoint
bool invert_affine(const float* m, float* out);
V3 xfm_point(const float* m, V3 q);

// the builders of a scene's accels (rt_prim_build.cpp, subdiv_build.cpp, rt_instance_build.cpp); Scene::commit runs them in slot order
void build_triangle_accel(Scene* s), build_trimb_accel(Scene* s), build_quad_accel(Scene* s), build_quadmb_accel(Scene* s), build_subdiv_accel(Scene* s),
    build_curve_accel(Scene* s), build_curvemb_accel(Scene* s), build_line_accel(Scene* s), build_linemb_accel(Scene* s), build_instance_accel(Scene* s),
    build_instance_subdiv_accel(Scene* s), build_round_curve_accel(Scene* s);

// One row per accel slot of a scene, in trace order - which is also Scene::commit's build order: where a scene has several faults, the
// order decides which refusal is reported, and build_instance_subdiv_accel relies on build_instance_accel having refused instances without
// a committed scene.  Adding a slot: an Accel member, an enum value and a row ("Adding a kind / adding a slot").
enum SlotSteps : uint8_t { STEPS_ONE, STEPS_SEVERAL, STEPS_ANY };
struct SlotRow
{
  int slot;                  // Scene::TRI .. (checked against the row's place below)
  Accel Scene::*accel;
  void (*build)(Scene*);
  // the verbose=2 line of an accel that keeps fixed-size records in `blobs` (Scene::commit); label nullptr: the slot has a line of its own
  const char *label, *records;
  size_t recordBytes;
  // the geometries that land in the slot: their type is one of `types` (a slot of one type names it twice) and their time step count fits `steps`
  RTCGeometryType types[2];
  SlotSteps steps;
  // the slot's exclusion list in a filter re-trace (rt_excl_list.h): entries carry the bits of t / the instance as well
  bool keyedByT, withInst;
  int exportRank;            // place in the order in which the inspection calls look for the first accel that is not empty (exported_accel)
};
inline constexpr SlotRow SCENE_SLOTS[] = {
  // triangles: (geomID, primID) names the candidate.  With time steps: one record per segment, a ray sees one segment, so the pair still does
  {Scene::TRI, &Scene::triAccel, build_triangle_accel, nullptr, nullptr, 0, {RTC_GEOMETRY_TYPE_TRIANGLE, RTC_GEOMETRY_TYPE_TRIANGLE}, STEPS_ONE, false, false, 1},
  {Scene::TRIMB, &Scene::triMBAccel, build_trimb_accel, "motion blur triangle", "segment records", sizeof(TriMBRecord), {RTC_GEOMETRY_TYPE_TRIANGLE, RTC_GEOMETRY_TYPE_TRIANGLE}, STEPS_SEVERAL, false, false, 2},
  // quads, static and (as for the moving triangles) with time steps: the two triangles of the quad are told apart by t
  {Scene::QUAD, &Scene::quadAccel, build_quad_accel, "quad", "quads", sizeof(QuadRecord), {RTC_GEOMETRY_TYPE_QUAD, RTC_GEOMETRY_TYPE_QUAD}, STEPS_ONE, true, false, 3},
  {Scene::QUADMB, &Scene::quadMBAccel, build_quadmb_accel, "motion blur quad", "segment records", sizeof(QuadMBRecord), {RTC_GEOMETRY_TYPE_QUAD, RTC_GEOMETRY_TYPE_QUAD}, STEPS_SEVERAL, true, false, 4},
  // eager grid cells: the triangles of a patch share (geomID, primID), t tells them apart
  {Scene::SUBDIV, &Scene::subdivAccel, build_subdiv_accel, nullptr, nullptr, 0, {RTC_GEOMETRY_TYPE_SUBDIVISION, RTC_GEOMETRY_TYPE_SUBDIVISION}, STEPS_ANY, true, false, 0},
  // the ribbon leaf offers up to N candidates per curve and ray, one per ribbon quad, all with the curve's (geomID, primID): t tells them apart,
  // so a second quad of a rejected curve can still be found (the retry loop of Intersect1EpilogMU, intersector_epilog.h:488-509)
  {Scene::CURVE, &Scene::curveAccel, build_curve_accel, "curve", "curves", sizeof(CurveRecord), {RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE, RTC_GEOMETRY_TYPE_FLAT_BSPLINE_CURVE}, STEPS_ONE, true, false, 5},
  // the motion-blur ribbon leaf: a ray sees one time segment's record of a curve, and that record offers up to N candidates told apart by t
  {Scene::CURVEMB, &Scene::curveMBAccel, build_curvemb_accel, "motion blur curve", "segment records", sizeof(CurveMBRecord), {RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE, RTC_GEOMETRY_TYPE_FLAT_BSPLINE_CURVE}, STEPS_SEVERAL, true, false, 6},
  // the line leaf scans with candidate_excluded(), which compares t as well (one candidate per segment and ray: t adds nothing, and takes nothing away)
  {Scene::LINE, &Scene::lineAccel, build_line_accel, "line", "segments", sizeof(LineRecord), {RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE, RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE}, STEPS_ONE, true, false, 7},
  // the motion-blur line leaf scans the same way: one record per time segment and a ray sees one segment, so (geomID, primID) names the candidate
  {Scene::LINEMB, &Scene::lineMBAccel, build_linemb_accel, "motion blur line", "segment records", sizeof(LineMBRecord), {RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE, RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE}, STEPS_SEVERAL, true, false, 8},
  // below a mesh instance: (instance, geomID, primID, bits of t) for every leaf type
  {Scene::INST, &Scene::instAccel, build_instance_accel, nullptr, nullptr, 0, {RTC_GEOMETRY_TYPE_INSTANCE, RTC_GEOMETRY_TYPE_INSTANCE}, STEPS_ANY, true, true, 9},
  // (no filter runs below a subdivision instance: the list stays empty)
  {Scene::INSTSUBDIV, &Scene::instSubdivAccel, build_instance_subdiv_accel, nullptr, nullptr, 0, {RTC_GEOMETRY_TYPE_INSTANCE, RTC_GEOMETRY_TYPE_INSTANCE}, STEPS_ANY, false, false, 10},
  // the tube leaf offers a front and a back candidate per curve and ray (entry and exit), both with the curve's (geomID, primID): t tells them apart.
  // Last, so that no older slot number, export rank, exclusion list or wave-log slice moves; a round curve with time steps fits no slot
  {Scene::ROUND, &Scene::roundCurveAccel, build_round_curve_accel, "round curve", "curves", sizeof(CurveRecord), {RTC_GEOMETRY_TYPE_ROUND_BEZIER_CURVE, RTC_GEOMETRY_TYPE_ROUND_BSPLINE_CURVE}, STEPS_ONE, true, false, 11},
};
static_assert(sizeof(SCENE_SLOTS) / sizeof(SCENE_SLOTS[0]) == Scene::NUM_ACCELS, "every accel slot needs a row in SCENE_SLOTS");
constexpr bool scene_slots_in_order(int i = 0) { return i == Scene::NUM_ACCELS || (SCENE_SLOTS[i].slot == i && scene_slots_in_order(i + 1)); }
static_assert(scene_slots_in_order(), "the rows of SCENE_SLOTS stand in slot order");

inline std::array<Accel*, Scene::NUM_ACCELS> Scene::accels()
{
  std::array<Accel*, NUM_ACCELS> a;
  for (const SlotRow& r : SCENE_SLOTS) a[r.slot] = &(this->*r.accel);
  return a;
}

// the slot a geometry's primitives land in (the two instance slots share a type: the first, Scene::INST); -1: no slot takes its type
inline int slot_of(const Geometry* g)
{
  for (const SlotRow& r : SCENE_SLOTS)
    if ((g->type == r.types[0] || g->type == r.types[1]) && (r.steps == STEPS_ANY || (r.steps == STEPS_SEVERAL) == (g->timeSteps > 1))) return r.slot;
  return -1;
}

} // namespace rtamd
