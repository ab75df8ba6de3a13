// Geometry / Scene objects, accel selection at commit, upload to HBM.
#include <algorithm>
#include <map>

#include "bvh8_builder.h"
#include "instance_xfm.h"
#include "rt_objects.h"
#include "rt_trace.h"
#include "subdiv_build.h"

namespace rtamd {

// ---- Geometry -------------------------------------------------------------------------------------------
Geometry::Geometry(Device* d, RTCGeometryType t) : device(d), type(t) { device->retain(); }

Geometry::~Geometry()
{
  for (auto& kv : views) kv.second.clear();
  if (instScene) instScene->release();
  device->release();
}

void Geometry::setInstancedScene(Scene* s)
{
  if (type != RTC_GEOMETRY_TYPE_INSTANCE) RT_THROW(RTC_ERROR_INVALID_OPERATION, "operation not supported for this geometry");
  if (s->device != device) RT_THROW(RTC_ERROR_INVALID_OPERATION, "inputs are from different devices");
  s->retain();
  if (instScene) instScene->release();
  instScene = s;
  committed = false;
}

BufferView* Geometry::view(RTCBufferType t, unsigned slot)
{
  auto it = views.find({(int)t, slot});
  return it == views.end() ? nullptr : &it->second;
}

const BufferView* Geometry::view(RTCBufferType t, unsigned slot) const
{
  auto it = views.find({(int)t, slot});
  return it == views.end() ? nullptr : &it->second;
}

static size_t format_bytes(RTCFormat f)
{
  const unsigned fam = ((unsigned)f) >> 12, n = ((unsigned)f) & 0xfff;
  if (f == RTC_FORMAT_UNDEFINED) return 0;
  if (((unsigned)f & 0xf00) != 0) { // matrices 0x9RCc
    const unsigned r = (n >> 4) & 0xf, c = n & 0xf;
    return 4 * r * c;
  }
  static const size_t scalar[10] = {0, 1, 1, 2, 2, 4, 4, 8, 8, 4};
  return fam < 10 ? scalar[fam] * n : 0;
}

void Geometry::bind(RTCBufferType t, unsigned slot, RTCFormat f, Buffer* b, size_t off, size_t stride, size_t count)
{
  // argument checks follow rtcSetGeometryBuffer (rtcore.cpp:1236-1290) and TriangleMesh::setBuffer
  // (scene_triangle_mesh.cpp): 4-byte aligned offset/stride, matching formats per slot type.
  if ((off & 3) || (stride & 3)) RT_THROW(RTC_ERROR_INVALID_OPERATION, "buffer offset and stride must be 4-byte aligned");
  if (b && off + (count ? (count - 1) * stride + format_bytes(f) : 0) > b->bytes && !b->shared)
    RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "buffer range out of bounds");
  switch (type) {
  case RTC_GEOMETRY_TYPE_TRIANGLE:
  case RTC_GEOMETRY_TYPE_QUAD: // TriangleMesh::setBuffer / QuadMesh::setBuffer (scene_quad_mesh.cpp): the index format differs
    if (t == RTC_BUFFER_TYPE_VERTEX) {
      if (f != RTC_FORMAT_FLOAT3) RT_THROW(RTC_ERROR_INVALID_OPERATION, "invalid vertex buffer format");
    } else if (t == RTC_BUFFER_TYPE_INDEX) {
      if (slot != 0) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "invalid buffer slot");
      if (f != (type == RTC_GEOMETRY_TYPE_QUAD ? RTC_FORMAT_UINT4 : RTC_FORMAT_UINT3)) RT_THROW(RTC_ERROR_INVALID_OPERATION, "invalid index buffer format");
    } else if (t != RTC_BUFFER_TYPE_VERTEX_ATTRIBUTE)
      RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown buffer type");
    break;
  case RTC_GEOMETRY_TYPE_SUBDIVISION:
    if (t == RTC_BUFFER_TYPE_VERTEX && f != RTC_FORMAT_FLOAT3) RT_THROW(RTC_ERROR_INVALID_OPERATION, "invalid vertex buffer format");
    if ((t == RTC_BUFFER_TYPE_INDEX || t == RTC_BUFFER_TYPE_FACE) && f != RTC_FORMAT_UINT)
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "invalid index/face buffer format");
    break;
  default: break;
  }
  if (t == RTC_BUFFER_TYPE_VERTEX && slot >= timeSteps) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "invalid vertex buffer slot");
  views[{(int)t, slot}].set(b, f, off, stride, count);
  committed = false;
}

size_t Geometry::numTriangles() const
{
  const BufferView* v = view(RTC_BUFFER_TYPE_INDEX, 0);
  return v && v->valid() ? v->count : 0;
}

size_t Geometry::numVertices() const
{
  const BufferView* v = view(RTC_BUFFER_TYPE_VERTEX, 0);
  return v && v->valid() ? v->count : 0;
}

void Geometry::triangle(size_t i, unsigned idx[3]) const
{
  const unsigned* p = (const unsigned*)view(RTC_BUFFER_TYPE_INDEX, 0)->at(i);
  idx[0] = p[0]; idx[1] = p[1]; idx[2] = p[2];
}

V3 Geometry::vertex(size_t i, unsigned slot) const
{
  const float* p = (const float*)view(RTC_BUFFER_TYPE_VERTEX, slot)->at(i);
  return V3(p[0], p[1], p[2]);
}

// the vertex test of TriangleMesh::valid / QuadMesh::valid: every index in range, every vertex finite and within FLT_LARGE
static bool valid_vertices(const Geometry& g, const unsigned* idx, int n, unsigned slot = 0)
{
  const BufferView* vv = g.view(RTC_BUFFER_TYPE_VERTEX, slot);
  const size_t nv = vv && vv->valid() ? vv->count : 0;
  for (int k = 0; k < n; k++) {
    if (idx[k] >= nv) return false;
    V3 p = g.vertex(idx[k], slot);
    if (!(std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z))) return false;
    if (fabsf(p.x) > 1.844e18f || fabsf(p.y) > 1.844e18f || fabsf(p.z) > 1.844e18f) return false; // FLT_LARGE
  }
  return true;
}

// TriangleMesh::valid (scene_triangle_mesh.h)
bool Geometry::validTriangle(size_t i, unsigned slot) const
{
  unsigned idx[3];
  triangle(i, idx);
  return valid_vertices(*this, idx, 3, slot);
}

void Geometry::quad(size_t i, unsigned idx[4]) const
{
  const unsigned* p = (const unsigned*)view(RTC_BUFFER_TYPE_INDEX, 0)->at(i);
  idx[0] = p[0]; idx[1] = p[1]; idx[2] = p[2]; idx[3] = p[3];
}

// QuadMesh::valid (scene_quad_mesh.h:121-138)
bool Geometry::validQuad(size_t i, unsigned slot) const
{
  unsigned idx[4];
  quad(i, idx);
  return valid_vertices(*this, idx, 4, slot);
}

// ---- Accel -------------------------------------------------------------------------------------------------
AccelDesc Accel::desc(size_t shard) const
{
  AccelDesc d;
  const DevCopy c = shard < dev.size() ? dev[shard] : DevCopy();
  d.nodes = (const QNode8*)c.dNodes;
  d.prims = (const TriRecord*)c.dPrims;
  d.blobs = (const uint8_t*)c.dBlobs;
  d.blobOffsets = (const uint32_t*)c.dBlobOffsets;
  d.root = root;
  d.kind = kind;
  d.robust = robust;
  d.blobStride = blobStride;
  return d;
}

size_t Accel::deviceBytes() const
{
  return nodeImageBytes() + prims.size() * sizeof(TriRecord) + blobs.size() + blobOffsets.size() * 4;
}

void Accel::freeDevice()
{
  for (size_t i = 0; i < dev.size(); i++) {
    DevCopy& c = dev[i];
    if (!(c.dNodes || c.dPrims || c.dBlobs || c.dBlobOffsets)) continue;
    hipSetDevice(devOrdinals[i]);
    if (c.dNodes) hipFree(c.dNodes);
    if (c.dPrims) hipFree(c.dPrims);
    if (c.dBlobs) hipFree(c.dBlobs);
    if (c.dBlobOffsets) hipFree(c.dBlobOffsets);
  }
  dev.clear();
  devOrdinals.clear();
}

void Accel::clear()
{
  nodes.clear();
  nodesMB.clear();
  nodeImage.clear();
  prims.clear();
  blobs.clear();
  blobOffsets.clear();
  root = REF_EMPTY;
  kind = ACCEL_NONE;
  maxDepth = 0;
  cbvhLevels = 0;
  leafCount = 0;
}

static void* upload_array(hipStream_t stream, const void* src, size_t bytes)
{
  if (bytes == 0) return nullptr;
  void* d = nullptr;
  HIP_CHECK(hipMalloc(&d, bytes + 64)); // slack: kernels may over-read one record at the array end
  HIP_CHECK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, stream));
  return d;
}

// The accel is replicated: one copy per shard of the device, uploaded on the shard's own stream.
void Accel::upload(Device* device)
{
  freeDevice();
  if (device->gpu < 0) return; // host-only device: keep the host mirror for inspection
  device->useDevice();
  dev.resize(device->shards.size());
  devOrdinals.resize(device->shards.size());
  for (size_t i = 0; i < device->shards.size(); i++) {
    Device::GpuShard& sh = *device->shards[i];
    sh.use();
    devOrdinals[i] = sh.ordinal;
    DevCopy& c = dev[i];
    c.dNodes = upload_array(sh.stream, nodeImageData(), nodeImageBytes());
    c.dPrims = upload_array(sh.stream, prims.data(), prims.size() * sizeof(TriRecord));
    c.dBlobs = upload_array(sh.stream, blobs.data(), blobs.size());
    c.dBlobOffsets = upload_array(sh.stream, blobOffsets.data(), blobOffsets.size() * 4);
  }
  for (auto& sh : device->shards) {
    sh->use();
    HIP_CHECK(hipStreamSynchronize(sh->stream));
  }
  device->useDevice();
}

// ---- Scene ---------------------------------------------------------------------------------------------------
Scene::Scene(Device* d) : device(d) { device->retain(); }

Scene::~Scene()
{
  service_quiesce(device); // freeing device memory synchronises the device: do not wait for the resident service kernel's idle exit
  for (Accel* a : accels()) a->freeDevice();
  if (device->gpu >= 0) hipSetDevice(device->gpu);
  for (Geometry* g : geometries)
    if (g) g->release();
  device->release();
}

unsigned Scene::attach(Geometry* g)
{
  unsigned id = 0;
  while (id < geometries.size() && geometries[id]) id++; // lowest free ID, like the reference's IDPool (scene.cpp:575-590)
  attachByID(g, id);
  return id;
}

void Scene::attachByID(Geometry* g, unsigned id)
{
  if (id == RTC_INVALID_GEOMETRY_ID) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "invalid geometry ID");
  if (id >= geometries.size()) geometries.resize(id + 1, nullptr);
  if (geometries[id]) RT_THROW(RTC_ERROR_INVALID_OPERATION, "geometry ID already in use");
  g->retain();
  geometries[id] = g;
  modified = true;
}

void Scene::detach(unsigned id)
{
  if (id >= geometries.size() || !geometries[id]) RT_THROW(RTC_ERROR_INVALID_OPERATION, "invalid geometry");
  geometries[id]->release();
  geometries[id] = nullptr;
  modified = true;
}

Geometry* Scene::get(unsigned id) const { return id < geometries.size() ? geometries[id] : nullptr; }

// The frame of the triangle and quad builders: one BVH8 (block 4, min leaf 4, max leaf 28: bvh_builder_sah.cpp:651-658) over the valid
// primitives, NV vertices each, of the scene's enabled geometries of `type`.  A leaf's records are appended to `recs` in leaf order:
// fill(rec, v) writes the vertices into a zeroed record, geomID / primID are set here.  false (and `A` untouched): no primitive.
template <int NV, class Rec, class Fill>
static bool build_mesh_bvh8(Scene* s, Accel& A, RTCGeometryType type, const char* tooMany, std::vector<Rec>& recs, const Fill& fill)
{
  struct Src { unsigned geomID, primID; };
  std::vector<Src> src;
  std::vector<BuildPrim> bp;
  // the index record of a primitive (UINT3 / UINT4), and its vertices
  auto vertices = [](const Geometry* g, size_t i, V3* v) {
    const unsigned* idx = (const unsigned*)g->view(RTC_BUFFER_TYPE_INDEX, 0)->at(i);
    for (int k = 0; k < NV; k++) v[k] = g->vertex(idx[k]);
  };
  for (unsigned gid = 0; gid < s->geometries.size(); gid++) {
    Geometry* g = s->geometries[gid];
    if (!g || !g->enabled || g->type != type) continue;
    if (g->timeSteps != 1) {
      if (type == RTC_GEOMETRY_TYPE_TRIANGLE) continue; // build_trimb_accel
      if (s->device->quads_mb_enabled()) continue;      // build_quadmb_accel
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "motion blur geometry is not supported by the device path");
    }
    const size_t n = g->numTriangles(); // index buffer records
    for (size_t i = 0; i < n; i++) {
      if (!(NV == 4 ? g->validQuad(i) : g->validTriangle(i))) continue;
      V3 v[NV];
      vertices(g, i, v);
      BuildPrim p;
      for (int k = 0; k < NV; k++) p.box.extend(v[k]);
      p.id = (uint32_t)src.size();
      src.push_back({gid, (unsigned)i});
      bp.push_back(p);
    }
  }
  if (bp.empty()) return false;
  if (bp.size() >= ((size_t)1 << TRI_START_BITS)) RT_THROW(RTC_ERROR_INVALID_OPERATION, tooMany);

  recs.reserve(bp.size());
  auto makeLeaf = [&](const BuildPrim* prims, size_t begin, size_t end) -> uint32_t {
    const uint32_t first = (uint32_t)recs.size();
    for (size_t i = begin; i < end; i++) {
      const Src& sr = src[prims[i].id];
      V3 v[NV];
      vertices(s->geometries[sr.geomID], sr.primID, v);
      Rec r;
      memset(&r, 0, sizeof(r));
      fill(r, v);
      r.geomID = sr.geomID;
      r.primID = sr.primID;
      recs.push_back(r);
    }
    return make_tri_leaf(first, (uint32_t)(end - begin));
  };
  BuildSettings cfg;
  cfg.threads = host_threads(s->device);
  BuildResult r = build_bvh8(bp, cfg, makeLeaf);
  A.nodes = std::move(r.nodes);
  A.root = r.root;
  A.maxDepth = r.maxDepth;
  A.leafCount = r.leafCount;
  for (const BuildPrim& p : bp) s->bounds.extend(p.box);
  return true;
}

static void build_triangle_accel(Scene* s)
{
  Accel& A = s->triAccel;
  A.clear();

  // accel selection: scene.cpp:130-211.  Everything is served by the one BVH8 layout; the name only picks
  // the leaf arithmetic (Triangle4v/Pluecker/robust vs Triangle4/Moeller/fast).
  const std::string& name = s->device->tri_accel;
  bool pluecker;
  if (name == "default") pluecker = s->isRobust();
  else if (name == "bvh8.triangle4v" || name == "bvh4.triangle4v") pluecker = true;
  else if (name == "bvh8.triangle4" || name == "bvh4.triangle4" || name == "qbvh8.triangle4") pluecker = false;
  else RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown triangle acceleration structure " + name);
  A.kind = pluecker ? ACCEL_TRI_PLUECKER : ACCEL_TRI_MOELLER;
  A.robust = pluecker ? 1 : 0;

  auto fill = [pluecker](TriRecord& t, const V3* v) {
    t.ax = v[0].x; t.ay = v[0].y; t.az = v[0].z;
    if (pluecker) {
      t.bx = v[1].x; t.by = v[1].y; t.bz = v[1].z;
      t.cx = v[2].x; t.cy = v[2].y; t.cz = v[2].z;
    } else { // TriangleM ctor: e1 = v0-v1, e2 = v2-v0 (triangle.h:52-53)
      t.bx = v[0].x - v[1].x; t.by = v[0].y - v[1].y; t.bz = v[0].z - v[1].z;
      t.cx = v[2].x - v[0].x; t.cy = v[2].y - v[0].y; t.cz = v[2].z - v[0].z;
    }
  };
  if (!build_mesh_bvh8<3>(s, A, RTC_GEOMETRY_TYPE_TRIANGLE, "too many triangles for the 26-bit leaf reference", A.prims, fill)) A.kind = ACCEL_NONE;
}

// Quad meshes: one BVH8 over whole quads with the triangle settings; the records keep the four vertices (QuadMv) and go to the
// accel's byte array.  Accel choice (scene.cpp:251-330, bvh8_factory.h:43): default = Pluecker + robust traversal for a robust scene,
// Moeller + fast traversal otherwise; an explicit quad4v / quad4i accel is the fast (Moeller) variant.
static void build_quad_accel(Scene* s)
{
  Accel& A = s->quadAccel;
  A.clear();
  const std::string& name = s->device->quad_accel;
  bool pluecker;
  if (name == "default") pluecker = s->isRobust();
  else if (name == "bvh8.quad4v" || name == "bvh4.quad4v" || name == "bvh8.quad4i" || name == "bvh4.quad4i" || name == "qbvh8.quad4i") pluecker = false;
  else RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown quad acceleration structure " + name);

  std::vector<QuadRecord> recs;
  auto fill = [](QuadRecord& q, const V3* v) {
    q.v0x = v[0].x; q.v0y = v[0].y; q.v0z = v[0].z;
    q.v1x = v[1].x; q.v1y = v[1].y; q.v1z = v[1].z;
    q.v2x = v[2].x; q.v2y = v[2].y; q.v2z = v[2].z;
    q.v3x = v[3].x; q.v3y = v[3].y; q.v3z = v[3].z;
  };
  if (!build_mesh_bvh8<4>(s, A, RTC_GEOMETRY_TYPE_QUAD, "too many quads for the 26-bit leaf reference", recs, fill)) return;
  A.kind = pluecker ? ACCEL_QUAD_PLUECKER : ACCEL_QUAD_MOELLER; // only once there are quads
  A.robust = pluecker ? 1 : 0;
  A.blobStride = sizeof(QuadRecord);
  A.blobs.resize(recs.size() * sizeof(QuadRecord));
  memcpy(A.blobs.data(), recs.data(), A.blobs.size());
}

// The frame of the motion-blur builders, as build_mesh_bvh8 is the one of the static builders: one BVH8 with the triangle settings over
// (primitive, time segment) pairs of the scene's enabled geometries of `type` with more than one time step.  A pair's box is the union
// of the primitive's boxes at the two ends of the segment - the vertices move on straight lines in between, so the box holds the
// primitive at every time of the segment (and, by the same argument, NOT at extrapolated times: a ray with a time outside [0, 1] sees
// the first / last segment only where it still is inside its box).  A pair gets a record only when the primitive is valid at both ends.
// fill(rec, v) writes the 2 * NV vertices (segment start, then segment end) into a zeroed record; the four id words are set here.
// false (and `A` untouched): no record.
// mb_bounds=linear (Device::mb_bounds): the same pairs, records and leaf conventions under time-dependent nodes (accel.h QNodeMB8, `A.nodesMB`).
//  * Topology: the SAH build runs over every pair's box at ONE instant, the midpoint of its segment (the box of the vertices'
//    midpoints) - not over the swept unions, whose overlap is what stops the swept build early on anything that really moves.
//  * Bounds, per child of every node, over the pairs below it (linear_bounds): two boxes B(0), B(1) whose interpolation holds every
//    pair at both ends of its segment, at the global times seg / S and (seg + 1) / S.  First guess: the union of the start boxes of
//    the pairs of segment 0 and the union of the end boxes of the pairs of the last segment (of all pairs when there is none); then
//    both ends are widened, per plane, by the largest amount any pair end sticks out of the interpolated guess (the reference's
//    linearBounds, kernels/common/scene_triangle_mesh.h).  For meshes with two time steps every end lies at time 0 or 1, nothing
//    sticks out, and the result is exactly the bounds at step 0 and at step 1.  Computed in double and rounded outward to fp32; what
//    double loses is covered, far over, by the quantizer's one-step padding.
//  * Scene::bounds is extended by the swept boxes, as in the swept build.
template <int NV, class Rec, class Fill>
static bool build_mb_bvh8(Scene* s, Accel& A, RTCGeometryType type, const char* tooMany, std::vector<Rec>& recs, const Fill& fill)
{
  const bool linear = s->device->mb_bounds == "linear";
  struct Src { unsigned geomID, primID, segment; };
  struct Ends { Box3 a, b; double ta, tb; }; // linear: a pair's boxes at the start / end of its segment and their global times
  std::vector<Src> src;
  std::vector<Ends> ends;
  std::vector<BuildPrim> bp;
  Box3 swept;
  auto vertices = [](const Geometry* g, size_t i, unsigned slot, V3* v) {
    const unsigned* idx = (const unsigned*)g->view(RTC_BUFFER_TYPE_INDEX, 0)->at(i);
    for (int k = 0; k < NV; k++) v[k] = g->vertex(idx[k], slot);
  };
  for (unsigned gid = 0; gid < s->geometries.size(); gid++) {
    Geometry* g = s->geometries[gid];
    if (!g || !g->enabled || g->type != type || g->timeSteps == 1) continue;
    for (unsigned t = 0; t < g->timeSteps; t++) {
      const BufferView* vv = g->view(RTC_BUFFER_TYPE_VERTEX, t);
      if (!vv || !vv->valid()) RT_THROW(RTC_ERROR_INVALID_OPERATION, "motion blur geometry: a time step has no vertex buffer");
    }
    const size_t n = g->numTriangles(); // index buffer records
    std::vector<char> ok(g->timeSteps);
    for (size_t i = 0; i < n; i++) {
      for (unsigned t = 0; t < g->timeSteps; t++) ok[t] = NV == 4 ? g->validQuad(i, t) : g->validTriangle(i, t);
      for (unsigned seg = 0; seg + 1 < g->timeSteps; seg++) {
        if (!ok[seg] || !ok[seg + 1]) continue; // invalid at either end of the segment: no record for it
        V3 v[2 * NV];
        vertices(g, i, seg, v);
        vertices(g, i, seg + 1, v + NV);
        BuildPrim p;
        if (linear) {
          Ends e;
          for (int k = 0; k < NV; k++) {
            e.a.extend(v[k]);
            e.b.extend(v[NV + k]);
            p.box.extend((v[k] + v[NV + k]) * 0.5f);
          }
          const double S = (double)(g->timeSteps - 1);
          e.ta = (double)seg / S;
          e.tb = (double)(seg + 1) / S;
          swept.extend(e.a);
          swept.extend(e.b);
          ends.push_back(e);
        } else
          for (int k = 0; k < 2 * NV; k++) p.box.extend(v[k]);
        p.id = (uint32_t)src.size();
        src.push_back({gid, (unsigned)i, seg});
        bp.push_back(p);
      }
    }
  }
  if (bp.empty()) return false;
  if (bp.size() >= ((size_t)1 << TRI_START_BITS)) RT_THROW(RTC_ERROR_INVALID_OPERATION, tooMany);

  recs.reserve(bp.size());
  auto makeLeaf = [&](const BuildPrim* prims, size_t begin, size_t end) -> uint32_t {
    const uint32_t first = (uint32_t)recs.size();
    for (size_t i = begin; i < end; i++) {
      const Src& sr = src[prims[i].id];
      const Geometry* g = s->geometries[sr.geomID];
      V3 v[2 * NV];
      vertices(g, sr.primID, sr.segment, v);
      vertices(g, sr.primID, sr.segment + 1, v + NV);
      Rec r;
      memset(&r, 0, sizeof(r));
      fill(r, v);
      r.geomID = sr.geomID;
      r.primID = sr.primID;
      r.segment = sr.segment;
      r.numSegments = g->timeSteps - 1;
      recs.push_back(r);
    }
    return make_tri_leaf(first, (uint32_t)(end - begin));
  };
  BuildSettings cfg;
  cfg.threads = host_threads(s->device);
  if (linear) {
    auto linear_bounds = [&](const BuildPrim* prims, size_t begin, size_t end, Box3& b0, Box3& b1) {
      const double inf = std::numeric_limits<double>::infinity();
      double lo0[3], hi0[3], lo1[3], hi1[3];
      for (int pass = 0; pass < 2; pass++) { // pass 0: the pairs of segment 0 / of the last segment; pass 1 (none there): all pairs
        for (int a = 0; a < 3; a++) { lo0[a] = lo1[a] = inf; hi0[a] = hi1[a] = -inf; }
        bool any0 = false, any1 = false;
        for (size_t i = begin; i < end; i++) {
          const Ends& e = ends[prims[i].id];
          if (pass == 1 || e.ta == 0.0) { any0 = true; for (int a = 0; a < 3; a++) { lo0[a] = std::min(lo0[a], (double)e.a.lo[a]); hi0[a] = std::max(hi0[a], (double)e.a.hi[a]); } }
          if (pass == 1 || e.tb == 1.0) { any1 = true; for (int a = 0; a < 3; a++) { lo1[a] = std::min(lo1[a], (double)e.b.lo[a]); hi1[a] = std::max(hi1[a], (double)e.b.hi[a]); } }
        }
        if (any0 && any1) break;
      }
      for (int a = 0; a < 3; a++) {
        double dlo = 0.0, dhi = 0.0; // how far any pair end sticks out of the interpolated guess
        for (size_t i = begin; i < end; i++) {
          const Ends& e = ends[prims[i].id];
          for (int k = 0; k < 2; k++) {
            const double t = k ? e.tb : e.ta;
            const Box3& b = k ? e.b : e.a;
            dlo = std::max(dlo, ((1.0 - t) * lo0[a] + t * lo1[a]) - (double)b.lo[a]);
            dhi = std::max(dhi, (double)b.hi[a] - ((1.0 - t) * hi0[a] + t * hi1[a]));
          }
        }
        auto down = [](double x) { float f = (float)x; return (double)f > x ? nextafterf(f, -std::numeric_limits<float>::infinity()) : f; };
        auto up = [](double x) { float f = (float)x; return (double)f < x ? nextafterf(f, std::numeric_limits<float>::infinity()) : f; };
        b0.lo[a] = down(lo0[a] - dlo); b1.lo[a] = down(lo1[a] - dlo);
        b0.hi[a] = up(hi0[a] + dhi); b1.hi[a] = up(hi1[a] + dhi);
      }
    };
    BuildResultMB r = build_bvh8_mb(bp, cfg, makeLeaf, linear_bounds);
    A.nodesMB = std::move(r.nodes);
    A.root = r.root;
    A.maxDepth = r.maxDepth;
    A.leafCount = r.leafCount;
    s->bounds.extend(swept);
  } else {
    BuildResult r = build_bvh8(bp, cfg, makeLeaf);
    A.nodes = std::move(r.nodes);
    A.root = r.root;
    A.maxDepth = r.maxDepth;
    A.leafCount = r.leafCount;
    for (const BuildPrim& p : bp) s->bounds.extend(p.box);
  }
  A.blobStride = sizeof(Rec);
  A.blobs.resize(recs.size() * sizeof(Rec));
  memcpy(A.blobs.data(), recs.data(), A.blobs.size());
  return true;
}

// Triangle meshes with more than one time step (scene.cpp:213-247).  Every name is served by the one TriMBRecord layout: default =
// Pluecker + robust traversal for a robust scene, Moeller + fast traversal otherwise; an explicit triangle4imb / triangle4vmb accel is
// the fast (Moeller) variant.
static void build_trimb_accel(Scene* s)
{
  Accel& A = s->triMBAccel;
  A.clear();
  const std::string& name = s->device->tri_accel_mb;
  bool pluecker;
  if (name == "default") pluecker = s->isRobust();
  else if (name == "bvh8.triangle4imb" || name == "bvh4.triangle4imb" || name == "bvh8.triangle4vmb" || name == "bvh4.triangle4vmb") pluecker = false;
  else RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown motion blur triangle acceleration structure " + name);

  std::vector<TriMBRecord> recs;
  auto fill = [](TriMBRecord& r, const V3* v) {
    r.a0x = v[0].x; r.a0y = v[0].y; r.a0z = v[0].z;
    r.b0x = v[1].x; r.b0y = v[1].y; r.b0z = v[1].z;
    r.c0x = v[2].x; r.c0y = v[2].y; r.c0z = v[2].z;
    r.a1x = v[3].x; r.a1y = v[3].y; r.a1z = v[3].z;
    r.b1x = v[4].x; r.b1y = v[4].y; r.b1z = v[4].z;
    r.c1x = v[5].x; r.c1y = v[5].y; r.c1z = v[5].z;
  };
  if (!build_mb_bvh8<3>(s, A, RTC_GEOMETRY_TYPE_TRIANGLE, "too many motion blur triangle segments for the 26-bit leaf reference", recs, fill)) return;
  A.kind = pluecker ? ACCEL_TRIMB_PLUECKER : ACCEL_TRIMB_MOELLER; // only once there are records
  if (s->device->mb_bounds == "linear") A.kind = pluecker ? ACCEL_TRIMB_LINEAR_PLUECKER : ACCEL_TRIMB_LINEAR_MOELLER;
  A.robust = pluecker ? 1 : 0;
}

// Quad meshes with more than one time step (scene.cpp:332-367): QuadMBRecords, default = Pluecker + robust traversal for a robust
// scene, Moeller + fast traversal otherwise; an explicit quad4imb accel is the fast (Moeller) variant.  A host-only device builds
// this accel only when its config names quad_accel_mb= (Device::quads_mb_enabled; build_mesh_bvh8 raises otherwise).
static void build_quadmb_accel(Scene* s)
{
  Accel& A = s->quadMBAccel;
  A.clear();
  const std::string& name = s->device->quad_accel_mb;
  bool pluecker;
  if (name == "default") pluecker = s->isRobust();
  else if (name == "bvh8.quad4imb" || name == "bvh4.quad4imb") pluecker = false;
  else RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown motion blur quad acceleration structure " + name);

  std::vector<QuadMBRecord> recs;
  auto fill = [](QuadMBRecord& q, const V3* v) {
    q.v0ax = v[0].x; q.v0ay = v[0].y; q.v0az = v[0].z;
    q.v1ax = v[1].x; q.v1ay = v[1].y; q.v1az = v[1].z;
    q.v2ax = v[2].x; q.v2ay = v[2].y; q.v2az = v[2].z;
    q.v3ax = v[3].x; q.v3ay = v[3].y; q.v3az = v[3].z;
    q.v0bx = v[4].x; q.v0by = v[4].y; q.v0bz = v[4].z;
    q.v1bx = v[5].x; q.v1by = v[5].y; q.v1bz = v[5].z;
    q.v2bx = v[6].x; q.v2by = v[6].y; q.v2bz = v[6].z;
    q.v3bx = v[7].x; q.v3by = v[7].y; q.v3bz = v[7].z;
  };
  if (!build_mb_bvh8<4>(s, A, RTC_GEOMETRY_TYPE_QUAD, "too many motion blur quad segments for the 26-bit leaf reference", recs, fill)) return;
  A.kind = pluecker ? ACCEL_QUADMB_PLUECKER : ACCEL_QUADMB_MOELLER; // only once there are records
  if (s->device->mb_bounds == "linear") A.kind = pluecker ? ACCEL_QUADMB_LINEAR_PLUECKER : ACCEL_QUADMB_LINEAR_MOELLER;
  A.robust = pluecker ? 1 : 0;
}

// world2local = inverse(local2world), both as the columns vx, vy, vz, p: inverted in double precision and rounded once to fp32
// (deviation: the reference inverts in fp32 with its rcp, affinespace.h rcp()).  false: singular (or not finite) - the caller stores
// an all-zero matrix, under which no triangle test passes (the local direction is 0: den == 0 in both tests).
static bool invert_affine(const float* m, float* out)
{
  const double a[3][3] = {{m[0], m[3], m[6]}, {m[1], m[4], m[7]}, {m[2], m[5], m[8]}}; // a[row][col], columns vx vy vz
  const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2], c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
  const double det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02;
  if (!(det != 0.0) || !std::isfinite(det)) return false;
  double inv[3][3];
  inv[0][0] = c00 / det;
  inv[1][0] = c01 / det;
  inv[2][0] = c02 / det;
  inv[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det;
  inv[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det;
  inv[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det;
  inv[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det;
  inv[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det;
  inv[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
  float r[12];
  for (int col = 0; col < 3; col++)
    for (int row = 0; row < 3; row++) r[3 * col + row] = (float)inv[row][col];
  for (int row = 0; row < 3; row++) r[9 + row] = (float)-(inv[row][0] * m[9] + inv[row][1] * m[10] + inv[row][2] * m[11]);
  for (int i = 0; i < 12; i++)
    if (!std::isfinite(r[i])) return false;
  memcpy(out, r, sizeof(r));
  return true;
}

void Geometry::local2worldAt(float time, float* out) const
{
  if (local2world.size() == 1) {
    memcpy(out, local2world[0].data(), sizeof(Xfm));
    return;
  }
  float f;
  const uint32_t itime = instance_time_segment(time, (uint32_t)local2world.size() - 1u, f);
  instance_lerp(local2world[itime].data(), local2world[itime + 1].data(), f, out);
}

bool Geometry::world2localAt(float time, float* out) const
{
  bool ok;
  if (local2world.size() == 1) ok = invert_affine(local2world[0].data(), out);
  else {
    float f;
    const uint32_t itime = instance_time_segment(time, (uint32_t)local2world.size() - 1u, f);
    ok = instance_world2local(local2world[itime].data(), local2world[itime + 1].data(), f, out);
  }
  if (!ok) memset(out, 0, sizeof(Xfm));
  return ok;
}

// xfmPoint (affinespace.h:110): madd(p.x, vx, madd(p.y, vy, madd(p.z, vz, p)))
static V3 xfm_point(const float* m, V3 q)
{
  V3 r;
  for (int k = 0; k < 3; k++) r[k] = fmaf(q.x, m[k], fmaf(q.y, m[3 + k], fmaf(q.z, m[6 + k], m[9 + k])));
  return r;
}

// Instances (RTC_GEOMETRY_TYPE_INSTANCE, one time step, one level): a top-level BVH8 over the instances' world bounds - xfmBounds of
// the instanced scene's bounds, its eight transformed corners (instance_intersector.cpp:24-39, affinespace.h:114-126) - with ONE
// instance per leaf, followed in the same arrays by the trees and records of every distinct instanced scene, rebased.  The instanced
// scenes were committed before; what this commit sees of them is their committed triangle and quad accels (their `bounds` cover both:
// build_mesh_bvh8 extends them per accel).
// As long as no instanced scene has a traceable quad accel the result is the triangle-only accel (kinds ACCEL_INST_TRI_*: triangle
// trees behind the top-level tree, TriRecords, InstanceRecords, `pad` zero); otherwise it is the layout of accel.h InstanceRecord
// (kinds ACCEL_INST_PLUECKER / ACCEL_INST_MOELLER).  A host-only device takes quads in an instanced scene only when its config names
// inst_accel= (Device::inst_quads_enabled), as it takes quad meshes at all only with quad_accel=.
// Instance motion blur: as soon as one enabled instance has more than one time step the kinds are ACCEL_INSTMB_* (chosen otherwise
// exactly as ACCEL_INST_*) and the steps' local-to-world transforms follow the quad records in `blobs` as InstanceSteps (accel.h).  The
// world box of a moving instance is the union over its steps of xfmBounds(local2world[i], scene bounds): the instanced scene is static
// and the lerp of two affine maps sends a point to the lerp of its images, so the union of the steps' boxes holds the object at every
// time - one box swept over the whole shutter, like the motion-blur mesh accels.  A host-only device takes
// such instances under the rule of quads (Device::inst_motion_enabled).
// Motion-blur meshes below an instance: as soon as one instanced scene has a traceable motion-blur accel (triangle or quad meshes with
// time steps) the kinds are ACCEL_INSTMESHMB_* and the layout is the general one of accel.h InstanceRecord: all four trees of every
// distinct scene behind the top-level tree, the roots in one InstanceSceneRecord per scene, the TriMBRecords and QuadMBRecords in
// sections of their own at the end of `blobs`.  The instanced scenes' bounds cover their moving meshes at every time (build_mb_bvh8
// extends them by the swept boxes).  A host-only device takes such scenes only when its config names inst_accel= and one of
// tri_accel_mb= / quad_accel_mb= (Device::inst_mesh_motion_enabled); a top scene without a motion-blur accel below it keeps the kinds
// 14..21 and their arrays.
// Linear node bounds below an instance (inst_mb_bounds=linear, Device::inst_mb_bounds; on a host-only device only where motion-blur
// meshes below an instance are taken at all): an instanced scene whose motion-blur accels were built under mb_bounds=linear (kinds
// 26..29) is then placed with its QNodeMB8s, and as soon as there is one the kinds are ACCEL_INSTMESHMB_LINEAR_*: `prims` and `blobs`
// as in the kinds ACCEL_INSTMESHMB_*, the node array in two sections (accel.h InstanceRecord) - `A.nodes` with the top-level tree and
// the static trees, `A.nodesMB` with the motion-blur trees, child indices counted in 144-byte units from the start of the uploaded
// buffer, and `A.nodeImage` the two with the padding between them.  One device has one mb_bounds and an instance cannot name a scene
// of another device (Geometry::setInstancedScene), so the motion-blur trees below one top scene are all of one node type.  Without
// the key such a scene is refused as before; with it and no such scene the accel is what it is without the key.
// Subdivision scenes below an instance: an instanced scene that enables a subdivision mesh is left to build_instance_subdiv_accel (a
// second accel of the top scene; this one and its kinds stay what they are) when the device takes such scenes
// (Device::inst_subdiv_enabled); otherwise it is refused here with the message of the config, as before.
// maxDepth (launch_on reserves 7 * (maxDepth + 1) + 2 stack entries) =
//     the top-level depth
//   + 1 for the exit marker
//   + the largest number of pending-tree markers any instanced scene can have stacked at once (its tree count - 1, at most 3; in the
//     kinds 14..21: 1 as soon as any scene has quads)
//   + the deepest of all instanced trees (the trees of a scene are never stacked together: a marker is popped only when the entries
//     of the tree before it are gone).
// First InstanceStep a record may name, in 64-byte units from the start of `blobs`, exclusive: 24 bits beside the segment count.
static const size_t INSTANCE_FIRST_STEP_LIMIT = (size_t)1 << 24;
// The class of an instanced scene: a subdivision scene as soon as it enables a subdivision mesh (build_instance_subdiv_accel refuses
// anything beside it), a mesh scene otherwise.
static bool is_subdivision_scene(const Scene* o)
{
  for (const Geometry* og : o->geometries)
    if (og && og->enabled && og->type == RTC_GEOMETRY_TYPE_SUBDIVISION) return true;
  return false;
}
static void build_instance_accel(Scene* s)
{
  Accel& A = s->instAccel;
  A.clear();
  if (s->device->inst_accel != "default") RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown instance acceleration structure " + s->device->inst_accel);
  const bool quadsOk = s->device->inst_quads_enabled();
  const bool subdivOk = s->device->inst_subdiv_enabled(); // implies quadsOk; scenes of subdivision meshes go to the second instance accel
  const char* const onlyTris = "an instanced scene may hold static triangle meshes only (no quads, time steps, subdivision meshes or instances)";
  const char* const onlyStatic = "an instanced scene may hold static triangle and quad meshes only (no time steps, subdivision meshes or instances)";
  const bool meshMotionOk = s->device->inst_mesh_motion_enabled(); // implies quadsOk
  const char* const onlyMeshes = "an instanced scene may hold triangle and quad meshes only (no subdivision meshes or instances)";
  // (the wording is from before subdivision scenes could be instanced and is kept: on a device that takes them, "no subdivision meshes"
  // reads "not beside meshes in one instanced scene" - a scene of subdivision meshes only never gets here)
  const char* const only = meshMotionOk ? onlyMeshes : quadsOk ? onlyStatic : onlyTris;
  struct Src { unsigned geomID; Scene* scene; };
  std::vector<Src> src;
  std::vector<BuildPrim> bp;
  bool haveKind = false, pluecker = false, anyQuads = false, anyMotion = false, anyMeshMotion = false;
  const bool linearOk = meshMotionOk && s->device->inst_mb_bounds == "linear";
  bool anyLinear = false, anySwept = false; // traceable motion-blur accels of the kinds 26..29 / 10..13 below this scene
  uint32_t pendingMax = 0; // most trees of one instanced scene, minus one
  unsigned kindGeom = 0;   // the instance whose scene fixed the arithmetic, and the accels that scene has: for the refusal below
  std::string kindNames;
  for (unsigned gid = 0; gid < s->geometries.size(); gid++) {
    Geometry* g = s->geometries[gid];
    if (!g || !g->enabled || g->type != RTC_GEOMETRY_TYPE_INSTANCE) continue;
    if (g->timeSteps != 1 && !s->device->inst_motion_enabled()) RT_THROW(RTC_ERROR_INVALID_OPERATION, "instances with more than one time step are not supported");
    Scene* o = g->instScene;
    if (!o) RT_THROW(RTC_ERROR_INVALID_OPERATION, "instance without an instanced scene");
    if (o->modified) RT_THROW(RTC_ERROR_INVALID_OPERATION, "instanced scene got not committed");
    if (subdivOk && is_subdivision_scene(o)) continue; // build_instance_subdiv_accel places it
    // without inst_mb_bounds=linear the instanced scenes' trees are copied behind the top-level tree as QNode8s: time-dependent nodes
    // have no place there
    if (!linearOk && (is_mb_linear_kind(o->triMBAccel.kind) || is_mb_linear_kind(o->quadMBAccel.kind)))
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "an instanced scene with a motion blur accel built under mb_bounds=linear is not supported (instance accels hold swept node boxes: use mb_bounds=swept)");
    for (Geometry* og : o->geometries) {
      if (!og || !og->enabled) continue;
      const bool mesh = og->type == RTC_GEOMETRY_TYPE_TRIANGLE || (quadsOk && og->type == RTC_GEOMETRY_TYPE_QUAD);
      if (!mesh || (og->timeSteps != 1 && !meshMotionOk)) RT_THROW(RTC_ERROR_INVALID_OPERATION, only);
      if (og->intersectFilter || og->occludedFilter) RT_THROW(RTC_ERROR_INVALID_OPERATION, "geometry filter functions inside an instanced scene are not supported");
    }
    for (const Accel* oa : o->accels())
      if (oa != &o->triAccel && !(quadsOk && oa == &o->quadAccel) && !(meshMotionOk && (oa == &o->triMBAccel || oa == &o->quadMBAccel)) && oa->kind != ACCEL_NONE)
        RT_THROW(RTC_ERROR_INVALID_OPERATION, only);
    if (o->triIntersectFilter || o->triOccludedFilter) RT_THROW(RTC_ERROR_INVALID_OPERATION, "geometry filter functions inside an instanced scene are not supported");
    const bool tris = o->triAccel.traceable(), quads = o->quadAccel.traceable();
    const bool trisMB = o->triMBAccel.traceable(), quadsMB = o->quadMBAccel.traceable();
    if (!tris && !quads && !trisMB && !quadsMB) continue; // empty scene: nothing to hit
    std::string names; // this scene's traceable accels
    for (const char* nm : {tris ? "triangle" : "", trisMB ? "motion blur triangle" : "", quads ? "quad" : "", quadsMB ? "motion blur quad" : ""})
      if (*nm) names += std::string(names.empty() ? "" : ", ") + nm;
    // scenes that disagree while a motion-blur accel is involved: the message names the accels on either side
    auto disagree = [&](bool thisPl) {
      const char* const ar[2] = {"Moeller / fast", "Pluecker / robust"};
      return "the instanced scenes of one scene disagree in accel kind (Pluecker / robust and Moeller / fast): the scene of instance " + std::to_string(gid) + " has " +
             ar[thisPl] + " accels (" + names + "), the scene of instance " + std::to_string(kindGeom) + " " + ar[!thisPl] + " ones (" + kindNames + "): instances need one arithmetic";
    };
    if (trisMB || quadsMB) {
      // one arithmetic per top scene, over all four trees of every instanced scene
      struct { bool have, pl; const char* name; } const t[4] = {{tris, o->triAccel.kind == ACCEL_TRI_PLUECKER, "triangle"},
                                                                {trisMB, is_mb_pluecker_kind(o->triMBAccel.kind), "motion blur triangle"},
                                                                {quads, o->quadAccel.kind == ACCEL_QUAD_PLUECKER, "quad"},
                                                                {quadsMB, is_mb_pluecker_kind(o->quadMBAccel.kind), "motion blur quad"}};
      std::string pl, mo;
      for (const auto& e : t)
        if (e.have) (e.pl ? pl : mo) += std::string((e.pl ? pl : mo).empty() ? "" : ", ") + e.name;
      if (!pl.empty() && !mo.empty())
        RT_THROW(RTC_ERROR_INVALID_OPERATION, "the accels of an instanced scene disagree in kind (Pluecker / robust: " + pl + "; Moeller / fast: " + mo + "): instances need one arithmetic");
      const bool scenePl = !pl.empty();
      if (haveKind && scenePl != pluecker) RT_THROW(RTC_ERROR_INVALID_OPERATION, disagree(scenePl));
      anyMeshMotion = true;
      for (const Accel* m : {trisMB ? &o->triMBAccel : nullptr, quadsMB ? &o->quadMBAccel : nullptr})
        if (m) (is_mb_linear_kind(m->kind) ? anyLinear : anySwept) = true;
    }
    pendingMax = std::max(pendingMax, (uint32_t)tris + (uint32_t)trisMB + (uint32_t)quads + (uint32_t)quadsMB - 1u);
    // the kernel runs ONE arithmetic on both levels and in both leaves: every accel below this scene is Pluecker / robust, or every one
    // Moeller / fast
    if (tris && quads && (o->triAccel.kind == ACCEL_TRI_PLUECKER) != (o->quadAccel.kind == ACCEL_QUAD_PLUECKER))
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "the triangle and quad accels of an instanced scene disagree in kind (Pluecker / robust triangles beside Moeller / fast quads, "
                                            "as a robust scene under quad_accel=bvh8.quad4v builds them): instances need one arithmetic");
    const bool pl = tris ? o->triAccel.kind == ACCEL_TRI_PLUECKER
                  : quads ? o->quadAccel.kind == ACCEL_QUAD_PLUECKER
                  : is_mb_pluecker_kind(trisMB ? o->triMBAccel.kind : o->quadMBAccel.kind);
    if (haveKind && pl != pluecker) {
      if (!anyQuads && !quads && !anyMeshMotion) RT_THROW(RTC_ERROR_INVALID_OPERATION, "the instanced scenes of one scene disagree in triangle accel kind (robust and not robust)");
      if (anyMeshMotion) RT_THROW(RTC_ERROR_INVALID_OPERATION, disagree(pl));
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "the instanced scenes of one scene disagree in accel kind (Pluecker / robust and Moeller / fast): instances need one arithmetic");
    }
    if (!haveKind) {
      kindGeom = gid;
      kindNames = names;
    }
    haveKind = true;
    pluecker = pl;
    anyQuads |= quads;
    anyMotion |= g->local2world.size() > 1;
    BuildPrim p;
    const V3 c[2] = {o->bounds.lo, o->bounds.hi};
    for (const Geometry::Xfm& step : g->local2world) // one step: xfmBounds; more: the union over the steps
      for (int i = 0; i < 8; i++) p.box.extend(xfm_point(step.data(), V3(c[i >> 2].x, c[(i >> 1) & 1].y, c[i & 1].z)));
    if (!(std::isfinite(p.box.lo.x) && std::isfinite(p.box.lo.y) && std::isfinite(p.box.lo.z) && std::isfinite(p.box.hi.x) && std::isfinite(p.box.hi.y) && std::isfinite(p.box.hi.z)))
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "instance transform yields bounds that are not finite");
    p.id = (uint32_t)src.size();
    src.push_back({gid, o});
    bp.push_back(p);
  }
  if (bp.empty()) return;
  if (bp.size() >= ((size_t)1 << TRI_START_BITS)) RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instances for the 26-bit leaf reference");
  if (anyLinear && anySwept) RT_THROW(RTC_ERROR_UNKNOWN, "instance builder: motion blur accels of both node types below one scene");

  // top-level tree, one instance per leaf: leaf reference = record index, count 1
  std::vector<InstanceRecord> recs(bp.size());
  std::vector<uint32_t> order; // record index -> src index, leaf order
  auto makeLeaf = [&](const BuildPrim* prims, size_t begin, size_t end) -> uint32_t {
    if (end - begin != 1) RT_THROW(RTC_ERROR_UNKNOWN, "instance builder: a leaf must hold one instance");
    order.push_back(prims[begin].id);
    return make_tri_leaf((uint32_t)order.size() - 1u, 1u);
  };
  BuildSettings cfg;
  cfg.blockSize = 1; cfg.minLeaf = 1; cfg.maxLeaf = 1;
  cfg.threads = 1; // the leaf callback appends in leaf order
  for (const BuildPrim& p : bp) s->bounds.extend(p.box);
  BuildResult r = build_bvh8(bp, cfg, makeLeaf);
  A.nodes = std::move(r.nodes);
  A.root = r.root;
  A.leafCount = r.leafCount;

  // the distinct instanced scenes' trees behind it, rebased: the triangle tree, then (anyQuads) the quad tree; with anyMeshMotion all
  // four trees in Scene::commit's order
  struct Roots { uint32_t tri, quad; };
  std::map<Scene*, Roots> rootsOf;
  std::vector<QuadRecord> quadRecs;
  uint32_t deepest = 0;
  // copies the nodes of O behind A.nodes; leaf references move by leafBase, which keeps the first record in bits 0..25 (guarded by the caller)
  auto append_tree = [&](const Accel& O, size_t leafBase) -> uint32_t {
    if (!O.traceable()) return REF_EMPTY;
    const size_t nodeBase = A.nodes.size();
    if (nodeBase + O.nodes.size() >= (size_t)REF_LEAF) RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instanced nodes for the 31-bit node reference");
    auto rebase = [&](uint32_t ref) -> uint32_t {
      if (ref == REF_EMPTY) return ref;
      if (ref & REF_LEAF) return ref + (uint32_t)leafBase;
      return ref + (uint32_t)nodeBase;
    };
    for (QNode8 n : O.nodes) {
      for (uint32_t& c : n.child) c = rebase(c);
      A.nodes.push_back(n);
    }
    deepest = std::max(deepest, O.maxDepth);
    return rebase(O.root);
  };
  // ACCEL_INSTMESHMB_LINEAR_*: the same for a tree of QNodeMB8s, into the second section of the node array, which starts mbNodeBase
  // 144-byte units into the buffer (computed below, from the number of QNode8s in front)
  size_t mbNodeBase = 0;
  auto append_tree_mb = [&](const Accel& O, size_t leafBase) -> uint32_t {
    if (!O.traceable()) return REF_EMPTY;
    const size_t nodeBase = mbNodeBase + A.nodesMB.size();
    if (nodeBase + O.nodesMB.size() >= (size_t)REF_LEAF)
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instanced motion blur nodes for the 31-bit node reference (they follow all other nodes in one buffer, counted in 144-byte units)");
    auto rebase = [&](uint32_t ref) -> uint32_t {
      if (ref == REF_EMPTY) return ref;
      if (ref & REF_LEAF) return ref + (uint32_t)leafBase;
      return ref + (uint32_t)nodeBase;
    };
    for (QNodeMB8 n : O.nodesMB) {
      for (uint32_t& c : n.child) c = rebase(c);
      A.nodesMB.push_back(n);
    }
    deepest = std::max(deepest, O.maxDepth);
    return rebase(O.root);
  };
  auto append_mb = [&](const Accel& O, size_t leafBase) -> uint32_t { return anyLinear ? append_tree_mb(O, leafBase) : append_tree(O, leafBase); };
  // ACCEL_INSTMESHMB_*: where the sections of `blobs` start follows from the counts of everything in front of them
  std::vector<InstanceSceneRecord> sceneRecs;
  std::map<Scene*, uint32_t> sceneRecOf; // -> index into sceneRecs
  std::vector<TriMBRecord> triMBRecs;
  std::vector<QuadMBRecord> quadMBRecs;
  size_t numSteps = 0, sceneRecBase = 0, triMBOffset = 0, quadMBOffset = 0; // sceneRecBase in 64-byte units, the offsets in bytes
  if (anyMeshMotion) {
    size_t nQuads = 0, nTriMB = 0, nScenes = 0, nQNodes = A.nodes.size();
    std::map<Scene*, int> seen;
    for (const Src& sr : src) {
      const size_t n = s->geometries[sr.geomID]->local2world.size();
      if (n > 1) numSteps += n;
      if (seen[sr.scene]++) continue;
      nScenes++;
      if (sr.scene->quadAccel.traceable()) nQuads += sr.scene->quadAccel.blobs.size() / sizeof(QuadRecord);
      if (sr.scene->triMBAccel.traceable()) nTriMB += sr.scene->triMBAccel.blobs.size() / sizeof(TriMBRecord);
      for (const Accel* st : {&sr.scene->triAccel, &sr.scene->quadAccel})
        if (st->traceable()) nQNodes += st->nodes.size();
    }
    mbNodeBase = (nQNodes * sizeof(QNode8) + sizeof(QNodeMB8) - 1) / sizeof(QNodeMB8);
    sceneRecBase = recs.size() + nQuads + numSteps;
    triMBOffset = ((sceneRecBase + nScenes) * sizeof(InstanceRecord) + sizeof(TriMBRecord) - 1) / sizeof(TriMBRecord) * sizeof(TriMBRecord);
    quadMBOffset = (triMBOffset + nTriMB * sizeof(TriMBRecord) + sizeof(QuadMBRecord) - 1) / sizeof(QuadMBRecord) * sizeof(QuadMBRecord);
  }
  for (const Src& sr : src) {
    if (rootsOf.count(sr.scene)) continue;
    Roots roots;
    InstanceSceneRecord sc;
    memset(&sc, 0, sizeof(sc));
    const Accel& O = sr.scene->triAccel;
    const size_t primBase = A.prims.size();
    if (primBase + O.prims.size() >= ((size_t)1 << TRI_START_BITS)) RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instanced triangles for the 26-bit leaf reference");
    roots.tri = append_tree(O, primBase);
    if (O.traceable()) A.prims.insert(A.prims.end(), O.prims.begin(), O.prims.end());
    sc.triMBRoot = REF_EMPTY;
    const Accel& TM = sr.scene->triMBAccel;
    if (anyMeshMotion && TM.traceable()) {
      // motion-blur triangle leaves index `blobs` as one array of 96-byte records
      const size_t n = TM.blobs.size() / sizeof(TriMBRecord), base = triMBOffset / sizeof(TriMBRecord) + triMBRecs.size();
      if (base + n >= ((size_t)1 << TRI_START_BITS))
        RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instanced motion blur triangle segments for the 26-bit leaf reference (their records follow the instance, quad, step and "
                                              "scene records in one array)");
      sc.triMBRoot = append_mb(TM, base);
      const TriMBRecord* t = (const TriMBRecord*)TM.blobs.data();
      triMBRecs.insert(triMBRecs.end(), t, t + n);
    }
    roots.quad = REF_EMPTY;
    const Accel& Q = sr.scene->quadAccel;
    if ((anyQuads || anyMeshMotion) && Q.traceable()) {
      // quad leaves index `blobs` as one array of 64-byte records: the instance records, then every scene's quads
      const size_t nq = Q.blobs.size() / sizeof(QuadRecord), quadBase = recs.size() + quadRecs.size();
      if (quadBase + nq >= ((size_t)1 << TRI_START_BITS))
        RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instances and instanced quads for the 26-bit leaf reference (quad records follow the instance records in one array)");
      roots.quad = append_tree(Q, quadBase);
      const QuadRecord* q = (const QuadRecord*)Q.blobs.data();
      quadRecs.insert(quadRecs.end(), q, q + nq);
    }
    sc.quadMBRoot = REF_EMPTY;
    const Accel& QM = sr.scene->quadMBAccel;
    if (anyMeshMotion && QM.traceable()) {
      // motion-blur quad leaves index `blobs` as one array of 128-byte records
      const size_t n = QM.blobs.size() / sizeof(QuadMBRecord), base = quadMBOffset / sizeof(QuadMBRecord) + quadMBRecs.size();
      if (base + n >= ((size_t)1 << TRI_START_BITS))
        RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instanced motion blur quad segments for the 26-bit leaf reference (their records follow all other records in one array)");
      sc.quadMBRoot = append_mb(QM, base);
      const QuadMBRecord* q = (const QuadMBRecord*)QM.blobs.data();
      quadMBRecs.insert(quadMBRecs.end(), q, q + n);
    }
    rootsOf[sr.scene] = roots;
    if (anyMeshMotion) {
      sc.triRoot = roots.tri;
      sc.quadRoot = roots.quad;
      sceneRecOf[sr.scene] = (uint32_t)sceneRecs.size();
      sceneRecs.push_back(sc);
    }
  }
  std::vector<InstanceStep> steps; // of the moving instances, in record order, behind the quad records
  for (size_t i = 0; i < order.size(); i++) {
    const Src& sr = src[order[i]];
    const Geometry* g = s->geometries[sr.geomID];
    InstanceRecord& rec = recs[i];
    memset(&rec, 0, sizeof(rec));
    if (!invert_affine(g->local2world[0].data(), rec.world2local)) memset(rec.world2local, 0, sizeof(rec.world2local)); // singular: never hit
    rec.geomID = sr.geomID;
    rec.root = rootsOf[sr.scene].tri;
    if (anyMeshMotion) rec.root = (uint32_t)sceneRecBase + sceneRecOf[sr.scene]; // its InstanceSceneRecord, in 64-byte units from the start of `blobs`
    else if (anyQuads) rec.pad[0] = rootsOf[sr.scene].quad;
    if (g->local2world.size() > 1) {
      const size_t firstStep = recs.size() + quadRecs.size() + steps.size();
      if (firstStep >= INSTANCE_FIRST_STEP_LIMIT)
        RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instances, instanced quads and instance time steps for the 24-bit step offset of an instance record");
      rec.pad[1] = ((uint32_t)(g->local2world.size() - 1) << 24) | (uint32_t)firstStep;
      for (const Geometry::Xfm& x : g->local2world) {
        InstanceStep st;
        memset(&st, 0, sizeof(st));
        memcpy(st.local2world, x.data(), sizeof(st.local2world));
        steps.push_back(st);
      }
    }
  }
  if (anyLinear) A.kind = pluecker ? ACCEL_INSTMESHMB_LINEAR_PLUECKER : ACCEL_INSTMESHMB_LINEAR_MOELLER;
  else if (anyMeshMotion) A.kind = pluecker ? ACCEL_INSTMESHMB_PLUECKER : ACCEL_INSTMESHMB_MOELLER;
  else if (anyMotion) A.kind = anyQuads ? (pluecker ? ACCEL_INSTMB_PLUECKER : ACCEL_INSTMB_MOELLER) : (pluecker ? ACCEL_INSTMB_TRI_PLUECKER : ACCEL_INSTMB_TRI_MOELLER);
  else if (anyQuads) A.kind = pluecker ? ACCEL_INST_PLUECKER : ACCEL_INST_MOELLER;
  else A.kind = pluecker ? ACCEL_INST_TRI_PLUECKER : ACCEL_INST_TRI_MOELLER;
  A.robust = pluecker ? 1 : 0;
  // launch_on's stack bound counts 7 entries per level.  Triangle-only: the top-level levels, the exit marker, the deepest instanced
  // tree.  With quads a ray in a triangle tree has the marker of the pending quad tree stacked as well - one more entry, counted as a
  // level - and the deepest tree is the deeper of all triangle and quad trees (the two trees of a scene are never stacked together:
  // the quad marker is popped only when the triangle tree's entries are gone).
  A.maxDepth = r.maxDepth + 1u + (anyMeshMotion ? pendingMax : anyQuads ? 1u : 0u) + deepest;
  A.blobStride = sizeof(InstanceRecord);
  A.blobs.assign(anyMeshMotion ? quadMBOffset + quadMBRecs.size() * sizeof(QuadMBRecord) : (recs.size() + quadRecs.size() + steps.size()) * sizeof(InstanceRecord), 0);
  if (anyMeshMotion) {
    if (recs.size() + quadRecs.size() + steps.size() != sceneRecBase) RT_THROW(RTC_ERROR_UNKNOWN, "instance builder: record counts");
    memcpy(A.blobs.data() + sceneRecBase * sizeof(InstanceRecord), sceneRecs.data(), sceneRecs.size() * sizeof(InstanceSceneRecord));
    if (!triMBRecs.empty()) memcpy(A.blobs.data() + triMBOffset, triMBRecs.data(), triMBRecs.size() * sizeof(TriMBRecord));
    if (!quadMBRecs.empty()) memcpy(A.blobs.data() + quadMBOffset, quadMBRecs.data(), quadMBRecs.size() * sizeof(QuadMBRecord));
  }
  memcpy(A.blobs.data(), recs.data(), recs.size() * sizeof(InstanceRecord));
  if (!quadRecs.empty()) memcpy(A.blobs.data() + recs.size() * sizeof(InstanceRecord), quadRecs.data(), quadRecs.size() * sizeof(QuadRecord));
  if (!steps.empty()) memcpy(A.blobs.data() + (recs.size() + quadRecs.size()) * sizeof(InstanceRecord), steps.data(), steps.size() * sizeof(InstanceStep));
  if (anyLinear) { // the node buffer: the QNode8s, zero padding, the QNodeMB8s from the multiple of 144 bytes their references count from
    if ((A.nodes.size() * sizeof(QNode8) + sizeof(QNodeMB8) - 1) / sizeof(QNodeMB8) != mbNodeBase) RT_THROW(RTC_ERROR_UNKNOWN, "instance builder: node counts");
    A.nodeImage.assign((mbNodeBase + A.nodesMB.size()) * sizeof(QNodeMB8), 0);
    if (!A.nodes.empty()) memcpy(A.nodeImage.data(), A.nodes.data(), A.nodes.size() * sizeof(QNode8));
    if (!A.nodesMB.empty()) memcpy(A.nodeImage.data() + mbNodeBase * sizeof(QNodeMB8), A.nodesMB.data(), A.nodesMB.size() * sizeof(QNodeMB8));
    A.blobOffsets = {(uint32_t)A.nodesMB.size(), (uint32_t)mbNodeBase};
  }
}

// Instances of subdivision scenes: the second instance accel of a scene (accel.h InstanceRecord, kinds ACCEL_INSTSUBDIV_*), laid out
// like the first.  One node array holds the top-level BVH8 over the instances' world boxes (one instance per leaf; the box is the union
// over the transform's time steps of xfmBounds(local2world, scene bounds), as above) and behind it the rebased subdivision BVH8 of every
// distinct instanced scene; `blobs` holds the InstanceRecords, the InstanceSteps of moving instances, and - from a multiple of the blob
// stride on - the leaf blobs of all instanced scenes, so that a rebased leaf reference indexes `blobs` the way the leaf functions of
// the subdivision kernels do (GridCellLeaf::intersect, CbvhLeaf::intersect).  Two subdivision accels are placed: the eager default
// (ACCEL_GRIDSOA) and bvh4.compressed.leaf at every compression level; the kernel is instantiated per leaf family and level, so all
// instanced subdivision scenes of one top scene must agree in both (their tessellation levels may differ).  A host-only device takes
// such instances only when its config names inst_accel= and subdiv_accel= (Device::inst_subdiv_enabled); otherwise
// build_instance_accel refuses them as it always did.
// maxDepth = the top-level depth + 1 for the exit marker + the deepest instanced tree.
static void build_instance_subdiv_accel(Scene* s)
{
  Accel& A = s->instSubdivAccel;
  A.clear();
  A.robust = 1; // the subdivision accels traverse robustly, on both levels here
  if (!s->device->inst_subdiv_enabled()) return;
  struct Src { unsigned geomID; Scene* scene; };
  std::vector<Src> src;
  std::vector<BuildPrim> bp;
  bool haveKind = false;
  uint32_t leafKind = ACCEL_NONE, levels = 0;
  unsigned kindGeom = 0;
  auto type_name = [](RTCGeometryType t) -> const char* {
    return t == RTC_GEOMETRY_TYPE_TRIANGLE ? "triangle mesh" : t == RTC_GEOMETRY_TYPE_QUAD ? "quad mesh" : t == RTC_GEOMETRY_TYPE_INSTANCE ? "instance" : "geometry of another type";
  };
  auto accel_name = [](uint32_t kind, uint32_t C) -> std::string {
    return kind == ACCEL_GRIDSOA ? std::string("the eager accel") : "bvh4.compressed.leaf at compression level " + std::to_string(C);
  };
  for (unsigned gid = 0; gid < s->geometries.size(); gid++) {
    Geometry* g = s->geometries[gid];
    if (!g || !g->enabled || g->type != RTC_GEOMETRY_TYPE_INSTANCE) continue;
    Scene* o = g->instScene; // present and committed: build_instance_accel has looked at every instance
    if (!o || !is_subdivision_scene(o)) continue;
    for (const Geometry* og : o->geometries) {
      if (!og || !og->enabled) continue;
      if (og->type == RTC_GEOMETRY_TYPE_INSTANCE)
        RT_THROW(RTC_ERROR_INVALID_OPERATION, "an instanced scene that enables subdivision meshes may hold nothing else: the scene of instance " + std::to_string(gid) +
                                              " also enables an instance (instances below instances are not supported)");
      if (og->type != RTC_GEOMETRY_TYPE_SUBDIVISION)
        RT_THROW(RTC_ERROR_INVALID_OPERATION, "an instanced scene that enables subdivision meshes may hold nothing else: the scene of instance " + std::to_string(gid) +
                                              " also enables a " + type_name(og->type));
      if (og->intersectFilter || og->occludedFilter)
        RT_THROW(RTC_ERROR_INVALID_OPERATION, "subdivision geometry with a filter function inside an instanced scene is not supported (instance " + std::to_string(gid) + ")");
    }
    const Accel& O = o->subdivAccel;
    if (O.kind == ACCEL_CBVH_BOX || O.kind == ACCEL_CBVH_GRID || O.kind == ACCEL_CBVH_FULL)
      RT_THROW(RTC_ERROR_INVALID_OPERATION, std::string("subdiv_accel=bvh4.compressed.") + (O.kind == ACCEL_CBVH_BOX ? "box" : O.kind == ACCEL_CBVH_GRID ? "grid" : "full") +
                                            " below an instance is not supported (the eager accel and bvh4.compressed.leaf are)");
    if (!O.traceable()) continue; // nothing to hit
    if (O.kind != ACCEL_GRIDSOA && O.kind != ACCEL_CBVH_LEAF) RT_THROW(RTC_ERROR_UNKNOWN, "instance builder: unknown subdivision accel kind");
    const uint32_t C = O.kind == ACCEL_CBVH_LEAF ? o->compressionLevel : 0u;
    if (haveKind && (O.kind != leafKind || C != levels))
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "the instanced subdivision scenes of one scene disagree in accel kind or compression level: the scene of instance " + std::to_string(gid) + " has " +
                                            accel_name(O.kind, C) + ", the scene of instance " + std::to_string(kindGeom) + " " + accel_name(leafKind, levels) +
                                            ": the instance kernel is instantiated per leaf kind and level");
    if (!haveKind) kindGeom = gid;
    haveKind = true;
    leafKind = O.kind;
    levels = C;
    BuildPrim p;
    const V3 c[2] = {o->bounds.lo, o->bounds.hi};
    for (const Geometry::Xfm& step : g->local2world) // one step: xfmBounds; more: the union over the steps
      for (int i = 0; i < 8; i++) p.box.extend(xfm_point(step.data(), V3(c[i >> 2].x, c[(i >> 1) & 1].y, c[i & 1].z)));
    if (!(std::isfinite(p.box.lo.x) && std::isfinite(p.box.lo.y) && std::isfinite(p.box.lo.z) && std::isfinite(p.box.hi.x) && std::isfinite(p.box.hi.y) && std::isfinite(p.box.hi.z)))
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "instance transform yields bounds that are not finite");
    p.id = (uint32_t)src.size();
    src.push_back({gid, o});
    bp.push_back(p);
  }
  if (bp.empty()) return;
  if (bp.size() >= ((size_t)1 << TRI_START_BITS)) RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instances for the 26-bit leaf reference");

  // top-level tree, one instance per leaf: leaf reference = record index, count 1
  std::vector<InstanceRecord> recs(bp.size());
  std::vector<uint32_t> order; // record index -> src index, leaf order
  auto makeLeaf = [&](const BuildPrim* prims, size_t begin, size_t end) -> uint32_t {
    if (end - begin != 1) RT_THROW(RTC_ERROR_UNKNOWN, "instance builder: a leaf must hold one instance");
    order.push_back(prims[begin].id);
    return make_tri_leaf((uint32_t)order.size() - 1u, 1u);
  };
  BuildSettings cfg;
  cfg.blockSize = 1; cfg.minLeaf = 1; cfg.maxLeaf = 1;
  cfg.threads = 1; // the leaf callback appends in leaf order
  for (const BuildPrim& p : bp) s->bounds.extend(p.box);
  BuildResult r = build_bvh8(bp, cfg, makeLeaf);
  A.nodes = std::move(r.nodes);
  A.root = r.root;
  A.leafCount = r.leafCount;

  // where the blob section starts follows from the counts in front of it
  const size_t stride = src[0].scene->subdivAccel.blobStride;
  size_t numSteps = 0;
  for (const Src& sr : src) {
    const size_t n = s->geometries[sr.geomID]->local2world.size();
    if (n > 1) numSteps += n;
  }
  const size_t blobBase = ((recs.size() + numSteps) * sizeof(InstanceRecord) + stride - 1) / stride; // index of the first leaf blob
  std::map<Scene*, uint32_t> rootOf;
  std::vector<const Accel*> placed; // the distinct scenes' accels, in the order of their blobs
  size_t numBlobs = 0;
  uint32_t deepest = 0;
  for (const Src& sr : src) {
    if (rootOf.count(sr.scene)) continue;
    const Accel& O = sr.scene->subdivAccel;
    if (O.blobStride != stride || O.blobs.size() % stride != 0) RT_THROW(RTC_ERROR_UNKNOWN, "instance builder: blob strides");
    const size_t n = O.blobs.size() / stride, leafBase = blobBase + numBlobs;
    if (leafBase + n >= ((size_t)1 << TRI_START_BITS))
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instanced subdivision leaf blobs for the 26-bit leaf reference (the blobs follow the instance and step records in one array)");
    const size_t nodeBase = A.nodes.size();
    if (nodeBase + O.nodes.size() >= (size_t)REF_LEAF) RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instanced nodes for the 31-bit node reference");
    auto rebase = [&](uint32_t ref) -> uint32_t {
      if (ref == REF_EMPTY) return ref;
      if (ref & REF_LEAF) return ref + (uint32_t)leafBase;
      return ref + (uint32_t)nodeBase;
    };
    for (QNode8 n8 : O.nodes) {
      for (uint32_t& c : n8.child) c = rebase(c);
      A.nodes.push_back(n8);
    }
    deepest = std::max(deepest, O.maxDepth);
    rootOf[sr.scene] = rebase(O.root);
    placed.push_back(&O);
    numBlobs += n;
  }
  std::vector<InstanceStep> steps; // of the moving instances, in record order, behind the instance records
  for (size_t i = 0; i < order.size(); i++) {
    const Src& sr = src[order[i]];
    const Geometry* g = s->geometries[sr.geomID];
    InstanceRecord& rec = recs[i];
    memset(&rec, 0, sizeof(rec));
    if (!invert_affine(g->local2world[0].data(), rec.world2local)) memset(rec.world2local, 0, sizeof(rec.world2local)); // singular: never hit
    rec.geomID = sr.geomID;
    rec.root = rootOf[sr.scene];
    if (g->local2world.size() > 1) {
      const size_t firstStep = recs.size() + steps.size();
      if (firstStep >= INSTANCE_FIRST_STEP_LIMIT)
        RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instances and instance time steps for the 24-bit step offset of an instance record");
      rec.pad[1] = ((uint32_t)(g->local2world.size() - 1) << 24) | (uint32_t)firstStep;
      for (const Geometry::Xfm& x : g->local2world) {
        InstanceStep st;
        memset(&st, 0, sizeof(st));
        memcpy(st.local2world, x.data(), sizeof(st.local2world));
        steps.push_back(st);
      }
    }
  }
  if (steps.size() != numSteps) RT_THROW(RTC_ERROR_UNKNOWN, "instance builder: record counts");
  A.kind = leafKind == ACCEL_GRIDSOA ? ACCEL_INSTSUBDIV_GRID : ACCEL_INSTSUBDIV_CBVH_LEAF;
  A.cbvhLevels = levels;
  A.maxDepth = r.maxDepth + 1u + deepest;
  A.blobStride = (uint32_t)stride;
  A.blobs.assign((blobBase + numBlobs) * stride, 0);
  memcpy(A.blobs.data(), recs.data(), recs.size() * sizeof(InstanceRecord));
  if (!steps.empty()) memcpy(A.blobs.data() + recs.size() * sizeof(InstanceRecord), steps.data(), steps.size() * sizeof(InstanceStep));
  size_t at = blobBase * stride;
  for (const Accel* O : placed) {
    memcpy(A.blobs.data() + at, O->blobs.data(), O->blobs.size());
    at += O->blobs.size();
  }
  A.blobOffsets = {(uint32_t)numBlobs, (uint32_t)blobBase};
}

void Scene::commit()
{
  std::lock_guard<std::mutex> g(buildMutex);
  service_quiesce(device); // the upload allocates device memory (see Scene::~Scene)
  for (Geometry* geo : geometries) {
    if (!geo || !geo->enabled) continue;
    switch (geo->type) {
    case RTC_GEOMETRY_TYPE_TRIANGLE:
    case RTC_GEOMETRY_TYPE_QUAD:
    case RTC_GEOMETRY_TYPE_SUBDIVISION:
    case RTC_GEOMETRY_TYPE_INSTANCE: break;
    default: // scene.cpp:25-30: geometry types compiled out raise INVALID_OPERATION
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "geometry type not supported by the MI355X traversal path");
    }
  }
  triIntersectFilter = triOccludedFilter = subdivFilter = false;
  for (Geometry* geo : geometries) {
    if (!geo || !geo->enabled) continue;
    if (geo->type == RTC_GEOMETRY_TYPE_TRIANGLE || geo->type == RTC_GEOMETRY_TYPE_QUAD) {
      triIntersectFilter |= geo->intersectFilter != nullptr;
      triOccludedFilter |= geo->occludedFilter != nullptr;
    } else if (geo->type == RTC_GEOMETRY_TYPE_SUBDIVISION)
      subdivFilter |= geo->intersectFilter != nullptr || geo->occludedFilter != nullptr;
  }
  if (progressFn && !progressFn(progressUser, 0.0)) RT_THROW(RTC_ERROR_CANCELLED, "progress monitor forced termination");
  bounds = Box3();
  build_triangle_accel(this);
  build_trimb_accel(this);
  build_quad_accel(this);
  build_quadmb_accel(this);
  build_subdiv_accel(this);
  build_instance_accel(this);
  build_instance_subdiv_accel(this);
  for (Accel* a : accels()) a->upload(device);
  if (progressFn) progressFn(progressUser, 1.0);
  if (device->verbose >= 2) {
    fprintf(stderr, "embree3-amd: tri accel kind %u: %zu nodes (%zu B), %zu tris, depth %u; subdiv accel kind %u: %zu nodes, %zu blobs (%zu B)\n",
            triAccel.kind, triAccel.nodes.size(), triAccel.nodes.size() * sizeof(QNode8), triAccel.prims.size(), triAccel.maxDepth,
            subdivAccel.kind, subdivAccel.nodes.size(), subdivAccel.blobOffsets.size(), subdivAccel.blobs.size());
    if (triMBAccel.kind != ACCEL_NONE)
      fprintf(stderr, "embree3-amd: motion blur triangle accel kind %u: %zu nodes (%zu B), %zu segment records (%zu B), depth %u\n", triMBAccel.kind, triMBAccel.nodeCount(),
              triMBAccel.nodeCount() * triMBAccel.nodeStride(), triMBAccel.blobs.size() / sizeof(TriMBRecord), triMBAccel.blobs.size(), triMBAccel.maxDepth);
    if (quadAccel.kind != ACCEL_NONE)
      fprintf(stderr, "embree3-amd: quad accel kind %u: %zu nodes (%zu B), %zu quads (%zu B), depth %u\n", quadAccel.kind, quadAccel.nodes.size(),
              quadAccel.nodes.size() * sizeof(QNode8), quadAccel.blobs.size() / sizeof(QuadRecord), quadAccel.blobs.size(), quadAccel.maxDepth);
    if (quadMBAccel.kind != ACCEL_NONE)
      fprintf(stderr, "embree3-amd: motion blur quad accel kind %u: %zu nodes (%zu B), %zu segment records (%zu B), depth %u\n", quadMBAccel.kind, quadMBAccel.nodeCount(),
              quadMBAccel.nodeCount() * quadMBAccel.nodeStride(), quadMBAccel.blobs.size() / sizeof(QuadMBRecord), quadMBAccel.blobs.size(), quadMBAccel.maxDepth);
  }
  if (instAccel.kind != ACCEL_NONE && device->verbose >= 2)
  {
    size_t nTriMB = 0, nQuadMB = 0, nQuads = instAccel.blobs.size() / sizeof(InstanceRecord) - instAccel.leafCount; // (kinds ACCEL_INSTMB_*: quads and InstanceSteps)
    // kinds ACCEL_INSTMESHMB_*: `blobs` holds more kinds of records and padding, so the records of the distinct instanced scenes are counted
    if (instAccel.kind == ACCEL_INSTMESHMB_PLUECKER || instAccel.kind == ACCEL_INSTMESHMB_MOELLER || is_inst_linear_kind(instAccel.kind)) {
      std::map<Scene*, int> seen;
      nQuads = 0;
      for (Geometry* geo : geometries)
        if (geo && geo->enabled && geo->type == RTC_GEOMETRY_TYPE_INSTANCE && geo->instScene && !seen[geo->instScene]++) {
          if (geo->instScene->quadAccel.traceable()) nQuads += geo->instScene->quadAccel.blobs.size() / sizeof(QuadRecord);
          if (geo->instScene->triMBAccel.traceable()) nTriMB += geo->instScene->triMBAccel.blobs.size() / sizeof(TriMBRecord);
          if (geo->instScene->quadMBAccel.traceable()) nQuadMB += geo->instScene->quadMBAccel.blobs.size() / sizeof(QuadMBRecord);
        }
    }
    fprintf(stderr, "embree3-amd: instance accel kind %u: %zu nodes (%zu B), %zu instances, %zu instanced triangles, %zu instanced quads, %zu instanced motion blur triangle "
                    "segment records, %zu instanced motion blur quad segment records, depth %u\n", instAccel.kind,
            instAccel.nodes.size(), instAccel.nodes.size() * sizeof(QNode8), instAccel.leafCount, instAccel.prims.size(),
            nQuads, nTriMB, nQuadMB, instAccel.maxDepth);
    if (is_inst_linear_kind(instAccel.kind))
      fprintf(stderr, "embree3-amd: instance accel kind %u: %zu time-dependent nodes (%zu B) from node index %u in 144-byte units, node buffer %zu B\n", instAccel.kind,
              instAccel.nodesMB.size(), instAccel.nodesMB.size() * sizeof(QNodeMB8), instAccel.blobOffsets[1], instAccel.nodeImage.size());
  }
  if (instSubdivAccel.kind != ACCEL_NONE && device->verbose >= 2)
    fprintf(stderr, "embree3-amd: subdivision instance accel kind %u (C %u): %zu nodes (%zu B), %zu instances, %u instanced leaf blobs of %u B from blob index %u, depth %u\n",
            instSubdivAccel.kind, instSubdivAccel.cbvhLevels, instSubdivAccel.nodes.size(), instSubdivAccel.nodes.size() * sizeof(QNode8), instSubdivAccel.leafCount,
            instSubdivAccel.blobOffsets[0], instSubdivAccel.blobStride, instSubdivAccel.blobOffsets[1], instSubdivAccel.maxDepth);
  modified = false;
}

} // namespace rtamd
