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
Geometry::Geometry(Device* d, RTCGeometryType t) : device(d), type(t)
{
  if (isFlatCubicCurve()) tessellationRate = 4.0f; // NativeCurves (scene_bezier_curves.cpp:28)
  device->retain();
}

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
  const bool lineFlags = (type == RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE || isFlatCubicCurve()) && t == RTC_BUFFER_TYPE_FLAGS; // bytes (scene_line_segments.cpp:63, scene_bezier_curves.cpp:63)
  if (!lineFlags && ((off & 3) || (stride & 3))) RT_THROW(RTC_ERROR_INVALID_OPERATION, "buffer offset and stride must be 4-byte aligned");
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
  case RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE:
  case RTC_GEOMETRY_TYPE_FLAT_BSPLINE_CURVE: // NativeCurves::setBuffer (scene_bezier_curves.cpp:60-110): the same formats and messages
  case RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE: // LineSegments::setBuffer (scene_line_segments.cpp)
    if (t == RTC_BUFFER_TYPE_VERTEX) {
      if (f != RTC_FORMAT_FLOAT4) RT_THROW(RTC_ERROR_INVALID_OPERATION, "invalid vertex buffer format");
    } else if (t == RTC_BUFFER_TYPE_INDEX) {
      if (slot != 0) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "invalid buffer slot");
      if (f != RTC_FORMAT_UINT) RT_THROW(RTC_ERROR_INVALID_OPERATION, "invalid index buffer format");
    } else if (t == RTC_BUFFER_TYPE_FLAGS) { // kept; no effect on the flat linear intersector
      if (slot != 0) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "invalid buffer slot");
      if (f != RTC_FORMAT_UCHAR) RT_THROW(RTC_ERROR_INVALID_OPERATION, "invalid flag buffer format");
    } else if (t != RTC_BUFFER_TYPE_VERTEX_ATTRIBUTE)
      RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown buffer type");
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

unsigned Geometry::segment(size_t i) const { return *(const unsigned*)view(RTC_BUFFER_TYPE_INDEX, 0)->at(i); }

// LineSegments::valid(i, itime) (scene_line_segments.h): both vertices in range of the time step's buffer, all eight floats finite and
// within FLT_LARGE (the bound of valid_vertices), both radii >= 0
bool Geometry::validSegment(size_t i, unsigned slot) const
{
  const BufferView* vv = view(RTC_BUFFER_TYPE_VERTEX, slot);
  const size_t nv = vv && vv->valid() ? vv->count : 0;
  const size_t i0 = segment(i);
  if (i0 + 1 >= nv) return false;
  for (size_t k = i0; k < i0 + 2; k++) {
    const float* p = (const float*)vv->at(k);
    for (int c = 0; c < 4; c++)
      if (!std::isfinite(p[c]) || fabsf(p[c]) > 1.844e18f) return false;
    if (p[3] < 0.0f) return false;
  }
  return true;
}

// NativeCurves::valid (scene_bezier_curves.h:193-218): index + 3 inside the vertex buffer, all sixteen floats finite, no radius negative
bool Geometry::validCurve(size_t i) const
{
  const BufferView* vv = view(RTC_BUFFER_TYPE_VERTEX, 0);
  const size_t nv = vv && vv->valid() ? vv->count : 0;
  const size_t i0 = segment(i);
  if (i0 + 3 >= nv) return false;
  for (size_t k = i0; k < i0 + 4; k++) {
    const float* p = (const float*)vv->at(k);
    for (int c = 0; c < 4; c++)
      if (!std::isfinite(p[c]) || fabsf(p[c]) > 1.844e18f) return false; // isvalid: FLT_LARGE
    if (p[3] < 0.0f) return false;
  }
  return true;
}

unsigned Geometry::curveRate() const
{
  const float r = tessellationRate;
  const int n = r >= 16.0f ? 16 : (r >= 1.0f ? (int)r : 1); // clamp((int)rate, 1, 16); a NaN gives 1
  return (unsigned)n;
}

// The native control points of curve i: the user's four for a Bezier geometry, convert(BSplineCurveT, BezierCurveT)
// (kernels/subdiv/bspline_curve.h:180-187) of them for a B-spline geometry - the reference's madd sequence in float32 on all four
// components, the radius included (Vec3fa arithmetic works on the whole register).
void Geometry::nativeCurve(size_t i, float out[16]) const
{
  const BufferView* vv = view(RTC_BUFFER_TYPE_VERTEX, 0);
  const size_t i0 = segment(i);
  const float *a = (const float*)vv->at(i0), *b = (const float*)vv->at(i0 + 1), *c = (const float*)vv->at(i0 + 2), *d = (const float*)vv->at(i0 + 3);
  if (type != RTC_GEOMETRY_TYPE_FLAT_BSPLINE_CURVE) {
    memcpy(out, a, 16); memcpy(out + 4, b, 16); memcpy(out + 8, c, 16); memcpy(out + 12, d, 16);
    return;
  }
  const float s6 = 1.0f / 6.0f, s3 = 1.0f / 3.0f, t3 = 2.0f / 3.0f;
  for (int k = 0; k < 4; k++) {
    out[k] = fmaf(s6, a[k], fmaf(t3, b[k], s6 * c[k]));
    out[4 + k] = fmaf(t3, b[k], s3 * c[k]);
    out[8 + k] = fmaf(s3, b[k], t3 * c[k]);
    out[12 + k] = fmaf(s6, b[k], fmaf(t3, c[k], s6 * d[k]));
  }
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

// Flat linear curves (Scene::createLineAccel, scene.cpp:444-468: bvh8.line4i; BVHNBuilderSAH<8,LineSegments,Line4i>(..., 4, 1.0f, 4, inf)):
// one BVH8 with the triangle settings over the valid segments of the scene's enabled line geometries, the sibling of build_mesh_bvh8 for
// a primitive that is read through one index word and whose box is not the box of its vertices: merge(p0, p1) enlarged on every side
// by max(r0, r1) (LineMi::bounds).  Every name builds the same accel; the reference has one line intersector, so the kind only tells
// the traversal: robust for a robust scene, fast otherwise.
static void build_line_accel(Scene* s)
{
  Accel& A = s->lineAccel;
  A.clear();
  const std::string& name = s->device->line_accel;
  if (name != "default" && name != "bvh8.line4i" && name != "bvh4.line4i") RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown line segment acceleration structure " + name);

  struct Src { unsigned geomID, primID; };
  std::vector<Src> src;
  std::vector<BuildPrim> bp;
  for (unsigned gid = 0; gid < s->geometries.size(); gid++) {
    Geometry* g = s->geometries[gid];
    if (!g || !g->enabled || g->type != RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE) continue;
    if (g->timeSteps != 1) {
      if (s->device->lines_mb_enabled()) continue; // build_linemb_accel
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "motion blur of line segments is not supported");
    }
    const size_t n = g->numSegments();
    for (size_t i = 0; i < n; i++) {
      if (!g->validSegment(i)) continue;
      const float* p0 = (const float*)g->view(RTC_BUFFER_TYPE_VERTEX, 0)->at(g->segment(i));
      const float* p1 = (const float*)g->view(RTC_BUFFER_TYPE_VERTEX, 0)->at(g->segment(i) + 1);
      const float r = std::max(p0[3], p1[3]);
      BuildPrim p;
      p.box.extend(V3(std::min(p0[0], p1[0]) - r, std::min(p0[1], p1[1]) - r, std::min(p0[2], p1[2]) - r));
      p.box.extend(V3(std::max(p0[0], p1[0]) + r, std::max(p0[1], p1[1]) + r, std::max(p0[2], p1[2]) + r));
      p.id = (uint32_t)src.size();
      src.push_back({gid, (unsigned)i});
      bp.push_back(p);
    }
  }
  if (bp.empty()) return;
  if (bp.size() >= ((size_t)1 << TRI_START_BITS)) RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many line segments for the 26-bit leaf reference");

  std::vector<LineRecord> recs;
  recs.reserve(bp.size());
  auto makeLeaf = [&](const BuildPrim* prims, size_t begin, size_t end) -> uint32_t {
    const uint32_t first = (uint32_t)recs.size();
    for (size_t i = begin; i < end; i++) {
      const Src& sr = src[prims[i].id];
      const Geometry* g = s->geometries[sr.geomID];
      const float* p0 = (const float*)g->view(RTC_BUFFER_TYPE_VERTEX, 0)->at(g->segment(sr.primID));
      const float* p1 = (const float*)g->view(RTC_BUFFER_TYPE_VERTEX, 0)->at(g->segment(sr.primID) + 1);
      LineRecord r;
      memset(&r, 0, sizeof(r));
      r.v0x = p0[0]; r.v0y = p0[1]; r.v0z = p0[2]; r.r0 = p0[3];
      r.v1x = p1[0]; r.v1y = p1[1]; r.v1z = p1[2]; r.r1 = p1[3];
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
  A.kind = s->isRobust() ? ACCEL_LINE_ROBUST : ACCEL_LINE_FAST; // only once there are segments
  A.robust = s->isRobust() ? 1 : 0;
  A.blobStride = sizeof(LineRecord);
  A.blobs.resize(recs.size() * sizeof(LineRecord));
  memcpy(A.blobs.data(), recs.data(), A.blobs.size());
}

// BezierBasis::eval (kernels/subdiv/bezier_curve.h:27-37) in float32, the products in the reference's order
static void bezier_basis_eval(float u, float B[4])
{
  const float t1 = u, t0 = 1.0f - t1;
  B[0] = t0 * t0 * t0;
  B[1] = 3.0f * t1 * (t0 * t0);
  B[2] = 3.0f * (t1 * t1) * t0;
  B[3] = t1 * t1 * t1;
}

// BezierCurve3fa::tessellatedBounds(N) (bezier_curve.h:298-331) in float32: the N tessellation points eval0(j, N), j = 0 .. N - 1 - the
// nested madd over the basis at float(j) / float(N) - and v3, enlarged on every side by the largest |radius| among them.
// Containment.  The leaf cuts the curve into the N quads between the points P_j = eval(float(j) / float(N)), j = 0 .. N, all four
// components with this very arithmetic (P_N: the basis at 1 is (0, 0, 0, 1), so the madd chain returns v3 itself, bit for bit).  The
// corners of quad j are P_j -+ w_j n_j and P_j+1 -+ w_j+1 n_j+1 with unit normals n (the normal is formed in ray space, which is an
// isometry of the x / y plane and keeps world distances).  So every corner lies within |w| of a point of this box's core, the box of
// P_0 .. P_N, and the enlargement by max |w_j| covers it; a quad is the convex hull of its corners and a box is convex.  In float32
// the leaf's corners carry the roundings of the ray-space transform, at most a few ulp of the coordinates: far inside the quantizer's
// one-step padding (accel.h QNode8), the argument of every other leaf.
static Box3 curve_tessellated_bounds(const float cp[16], unsigned N)
{
  Box3 b;
  float rmax = 0.0f;
  for (unsigned j = 0; j <= N; j++) {
    float p[4];
    if (j < N) {
      float B[4];
      bezier_basis_eval((float)j / (float)N, B);
      for (int c = 0; c < 4; c++) p[c] = fmaf(B[0], cp[c], fmaf(B[1], cp[4 + c], fmaf(B[2], cp[8 + c], B[3] * cp[12 + c])));
    } else
      memcpy(p, cp + 12, 16);
    b.extend(V3(p[0], p[1], p[2]));
    rmax = std::max(rmax, fabsf(p[3]));
  }
  Box3 e;
  e.extend(V3(b.lo.x - rmax, b.lo.y - rmax, b.lo.z - rmax));
  e.extend(V3(b.hi.x + rmax, b.hi.y + rmax, b.hi.z + rmax));
  return e;
}

// Flat Bezier and B-spline curves (Scene::createHairAccel, scene.cpp:370-416): one BVH8 with the line accel's builder settings over the
// valid curves of the scene's enabled flat cubic curve geometries, CurveRecords in `blobs`.  Every name the reference accepts builds
// this accel; its oriented-box nodes (bvh4obb / bvh8obb) are not built.  The reference has one ribbon intersector, so the kind only
// tells the traversal: robust for a robust scene, fast otherwise.
static void build_curve_accel(Scene* s)
{
  Accel& A = s->curveAccel;
  A.clear();
  if (!s->device->curves_enabled()) return; // (no curve geometry can exist on such a device)
  const std::string& name = s->device->hair_accel;
  if (name != "default" && name != "bvh4.bezier1v" && name != "bvh4.bezier1i" && name != "bvh4obb.bezier1v" && name != "bvh4obb.bezier1i" && name != "bvh8obb.bezier1v" &&
      name != "bvh8obb.bezier1i")
    RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown hair acceleration structure " + name);

  struct Src { unsigned geomID, primID; };
  std::vector<Src> src;
  std::vector<BuildPrim> bp;
  for (unsigned gid = 0; gid < s->geometries.size(); gid++) {
    Geometry* g = s->geometries[gid];
    if (!g || !g->enabled || !g->isFlatCubicCurve()) continue;
    if (g->timeSteps != 1) RT_THROW(RTC_ERROR_INVALID_OPERATION, "motion blur of flat Bezier and B-spline curves is not supported");
    const unsigned N = g->curveRate();
    const size_t n = g->numCurves();
    for (size_t i = 0; i < n; i++) {
      if (!g->validCurve(i)) continue;
      float cp[16];
      g->nativeCurve(i, cp);
      BuildPrim p;
      p.box = curve_tessellated_bounds(cp, N);
      p.id = (uint32_t)src.size();
      src.push_back({gid, (unsigned)i});
      bp.push_back(p);
    }
  }
  if (bp.empty()) return;
  if (bp.size() >= ((size_t)1 << TRI_START_BITS)) RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many curves for the 26-bit leaf reference");

  std::vector<CurveRecord> recs;
  recs.reserve(bp.size());
  auto makeLeaf = [&](const BuildPrim* prims, size_t begin, size_t end) -> uint32_t {
    const uint32_t first = (uint32_t)recs.size();
    for (size_t i = begin; i < end; i++) {
      const Src& sr = src[prims[i].id];
      const Geometry* g = s->geometries[sr.geomID];
      CurveRecord r;
      memset(&r, 0, sizeof(r));
      g->nativeCurve(sr.primID, &r.v0x);
      r.geomID = sr.geomID;
      r.primID = sr.primID;
      r.N = g->curveRate();
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
  A.kind = s->isRobust() ? ACCEL_CURVE_ROBUST : ACCEL_CURVE_FAST; // only once there are curves
  A.robust = s->isRobust() ? 1 : 0;
  A.blobStride = sizeof(CurveRecord);
  A.blobs.resize(recs.size() * sizeof(CurveRecord));
  memcpy(A.blobs.data(), recs.data(), A.blobs.size());
}

// The frame of the motion-blur builders, as build_mesh_bvh8 is the one of the static builders: one BVH8 with the triangle settings over
// (primitive, time segment) pairs of the scene's enabled geometries of `type` with more than one time step.  A pair's box is the union
// of the primitive's boxes at the two ends of the segment - the vertices move on straight lines in between, so the box holds the
// primitive at every time of the segment (and, by the same argument, NOT at extrapolated times: a ray with a time outside [0, 1] sees
// the first / last segment only where it still is inside its box).  A pair gets a record only when the primitive is valid at both ends.
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
// Where a primitive's end boxes and record come from is the Source's business (MeshMBSource: NV vertices through an index record;
// LineMBSource: two FLOAT4 vertices through one index word, boxes enlarged by the radius):
//   valid(g, i, step)              the primitive at a time step (TriangleMesh / QuadMesh / LineSegments::valid(i, itime))
//   boxes(g, i, seg, a, b, mid)    its boxes at steps seg and seg + 1 and at mid-segment
//   fill(rec, g, i, seg)           the geometry of the record; the four id words are set here
template <class Rec, class Source>
static bool build_mb_bvh8(Scene* s, Accel& A, RTCGeometryType type, const char* tooMany, std::vector<Rec>& recs, const Source& source)
{
  const bool linear = s->device->mb_bounds == "linear";
  struct Src { unsigned geomID, primID, segment; };
  struct Ends { Box3 a, b; double ta, tb; }; // linear: a pair's boxes at the start / end of its segment and their global times
  std::vector<Src> src;
  std::vector<Ends> ends;
  std::vector<BuildPrim> bp;
  Box3 swept;
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
      for (unsigned t = 0; t < g->timeSteps; t++) ok[t] = source.valid(g, i, t);
      for (unsigned seg = 0; seg + 1 < g->timeSteps; seg++) {
        if (!ok[seg] || !ok[seg + 1]) continue; // invalid at either end of the segment: no record for it
        Ends e;
        Box3 mid;
        source.boxes(g, i, seg, e.a, e.b, mid);
        BuildPrim p;
        if (linear) {
          p.box = mid;
          const double S = (double)(g->timeSteps - 1);
          e.ta = (double)seg / S;
          e.tb = (double)(seg + 1) / S;
          swept.extend(e.a);
          swept.extend(e.b);
          ends.push_back(e);
        } else {
          p.box.extend(e.a);
          p.box.extend(e.b);
        }
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
      Rec r;
      memset(&r, 0, sizeof(r));
      source.fill(r, g, sr.primID, sr.segment);
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

// The Source of the triangle and quad meshes: NV vertices through the index record (UINT3 / UINT4), a box is the box of the vertices, the
// mid-segment box the box of the vertices' midpoints; fill(rec, v) writes the 2 * NV vertices (segment start, then segment end) into the
// zeroed record.
template <int NV, class Rec, class Fill> struct MeshMBSource
{
  const Fill& fillVertices;
  static void vertices(const Geometry* g, size_t i, unsigned slot, V3* v)
  {
    const unsigned* idx = (const unsigned*)g->view(RTC_BUFFER_TYPE_INDEX, 0)->at(i);
    for (int k = 0; k < NV; k++) v[k] = g->vertex(idx[k], slot);
  }
  bool valid(const Geometry* g, size_t i, unsigned step) const { return NV == 4 ? g->validQuad(i, step) : g->validTriangle(i, step); }
  void boxes(const Geometry* g, size_t i, unsigned seg, Box3& a, Box3& b, Box3& mid) const
  {
    V3 v[2 * NV];
    vertices(g, i, seg, v);
    vertices(g, i, seg + 1, v + NV);
    for (int k = 0; k < NV; k++) {
      a.extend(v[k]);
      b.extend(v[NV + k]);
      mid.extend((v[k] + v[NV + k]) * 0.5f);
    }
  }
  void fill(Rec& r, const Geometry* g, size_t i, unsigned seg) const
  {
    V3 v[2 * NV];
    vertices(g, i, seg, v);
    vertices(g, i, seg + 1, v + NV);
    fillVertices(r, v);
  }
};

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
  if (!build_mb_bvh8(s, A, RTC_GEOMETRY_TYPE_TRIANGLE, "too many motion blur triangle segments for the 26-bit leaf reference", recs, MeshMBSource<3, TriMBRecord, decltype(fill)>{fill})) return;
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
  if (!build_mb_bvh8(s, A, RTC_GEOMETRY_TYPE_QUAD, "too many motion blur quad segments for the 26-bit leaf reference", recs, MeshMBSource<4, QuadMBRecord, decltype(fill)>{fill})) return;
  A.kind = pluecker ? ACCEL_QUADMB_PLUECKER : ACCEL_QUADMB_MOELLER; // only once there are records
  if (s->device->mb_bounds == "linear") A.kind = pluecker ? ACCEL_QUADMB_LINEAR_PLUECKER : ACCEL_QUADMB_LINEAR_MOELLER;
  A.robust = pluecker ? 1 : 0;
}

// The Source of the line segments: two FLOAT4 vertices (x, y, z, radius) through one index word.  A segment's box at a step is
// LineMi::bounds(i, itime): merge(p0, p1) enlarged on every side by max(r0, r1) of that step; the mid-segment box is that of the
// midpoint vertices with the midpoint radii.
// Containment (swept and linear): at ftime f the leaf tests the segment lerp(p0a, p0b, f) - lerp(p1a, p1b, f) with the radii
// lerp(r0a, r0b, f), lerp(r1a, r1b, f).  Per axis its box is min(x0(f), x1(f)) - max(r0(f), r1(f)) below and max(x0(f), x1(f)) +
// max(r0(f), r1(f)) above, with all four functions linear in f.  min is concave and max is convex, so the lower plane is a concave
// function of f and lies ON OR ABOVE the chord of its end values, the upper plane a convex one ON OR BELOW its chord: the box of the
// interpolated segment with interpolated radii lies inside the interpolation of the two end boxes, which is what linear_bounds needs
// of a pair's ends (and the interpolation lies inside their union, the swept box).  In fp32 (the budget of accel.h QNodeMB8, one grid
// step s >= 2^-21 R): the radius is at most half a box's extent, so |r| <= R, and its lerp adds three roundings of at most 2^-24 R to
// the three of the coordinate; with the plane's own two (2^-17 s + 2^-24 R) and time_segment's 2^-9 s on coordinate and radius that is
// 7 * 2^-24 R + 2^-8 s + 2^-17 s <= 7 s / 8 + s / 256 + 2^-17 s < s: still inside the quantizer's one-step padding.
struct LineMBSource
{
  static const float* vertex(const Geometry* g, size_t i, unsigned slot, int end) { return (const float*)g->view(RTC_BUFFER_TYPE_VERTEX, slot)->at((size_t)g->segment(i) + end); }
  static void box_of(const float* p0, const float* p1, Box3& b)
  {
    const float r = std::max(p0[3], p1[3]);
    b.extend(V3(std::min(p0[0], p1[0]) - r, std::min(p0[1], p1[1]) - r, std::min(p0[2], p1[2]) - r));
    b.extend(V3(std::max(p0[0], p1[0]) + r, std::max(p0[1], p1[1]) + r, std::max(p0[2], p1[2]) + r));
  }
  bool valid(const Geometry* g, size_t i, unsigned step) const { return g->validSegment(i, step); }
  void boxes(const Geometry* g, size_t i, unsigned seg, Box3& a, Box3& b, Box3& mid) const
  {
    const float *p0a = vertex(g, i, seg, 0), *p1a = vertex(g, i, seg, 1), *p0b = vertex(g, i, seg + 1, 0), *p1b = vertex(g, i, seg + 1, 1);
    box_of(p0a, p1a, a);
    box_of(p0b, p1b, b);
    float m0[4], m1[4];
    for (int c = 0; c < 4; c++) {
      m0[c] = (p0a[c] + p0b[c]) * 0.5f;
      m1[c] = (p1a[c] + p1b[c]) * 0.5f;
    }
    box_of(m0, m1, mid);
  }
  void fill(LineMBRecord& r, const Geometry* g, size_t i, unsigned seg) const
  {
    memcpy(&r.v0ax, vertex(g, i, seg, 0), 16);
    memcpy(&r.v1ax, vertex(g, i, seg, 1), 16);
    memcpy(&r.v0bx, vertex(g, i, seg + 1, 0), 16);
    memcpy(&r.v1bx, vertex(g, i, seg + 1, 1), 16);
  }
};

// Flat linear curves with more than one time step (Scene::createLineMBAccel, scene.cpp:470-494: bvh8.line4imb): LineMBRecords under the
// frame of the motion-blur meshes.  Every name builds the same accel; the kind tells the traversal (robust for a robust scene) and the
// node type (mb_bounds).  A host-only device builds this accel only when its config names line_accel_mb= (Device::lines_mb_enabled;
// build_line_accel raises otherwise).
static void build_linemb_accel(Scene* s)
{
  Accel& A = s->lineMBAccel;
  A.clear();
  if (!s->device->lines_mb_enabled()) return;
  const std::string& name = s->device->line_accel_mb;
  if (name != "default" && name != "bvh8.line4imb" && name != "bvh4.line4imb")
    RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown motion blur line segment acceleration structure " + name);

  std::vector<LineMBRecord> recs;
  if (!build_mb_bvh8(s, A, RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE, "too many motion blur line segments for the 26-bit leaf reference", recs, LineMBSource())) return;
  const bool robust = s->isRobust();
  A.kind = robust ? ACCEL_LINEMB_ROBUST : ACCEL_LINEMB_FAST; // only once there are records
  if (s->device->mb_bounds == "linear") A.kind = robust ? ACCEL_LINEMB_LINEAR_ROBUST : ACCEL_LINEMB_LINEAR_FAST;
  A.robust = robust ? 1 : 0;
}

// world2local = inverse(local2world), both as the columns vx, vy, vz, p: inverted in double precision and rounded once to fp32
// (deviation: the reference inverts in fp32 with its rcp, affinespace.h rcp()).  false: singular (or not finite) - the caller stores
// an all-zero matrix, under which no triangle test passes (the local direction is 0: den == 0 in both tests).
bool invert_affine(const float* m, float* out)
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
V3 xfm_point(const float* m, V3 q)
{
  V3 r;
  for (int k = 0; k < 3; k++) r[k] = fmaf(q.x, m[k], fmaf(q.y, m[3 + k], fmaf(q.z, m[6 + k], m[9 + k])));
  return r;
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
    case RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE:
    case RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE:
    case RTC_GEOMETRY_TYPE_FLAT_BSPLINE_CURVE:
    case RTC_GEOMETRY_TYPE_INSTANCE: break;
    default: // scene.cpp:25-30: geometry types compiled out raise INVALID_OPERATION
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "geometry type not supported by the MI355X traversal path");
    }
  }
  triIntersectFilter = triOccludedFilter = subdivFilter = false;
  lineIntersectFilter = lineOccludedFilter = false;
  for (Geometry* geo : geometries) {
    if (!geo || !geo->enabled) continue;
    if (geo->type == RTC_GEOMETRY_TYPE_TRIANGLE || geo->type == RTC_GEOMETRY_TYPE_QUAD) {
      triIntersectFilter |= geo->intersectFilter != nullptr;
      triOccludedFilter |= geo->occludedFilter != nullptr;
    } else if (geo->type == RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE || geo->isFlatCubicCurve()) {
      lineIntersectFilter |= geo->intersectFilter != nullptr;
      lineOccludedFilter |= geo->occludedFilter != nullptr;
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
  build_curve_accel(this);
  build_line_accel(this);
  build_linemb_accel(this);
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
  if (curveAccel.kind != ACCEL_NONE && device->verbose >= 2)
    fprintf(stderr, "embree3-amd: curve accel kind %u: %zu nodes (%zu B), %zu curves (%zu B), depth %u\n", curveAccel.kind, curveAccel.nodes.size(),
            curveAccel.nodes.size() * sizeof(QNode8), curveAccel.blobs.size() / sizeof(CurveRecord), curveAccel.blobs.size(), curveAccel.maxDepth);
  if (lineAccel.kind != ACCEL_NONE && device->verbose >= 2)
    fprintf(stderr, "embree3-amd: line accel kind %u: %zu nodes (%zu B), %zu segments (%zu B), depth %u\n", lineAccel.kind, lineAccel.nodes.size(),
            lineAccel.nodes.size() * sizeof(QNode8), lineAccel.blobs.size() / sizeof(LineRecord), lineAccel.blobs.size(), lineAccel.maxDepth);
  if (lineMBAccel.kind != ACCEL_NONE && device->verbose >= 2)
    fprintf(stderr, "embree3-amd: motion blur line accel kind %u: %zu nodes (%zu B), %zu segment records (%zu B), depth %u\n", lineMBAccel.kind, lineMBAccel.nodeCount(),
            lineMBAccel.nodeCount() * lineMBAccel.nodeStride(), lineMBAccel.blobs.size() / sizeof(LineMBRecord), lineMBAccel.blobs.size(), lineMBAccel.maxDepth);
  if (instAccel.kind != ACCEL_NONE && device->verbose >= 2)
  {
    // the record counts of the layout (build_instance_accel).  Below the kinds ACCEL_INSTMESHMB_* "instanced quads" has always counted
    // every 64-byte record behind the instance records: quads and InstanceSteps
    const bool general = is_inst_general_kind(instAccel.kind);
    const size_t nQuads = instCounts.quads + (general ? 0 : instCounts.steps), nTriMB = instCounts.triMB, nQuadMB = instCounts.quadMB;
    fprintf(stderr, "embree3-amd: instance accel kind %u: %zu nodes (%zu B), %zu instances, %zu instanced triangles, %zu instanced quads, %zu instanced motion blur triangle "
                    "segment records, %zu instanced motion blur quad segment records, depth %u\n", instAccel.kind,
            instAccel.nodes.size(), instAccel.nodes.size() * sizeof(QNode8), instAccel.leafCount, instAccel.prims.size(),
            nQuads, nTriMB, nQuadMB, instAccel.maxDepth);
    if (is_inst_two_section_kind(instAccel.kind))
      fprintf(stderr, "embree3-amd: instance accel kind %u: %zu time-dependent nodes (%zu B) from node index %u in 144-byte units, node buffer %zu B\n", instAccel.kind,
              instAccel.nodesMB.size(), instAccel.nodesMB.size() * sizeof(QNodeMB8), instAccel.blobOffsets[1], instAccel.nodeImage.size());
  }
  if (instSubdivAccel.kind != ACCEL_NONE && device->verbose >= 2)
    fprintf(stderr, "embree3-amd: subdivision instance accel kind %u (C %u): %zu nodes (%zu B), %zu instances, %u instanced leaf blobs of %u B from blob index %u, depth %u\n",
            instSubdivAccel.kind, instSubdivAccel.cbvhLevels, instSubdivAccel.nodes.size(), instSubdivAccel.nodes.size() * sizeof(QNode8), instSubdivAccel.leafCount,
            instSubdivAccel.blobOffsets[0], instSubdivAccel.blobStride, instSubdivAccel.blobOffsets[1], instSubdivAccel.maxDepth);
  if (is_inst_subdiv_top_linear_kind(instSubdivAccel.kind) && device->verbose >= 2)
    fprintf(stderr, "embree3-amd: subdivision instance accel kind %u: %zu time-dependent nodes (%zu B) from node index %u in 144-byte units, node buffer %zu B\n", instSubdivAccel.kind,
            instSubdivAccel.nodesMB.size(), instSubdivAccel.nodesMB.size() * sizeof(QNodeMB8), instSubdivAccel.blobOffsets[3], instSubdivAccel.nodeImage.size());
  modified = false;
}

} // namespace rtamd
