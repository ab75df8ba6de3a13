// Geometry / Scene objects, the commit sequence (the builders: rt_prim_build.cpp, subdiv_build.cpp, rt_instance_build.cpp), upload to HBM.
#include <algorithm>
#include <map>

#include "instance_xfm.h"
#include "rt_objects.h"
#include "rt_trace.h"
#include "subdiv_build.h"

namespace rtamd {

// ---- Geometry -------------------------------------------------------------------------------------------
Geometry::Geometry(Device* d, RTCGeometryType t) : device(d), type(t)
{
  if (isCubicCurve()) tessellationRate = 4.0f; // NativeCurves (scene_bezier_curves.cpp:28); kept and without effect on the round types
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
  const bool lineFlags = (type == RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE || isCubicCurve()) && t == RTC_BUFFER_TYPE_FLAGS; // bytes (scene_line_segments.cpp:63, scene_bezier_curves.cpp:63)
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
  case RTC_GEOMETRY_TYPE_ROUND_BEZIER_CURVE:
  case RTC_GEOMETRY_TYPE_ROUND_BSPLINE_CURVE: // (the reference's round types are NativeCurves too)
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

// the point test of LineSegments::valid / NativeCurves::valid: the n consecutive FLOAT4 points (x, y, z, radius) from index[i] on lie
// inside the vertex buffer of `slot`, all their floats are finite and within FLT_LARGE (the bound of valid_vertices), no radius is negative
static bool valid_points(const Geometry& g, size_t i, size_t n, unsigned slot)
{
  const BufferView* vv = g.view(RTC_BUFFER_TYPE_VERTEX, slot);
  const size_t nv = vv && vv->valid() ? vv->count : 0;
  const size_t i0 = g.segment(i);
  if (i0 + n - 1 >= nv) return false;
  for (size_t k = i0; k < i0 + n; k++) {
    const float* p = (const float*)vv->at(k);
    for (int c = 0; c < 4; c++)
      if (!std::isfinite(p[c]) || fabsf(p[c]) > 1.844e18f) return false; // isvalid: FLT_LARGE
    if (p[3] < 0.0f) return false;
  }
  return true;
}

// LineSegments::valid(i, itime) (scene_line_segments.h): both end points, against the time step's buffer
bool Geometry::validSegment(size_t i, unsigned slot) const { return valid_points(*this, i, 2, slot); }

// NativeCurves::valid (scene_bezier_curves.h:193-218) at one time step: the four control points, against the time step's buffer
bool Geometry::validCurve(size_t i, unsigned slot) const { return valid_points(*this, i, 4, slot); }

unsigned Geometry::curveRate() const
{
  const float r = tessellationRate;
  const int n = r >= 16.0f ? 16 : (r >= 1.0f ? (int)r : 1); // clamp((int)rate, 1, 16); a NaN gives 1
  return (unsigned)n;
}

// The native control points of curve i at time step `slot`: the user's four for a Bezier geometry, convert(BSplineCurveT, BezierCurveT)
// (kernels/subdiv/bspline_curve.h:180-187) of them for a B-spline geometry - the reference's madd sequence in float32 on all four
// components, the radius included (Vec3fa arithmetic works on the whole register).
void Geometry::nativeCurve(size_t i, float out[16], unsigned slot) const
{
  const BufferView* vv = view(RTC_BUFFER_TYPE_VERTEX, slot);
  const size_t i0 = segment(i);
  const float *a = (const float*)vv->at(i0), *b = (const float*)vv->at(i0 + 1), *c = (const float*)vv->at(i0 + 2), *d = (const float*)vv->at(i0 + 3);
  if (!isBSplineCurve()) {
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
  robust = 0;
  maxDepth = 0;
  blobStride = 0;
  cbvhLevels = 0;
  instHair = 0;
  roundCurves = 0;
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
    if (geo->isRoundCurve() && geo->timeSteps != 1) // (the slot of the round curves takes one time step only)
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "motion blur of round Bezier and B-spline curves is not supported");
    if (slot_of(geo) < 0) // no slot takes the type (SCENE_SLOTS).  scene.cpp:25-30: geometry types compiled out raise INVALID_OPERATION
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "geometry type not supported by the MI355X traversal path");
  }
  triIntersectFilter = triOccludedFilter = subdivFilter = false;
  lineIntersectFilter = lineOccludedFilter = false;
  for (Geometry* geo : geometries) {
    if (!geo || !geo->enabled) continue;
    if (geo->type == RTC_GEOMETRY_TYPE_TRIANGLE || geo->type == RTC_GEOMETRY_TYPE_QUAD) {
      triIntersectFilter |= geo->intersectFilter != nullptr;
      triOccludedFilter |= geo->occludedFilter != nullptr;
    } else if (geo->type == RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE || geo->isCubicCurve()) {
      lineIntersectFilter |= geo->intersectFilter != nullptr;
      lineOccludedFilter |= geo->occludedFilter != nullptr;
    } else if (geo->type == RTC_GEOMETRY_TYPE_SUBDIVISION)
      subdivFilter |= geo->intersectFilter != nullptr || geo->occludedFilter != nullptr;
  }
  if (progressFn && !progressFn(progressUser, 0.0)) RT_THROW(RTC_ERROR_CANCELLED, "progress monitor forced termination");
  bounds = Box3();
  for (const SlotRow& r : SCENE_SLOTS) r.build(this);
  for (Accel* a : accels()) a->upload(device);
  if (progressFn) progressFn(progressUser, 1.0);
  if (device->verbose >= 2) {
    fprintf(stderr, "embree3-amd: tri accel kind %u: %zu nodes (%zu B), %zu tris, depth %u; subdiv accel kind %u: %zu nodes, %zu blobs (%zu B)\n",
            triAccel.kind, triAccel.nodes.size(), triAccel.nodes.size() * sizeof(QNode8), triAccel.prims.size(), triAccel.maxDepth,
            subdivAccel.kind, subdivAccel.nodes.size(), subdivAccel.blobOffsets.size(), subdivAccel.blobs.size());
    for (const SlotRow& r : SCENE_SLOTS) { // the line of an accel that keeps fixed-size records in `blobs`; nothing for an empty accel
      const Accel& A = this->*r.accel;
      if (r.label && A.kind != ACCEL_NONE)
        fprintf(stderr, "embree3-amd: %s accel kind %u: %zu nodes (%zu B), %zu %s (%zu B), depth %u\n", r.label, A.kind, A.nodeCount(), A.nodeCount() * A.nodeStride(),
                A.blobs.size() / r.recordBytes, r.records, A.blobs.size(), A.maxDepth);
    }
  }
  if (instAccel.kind != ACCEL_NONE && device->verbose >= 2)
  {
    // the record counts of the layout (build_instance_accel).  Below the kinds ACCEL_INSTMESHMB_* "instanced quads" has always counted
    // every 64-byte record behind the instance records: quads and InstanceSteps
    const bool general = kind_row(instAccel.kind).instGeneral;
    const size_t nQuads = instCounts.quads + (general ? 0 : instCounts.steps), nTriMB = instCounts.triMB, nQuadMB = instCounts.quadMB;
    fprintf(stderr, "embree3-amd: instance accel kind %u: %zu nodes (%zu B), %zu instances, %zu instanced triangles, %zu instanced quads, %zu instanced motion blur triangle "
                    "segment records, %zu instanced motion blur quad segment records, depth %u\n", instAccel.kind,
            instAccel.nodes.size(), instAccel.nodes.size() * sizeof(QNode8), instAccel.leafCount, instAccel.prims.size(),
            nQuads, nTriMB, nQuadMB, instAccel.maxDepth);
    if (instAccel.instHair) // inst_hair=1 and a curve or line tree below an instance
      fprintf(stderr, "embree3-amd: instance accel kind %u: %zu instanced curves, %zu instanced line segments\n", instAccel.kind, instCounts.curves, instCounts.lines);
    if (instAccel.instHair == 2) // inst_hair_mb=1 and a motion-blur curve or line tree below an instance (hair level 2: the HAIRMB form of the kernel)
      fprintf(stderr, "embree3-amd: instance accel kind %u: hair level 2, %zu instanced motion blur curve segment records, %zu instanced motion blur line segment records\n", instAccel.kind,
              instCounts.curveMB, instCounts.lineMB);
    if (instAccel.twoSections())
      fprintf(stderr, "embree3-amd: instance accel kind %u: %zu time-dependent nodes (%zu B) from node index %u in 144-byte units, node buffer %zu B\n", instAccel.kind,
              instAccel.nodesMB.size(), instAccel.nodesMB.size() * sizeof(QNodeMB8), instAccel.blobOffsets[1], instAccel.nodeImage.size());
  }
  if (instSubdivAccel.kind != ACCEL_NONE && device->verbose >= 2)
    fprintf(stderr, "embree3-amd: subdivision instance accel kind %u (C %u): %zu nodes (%zu B), %zu instances, %u instanced leaf blobs of %u B from blob index %u, depth %u\n",
            instSubdivAccel.kind, instSubdivAccel.cbvhLevels, instSubdivAccel.nodes.size(), instSubdivAccel.nodes.size() * sizeof(QNode8), instSubdivAccel.leafCount,
            instSubdivAccel.blobOffsets[0], instSubdivAccel.blobStride, instSubdivAccel.blobOffsets[1], instSubdivAccel.maxDepth);
  if (instSubdivAccel.twoSections() && device->verbose >= 2)
    fprintf(stderr, "embree3-amd: subdivision instance accel kind %u: %zu time-dependent nodes (%zu B) from node index %u in 144-byte units, node buffer %zu B\n", instSubdivAccel.kind,
            instSubdivAccel.nodesMB.size(), instSubdivAccel.nodesMB.size() * sizeof(QNodeMB8), instSubdivAccel.blobOffsets[3], instSubdivAccel.nodeImage.size());
  modified = false;
}

} // namespace rtamd
