// The nine primitive accels of a scene - triangles, quads, flat cubic curves and line segments, static and with time steps, and the static round cubic curves - built at
// commit from two frames: build_static_bvh8 and build_mb_bvh8.  A frame gathers the valid primitives of the scene's enabled geometries
// of one type, builds one BVH8 (block 4, min leaf 4, max leaf 28: bvh_builder_sah.cpp:651-658) over them and stores the leaves' records;
// where a primitive's box and record come from is the business of a Source.  What a builder keeps is the accel-name check and the kind.
#include <algorithm>
#include <initializer_list>

#include "bvh8_builder.h"
#include "rt_objects.h"
#include "subdiv_build.h"

namespace rtamd {

// ---- the steps both frames share --------------------------------------------------------------------------------------------------------
struct Src { unsigned geomID, primID, segment; }; // what a BuildPrim's id stands for (segment: 0 in the static frame)

static void check_leaf_limit(size_t n, const char* tooMany)
{
  if (n >= ((size_t)1 << TRI_START_BITS)) RT_THROW(RTC_ERROR_INVALID_OPERATION, tooMany);
}

// The leaf callback of the builder: a leaf's records are appended to `recs` in leaf order.  fill(rec, g, src) writes the geometry (and
// whatever else the type keeps) into a zeroed record; geomID / primID are set here.
template <class Rec, class Fill> static MakeLeafFn leaf_maker(const Scene* s, const std::vector<Src>& src, std::vector<Rec>& recs, const Fill& fill)
{
  recs.reserve(src.size());
  return [s, &src, &recs, fill](const BuildPrim* prims, size_t begin, size_t end) -> uint32_t {
    const uint32_t first = (uint32_t)recs.size();
    for (size_t i = begin; i < end; i++) {
      const Src& sr = src[prims[i].id];
      Rec r;
      memset(&r, 0, sizeof(r));
      fill(r, s->geometries[sr.geomID], sr);
      r.geomID = sr.geomID;
      r.primID = sr.primID;
      recs.push_back(r);
    }
    return make_tri_leaf(first, (uint32_t)(end - begin));
  };
}

static BuildSettings build_settings(const Scene* s)
{
  BuildSettings cfg;
  cfg.threads = host_threads(s->device);
  return cfg;
}

// the builder's result into the accel: `nodes` is A.nodes, or A.nodesMB for time-dependent nodes
template <class Result, class Node> static void store_tree(Accel& A, std::vector<Node>& nodes, Result&& r)
{
  nodes = std::move(r.nodes);
  A.root = r.root;
  A.maxDepth = r.maxDepth;
  A.leafCount = r.leafCount;
}

// The records and what describes them, set only once there are records (an empty accel stays as Accel::clear() left it): triangle
// records go to `prims`, all others as bytes to `blobs`.
static void store_records(Accel& A, std::vector<TriRecord>& recs) { A.prims = std::move(recs); }
template <class Rec> static void store_records(Accel& A, std::vector<Rec>& recs)
{
  A.blobStride = sizeof(Rec);
  A.blobs.resize(recs.size() * sizeof(Rec));
  memcpy(A.blobs.data(), recs.data(), A.blobs.size());
}
template <class Rec> static void finish_accel(Accel& A, std::vector<Rec>& recs, uint32_t kind, bool robust)
{
  store_records(A, recs);
  A.kind = kind;
  A.robust = robust ? 1 : 0;
}

// ---- accel names ------------------------------------------------------------------------------------------------------------------------
static bool one_of(const std::string& name, std::initializer_list<const char*> names)
{
  return std::any_of(names.begin(), names.end(), [&](const char* n) { return name == n; });
}

// The leaf arithmetic a mesh accel name asks for: "default" is Pluecker (with the robust traversal) for a robust scene and Moeller (fast
// traversal) otherwise, every other name is explicit.  `unknown` + name is the message for a name of neither list.
static bool wants_pluecker(const Scene* s, const std::string& name, std::initializer_list<const char*> pluecker, std::initializer_list<const char*> moeller, const char* unknown)
{
  if (name == "default") return s->isRobust();
  if (one_of(name, pluecker)) return true;
  if (!one_of(name, moeller)) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, unknown + name);
  return false;
}

// ---- primitives as the Sources read them ----------------------------------------------------------------------------------------------
// the NV vertices of a mesh primitive at a time step, through its index record (UINT3 / UINT4)
template <int NV> static void mesh_vertices(const Geometry* g, size_t i, unsigned slot, V3* v)
{
  const unsigned* idx = (const unsigned*)g->view(RTC_BUFFER_TYPE_INDEX, 0)->at(i);
  for (int k = 0; k < NV; k++) v[k] = g->vertex(idx[k], slot);
}

// an end point (x, y, z, radius) of a line segment at a time step, through the segment's one index word
static const float* line_vertex(const Geometry* g, size_t i, unsigned slot, int end) { return (const float*)g->view(RTC_BUFFER_TYPE_VERTEX, slot)->at((size_t)g->segment(i) + end); }

// LineMi::bounds: merge(p0, p1) enlarged on every side by max(r0, r1)
static void line_box_of(const float* p0, const float* p1, Box3& b)
{
  const float r = std::max(p0[3], p1[3]);
  b.extend(V3(std::min(p0[0], p1[0]) - r, std::min(p0[1], p1[1]) - r, std::min(p0[2], p1[2]) - r));
  b.extend(V3(std::max(p0[0], p1[0]) + r, std::max(p0[1], p1[1]) + r, std::max(p0[2], p1[2]) + r));
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

// BezierBasis::derivative (bezier_curve.h:39-49) in float32, the products in the reference's order
static void bezier_basis_derivative(float u, float D[4])
{
  const float t1 = u, t0 = 1.0f - t1;
  D[0] = 3.0f * -(t0 * t0);
  D[1] = 3.0f * fmaf(-2.0f, t0 * t1, t0 * t0);
  D[2] = 3.0f * fmaf(2.0f, t0 * t1, -(t1 * t1));
  D[3] = 3.0f * (t1 * t1);
}

// BezierCurve3fa::accurateBounds() (bezier_curve.h:273-295) in float32, the box of a round curve: at the parameters float(j) / 7.0f,
// j = 0 .. 7, the point p = eval0(j, 7) and the derivative dp = derivative0(j, 7) - the nested madd over the basis values - and the two
// neighbours p - dp / 18 (not at j = 0) and p + dp / 18 (not at j = 7): a product and a difference, not fused, with scale = 1 / (3 * 6).
// Minimum and maximum over all of them in x, y, z and w, the box enlarged on every side by max(|w_min|, |w_max|).
// Containment.  Between two parameters the curve is a Bezier segment whose inner control points are p_j + dp_j / 21 and p_j+1 - dp_j+1 / 21;
// they lie on the segments from p to p +- dp / 18, so the core box holds the control polygon of every seventh and with it the axis and -
// in w - the radius, which the enlargement covers: a surface point lies within r(u) <= max |w| of the axis.  The tube leaf's own float32
// roundings are a few ulp of the coordinates, inside the quantizer's one-step padding like those of every other leaf.
static Box3 curve_accurate_bounds(const float cp[16])
{
  const int N = 7;
  const float scale = 1.0f / (3.0f * (float)(N - 1));
  float lo[4], hi[4];
  for (int c = 0; c < 4; c++) { lo[c] = INFINITY; hi[c] = -INFINITY; }
  for (int j = 0; j <= N; j++) {
    float B[4], D[4];
    bezier_basis_eval((float)j / (float)N, B);
    bezier_basis_derivative((float)j / (float)N, D);
    for (int c = 0; c < 4; c++) {
      const float p = fmaf(B[0], cp[c], fmaf(B[1], cp[4 + c], fmaf(B[2], cp[8 + c], B[3] * cp[12 + c])));
      const float dp = fmaf(D[0], cp[c], fmaf(D[1], cp[4 + c], fmaf(D[2], cp[8 + c], D[3] * cp[12 + c])));
      const float pm = p - scale * (j != 0 ? dp : 0.0f), pp = p + scale * (j != N ? dp : 0.0f);
      lo[c] = std::min(lo[c], std::min(p, std::min(pm, pp)));
      hi[c] = std::max(hi[c], std::max(p, std::max(pm, pp)));
    }
  }
  const float r = std::max(fabsf(lo[3]), fabsf(hi[3]));
  Box3 e;
  e.extend(V3(lo[0] - r, lo[1] - r, lo[2] - r));
  e.extend(V3(hi[0] + r, hi[1] + r, hi[2] + r));
  return e;
}

// ---- the static frame -------------------------------------------------------------------------------------------------------------------
// The frame of the static builders (build_mesh_bvh8 of the triangle and quad builders once, now of the lines and curves too): one BVH8
// over the valid primitives of the scene's enabled geometries the Source takes; a primitive's record is filled from the Source and gets
// its geomID / primID here.  `A` is untouched when there is no primitive; kind, robust and the records are stored once there are some.
// A Source says (MeshSource: NV vertices through an index record; LineSource: two FLOAT4 vertices through one index word; CurveSource:
// four control points through one index word):
//   takes(s, g)        the geometry is of the Source's type and static; what a geometry of the type with time steps means - left to the
//                      motion-blur builder, or refused with the type's own message - is decided here
//   count(g)           its primitives
//   valid(g, i)        TriangleMesh / QuadMesh / LineSegments / NativeCurves::valid
//   box(g, i)          the box the tree is built over
//   fill(rec, g, i)    the geometry of the zeroed record
template <class Rec, class Source> static void build_static_bvh8(Scene* s, Accel& A, const Source& source, const char* tooMany, uint32_t kind, bool robust)
{
  std::vector<Src> src;
  std::vector<BuildPrim> bp;
  for (unsigned gid = 0; gid < s->geometries.size(); gid++) {
    const Geometry* g = s->geometries[gid];
    if (!g || !g->enabled || !source.takes(s, g)) continue;
    const size_t n = source.count(g);
    for (size_t i = 0; i < n; i++) {
      if (!source.valid(g, i)) continue;
      BuildPrim p;
      p.box = source.box(g, i);
      p.id = (uint32_t)src.size();
      src.push_back({gid, (unsigned)i, 0});
      bp.push_back(p);
    }
  }
  if (bp.empty()) return;
  check_leaf_limit(bp.size(), tooMany);

  std::vector<Rec> recs;
  const MakeLeafFn makeLeaf = leaf_maker(s, src, recs, [&source](Rec& r, const Geometry* g, const Src& sr) { source.fill(r, g, sr.primID); });
  store_tree(A, A.nodes, build_bvh8(bp, build_settings(s), makeLeaf));
  for (const BuildPrim& p : bp) s->bounds.extend(p.box);
  finish_accel(A, recs, kind, robust);
}

// The static Source of the triangle and quad meshes: the box of a primitive is the box of its NV vertices; fillVertices(rec, v) writes
// them into the zeroed record.  A mesh with time steps belongs to build_trimb_accel / build_quadmb_accel; quads with time steps are
// refused on a host-only device that does not build the motion-blur quad accel (Device::quads_mb_enabled).
template <int NV, class Rec, class Fill> struct MeshSource
{
  const Fill& fillVertices;
  bool takes(const Scene* s, const Geometry* g) const
  {
    if (g->type != (NV == 4 ? RTC_GEOMETRY_TYPE_QUAD : RTC_GEOMETRY_TYPE_TRIANGLE)) return false;
    if (g->timeSteps == 1) return true;
    if (NV == 4 && !s->device->quads_mb_enabled()) RT_THROW(RTC_ERROR_INVALID_OPERATION, "motion blur geometry is not supported by the device path");
    return false;
  }
  size_t count(const Geometry* g) const { return g->numTriangles(); } // index buffer records
  bool valid(const Geometry* g, size_t i) const { return NV == 4 ? g->validQuad(i) : g->validTriangle(i); }
  Box3 box(const Geometry* g, size_t i) const
  {
    V3 v[NV];
    mesh_vertices<NV>(g, i, 0, v);
    Box3 b;
    for (int k = 0; k < NV; k++) b.extend(v[k]);
    return b;
  }
  void fill(Rec& r, const Geometry* g, size_t i) const
  {
    V3 v[NV];
    mesh_vertices<NV>(g, i, 0, v);
    fillVertices(r, v);
  }
};

// The static Source of the line segments: a primitive that is read through one index word and whose box is not the box of its vertices
// but LineMi::bounds (line_box_of).  Segments with time steps belong to build_linemb_accel, and are refused on a host-only device that
// does not build it (Device::lines_mb_enabled).
struct LineSource
{
  bool takes(const Scene* s, const Geometry* g) const
  {
    if (g->type != RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE) return false;
    if (g->timeSteps == 1) return true;
    if (!s->device->lines_mb_enabled()) RT_THROW(RTC_ERROR_INVALID_OPERATION, "motion blur of line segments is not supported");
    return false;
  }
  size_t count(const Geometry* g) const { return g->numSegments(); }
  bool valid(const Geometry* g, size_t i) const { return g->validSegment(i); }
  Box3 box(const Geometry* g, size_t i) const
  {
    Box3 b;
    line_box_of(line_vertex(g, i, 0, 0), line_vertex(g, i, 0, 1), b);
    return b;
  }
  void fill(LineRecord& r, const Geometry* g, size_t i) const
  {
    memcpy(&r.v0x, line_vertex(g, i, 0, 0), 16);
    memcpy(&r.v1x, line_vertex(g, i, 0, 1), 16);
  }
};

// The Source of the flat Bezier and B-spline curves: the record keeps the native (Bezier) control points and the geometry's tessellation
// rate N, the box is that of the N ribbon quads the leaf tests (curve_tessellated_bounds).  Curves with time steps belong to
// build_curvemb_accel, and are refused on a host-only device that does not build it (Device::curves_mb_enabled).
struct CurveSource
{
  bool takes(const Scene* s, const Geometry* g) const
  {
    if (!g->isFlatCubicCurve()) return false;
    if (g->timeSteps == 1) return true;
    if (!s->device->curves_mb_enabled()) RT_THROW(RTC_ERROR_INVALID_OPERATION, "motion blur of flat Bezier and B-spline curves is not supported");
    return false;
  }
  size_t count(const Geometry* g) const { return g->numCurves(); }
  bool valid(const Geometry* g, size_t i) const { return g->validCurve(i); }
  Box3 box(const Geometry* g, size_t i) const
  {
    float cp[16];
    g->nativeCurve(i, cp);
    return curve_tessellated_bounds(cp, g->curveRate());
  }
  void fill(CurveRecord& r, const Geometry* g, size_t i) const
  {
    g->nativeCurve(i, &r.v0x);
    r.N = g->curveRate();
  }
};

// The Source of the round Bezier and B-spline curves (round_curves=1): the record of the flat curves - the native control points - with
// N = 0 (a tube has no tessellation rate), the box the reference's accurateBounds().  One time step only: Scene::commit has refused the rest.
struct RoundCurveSource
{
  bool takes(const Scene*, const Geometry* g) const { return g->isRoundCurve() && g->timeSteps == 1; }
  size_t count(const Geometry* g) const { return g->numCurves(); }
  bool valid(const Geometry* g, size_t i) const { return g->validCurve(i); }
  Box3 box(const Geometry* g, size_t i) const
  {
    float cp[16];
    g->nativeCurve(i, cp);
    return curve_accurate_bounds(cp);
  }
  void fill(CurveRecord& r, const Geometry* g, size_t i) const { g->nativeCurve(i, &r.v0x); }
};

// ---- the motion-blur frame ----------------------------------------------------------------------------------------------------------------
// The frame of the motion-blur builders, as build_static_bvh8 is the one of the static builders: one BVH8 with the triangle settings over
// (primitive, time segment) pairs of the scene's enabled geometries with more than one time step that the Source takes.  A pair's box is the union
// of the primitive's boxes at the two ends of the segment - the vertices move on straight lines in between, so the box holds the
// primitive at every time of the segment (and, by the same argument, NOT at extrapolated times: a ray with a time outside [0, 1] sees
// the first / last segment only where it still is inside its box).  A pair gets a record only when the primitive is valid at both ends.
// `A` is untouched when there is no record; the kind - kindSwept, or kindLinear under mb_bounds=linear -, robust and the records are
// stored once there are some.
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
// Which geometries, and where a primitive's end boxes and record come from, is the Source's business (MeshMBSource: NV vertices through
// an index record; LineMBSource: two FLOAT4 vertices through one index word, boxes enlarged by the radius; CurveMBSource: four native
// control points through one index word, boxes of the tessellated ribbon):
//   takes(s, g)                    the geometry is of the Source's type and has more than one time step
//   count(g)                       its primitives
//   valid(g, i, step)              the primitive at a time step (TriangleMesh / QuadMesh / LineSegments::valid(i, itime))
//   boxes(g, i, seg, a, b, mid)    its boxes at steps seg and seg + 1 and at mid-segment
//   fill(rec, g, i, seg)           the geometry of the record; the four id words are set here
template <class Rec, class Source>
static void build_mb_bvh8(Scene* s, Accel& A, const Source& source, const char* tooMany, uint32_t kindSwept, uint32_t kindLinear, bool robust)
{
  const bool linear = s->device->mb_bounds == "linear";
  struct Ends { Box3 a, b; double ta, tb; }; // linear: a pair's boxes at the start / end of its segment and their global times
  std::vector<Src> src;
  std::vector<Ends> ends;
  std::vector<BuildPrim> bp;
  Box3 swept;
  for (unsigned gid = 0; gid < s->geometries.size(); gid++) {
    const Geometry* g = s->geometries[gid];
    if (!g || !g->enabled || !source.takes(s, g)) continue;
    for (unsigned t = 0; t < g->timeSteps; t++) {
      const BufferView* vv = g->view(RTC_BUFFER_TYPE_VERTEX, t);
      if (!vv || !vv->valid()) RT_THROW(RTC_ERROR_INVALID_OPERATION, "motion blur geometry: a time step has no vertex buffer");
    }
    const size_t n = source.count(g);
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
  if (bp.empty()) return;
  check_leaf_limit(bp.size(), tooMany);

  std::vector<Rec> recs;
  const MakeLeafFn makeLeaf = leaf_maker(s, src, recs, [&source](Rec& r, const Geometry* g, const Src& sr) {
    source.fill(r, g, sr.primID, sr.segment);
    r.segment = sr.segment;
    r.numSegments = g->timeSteps - 1;
  });
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
    store_tree(A, A.nodesMB, build_bvh8_mb(bp, build_settings(s), makeLeaf, linear_bounds));
    s->bounds.extend(swept);
  } else {
    store_tree(A, A.nodes, build_bvh8(bp, build_settings(s), makeLeaf));
    for (const BuildPrim& p : bp) s->bounds.extend(p.box);
  }
  finish_accel(A, recs, linear ? kindLinear : kindSwept, robust);
}

// The Source of the triangle and quad meshes: NV vertices through the index record (UINT3 / UINT4), a box is the box of the vertices, the
// mid-segment box the box of the vertices' midpoints; fill(rec, v) writes the 2 * NV vertices (segment start, then segment end) into the
// zeroed record.
template <int NV, class Rec, class Fill> struct MeshMBSource
{
  const Fill& fillVertices;
  bool takes(const Scene*, const Geometry* g) const { return g->type == (NV == 4 ? RTC_GEOMETRY_TYPE_QUAD : RTC_GEOMETRY_TYPE_TRIANGLE) && g->timeSteps != 1; }
  size_t count(const Geometry* g) const { return g->numTriangles(); } // index buffer records
  bool valid(const Geometry* g, size_t i, unsigned step) const { return NV == 4 ? g->validQuad(i, step) : g->validTriangle(i, step); }
  void boxes(const Geometry* g, size_t i, unsigned seg, Box3& a, Box3& b, Box3& mid) const
  {
    V3 v[2 * NV];
    mesh_vertices<NV>(g, i, seg, v);
    mesh_vertices<NV>(g, i, seg + 1, v + NV);
    for (int k = 0; k < NV; k++) {
      a.extend(v[k]);
      b.extend(v[NV + k]);
      mid.extend((v[k] + v[NV + k]) * 0.5f);
    }
  }
  void fill(Rec& r, const Geometry* g, size_t i, unsigned seg) const
  {
    V3 v[2 * NV];
    mesh_vertices<NV>(g, i, seg, v);
    mesh_vertices<NV>(g, i, seg + 1, v + NV);
    fillVertices(r, v);
  }
};

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
  bool takes(const Scene*, const Geometry* g) const { return g->type == RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE && g->timeSteps != 1; }
  size_t count(const Geometry* g) const { return g->numSegments(); }
  bool valid(const Geometry* g, size_t i, unsigned step) const { return g->validSegment(i, step); }
  void boxes(const Geometry* g, size_t i, unsigned seg, Box3& a, Box3& b, Box3& mid) const
  {
    const float *p0a = line_vertex(g, i, seg, 0), *p1a = line_vertex(g, i, seg, 1), *p0b = line_vertex(g, i, seg + 1, 0), *p1b = line_vertex(g, i, seg + 1, 1);
    line_box_of(p0a, p1a, a);
    line_box_of(p0b, p1b, b);
    float m0[4], m1[4];
    for (int c = 0; c < 4; c++) {
      m0[c] = (p0a[c] + p0b[c]) * 0.5f;
      m1[c] = (p1a[c] + p1b[c]) * 0.5f;
    }
    line_box_of(m0, m1, mid);
  }
  void fill(LineMBRecord& r, const Geometry* g, size_t i, unsigned seg) const
  {
    memcpy(&r.v0ax, line_vertex(g, i, seg, 0), 16);
    memcpy(&r.v1ax, line_vertex(g, i, seg, 1), 16);
    memcpy(&r.v0bx, line_vertex(g, i, seg + 1, 0), 16);
    memcpy(&r.v1bx, line_vertex(g, i, seg + 1, 1), 16);
  }
};

// The Source of the flat Bezier and B-spline curves: four native (Bezier) control points (x, y, z, radius) through one index word, B-spline
// input converted per time step (Geometry::nativeCurve(i, out, step)).  A curve's box at a step is curve_tessellated_bounds of its native
// points at that step with the geometry's rate N; the mid-segment box is that of the midpoints of the native points.
// Containment (swept and linear): at ftime f the leaf interpolates the four native points in all four components and cuts the result
// into the N quads between the tessellation points P_j(f), j = 0 .. N, with half widths w_j(f) (CurveMBLeaf, trace_curve_mb.hip).  P_j
// and w_j are Bezier combinations - fixed weights per j - of the control points, hence LINEAR in the control points, and the control
// points are linear in f: x_j(f) and w_j(f) are linear in f.  Per axis the box of the ribbon (curve_tessellated_bounds' argument) is
// min_j x_j(f) - max_j |w_j(f)| below and max_j x_j(f) + max_j |w_j(f)| above.  A minimum of linear functions is concave, a maximum of
// linear functions and of their absolute values convex: the lower plane is a concave function of f and lies ON OR ABOVE the chord of its
// end values, the upper plane a convex one ON OR BELOW its chord.  So the box at f lies inside the interpolation of the two end boxes,
// which is what linear_bounds needs of a pair's ends, and the interpolation lies inside their union, the swept box.
// In fp32 (the budget of accel.h QNodeMB8, one grid step s >= 2^-21 R): interpolating the control points costs what it costs the line
// leaf - three roundings on the coordinate, three on the radius, the plane's own two and time_segment's 2^-9 s on both: 7 * 2^-24 R +
// 2^-8 s + 2^-17 s < s (LineMBSource) - and that alone leaves s / 8.  The Bezier combine comes on top, which the line leaf does not
// have: a basis weight carries at most 4 roundings, the weights are non-negative and sum to 1, so with M the largest |x|, |y|, |z|,
// |radius| among the four control points the weights' errors move a tessellation point by at most 4 * 2^-24 M and the product and three
// madds of the combine by another 4 * 2^-24 M; the same again for the half width: 16 * 2^-24 M per evaluation.  It is evaluated twice,
// on the host for the end boxes and in the leaf for the quads, and the host result is not the exact one either: 32 * 2^-24 M = 2^-19 M,
// which can be four grid steps.  The padding does not cover that, so the END BOXES are widened here, each by 3 * 2^-20 M of its own
// step's control points (2^-19 M and half as much again for the subtraction's own rounding and for M being rounded); the quantizer is
// untouched.  M(f) of the interpolated points is at most the interpolation of M at the two ends (|.| is convex), so the interpolated
// margin covers the budget at every f.  The mid-segment box only places the pair in the tree and is not widened.
struct CurveMBSource
{
  bool takes(const Scene*, const Geometry* g) const { return g->isFlatCubicCurve() && g->timeSteps != 1; }
  size_t count(const Geometry* g) const { return g->numCurves(); }
  bool valid(const Geometry* g, size_t i, unsigned step) const { return g->validCurve(i, step); }
  static Box3 widened_bounds(const float cp[16], unsigned N)
  {
    float M = 0.0f;
    for (int k = 0; k < 16; k++) M = std::max(M, fabsf(cp[k]));
    const float e = M * (3.0f / 1048576.0f);
    const Box3 b = curve_tessellated_bounds(cp, N);
    Box3 w;
    w.extend(V3(b.lo.x - e, b.lo.y - e, b.lo.z - e));
    w.extend(V3(b.hi.x + e, b.hi.y + e, b.hi.z + e));
    return w;
  }
  void boxes(const Geometry* g, size_t i, unsigned seg, Box3& a, Box3& b, Box3& mid) const
  {
    float ca[16], cb[16], cm[16];
    g->nativeCurve(i, ca, seg);
    g->nativeCurve(i, cb, seg + 1);
    for (int k = 0; k < 16; k++) cm[k] = (ca[k] + cb[k]) * 0.5f;
    const unsigned N = g->curveRate();
    a = widened_bounds(ca, N);
    b = widened_bounds(cb, N);
    mid = curve_tessellated_bounds(cm, N);
  }
  void fill(CurveMBRecord& r, const Geometry* g, size_t i, unsigned seg) const
  {
    g->nativeCurve(i, &r.v0ax, seg);
    g->nativeCurve(i, &r.v0bx, seg + 1);
    r.N = g->curveRate();
  }
};

// ---- the builders, in Scene::commit's order -------------------------------------------------------------------------------------------
// Triangle meshes, accel selection: scene.cpp:130-211.  Everything is served by the one BVH8 layout; the name only picks the leaf
// arithmetic (Triangle4v/Pluecker/robust vs Triangle4/Moeller/fast).  TriRecords, in `prims`.
void build_triangle_accel(Scene* s)
{
  Accel& A = s->triAccel;
  A.clear();
  const bool pluecker = wants_pluecker(s, s->device->tri_accel, {"bvh8.triangle4v", "bvh4.triangle4v"}, {"bvh8.triangle4", "bvh4.triangle4", "qbvh8.triangle4"},
                                       "unknown triangle acceleration structure ");
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
  build_static_bvh8<TriRecord>(s, A, MeshSource<3, TriRecord, decltype(fill)>{fill}, "too many triangles for the 26-bit leaf reference",
                               pluecker ? ACCEL_TRI_PLUECKER : ACCEL_TRI_MOELLER, pluecker);
}

// Triangle meshes with more than one time step (scene.cpp:213-247).  Every name is served by the one TriMBRecord layout: default =
// Pluecker + robust traversal for a robust scene, Moeller + fast traversal otherwise; an explicit triangle4imb / triangle4vmb accel is
// the fast (Moeller) variant.
void build_trimb_accel(Scene* s)
{
  Accel& A = s->triMBAccel;
  A.clear();
  const bool pluecker = wants_pluecker(s, s->device->tri_accel_mb, {}, {"bvh8.triangle4imb", "bvh4.triangle4imb", "bvh8.triangle4vmb", "bvh4.triangle4vmb"},
                                       "unknown motion blur triangle acceleration structure ");
  auto fill = [](TriMBRecord& r, const V3* v) {
    r.a0x = v[0].x; r.a0y = v[0].y; r.a0z = v[0].z;
    r.b0x = v[1].x; r.b0y = v[1].y; r.b0z = v[1].z;
    r.c0x = v[2].x; r.c0y = v[2].y; r.c0z = v[2].z;
    r.a1x = v[3].x; r.a1y = v[3].y; r.a1z = v[3].z;
    r.b1x = v[4].x; r.b1y = v[4].y; r.b1z = v[4].z;
    r.c1x = v[5].x; r.c1y = v[5].y; r.c1z = v[5].z;
  };
  build_mb_bvh8<TriMBRecord>(s, A, MeshMBSource<3, TriMBRecord, decltype(fill)>{fill}, "too many motion blur triangle segments for the 26-bit leaf reference",
                             pluecker ? ACCEL_TRIMB_PLUECKER : ACCEL_TRIMB_MOELLER, pluecker ? ACCEL_TRIMB_LINEAR_PLUECKER : ACCEL_TRIMB_LINEAR_MOELLER, pluecker);
}

// Quad meshes: one BVH8 over whole quads with the triangle settings; the records keep the four vertices (QuadMv) and go to the
// accel's byte array.  Accel choice (scene.cpp:251-330, bvh8_factory.h:43): default = Pluecker + robust traversal for a robust scene,
// Moeller + fast traversal otherwise; an explicit quad4v / quad4i accel is the fast (Moeller) variant.
void build_quad_accel(Scene* s)
{
  Accel& A = s->quadAccel;
  A.clear();
  const bool pluecker = wants_pluecker(s, s->device->quad_accel, {}, {"bvh8.quad4v", "bvh4.quad4v", "bvh8.quad4i", "bvh4.quad4i", "qbvh8.quad4i"}, "unknown quad acceleration structure ");
  auto fill = [](QuadRecord& q, const V3* v) {
    q.v0x = v[0].x; q.v0y = v[0].y; q.v0z = v[0].z;
    q.v1x = v[1].x; q.v1y = v[1].y; q.v1z = v[1].z;
    q.v2x = v[2].x; q.v2y = v[2].y; q.v2z = v[2].z;
    q.v3x = v[3].x; q.v3y = v[3].y; q.v3z = v[3].z;
  };
  build_static_bvh8<QuadRecord>(s, A, MeshSource<4, QuadRecord, decltype(fill)>{fill}, "too many quads for the 26-bit leaf reference",
                                pluecker ? ACCEL_QUAD_PLUECKER : ACCEL_QUAD_MOELLER, pluecker);
}

// Quad meshes with more than one time step (scene.cpp:332-367): QuadMBRecords, default = Pluecker + robust traversal for a robust
// scene, Moeller + fast traversal otherwise; an explicit quad4imb accel is the fast (Moeller) variant.  A host-only device builds
// this accel only when its config names quad_accel_mb= (Device::quads_mb_enabled; MeshSource::takes raises otherwise).
void build_quadmb_accel(Scene* s)
{
  Accel& A = s->quadMBAccel;
  A.clear();
  const bool pluecker = wants_pluecker(s, s->device->quad_accel_mb, {}, {"bvh8.quad4imb", "bvh4.quad4imb"}, "unknown motion blur quad acceleration structure ");
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
  build_mb_bvh8<QuadMBRecord>(s, A, MeshMBSource<4, QuadMBRecord, decltype(fill)>{fill}, "too many motion blur quad segments for the 26-bit leaf reference",
                              pluecker ? ACCEL_QUADMB_PLUECKER : ACCEL_QUADMB_MOELLER, pluecker ? ACCEL_QUADMB_LINEAR_PLUECKER : ACCEL_QUADMB_LINEAR_MOELLER, pluecker);
}

// Flat Bezier and B-spline curves (Scene::createHairAccel, scene.cpp:370-416): one BVH8 with the line accel's builder settings over the
// valid curves of the scene's enabled flat cubic curve geometries, CurveRecords in `blobs`.  Every name the reference accepts builds
// this accel; its oriented-box nodes (bvh4obb / bvh8obb) are not built.  The reference has one ribbon intersector, so the kind only
// tells the traversal: robust for a robust scene, fast otherwise.
void build_curve_accel(Scene* s)
{
  Accel& A = s->curveAccel;
  A.clear();
  if (!s->device->curves_enabled()) return; // (no curve geometry can exist on such a device)
  const std::string& name = s->device->hair_accel;
  if (!one_of(name, {"default", "bvh4.bezier1v", "bvh4.bezier1i", "bvh4obb.bezier1v", "bvh4obb.bezier1i", "bvh8obb.bezier1v", "bvh8obb.bezier1i"}))
    RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown hair acceleration structure " + name);
  build_static_bvh8<CurveRecord>(s, A, CurveSource(), "too many curves for the 26-bit leaf reference", s->isRobust() ? ACCEL_CURVE_ROBUST : ACCEL_CURVE_FAST, s->isRobust());
}

// Flat Bezier and B-spline curves with more than one time step (Scene::createHairMBAccel, scene.cpp:418-441): CurveMBRecords under the
// frame of the motion-blur meshes.  Every name the reference accepts builds this accel; its oriented-box nodes (bvh4obb / bvh8obb under
// `default`) are not built.  The kind tells the traversal (robust for a robust scene) and the node type (mb_bounds).  A host-only
// device builds this accel only when its config names hair_accel_mb= (Device::curves_mb_enabled; CurveSource::takes raises otherwise).
void build_curvemb_accel(Scene* s)
{
  Accel& A = s->curveMBAccel;
  A.clear();
  if (!s->device->curves_enabled() || !s->device->curves_mb_enabled()) return;
  const std::string& name = s->device->hair_accel_mb;
  if (!one_of(name, {"default", "bvh4.bezier1imb", "bvh8.bezier1imb"})) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown motion blur hair acceleration structure " + name);
  const bool robust = s->isRobust();
  build_mb_bvh8<CurveMBRecord>(s, A, CurveMBSource(), "too many motion blur curve segments for the 26-bit leaf reference",
                               robust ? ACCEL_CURVEMB_ROBUST : ACCEL_CURVEMB_FAST, robust ? ACCEL_CURVEMB_LINEAR_ROBUST : ACCEL_CURVEMB_LINEAR_FAST, robust);
}

// Flat linear curves (Scene::createLineAccel, scene.cpp:444-468: bvh8.line4i; BVHNBuilderSAH<8,LineSegments,Line4i>(..., 4, 1.0f, 4, inf)):
// one BVH8 with the triangle settings over the valid segments of the scene's enabled line geometries, LineRecords in `blobs`.  Every name
// builds the same accel; the reference has one line intersector, so the kind only tells the traversal: robust for a robust scene, fast
// otherwise.
void build_line_accel(Scene* s)
{
  Accel& A = s->lineAccel;
  A.clear();
  const std::string& name = s->device->line_accel;
  if (!one_of(name, {"default", "bvh8.line4i", "bvh4.line4i"})) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown line segment acceleration structure " + name);
  build_static_bvh8<LineRecord>(s, A, LineSource(), "too many line segments for the 26-bit leaf reference", s->isRobust() ? ACCEL_LINE_ROBUST : ACCEL_LINE_FAST, s->isRobust());
}

// Flat linear curves with more than one time step (Scene::createLineMBAccel, scene.cpp:470-494: bvh8.line4imb): LineMBRecords under the
// frame of the motion-blur meshes.  Every name builds the same accel; the kind tells the traversal (robust for a robust scene) and the
// node type (mb_bounds).  A host-only device builds this accel only when its config names line_accel_mb= (Device::lines_mb_enabled;
// LineSource::takes raises otherwise).
void build_linemb_accel(Scene* s)
{
  Accel& A = s->lineMBAccel;
  A.clear();
  if (!s->device->lines_mb_enabled()) return;
  const std::string& name = s->device->line_accel_mb;
  if (!one_of(name, {"default", "bvh8.line4imb", "bvh4.line4imb"})) RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown motion blur line segment acceleration structure " + name);
  const bool robust = s->isRobust();
  build_mb_bvh8<LineMBRecord>(s, A, LineMBSource(), "too many motion blur line segments for the 26-bit leaf reference",
                              robust ? ACCEL_LINEMB_ROBUST : ACCEL_LINEMB_FAST, robust ? ACCEL_LINEMB_LINEAR_ROBUST : ACCEL_LINEMB_LINEAR_FAST, robust);
}

// Round Bezier and B-spline curves (round_curves=1).  The reference keeps them in the hair accel beside the flat ones (createHairAccel);
// here they get a BVH8 of their own, under the static frame and with the hair accel's names (oriented-box nodes are not built), over the
// boxes of accurateBounds().  The accel has the flat curves' kinds - the kind tells the traversal only - and says with Accel::roundCurves
// that its CurveRecords are tubes: launch_trace_curve hands such a launch to launch_trace_round_curve (trace_round_curve.hip).
void build_round_curve_accel(Scene* s)
{
  Accel& A = s->roundCurveAccel;
  A.clear();
  if (!s->device->round_curves_enabled()) return; // (no round curve geometry can exist on such a device)
  const std::string& name = s->device->hair_accel;
  if (!one_of(name, {"default", "bvh4.bezier1v", "bvh4.bezier1i", "bvh4obb.bezier1v", "bvh4obb.bezier1i", "bvh8obb.bezier1v", "bvh8obb.bezier1i"}))
    RT_THROW(RTC_ERROR_INVALID_ARGUMENT, "unknown hair acceleration structure " + name);
  build_static_bvh8<CurveRecord>(s, A, RoundCurveSource(), "too many round curves for the 26-bit leaf reference", s->isRobust() ? ACCEL_CURVE_ROBUST : ACCEL_CURVE_FAST, s->isRobust());
  A.roundCurves = A.kind != ACCEL_NONE ? 1u : 0u;
}

} // namespace rtamd
