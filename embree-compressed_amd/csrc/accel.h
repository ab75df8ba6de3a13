// Device-resident acceleration-structure records shared by the host builders and the HIP kernels.
//
// Everything the kernels read lives in four flat HBM arrays per committed scene:
//   nodes   : QNode8[]       96-byte quantized BVH8 nodes, index 0 = root (if the root is inner);
//                            QNodeMB8[] (144-byte time-dependent nodes) in the motion-blur accels built with mb_bounds=linear
//   prims   : TriRecord[]    48-byte triangle records (v0,v1,v2 or v0,e1,e2 + ids), leaf-contiguous
//   blobs   : bytes          cBVH / GridSOA leaf blobs for subdivision geometry (16-byte aligned each),
//                            or QuadRecord[] (64-byte quad records, leaf-contiguous) for quad geometry,
//                            or TriMBRecord[] (96-byte motion-blur triangle records, leaf-contiguous) for triangle meshes with time steps,
//                            or QuadMBRecord[] (128-byte motion-blur quad records, leaf-contiguous) for quad meshes with time steps,
//                            or LineRecord[] (48-byte line segment records, leaf-contiguous) for flat linear curves,
//                            or LineMBRecord[] (80-byte motion-blur line segment records, leaf-contiguous) for flat linear curves with time steps,
//                            or CurveRecord[] (80-byte flat cubic curve records, leaf-contiguous) for flat Bezier and B-spline curves,
//                            or CurveMBRecord[] (160-byte motion-blur flat cubic curve records, leaf-contiguous) for such curves with time steps,
//                            or InstanceRecord[] (64-byte instance records, one per top-level leaf) for instances, followed in
//                            the kinds ACCEL_INST_PLUECKER / ACCEL_INST_MOELLER by the instanced scenes' QuadRecord[], in the kinds
//                            ACCEL_INSTMESHMB_* also by InstanceSceneRecord[], TriMBRecord[] and QuadMBRecord[] (see InstanceRecord)
// The reference keeps the same information behind 64-bit tagged pointers (kernels/bvh/bvh.h:150-396,
// AlignedNode :433-594, QuantizedNode :1150-1324, Triangle4v kernels/geometry/trianglev.h:24-162).
#pragma once
#include <stddef.h>
#include <stdint.h>
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace rtamd {

// ---- child / node references (32 bit) -------------------------------------------------------------
// bit 31      : leaf flag
// inner       : bits 0..30 = node index
// triangle leaf: bits 26..30 = triangle count (1..28, i.e. up to 7 blocks of 4 like bvh.h:140), bits 0..25 = first record
// quad leaf   : the same form, counting quads
// MB tri leaf : the same form, counting TriMBRecords (one per triangle and time segment)
// MB quad leaf: the same form, counting QuadMBRecords (one per quad and time segment)
// line leaf   : the same form, counting LineRecords
// MB line leaf: the same form, counting LineMBRecords (one per segment and time segment)
// curve leaf  : the same form, counting CurveRecords (one per curve)
// MB curve leaf: the same form, counting CurveMBRecords (one per curve and time segment)
// subdiv leaf : bits 0..30 = blob index (one blob per leaf, like encodeTypedLeaf(ptr,1) bvh_builder_subdiv.cpp:728)
static const uint32_t REF_EMPTY = 0xFFFFFFFFu; // no child (reference: BVH::emptyNode, bvh.h:117-132)
static const uint32_t REF_LEAF = 0x80000000u;
static const uint32_t TRI_LEAF_MAX = 28;
static const uint32_t TRI_START_BITS = 26;

inline __host__ __device__ uint32_t make_tri_leaf(uint32_t first, uint32_t count)
{
  return REF_LEAF | (count << TRI_START_BITS) | first;
}

// ---- quantized BVH8 node, 96 bytes = 6 x dwordx4 ----------------------------------------------------
// Child i box, per axis a:  lo = fmaf(float(qlo[a][i]), scale[a], origin[a]),  hi likewise with qhi,
// scale[a] = as_float(uint32(exp[a]) << 23)  (a power of two, or 0.0 for a flat axis).
// The builder guarantees lo <= exact child lower and hi >= exact child upper under exactly this fp32
// formula, so the box test is conservative.  Empty children have child == REF_EMPTY and an inverted box.
struct alignas(16) QNode8
{
  float origin[3];
  uint8_t exp[3];
  uint8_t pad;
  uint32_t child[8];
  uint8_t q[6][8]; // lo_x, hi_x, lo_y, hi_y, lo_z, hi_z  (same plane order as AlignedNode, bvh.h:588-593)
};
static_assert(sizeof(QNode8) == 96, "QNode8 must be 96 bytes");

// ---- time-dependent quantized BVH8 node (linear bounds), 144 bytes = 9 x dwordx4 ------------------------------
// The node of the motion-blur accels built with mb_bounds=linear (kinds ACCEL_*MB_LINEAR_*): the 96 bytes of a QNode8 - whose plane
// block q holds the children's boxes at time 0 - followed by a second plane block q1 with their boxes at time 1, both on ONE origin /
// exponent grid (the reference keeps a float box and its change over the shutter per child, AlignedNodeMB, bvh.h:597-835).  Child i's plane p at ray time t, with
// t the ray's time on the global [0, 1] axis (NOT a per-mesh segment time), is interpolated in grid units and decoded once:
//   tc = fminf(fmaxf(t, 0), 1)
//   qf = fmaf(tc, float(q1[p][i]) - float(q[p][i]), float(q[p][i]))          (the difference of two bytes is exact)
//   plane = fmaf(qf, scale[a], origin[a])                                    (scale[a] as in QNode8, never 0.0 here: exp >= 1)
// Guarantee (quantize_node_mb): for every t in [0, 1] the box so decoded holds every vertex that any record below the child produces
// for a ray at time t that the record accepts - time_segment() is true and the vertices go through lerp_vertex() (trace_mb.hip.h) -
// under exactly these fp32 formulas.  The argument:
//  * In real arithmetic the plane is lerp(P0, P1, t) of the two decoded end planes.  The builder hands over end boxes B(0), B(1)
//    whose real lerp holds every record at both global ends of its segment, hence (both sides are linear) at every time of it, and
//    the quantizer moves every end plane outward by at least ONE grid step s beyond B: lower planes lie in (lo - 2 s, lo - s], upper
//    planes in [hi + s, hi + 2 s).  The real interpolated plane is therefore at least s outside the real interpolated vertex.
//  * What fp32 adds, with R the largest magnitude on the node's grid (all planes and all vertices below lie on it, so |x| <= R and
//    |p1 - p0| <= 255 s for a record's two ends): the plane's two roundings are at most 2^-17 s + 2^-24 R; lerp_vertex's three at
//    most 3 * 2^-24 R; time_segment's product time * S is off by at most 2^-24 S, which moves the vertex by at most 255 s * 2^-24 S
//    <= 2^-9 s for the at most 128 segments of a mesh (the same bound holds for a ray whose product rounds onto the next segment's
//    first instant).  The quantizer picks the exponent so that s >= 2^-21 R, and the origin as a multiple of s; the sum is then
//    below s / 2 + s / 256 < s.
// At t = 0 and t = 1 the decode is exact (origin and planes are multiples of s below 2^24 s), so the box there exceeds B by at least
// one and by less than two grid steps per side.  Times outside [0, 1] are clamped: the box stays the one of the nearer end while a
// record extrapolates, so such rays are no more conservative than under swept boxes - and never fault.
// Empty children have child == REF_EMPTY and inverted boxes in both blocks.
struct alignas(16) QNodeMB8
{
  float origin[3];
  uint8_t exp[3];
  uint8_t pad;
  uint32_t child[8];
  uint8_t q[6][8];  // time 0: lo_x, hi_x, lo_y, hi_y, lo_z, hi_z
  uint8_t q1[6][8]; // time 1, same order
};
static_assert(sizeof(QNodeMB8) == 144, "QNodeMB8 must be 144 bytes");

// ---- triangle record, 48 bytes = 3 x dwordx4 ----------------------------------------------------------
// Pluecker accel (robust):  a = v0, b = v1, c = v2            (TriangleMv, trianglev.h:156-161)
// Moeller  accel (default): a = v0, b = e1 = v0-v1, c = e2 = v2-v0   (TriangleM, triangle.h:52-53)
// Records of one leaf are contiguous; every group of 4 from the leaf start is one "block" and keeps the
// reference's 4-wide SIMD semantics (all 4 tested against the tfar at block entry, lowest lane wins ties).
struct alignas(16) TriRecord
{
  float ax, ay, az;
  uint32_t geomID;
  float bx, by, bz;
  uint32_t primID;
  float cx, cy, cz;
  uint32_t pad;
};
static_assert(sizeof(TriRecord) == 48, "TriRecord must be 48 bytes");

// ---- quad record, 64 bytes = 4 x dwordx4 ---------------------------------------------------------------------
// The four vertices as given (QuadMv, quadv.h); both accels (Pluecker / Moeller) read the same record and split the quad into
// triangle A = (v0, v1, v3) and B = (v2, v1, v3) at run time.  Every group of 4 records from the leaf start is one block of 4 quads =
// one 8-wide block of triangles (the reference's AVX form, quad_intersector_pluecker.h:264-299).
struct alignas(16) QuadRecord
{
  float v0x, v0y, v0z;
  uint32_t geomID;
  float v1x, v1y, v1z;
  uint32_t primID;
  float v2x, v2y, v2z;
  uint32_t pad0;
  float v3x, v3y, v3z;
  uint32_t pad1;
};
static_assert(sizeof(QuadRecord) == 64, "QuadRecord must be 64 bytes");

// ---- line segment record, 48 bytes = 3 x dwordx4 -----------------------------------------------------------------------
// One segment of a flat linear curve (RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE): its two end points with their radii, gathered at commit
// (the reference keeps the index of the first vertex and gathers per visit, LineMi<4> / Line4i, kernels/geometry/linei.h; here the
// record stands in for it as QuadRecord does for Quad4i).  One record serves the robust and the fast accel: the reference has a single
// line intersector (LineIntersector1, line_intersector.h).  Every group of 4 records from the leaf start is one block of the
// reference's 4-wide form: all 4 tested against the tfar at block entry, lowest lane wins ties.
struct alignas(16) LineRecord
{
  float v0x, v0y, v0z, r0;
  float v1x, v1y, v1z, r1;
  uint32_t geomID, primID;
  uint32_t pad[2];
};
static_assert(sizeof(LineRecord) == 48, "LineRecord must be 48 bytes");

// ---- motion-blur line segment record, 80 bytes = 5 x dwordx4 ------------------------------------------------------------
// One segment of a flat linear curve with time steps at both ends of ONE time segment of its geometry: the end points with their
// radii at step `segment` (v0a, v1a) and at step `segment` + 1 (v0b, v1b).  Time segments, record selection and blocks as for
// TriMBRecord; the end points are interpolated in ALL FOUR components, the radius included (the reference lerps Vec4vf, LineMi::gather
// with a time, linei.h:276-277), and go through the test of the static line leaf.  The radius fills the w of every vertex, so the four
// id words have a dwordx4 of their own (TriMBRecord keeps them in the vertices' w).
struct alignas(16) LineMBRecord
{
  float v0ax, v0ay, v0az, r0a;
  float v1ax, v1ay, v1az, r1a;
  float v0bx, v0by, v0bz, r0b;
  float v1bx, v1by, v1bz, r1b;
  uint32_t geomID, primID;
  uint32_t segment;     // itime this record serves
  uint32_t numSegments; // S of the geometry
};
static_assert(sizeof(LineMBRecord) == 80, "LineMBRecord must be 80 bytes");

// ---- flat cubic curve record, 80 bytes = 5 x dwordx4 -------------------------------------------------------------------
// One curve of a flat Bezier or B-spline geometry (RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE / _FLAT_BSPLINE_CURVE) as its four NATIVE control
// points, Bezier ones, with their radii in w: B-spline input is converted at commit (convert(BSplineCurveT, BezierCurveT),
// kernels/subdiv/bspline_curve.h:180-187), so every curve has four points of its own - control points are shared between curves in the
// user's buffer only.  N is the geometry's tessellation rate, clamp((int)rate, 1, 16): the leaf cuts the curve into N ribbon quads and
// has no geometry table to look the rate up in.
struct alignas(16) CurveRecord
{
  float v0x, v0y, v0z, r0;
  float v1x, v1y, v1z, r1;
  float v2x, v2y, v2z, r2;
  float v3x, v3y, v3z, r3;
  uint32_t geomID, primID;
  uint32_t N;   // ribbon quads per curve, 1..16
  uint32_t pad;
};
static_assert(sizeof(CurveRecord) == 80, "CurveRecord must be 80 bytes");

// ---- motion-blur flat cubic curve record, 160 bytes = 10 x dwordx4 ----------------------------------------------------------
// One curve of a flat Bezier or B-spline geometry with time steps at both ends of ONE time segment of its geometry: the four native
// control points with their radii at step `segment` (v0a .. v3a) and at step `segment` + 1 (v0b .. v3b); B-spline input is converted per
// time step at commit.  Time segments and record selection as for TriMBRecord; the control points are interpolated in ALL FOUR
// components, the radius included (NativeCurves::gather with a time, scene_bezier_curves.h:138-158), and go through the ribbon test of
// the static curve leaf.
// Layout: the plain 160 bytes, not the 144 that packing N (<= 16) and numSegments (<= 128) into one word would give.  The ninth row is
// word for word the id row of LineMBRecord - geomID, primID, segment, numSegments - so the build frame writes the ids of every
// motion-blur record type alike, and the leaf decides from this ONE row, read first, whether the record serves the ray's time segment:
// a record of another segment (S - 1 of S below a leaf under swept boxes) costs one dwordx4 and no unpacking.  N has the tenth row; it
// is read with the control points.  A leaf reads whole 16-byte rows either way, so 144 bytes would save a row of memory per record but
// no request on the records that are skipped.
struct alignas(16) CurveMBRecord
{
  float v0ax, v0ay, v0az, r0a;
  float v1ax, v1ay, v1az, r1a;
  float v2ax, v2ay, v2az, r2a;
  float v3ax, v3ay, v3az, r3a;
  float v0bx, v0by, v0bz, r0b;
  float v1bx, v1by, v1bz, r1b;
  float v2bx, v2by, v2bz, r2b;
  float v3bx, v3by, v3bz, r3b;
  uint32_t geomID, primID;
  uint32_t segment;     // itime this record serves
  uint32_t numSegments; // S of the geometry
  uint32_t N;           // ribbon quads per curve, 1..16
  uint32_t pad[3];
};
static_assert(sizeof(CurveMBRecord) == 160, "CurveMBRecord must be 160 bytes");

// ---- motion-blur triangle record, 96 bytes = 6 x dwordx4 -------------------------------------------------------------
// The three vertices of a triangle at both ends of ONE time segment of its mesh (a0..c0 at step `segment`, a1..c1 at step `segment` + 1).
// A mesh with N time steps has S = N - 1 segments and contributes S records per triangle.  For a ray (getTimeSegment, geometry.h:28-34):
//   ts = time * S, itime = clamp(floor(ts), 0, S - 1), ftime = ts - itime   (times outside [0, 1] extrapolate the first / last segment)
// a record is tested only when itime == segment; its vertices are then lerp(p0, p1, ftime) = fmaf(1 - ftime, p0, ftime * p1)
// (TriangleMi::gather with a time, trianglei.h:343-364) and go through the Pluecker / Moeller test of the static leaf.  Blocks are
// groups of 4 records from the leaf start, as for TriRecord.
struct alignas(16) TriMBRecord
{
  float a0x, a0y, a0z;
  uint32_t geomID;
  float b0x, b0y, b0z;
  uint32_t primID;
  float c0x, c0y, c0z;
  uint32_t segment;     // itime this record serves
  float a1x, a1y, a1z;
  uint32_t numSegments; // S of the mesh
  float b1x, b1y, b1z;
  uint32_t pad0;
  float c1x, c1y, c1z;
  uint32_t pad1;
};
static_assert(sizeof(TriMBRecord) == 96, "TriMBRecord must be 96 bytes");

// ---- motion-blur quad record, 128 bytes = 8 x dwordx4 ----------------------------------------------------------------
// The four vertices of a quad at both ends of ONE time segment of its mesh (v0a..v3a at step `segment`, v0b..v3b at step `segment` + 1);
// segments, record selection and interpolation as for TriMBRecord (QuadMi::gather with a time, quadi.h:441-457), then the A / B split
// and the tests of the static quad leaf.  Blocks are groups of 4 records from the leaf start = one 8-wide block of triangles, as for
// QuadRecord.  The four id words sit in the w of v1 and v3, the vertices BOTH triangles of a quad read (A = v0 v1 v3, B = v2 v1 v3):
// a lane of the octet form that tests B never loads v0 and still has all ids (the static record keeps geomID in v0.w and moves it
// across lanes).
struct alignas(16) QuadMBRecord
{
  float v0ax, v0ay, v0az;
  uint32_t pad0;
  float v1ax, v1ay, v1az;
  uint32_t primID;
  float v2ax, v2ay, v2az;
  uint32_t pad1;
  float v3ax, v3ay, v3az;
  uint32_t geomID;
  float v0bx, v0by, v0bz;
  uint32_t pad2;
  float v1bx, v1by, v1bz;
  uint32_t segment;     // itime this record serves
  float v2bx, v2by, v2bz;
  uint32_t pad3;
  float v3bx, v3by, v3bz;
  uint32_t numSegments; // S of the mesh
};
static_assert(sizeof(QuadMBRecord) == 128, "QuadMBRecord must be 128 bytes");

// ---- instance record, 64 bytes = 4 x dwordx4 -------------------------------------------------------------------------
// One per enabled instance of the scene (Instance, kernels/common/scene_instance.h).  The instance accel keeps, in ONE node array, a
// top-level BVH8 over the instances' world bounds with exactly one instance per leaf (leaf reference = make_tri_leaf(record index, 1))
// and behind it a copy of the triangle tree of every distinct instanced scene, child indices and leaf record offsets rebased into the
// accel's own `nodes` / `prims`; `root` is the rebased root reference of this instance's scene.
// world2local = inverse(local2world) as the columns vx, vy, vz, p of an AffineSpace3f: a ray enters the instance as
// org' = xfmPoint(world2local, org), dir' = xfmVector(world2local, dir) (instance_intersector.cpp:51-56); t is common to both spaces.
//
// Kinds ACCEL_INST_TRI_*: every instanced scene holds triangles only; the arrays are as above and `pad` is zero.
// Kinds ACCEL_INST_PLUECKER / ACCEL_INST_MOELLER: at least one instanced scene has a quad tree.  Per distinct instanced scene (stored once,
// however many instances share it), in the order of first use:
//   nodes : top-level tree | scene 0: triangle nodes, quad nodes | scene 1: triangle nodes, quad nodes | ...   (child indices rebased)
//   prims : scene 0's TriRecords | scene 1's | ...                                                          (triangle leaves rebased)
//   blobs : the N InstanceRecords | scene 0's QuadRecords | scene 1's | ...
// A quad leaf reference is rebased by N + the scene's quad base, so that the kernel indexes `blobs` as ONE array of 64-byte records
// (sizeof(InstanceRecord) == sizeof(QuadRecord)); the rebased first record must stay below 2^26.  `root` is REF_EMPTY for a scene
// without triangles, pad[0] the rebased quad root, REF_EMPTY for a scene without quads.
//
// Kinds ACCEL_INSTMB_*: at least one enabled instance has more than one time step (instance motion blur).  The layout is that of the
// static kind with the same triangle / quad content (ACCEL_INSTMB_TRI_* <-> ACCEL_INST_TRI_*, ACCEL_INSTMB_PLUECKER / _MOELLER <->
// ACCEL_INST_PLUECKER / _MOELLER), with the moving instances' local-to-world transforms appended to `blobs`:
//   blobs : the N InstanceRecords | the QuadRecords | instance a's InstanceSteps (one per time step) | instance b's | ...
// A moving instance's record has pad[1] = (S << 24) | firstStep: S = time steps - 1 segments (1..128), firstStep the index of its
// first InstanceStep in 64-byte units from the start of `blobs` (below 2^24, or the commit is refused).  A ray at `time` enters it
// through world2local(time) = inverse(lerp(step[itime], step[itime + 1], ftime)) (instance_xfm.h; itime / ftime as in the motion-blur
// records above); the record's world2local is the inverse of step 0 as the static path computes it and is not used by the kernel.
// An instance with one time step in such a scene has pad[1] == 0 and is entered through its record exactly as in the static kinds.
// The top-level box of a moving instance is the union over its steps of the transformed scene bounds.
//
// Kinds ACCEL_INSTMESHMB_PLUECKER / _MOELLER: at least one instanced scene has a motion-blur accel (triangle or quad meshes with time
// steps).  One general layout, whatever else the scenes hold (quads and instance steps are always allowed).  Per distinct instanced
// scene, stored once, in the order of first use, its up to four trees in Scene::commit's order:
//   nodes : top-level tree | scene 0: triangle, MB triangle, quad, MB quad nodes | scene 1: ... | ...          (child indices rebased)
//   prims : scene 0's TriRecords | scene 1's | ...
//   blobs : the N InstanceRecords | the QuadRecords | the InstanceSteps | one InstanceSceneRecord per scene |
//           zero padding to a multiple of 96 bytes | scene 0's TriMBRecords | scene 1's | ... |
//           zero padding to a multiple of 128 bytes | scene 0's QuadMBRecords | scene 1's | ...
// `root` of an InstanceRecord is the index, in 64-byte units from the start of `blobs`, of its scene's InstanceSceneRecord, which holds
// the four rebased roots (REF_EMPTY for a tree the scene does not have); pad[0] is zero, pad[1] as in the kinds ACCEL_INSTMB_*.
// A motion-blur triangle leaf is rebased by (byte offset of the TriMBRecord section) / 96 + the scene's base, a motion-blur quad leaf by
// (byte offset of the QuadMBRecord section) / 128 + the scene's base: the kernel indexes `blobs` as ONE array of that record type.
// Every rebased first record must stay below 2^26.  Inside an instance the trees are traversed one after the other, each against the
// tfar the previous one left; while a tree is traversed the later ones wait on the stack as markers (REF_INST_TREE).
// With line segments or flat curves below an instance (device config inst_hair=1; Accel::instHair, LaunchParams::instHair - the kinds stay
// 22 / 23, also when nothing below the instances moves) a scene has up to six trees, the curve and the line tree last:
//   nodes : ... | scene 0: triangle, MB triangle, quad, MB quad, curve, line nodes | scene 1: ... | ...
//   blobs : ... the QuadMBRecords | zero padding to a multiple of 80 bytes | scene 0's CurveRecords | scene 1's | ... |
//           zero padding to a multiple of 48 bytes | scene 0's LineRecords | scene 1's | ...
// and every InstanceSceneRecord of the accel holds curveRoot and lineRoot in words 4 and 5 (REF_EMPTY for a missing tree).  A curve leaf is
// rebased by (byte offset of the CurveRecord section) / 80 + the scene's base, a line leaf by (byte offset of the LineRecord section) / 48 +
// the scene's base: CurveLeaf::intersect and LineLeaf::intersect index `blobs` as ONE array of their record type.  An accel without such
// trees ends behind the QuadMBRecords and keeps words 4 and 5 of its scene records zero, byte for byte what it was before the key existed.
// With line segments or flat curves that have time steps below an instance (inst_hair_mb=1 beside inst_hair=1; Accel::instHair and
// LaunchParams::instHair are 2) a scene has up to eight trees, in the slot order of Scene: triangle, MB triangle, quad, MB quad, curve,
// MB curve, line, MB line (the visiting order).  The two further trees are QNode8 trees over swept boxes, their nodes placed behind the
// scene's line tree's, and `blobs` continues behind the LineRecords:
//   blobs : ... the LineRecords | zero padding to a multiple of 160 bytes | scene 0's CurveMBRecords | scene 1's | ... |
//           zero padding to a multiple of 80 bytes | scene 0's LineMBRecords | scene 1's | ...
// Every InstanceSceneRecord of such an accel holds curveMBRoot and lineMBRoot in words 6 and 7 (REF_EMPTY for a missing tree); their leaves
// are rebased by (byte offset of the section) / 160 or / 80 + the scene's base, so that CurveMBLeaf::intersect and LineMBLeaf::intersect
// index `blobs` as ONE array of their record type.  An accel without such a tree below it is what it is without the key: words 6 and 7
// zero, instHair 0 or 1, its end behind the LineRecords or the QuadMBRecords.
//
// Kinds ACCEL_INSTMESHMB_LINEAR_PLUECKER / _MOELLER (inst_mb_bounds=linear over scenes built under mb_bounds=linear): `prims` and `blobs`
// are those of the kinds ACCEL_INSTMESHMB_*; the motion-blur trees keep their time-dependent nodes, so the node array has two sections:
//   nodes : top-level tree | every scene's static triangle and quad trees (QNode8, in the order above without the motion-blur trees) |
//           zero padding up to a multiple of 144 bytes from the start of the buffer |
//           scene 0: MB triangle, MB quad nodes | scene 1: ... | ...                                          (QNodeMB8)
// A child or root reference inside a motion-blur tree indexes the buffer as ONE array of QNodeMB8: (the section's byte offset) / 144 +
// the node's place in the section (below 2^31, or the commit is refused).  The QNodeMB8s are the instanced scene's own nodes, byte for
// byte apart from the rebased child words, so the containment guarantee of QNodeMB8 holds below an instance as it stands.  The
// top-level tree and the boxes of moving instances are QNode8s over swept boxes as in all instance kinds but ACCEL_INSTTOP_LINEAR_*.  Which node type a reference
// names follows from where it was found: the roots triMBRoot / quadMBRoot of an InstanceSceneRecord and every child below them name
// QNodeMB8s, everything else QNode8s (the kernel keeps the tree's code in its lane state, INST_TREE_*: bit 1 = a motion-blur tree).
// blobOffsets holds two words for inspection: the number of QNodeMB8s and the index of the first one, in 144-byte units.
//
// Kinds ACCEL_INSTTOP_LINEAR_PLUECKER / _MOELLER (inst_bounds=linear, at least one enabled instance with more than one time step): the
// top-level tree itself is made of time-dependent nodes, so a ray enters a moving instance only where the instance is at the ray's time.
// `prims` and `blobs` are ALWAYS the general layout of the kinds ACCEL_INSTMESHMB_* (one InstanceSceneRecord per distinct scene, the
// InstanceSteps, quad, TriMBRecord and QuadMBRecord sections - the last two empty when no instanced scene has moving meshes), so that
// one kernel form serves; `root` of an InstanceRecord names its scene's InstanceSceneRecord.  The node array has the two sections of
// the kinds ACCEL_INSTMESHMB_LINEAR_*, with the top-level tree in the second:
//   nodes : every scene's static triangle and quad trees (QNode8, scene by scene in the order of first use) |
//           zero padding up to a multiple of 144 bytes from the start of the buffer |
//           top-level tree | scene 0: MB triangle, MB quad nodes | scene 1: ... | ...                         (QNodeMB8)
// AccelDesc::root and the inner child references of the top-level tree index the buffer as ONE array of QNodeMB8, as the references
// of the motion-blur trees do (below 2^31, or the commit is refused); a top scene of a single instance still gets a root node, of one
// child, so that its box is tested.  Motion-blur trees exist below such a top scene only on a device that also has
// mb_bounds=linear,inst_mb_bounds=linear - they are QNodeMB8s then, so the code bit INST_TREE_* & 2 keeps its one meaning - and the
// commit refuses moving meshes below the instances otherwise.  Which node type a reference names: everything found outside an
// instance and in a motion-blur tree names QNodeMB8s, the static trees of the instanced scenes QNode8s.
// Child i of a top-level node holds, at every time t in [0, 1], the images of the eight corners of the instanced scenes' bounds
// under lerp(step[k], step[k + 1], f) of every instance below it (instance_linear_bounds, rt_instance_build.cpp, hands quantize_node_mb
// end boxes whose interpolation does; the quantizer's one-step padding covers fp32 as argued at QNodeMB8: all that enters the argument
// is that the bounded points move on straight lines between step times, with |p1 - p0| on the node's grid).  A static instance has
// equal boxes at both ends.  blobOffsets holds the two inspection words of the kinds ACCEL_INSTMESHMB_LINEAR_*; Accel::maxDepth and
// Scene::bounds (extended by the swept unions) are what they are in every instance kind.
//
// Kinds ACCEL_INSTSUBDIV_GRID / ACCEL_INSTSUBDIV_CBVH_LEAF (Scene::instSubdivAccel, an accel of its own beside the one above): instances
// of scenes that hold subdivision meshes only, all with the eager accel or all with bvh4.compressed.leaf at one compression level C.  Per
// distinct instanced scene, stored once, in the order of first use:
//   nodes : top-level tree | scene 0's subdivision BVH8 | scene 1's | ...                                   (child indices rebased)
//   prims : empty
//   blobs : the N InstanceRecords | the InstanceSteps | zero padding to a multiple of the blob stride | scene 0's leaf blobs | scene 1's | ...
// The leaf blobs are GridCells (stride 160) or cBVH blobs (stride cbvh_stride(C, leaf mode), a multiple of 128); AccelDesc::blobStride is
// that stride.  A subdivision leaf reference (REF_LEAF | blob index) is rebased by (byte offset of the blob section) / stride + the
// scene's base, so that the leaf functions' own addressing, blobs + index * stride, finds the blob; the rebased index is at least 1 (the
// records come first), so no leaf reference equals REF_INST_EXIT, and stays below 2^26.  `root` of an InstanceRecord is the rebased root
// of its scene's tree, pad[0] is zero, pad[1] as in the kinds ACCEL_INSTMB_* (firstStep counts the InstanceRecords in front).
// blobOffsets holds two words for inspection: the number of leaf blobs and the index of the first one.
//
// Kinds ACCEL_INSTSUBDIV_TOP_LINEAR_GRID / _CBVH_LEAF (inst_subdiv_bounds=linear, at least one placed subdivision instance with more than
// one time step): the kinds above with a top-level tree of time-dependent nodes, so that a ray enters a moving subdivision instance only
// where the instance is at the ray's time.  `prims` and `blobs` are those of the kinds ACCEL_INSTSUBDIV_* byte for byte apart from the
// `root` words of the InstanceRecords; the node array has two sections as in the kinds ACCEL_INSTTOP_LINEAR_*:
//   nodes : scene 0's subdivision BVH8 | scene 1's | ...   (QNode8, child indices rebased, in order of first use) |
//           zero padding up to a multiple of 144 bytes from the start of the buffer |
//           top-level tree                                                                                     (QNodeMB8)
// AccelDesc::root and the inner child references of the top-level tree index the buffer as ONE array of QNodeMB8 (below 2^31, or the
// commit is refused); the instanced trees lead the buffer, so their rebased roots differ from those of the swept layout.  A top scene of a
// single instance gets a root node of one child.  Which node type a reference names: everything found outside an instance names
// QNodeMB8s, everything inside QNode8s.  The containment guarantee of the top-level boxes is that of the kinds ACCEL_INSTTOP_LINEAR_*
// (instance_linear_bounds over the instanced scene's bounds).  blobOffsets holds FOUR words: the number of leaf blobs, the index of the
// first one, the number of QNodeMB8s and the index of the first one in 144-byte units.  Accel::maxDepth = the top-level depth + 1 for the
// exit marker + the deepest instanced tree; Scene::bounds is extended by the swept unions as in every instance kind.
struct alignas(16) InstanceRecord
{
  float world2local[12]; // vx.xyz, vy.xyz, vz.xyz, p.xyz
  uint32_t geomID;       // of the instance in the top scene: the hit's instID (instance_intersector.cpp:57)
  uint32_t root;         // rebased root reference of the instanced scene's triangle tree
  uint32_t pad[2];       // pad[0]: rebased root reference of the instanced scene's quad tree (kinds ACCEL_INST[MB]_PLUECKER / _MOELLER only)
                         // pad[1]: (S << 24) | firstStep of a moving instance (kinds ACCEL_INSTMB_* only), else 0
};
static_assert(sizeof(InstanceRecord) == 64, "InstanceRecord must be 64 bytes");
// One time step of a moving instance (kinds ACCEL_INSTMB_*), 64 bytes = 4 x dwordx4, of which the kernel loads three
struct alignas(16) InstanceStep
{
  float local2world[12]; // vx.xyz, vy.xyz, vz.xyz, p.xyz
  uint32_t pad[4];       // zero
};
static_assert(sizeof(InstanceStep) == sizeof(InstanceRecord), "the instance kernel indexes InstanceRecords and InstanceSteps as one array");
// Marker on the traversal stack of the instance kernel (trace_instance.hip): popping it leaves the instance.  A leaf-flagged reference with
// count 0, which make_tri_leaf never produces (counts are 1..28), and not REF_EMPTY.
static const uint32_t REF_INST_EXIT = 0x80000000u;
// Second marker of the kernel's QUADS form: stacked above the exit marker when the ray enters an instance whose scene has triangles
// and quads, with the quad root in the entry's distance word; popping it continues in the quad tree.  Leaf-flagged with count 0 too.
static const uint32_t REF_INST_QUADS = 0x80000001u;
static_assert(sizeof(InstanceRecord) == sizeof(QuadRecord), "the instance kernel indexes InstanceRecords and QuadRecords as one array");
// The roots of one instanced scene (kinds ACCEL_INSTMESHMB_*), 64 bytes, of which the kernel loads the first dwordx4.  INST_TREE_*: the
// code of a tree = of the leaf kind the lane runs while it is in that tree; roots[] is in visiting order.
// inst_hair=1 (an accel with Accel::instHair set): the scene's curve and line tree follow in the second dwordx4, which the kernel's HAIR form
// loads as well; their codes keep bit 1 clear ("bit 1 = a motion-blur tree").  Visiting order: triangles, motion-blur triangles, quads,
// motion-blur quads, curves, lines (Scene::commit's).  An accel without hair trees keeps these two words zero and is never read there.
// inst_hair_mb=1 (Accel::instHair == 2): the motion-blur curve and line tree fill the rest of the second dwordx4, words 6 and 7, read by the
// kernel's HAIRMB form; their codes have bit 1 set like the other motion-blur trees' and still fit three bits.  Visiting order: triangles,
// motion-blur triangles, quads, motion-blur quads, curves, motion-blur curves, lines, motion-blur lines - not the word order.  An accel
// without such trees keeps the two words zero.
enum : uint32_t { INST_TREE_TRI = 0, INST_TREE_QUAD = 1, INST_TREE_TRIMB = 2, INST_TREE_QUADMB = 3, INST_TREE_CURVE = 4, INST_TREE_LINE = 5,
                  INST_TREE_CURVEMB = 6, INST_TREE_LINEMB = 7 };
struct alignas(16) InstanceSceneRecord
{
  uint32_t triRoot, triMBRoot, quadRoot, quadMBRoot; // rebased root references, REF_EMPTY for a missing tree
  uint32_t curveRoot, lineRoot;                      // (words 4 and 5) accels with hair trees: the same for the curve and the line tree; zero otherwise
  uint32_t curveMBRoot, lineMBRoot;                  // (words 6 and 7) accels with moving-hair trees: the same for the motion-blur curve and line tree; zero otherwise
  uint32_t pad[8];                                   // zero
};
static_assert(offsetof(InstanceSceneRecord, curveRoot) == 16 && offsetof(InstanceSceneRecord, lineRoot) == 20, "the hair roots lead the second dwordx4");
static_assert(offsetof(InstanceSceneRecord, curveMBRoot) == 24 && offsetof(InstanceSceneRecord, lineMBRoot) == 28, "the moving-hair roots end the second dwordx4");
static_assert(sizeof(InstanceSceneRecord) == sizeof(InstanceRecord), "the instance kernel indexes InstanceRecords and InstanceSceneRecords as one array");
// Markers of the kernel's MESHMB form, one value per pending tree: REF_INST_TREE(code), stacked above the exit marker in reverse
// visiting order with the tree's root in the distance word; popping one switches the lane's leaf kind to `code` and continues at that
// root.  REF_INST_TREE(INST_TREE_QUAD) is REF_INST_QUADS; the triangle tree is always the first one and never waits.  Every marker up to
// REF_INST_TREE(INST_TREE_LINEMB) = REF_INST_TREE(7) is leaf-flagged with count 0 like the exit marker: codes stay below 2^26, the count field.
inline constexpr uint32_t REF_INST_TREE(uint32_t code) { return 0x80000000u + code; }
static_assert(REF_INST_TREE(INST_TREE_QUAD) == REF_INST_QUADS, "the quad tree's marker is the one of the QUADS form");

// ---- eager subdivision leaf: one 3x3-vertex cell (2x2 quads = 8 triangles), 160 bytes = 10 x dwordx4 ------
// Replaces the inner leaves of GridSOA (kernels/geometry/grid_soa.h:267-286, :85-90): the reference stores whole
// <=9x9 sub-grids in SoA form and a private BVH4 down to 3x3-vertex cells; here every cell is self-contained and the
// scene BVH8 goes straight down to cells.  p[r*3+c] is the vertex in row r (v direction), column c (u direction);
// uv[] holds the reference's packed patch coordinates (v16<<16 | u16, scale 8/65536, grid_soa.cpp:48-52).
struct alignas(16) GridCell
{
  float px[9], py[9], pz[9];
  uint32_t uv[9];
  uint32_t geomID, primID;
  uint32_t pad[2];
};
static_assert(sizeof(GridCell) == 160, "GridCell must be 160 bytes");

// ---- fork: compressed per-sub-grid BVH ("cBVH") blob -------------------------------------------------------------
// Mirrors CompressedBVH's members (kernels/geometry/compressed.h:408-433) with offsets instead of host pointers, the 3x3 inverse
// of proj precomputed (the reference inverts at run time, compressed.h:585,647), and the leaf's world bounds kept for the any-hit
// stub.  Round 3 layout, ordered by WHEN a visit needs a field, in 128-byte lines (the blob stride is a multiple of 128 and the
// blob array is 128-byte aligned, so a line of a blob is a line of L2 / HBM):
//   line 0  (CbvhHeader, bytes 0..127)   everything up to and including the frustum test and the projected ray: space, box, proj, a
//           copy of the root node's word, rcp_edges, extent.  The visits that end at the frustum test (compressed_help.h:109-133; 28 % of the
//           metric's, nearly all of a grazing ray's) and the test stage of the two-stage visits touch this ONE line (round 2: the same fields lay in two or three lines of a 448-byte
//           record that started on a line boundary only every other blob).
//   line 1  (CbvhMid, bytes 128..159, then the nodes from byte 160)   ids + uv window (commit only) and the 4-byte node words
//           (compressed_node.h:261-295); C = 3: 32 + 84 bytes, one line.
//   then    (leaf mode) 4^C 2-byte height patches (compressed_leaf.h:21-47), or (grid mode) (2^C+1)^2 float3 vertices, 16-byte
//           aligned; C = 3 leaf mode: bytes 256..383, exactly line 2.
//   tail    (CbvhTail, 64 bytes, 16-byte aligned)   iproj (flat-frame commits only) and the world bounds (any-hit stub only).
// bomberman L6/C3 leaf mode: 512 B per blob (reference 396), 46 528 blobs = 23.8 MB.
struct alignas(16) CbvhHeader
{
  float space[9];       // rows of the 3x3 world->local matrix: l = (dot(row0,p), dot(row1,p), dot(row2,p))
  float box[10];        // frustum: z slab + four 2-D corner points (compressed.h:278-292)
  float proj[9];        // row-major homography
  uint32_t rootWord;    // copy of the first node word (coded modes), so that a visit rejected by the frustum test never leaves line 0
  float rcp_edges;
  float extent;
  uint32_t levels;      // C
};
struct alignas(16) CbvhMid
{
  uint32_t geomID, primID;
  float uv0x, uv0y, uv1x, uv1y; // uv[0], uv[1]
  uint32_t elems;       // (4^C-1)/3 inner nodes
  uint32_t grid_width;  // 2^C+1
};
struct alignas(16) CbvhTail
{
  float iproj[9];       // row-major inverse homography
  float wlo[3], whi[3]; // world-space bounds handed to the outer BVH (bounds_o)
  float pad;
};
static const uint32_t CBVH_HEADER_BYTES = 128, CBVH_MID_BYTES = 32, CBVH_TAIL_BYTES = 64, CBVH_NODES_OFFSET = CBVH_HEADER_BYTES + CBVH_MID_BYTES;
// bvh4.compressed.full: a quadtree node holds its four child boxes as floats (the reference's NodeStorage<flavor::ref,32,32,32>,
// compressed_node.h:371-389, 24 floats); here plane-major so that a quad reads one plane of its four children with one access:
// lx[4], ux[4], ly[4], uy[4], lz[4], uz[4]
static const uint32_t CBVH_FULL_NODE_BYTES = 96;
static_assert(sizeof(CbvhHeader) == CBVH_HEADER_BYTES && sizeof(CbvhMid) == CBVH_MID_BYTES && sizeof(CbvhTail) == CBVH_TAIL_BYTES, "cBVH blob sections");
// section offsets of a blob of compression level C; mode: 0 box, 1 leaf, 2 grid, 3 full (CbvhMode / MODE_* of the kernels)
constexpr uint32_t cbvh_elems(uint32_t C) { return ((1u << (2u * C)) - 1u) / 3u; }
constexpr uint32_t cbvh_payload_offset(uint32_t C, uint32_t mode) { return (CBVH_NODES_OFFSET + cbvh_elems(C) * (mode == 3u ? CBVH_FULL_NODE_BYTES : 4u) + 15u) & ~15u; } // cells / grid
constexpr uint32_t cbvh_tail_offset(uint32_t C, uint32_t mode)
{
  return (cbvh_payload_offset(C, mode) + (mode == 1u ? 2u << (2u * C) : (mode == 2u ? 12u * ((1u << C) + 1u) * ((1u << C) + 1u) : 0u)) + 15u) & ~15u;
}
constexpr uint32_t cbvh_stride(uint32_t C, uint32_t mode) { return (cbvh_tail_offset(C, mode) + CBVH_TAIL_BYTES + 127u) & ~127u; }
static_assert(cbvh_payload_offset(3, 1) == 256 && cbvh_tail_offset(3, 1) == 384 && cbvh_stride(3, 1) == 512, "C = 3 leaf mode: header | mid + nodes | cells | tail, one line each");

enum AccelKind : uint32_t
{
  ACCEL_NONE = 0,
  ACCEL_TRI_PLUECKER = 1, // tri_accel=bvh8.triangle4v, or RTC_SCENE_FLAG_ROBUST (scene.cpp:158-164,204)
  ACCEL_TRI_MOELLER = 2,  // default / tri_accel=bvh8.triangle4 / qbvh8.triangle4 (scene.cpp:130-211)
  ACCEL_CBVH_BOX = 3,     // subdiv_accel=bvh4.compressed.box
  ACCEL_CBVH_LEAF = 4,    // subdiv_accel=bvh4.compressed.leaf
  ACCEL_CBVH_GRID = 5,    // subdiv_accel=bvh4.compressed.grid
  ACCEL_GRIDSOA = 6,      // eager subdiv (default subdiv accel)
  ACCEL_CBVH_FULL = 7,    // subdiv_accel=bvh4.compressed.full: the fork's box mode over UNcompressed quadtree nodes (compressed.h:40,774)
  ACCEL_QUAD_PLUECKER = 8, // quad_accel=default with RTC_SCENE_FLAG_ROBUST (scene.cpp:251-330): QuadMv + Pluecker, robust traversal
  ACCEL_QUAD_MOELLER = 9,  // quad_accel=default / bvh8.quad4v / bvh4.quad4v / *.quad4i: QuadMv + Moeller, fast traversal
  ACCEL_TRIMB_PLUECKER = 10, // tri_accel_mb=default with RTC_SCENE_FLAG_ROBUST (scene.cpp:213-247): interpolated triangle + Pluecker, robust traversal
  ACCEL_TRIMB_MOELLER = 11,  // tri_accel_mb=default / bvh8.triangle4imb / bvh4.triangle4imb / *.triangle4vmb: interpolated triangle + Moeller, fast traversal
  ACCEL_QUADMB_PLUECKER = 12, // quad_accel_mb=default with RTC_SCENE_FLAG_ROBUST (scene.cpp:332-367): interpolated quad + Pluecker, robust traversal
  ACCEL_QUADMB_MOELLER = 13,  // quad_accel_mb=default / bvh8.quad4imb / bvh4.quad4imb: interpolated quad + Moeller, fast traversal
  ACCEL_INST_TRI_PLUECKER = 14, // instances of scenes whose triangle accel is ACCEL_TRI_PLUECKER: robust traversal on both levels
  ACCEL_INST_TRI_MOELLER = 15,  // instances of scenes whose triangle accel is ACCEL_TRI_MOELLER: fast traversal on both levels
  ACCEL_INST_PLUECKER = 16,     // instances of scenes with triangles (Pluecker) and / or quads (Pluecker): robust traversal on both levels
  ACCEL_INST_MOELLER = 17,      // instances of scenes with triangles (Moeller) and / or quads (Moeller): fast traversal on both levels
  // instance motion blur: the four kinds above when at least one enabled instance has more than one time step (InstanceStep)
  ACCEL_INSTMB_TRI_PLUECKER = 18,
  ACCEL_INSTMB_TRI_MOELLER = 19,
  ACCEL_INSTMB_PLUECKER = 20,
  ACCEL_INSTMB_MOELLER = 21,
  // at least one instanced scene holds meshes with time steps: one general layout (quads and instance steps allowed), see InstanceRecord
  ACCEL_INSTMESHMB_PLUECKER = 22,
  ACCEL_INSTMESHMB_MOELLER = 23,
  // instances of scenes that hold subdivision meshes only (Scene::instSubdivAccel, see InstanceRecord): one kind per leaf family; the
  // compression level C of the cBVH blobs travels beside the accel (Accel::cbvhLevels -> LaunchParams::cbvhLevels)
  ACCEL_INSTSUBDIV_GRID = 24,     // instanced scenes whose subdivision accel is ACCEL_GRIDSOA (eager): GridCells below the instances
  ACCEL_INSTSUBDIV_CBVH_LEAF = 25, // instanced scenes whose subdivision accel is ACCEL_CBVH_LEAF, all at one C: cBVH blobs below the instances
  // mb_bounds=linear: the four motion-blur mesh accels over time-dependent nodes (QNodeMB8[] in `nodes`, 144-byte stride); records,
  // leaves and the Pluecker / Moeller choice are those of the kinds 10..13.
  ACCEL_TRIMB_LINEAR_PLUECKER = 26,
  ACCEL_TRIMB_LINEAR_MOELLER = 27,
  ACCEL_QUADMB_LINEAR_PLUECKER = 28,
  ACCEL_QUADMB_LINEAR_MOELLER = 29,
  // inst_mb_bounds=linear: the kinds 22 / 23 when at least one instanced scene's motion-blur accel is of the kinds 26..29.  `nodes` holds
  // two sections, QNode8s and then QNodeMB8s (see InstanceRecord); `blobs` and `prims` are those of the kinds 22 / 23
  ACCEL_INSTMESHMB_LINEAR_PLUECKER = 30,
  ACCEL_INSTMESHMB_LINEAR_MOELLER = 31,
  // inst_bounds=linear: the mesh instance accel of a top scene with at least one moving instance.  The top-level tree is made of QNodeMB8s
  // in the second section of `nodes`; `blobs` and `prims` are the general layout of the kinds 22 / 23 / 30 / 31 (see InstanceRecord)
  ACCEL_INSTTOP_LINEAR_PLUECKER = 32,
  ACCEL_INSTTOP_LINEAR_MOELLER = 33,
  // inst_subdiv_bounds=linear: the subdivision instance accel (kinds 24 / 25) of a top scene with at least one moving subdivision instance.
  // The top-level tree is made of QNodeMB8s in the second section of `nodes`, behind the instanced scenes' QNode8 trees (see InstanceRecord)
  ACCEL_INSTSUBDIV_TOP_LINEAR_GRID = 34,
  ACCEL_INSTSUBDIV_TOP_LINEAR_CBVH_LEAF = 35,
  // flat linear curves (Scene::lineAccel, line_accel=default / bvh8.line4i / bvh4.line4i): LineRecord[] in `blobs`, one leaf arithmetic;
  // robust traversal for RTC_SCENE_FLAG_ROBUST scenes, fast traversal otherwise.
  ACCEL_LINE_ROBUST = 36,
  ACCEL_LINE_FAST = 37,
  // flat linear curves with time steps (Scene::lineMBAccel, line_accel_mb=default / bvh8.line4imb / bvh4.line4imb): LineMBRecord[] in
  // `blobs`, the static line leaf's arithmetic on the interpolated end points; robust / fast traversal as for the kinds 36 / 37.  Lane kernel only.
  ACCEL_LINEMB_ROBUST = 38,
  ACCEL_LINEMB_FAST = 39,
  // the same under mb_bounds=linear: QNodeMB8[] in `nodes`, 144-byte stride, as the kinds 26..29
  ACCEL_LINEMB_LINEAR_ROBUST = 40,
  ACCEL_LINEMB_LINEAR_FAST = 41,
  // flat Bezier and B-spline curves (Scene::curveAccel, hair_accel=default / bvh4.bezier1v / ...): CurveRecord[] in `blobs`, one leaf
  // arithmetic (the ribbon intersector); robust traversal for RTC_SCENE_FLAG_ROBUST scenes, fast traversal otherwise.  Lane
  // kernel only (lane and octet form), no pool form and no service kernel.
  ACCEL_CURVE_ROBUST = 42,
  ACCEL_CURVE_FAST = 43,
  // flat Bezier and B-spline curves with time steps (Scene::curveMBAccel, hair_accel_mb=default / bvh4.bezier1imb / bvh8.bezier1imb):
  // CurveMBRecord[] in `blobs`, the static curve leaf's arithmetic on the interpolated control points; robust / fast traversal as for the
  // kinds 42 / 43.  Lane kernel only, no service kernel.
  ACCEL_CURVEMB_ROBUST = 44,
  ACCEL_CURVEMB_FAST = 45,
  // the same under mb_bounds=linear: QNodeMB8[] in `nodes`, 144-byte stride, as the kinds 26..29
  ACCEL_CURVEMB_LINEAR_ROBUST = 46,
  ACCEL_CURVEMB_LINEAR_FAST = 47,
  NUM_ACCEL_KINDS // a new kind goes above this line and gets a row in accel_kinds.h
};
// (what the host code asks of a kind - launcher, node test, node array, instance level, kernel forms - is one table: accel_kinds.h)

// What a kernel launch needs to know about one committed scene.
struct AccelDesc
{
  const QNode8* nodes;         // QNodeMB8[] in the kinds ACCEL_*MB_LINEAR_*; QNode8[] | padding | QNodeMB8[] in the kinds ACCEL_INSTMESHMB_LINEAR_* / ACCEL_INSTTOP_LINEAR_* / ACCEL_INSTSUBDIV_TOP_LINEAR_*
  const TriRecord* prims;
  const uint8_t* blobs;        // subdivision blobs, or the QuadRecord[] of a quad accel, or the LineRecord[] of a line accel, or the CurveRecord[] of a curve accel, or the TriMBRecord[] / QuadMBRecord[] / LineMBRecord[] / CurveMBRecord[] of a motion-blur accel, or InstanceRecord[] (+ QuadRecord[] ...)
  const uint32_t* blobOffsets; // blob index -> byte offset / 16
  uint32_t root;               // REF_EMPTY for an empty scene
  uint32_t kind;               // AccelKind
  uint32_t robust;             // 1: robust node test (TravRay<...,true>), 0: fast test
  uint32_t blobStride;          // bytes per leaf blob (GridCell: 160; cBVH: header + nodes + leaves/grid)
};

// What one wavefront of an instrumented kernel reports (plain stores into its own slot: atomics on shared words
// serialise in L2 at ~70 ns each and slow the very batch they are meant to describe).
struct WaveRecord
{
  unsigned long long start, end;               // s_memrealtime ticks (100 MHz)
  unsigned long long iterations, leafPhases, laneIters;
  unsigned long long cyclesFetch, cyclesNode, cyclesLeaf, cyclesPop, cyclesTotal;
  unsigned long long rays, nodes, leaves, prims, inner, hits, spills;
  unsigned long long lastGrab, maxRaySteps;
  unsigned long long valid;
};
static const uint32_t WAVE_LOG_CAPACITY = 16384; // wave records per launch (one slice per accel slot of a scene: SCENE_SLOTS, rt_objects.h)

// Work counters of the instrumented kernels (mirrors RTCAMDTraceCounters).
struct TraceCounters
{
  unsigned long long rays, nodeVisits, leafVisits, primTests, innerVisits, hits, stackSpills, reserved;
  unsigned long long cyclesFetch, cyclesNode, cyclesLeaf, cyclesPop, cyclesTotal, iterations, leafPhases, waves;
  unsigned long long activeLaneIters, startInv;
  unsigned long long maxRaySteps, drainTicksSum, drainTicksMax;
  unsigned long long waveEndHist[64], waveIterHist[64];
};

} // namespace rtamd
