// The two instance accels of a scene, built at commit from the committed accels of the instanced scenes (layouts: accel.h InstanceRecord).
// build_instance_accel places the instances of mesh scenes (kinds 14..23, 30..33), build_instance_subdiv_accel those of subdivision
// scenes (kinds 24, 25, 34, 35).  Each is: classify (which instances take part, which arithmetic, every refusal that depends on what the scenes
// hold), then lay out (where things go), and the layouts are put together from one set of stages:
//   instance_world_box        the box of one instance in the top scene
//   distinct_scenes           the instanced scenes in order of first use: each is stored once, however many instances share it
//   build_top_level           the BVH8 over the instances' boxes, one instance per leaf
//   build_top_level_linear    the same over time-dependent boxes (inst_bounds=linear, inst_subdiv_bounds=linear; instance_time_boxes,
//                             instance_linear_bounds)
//   Section, add_section      where the sections of a byte array start (`blobs`, and the node buffer of the kinds 30 / 31)
//   place_leaf_records        one scene's leaf records into their section
//   append_tree               one scene's tree behind the nodes placed so far, references rebased
//   write_instance_records    the InstanceRecords and InstanceSteps
#include <algorithm>
#include <map>

#include "bvh8_builder.h"
#include "rt_objects.h"

namespace rtamd {
namespace {

// First InstanceStep a record may name, in 64-byte units from the start of `blobs`, exclusive: 24 bits beside the segment count.
const size_t INSTANCE_FIRST_STEP_LIMIT = (size_t)1 << 24;
// First record a leaf reference may name, exclusive (make_tri_leaf: the count sits above).
const size_t LEAF_RECORD_LIMIT = (size_t)1 << TRI_START_BITS;

// The class of an instanced scene: a subdivision scene as soon as it enables a subdivision mesh (build_instance_subdiv_accel refuses
// anything beside it), a mesh scene otherwise.
bool is_subdivision_scene(const Scene* o)
{
  for (const Geometry* og : o->geometries)
    if (og && og->enabled && og->type == RTC_GEOMETRY_TYPE_SUBDIVISION) return true;
  return false;
}

// An instance that takes part in an accel: classification found its scene placeable and not empty.
struct PlacedInstance
{
  const Geometry* geom;
  unsigned geomID;
  Scene* scene; // the instanced one
  Box3 box;     // in the top scene
};

// The world box of an instance: xfmBounds of the instanced scene's bounds, its eight transformed corners (instance_intersector.cpp:24-39,
// affinespace.h:114-126).  The instanced scene was committed before and its `bounds` cover all its accels (build_mesh_bvh8 extends them
// per accel, build_mb_bvh8 by the swept boxes of moving meshes).  A moving instance gets the union over its steps: the instanced scene
// is static in its own space and the lerp of two affine maps sends a point to the lerp of its images, so the union of the steps' boxes
// holds the object at every time - one box swept over the whole shutter, like the motion-blur mesh accels.
Box3 instance_world_box(const Geometry* g, const Scene* o)
{
  Box3 box;
  const V3 c[2] = {o->bounds.lo, o->bounds.hi};
  for (const Geometry::Xfm& step : g->local2world) // one step: xfmBounds; more: the union over the steps
    for (int i = 0; i < 8; i++) box.extend(xfm_point(step.data(), V3(c[i >> 2].x, c[(i >> 1) & 1].y, c[i & 1].z)));
  if (!(std::isfinite(box.lo.x) && std::isfinite(box.lo.y) && std::isfinite(box.lo.z) && std::isfinite(box.hi.x) && std::isfinite(box.hi.y) && std::isfinite(box.hi.z)))
    RT_THROW(RTC_ERROR_INVALID_OPERATION, "instance transform yields bounds that are not finite");
  return box;
}

// inst_bounds=linear: the box of an instance at each of its time steps and at mid-shutter, in double (a static instance: none, its
// `box` serves at every time).  Step k is at the global time k / S, S = steps - 1.
struct InstanceTimeBoxes
{
  struct BoxD
  {
    double lo[3], hi[3];
    BoxD() { for (int a = 0; a < 3; a++) { lo[a] = std::numeric_limits<double>::infinity(); hi[a] = -lo[a]; } }
    void extend(const double* p) { for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); } }
  };
  std::vector<BoxD> steps;
  Box3 mid; // topology only: rounded to fp32 as it comes
};

// the eight corners of `b` through the affine map m (columns vx, vy, vz, p), in double
void extend_by_image(InstanceTimeBoxes::BoxD& box, const double* m, const Box3& b)
{
  const V3 c[2] = {b.lo, b.hi};
  for (int i = 0; i < 8; i++) {
    const double q[3] = {(double)c[i >> 2].x, (double)c[(i >> 1) & 1].y, (double)c[i & 1].z};
    double r[3];
    for (int k = 0; k < 3; k++) r[k] = q[0] * m[k] + q[1] * m[3 + k] + q[2] * m[6 + k] + m[9 + k];
    box.extend(r);
  }
}

InstanceTimeBoxes instance_time_boxes(const Geometry* g, const Scene* o)
{
  InstanceTimeBoxes tb;
  const size_t n = g->local2world.size();
  if (n < 2) return tb;
  double m[12];
  for (const Geometry::Xfm& step : g->local2world) {
    for (int k = 0; k < 12; k++) m[k] = (double)step[k];
    tb.steps.emplace_back();
    extend_by_image(tb.steps.back(), m, o->bounds);
  }
  // mid-shutter: lerp(step[k], step[k + 1], f) at time 0.5
  const double ts = 0.5 * (double)(n - 1);
  const size_t k = std::min((size_t)ts, n - 2);
  const double f = ts - (double)k;
  for (int j = 0; j < 12; j++) m[j] = (1.0 - f) * (double)g->local2world[k][j] + f * (double)g->local2world[k + 1][j];
  InstanceTimeBoxes::BoxD mid;
  extend_by_image(mid, m, o->bounds);
  for (int a = 0; a < 3; a++) { tb.mid.lo[a] = (float)mid.lo[a]; tb.mid.hi[a] = (float)mid.hi[a]; }
  return tb;
}

// The distinct instanced scenes in order of first use, and which of them each placed instance names.
struct DistinctScenes
{
  std::vector<Scene*> scenes;
  std::vector<uint32_t> of; // placed instance -> index into `scenes`
};

DistinctScenes distinct_scenes(const std::vector<PlacedInstance>& placed)
{
  DistinctScenes d;
  std::map<Scene*, uint32_t> index;
  for (const PlacedInstance& p : placed) {
    auto it = index.emplace(p.scene, (uint32_t)d.scenes.size());
    if (it.second) d.scenes.push_back(p.scene);
    d.of.push_back(it.first->second);
  }
  return d;
}

// InstanceSteps the placed instances need: one per time step of every moving instance.
size_t count_steps(const std::vector<PlacedInstance>& placed)
{
  size_t n = 0;
  for (const PlacedInstance& p : placed)
    if (p.geom->local2world.size() > 1) n += p.geom->local2world.size();
  return n;
}

// The top-level tree, ONE instance per leaf: leaf reference = make_tri_leaf(record index, 1), the records in leaf order.  Starts the accel
// with it (nodes, root, leaf count, and its depth as maxDepth), extends the top scene's bounds by the instances' boxes and returns the
// leaf order: record index -> placed instance.
std::vector<uint32_t> build_top_level(Scene* s, const std::vector<PlacedInstance>& placed, Accel& A)
{
  if (placed.size() >= LEAF_RECORD_LIMIT) RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instances for the 26-bit leaf reference");
  std::vector<uint32_t> order;
  std::vector<BuildPrim> bp(placed.size());
  for (size_t i = 0; i < placed.size(); i++) {
    bp[i].box = placed[i].box;
    bp[i].id = (uint32_t)i;
  }
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
  A.maxDepth = r.maxDepth;
  A.leafCount = r.leafCount;
  return order;
}

// inst_bounds=linear: the end boxes B(0), B(1) of one child of a top-level node over the instances prims[begin, end), whose linear
// interpolation holds every instance below the child at every time in [0, 1].  The construction is linear_bounds' of rt_scene.cpp (the
// reference's linearBounds): the first guess is the union of the instances' boxes at their first step and the union of their boxes at
// their last step; both ends are then widened, per plane, by the largest amount by which any instance's box at any of its step times
// k / S sticks out of the interpolated guess.  A static instance contributes its one box at both ends and never sticks out.
// Why the result holds a moving instance BETWEEN its steps too:
//  1. Between two steps the instance's transform is lerp(step[k], step[k + 1], f), and the lerp of two affine maps sends a point to the
//     lerp of its images: every corner of the instanced scene's bounds (hence, the maps being affine, everything inside them) moves on
//     a straight line from its place at step k to its place at step k + 1.
//  2. Each plane of the instance's true box at time t is therefore bounded by the piecewise-linear interpolant of the planes of its
//     step boxes (a max / min of linear functions lies below / above the chord of its end values).
//  3. A plane that is linear in t and lies outside every step box at that step's time lies outside that interpolant on every piece,
//     both being linear there - and after the widening the planes of lerp(B(0), B(1), t) are such planes.
// Computed in double and rounded outward to fp32; what double loses, and the fp32 arithmetic of the kernel's decode and of its
// interpolated transform, is covered by the one-grid-step padding of quantize_node_mb as argued in accel.h (QNodeMB8, InstanceRecord).
void instance_linear_bounds(const std::vector<PlacedInstance>& placed, const std::vector<InstanceTimeBoxes>& time, const BuildPrim* prims, size_t begin, size_t end, Box3& b0, Box3& b1)
{
  typedef InstanceTimeBoxes::BoxD BoxD;
  auto static_box = [&](size_t id) {
    BoxD b;
    for (int a = 0; a < 3; a++) { b.lo[a] = (double)placed[id].box.lo[a]; b.hi[a] = (double)placed[id].box.hi[a]; }
    return b;
  };
  BoxD g0, g1; // the guess
  for (size_t i = begin; i < end; i++) {
    const std::vector<BoxD>& st = time[prims[i].id].steps;
    const BoxD first = st.empty() ? static_box(prims[i].id) : st.front(), last = st.empty() ? first : st.back();
    g0.extend(first.lo); g0.extend(first.hi);
    g1.extend(last.lo); g1.extend(last.hi);
  }
  for (int a = 0; a < 3; a++) {
    double dlo = 0.0, dhi = 0.0; // how far any step box sticks out of the interpolated guess
    for (size_t i = begin; i < end; i++) {
      const std::vector<BoxD>& st = time[prims[i].id].steps;
      for (size_t k = 0; k < st.size(); k++) {
        const double t = (double)k / (double)(st.size() - 1);
        dlo = std::max(dlo, ((1.0 - t) * g0.lo[a] + t * g1.lo[a]) - st[k].lo[a]);
        dhi = std::max(dhi, st[k].hi[a] - ((1.0 - t) * g0.hi[a] + t * g1.hi[a]));
      }
    }
    // (the interpolated guess is itself rounded: one more ulp of double on each side, far inside the quantizer's padding)
    auto down = [](double x) { float f = (float)x; return (double)f > x ? nextafterf(f, -std::numeric_limits<float>::infinity()) : f; };
    auto up = [](double x) { float f = (float)x; return (double)f < x ? nextafterf(f, std::numeric_limits<float>::infinity()) : f; };
    b0.lo[a] = down(g0.lo[a] - dlo); b1.lo[a] = down(g1.lo[a] - dlo);
    b0.hi[a] = up(g0.hi[a] + dhi); b1.hi[a] = up(g1.hi[a] + dhi);
  }
}

// The top-level tree under inst_bounds=linear: QNodeMB8s, one instance per leaf as in build_top_level.  The topology is the midpoint SAH
// build over every instance's box at mid-shutter (a static instance: its box); the boxes stored are instance_linear_bounds'.  Returns the
// nodes with references that count from the tree's own first node - the layout rebases them - and fills A.root likewise, A.maxDepth
// and A.leafCount.  A single instance makes a tree that is one leaf: it gets a root node of one child, so that a ray is tested against
// the instance's box at its time before it pays for the entry (depth 1).
std::vector<QNodeMB8> build_top_level_linear(Scene* s, const std::vector<PlacedInstance>& placed, Accel& A, std::vector<uint32_t>& order)
{
  if (placed.size() >= LEAF_RECORD_LIMIT) RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instances for the 26-bit leaf reference");
  std::vector<InstanceTimeBoxes> time(placed.size());
  std::vector<BuildPrim> bp(placed.size());
  for (size_t i = 0; i < placed.size(); i++) {
    time[i] = instance_time_boxes(placed[i].geom, placed[i].scene);
    bp[i].box = time[i].steps.empty() ? placed[i].box : time[i].mid;
    bp[i].id = (uint32_t)i;
    s->bounds.extend(placed[i].box); // the swept union, as in build_top_level
  }
  auto makeLeaf = [&](const BuildPrim* prims, size_t begin, size_t end) -> uint32_t {
    if (end - begin != 1) RT_THROW(RTC_ERROR_UNKNOWN, "instance builder: a leaf must hold one instance");
    order.push_back(prims[begin].id);
    return make_tri_leaf((uint32_t)order.size() - 1u, 1u);
  };
  auto bounds = [&](const BuildPrim* prims, size_t begin, size_t end, Box3& b0, Box3& b1) { instance_linear_bounds(placed, time, prims, begin, end, b0, b1); };
  BuildSettings cfg;
  cfg.blockSize = 1; cfg.minLeaf = 1; cfg.maxLeaf = 1;
  cfg.threads = 1; // the leaf callback appends in leaf order
  BuildResultMB r = build_bvh8_mb(bp, cfg, makeLeaf, bounds);
  if (r.root & REF_LEAF) {
    Box3 b0, b1;
    bounds(bp.data(), 0, 1, b0, b1);
    QNodeMB8 q;
    quantize_node_mb(&b0, &b1, &r.root, 1, q);
    r.nodes.assign(1, q);
    r.root = 0u;
    r.maxDepth = 1u;
  }
  A.root = r.root;
  A.maxDepth = r.maxDepth;
  A.leafCount = r.leafCount;
  return std::move(r.nodes);
}

// Where the sections of one byte array start.  A section holds records of `recordBytes` each and starts at the next multiple of its own
// record size behind the section before it (an empty section still moves the end there), so that whoever reads the array as ONE array
// of that record type finds the section's first record at index base().  Everything that needs an offset reads it from here.
struct Section
{
  size_t offset, recordBytes; // offset in bytes
  size_t used = 0;            // records placed so far (place_leaf_records)
  size_t base() const { return offset / recordBytes; }
};

// appends a section of `count` records to an array of `bytes` bytes so far
Section add_section(size_t& bytes, size_t count, size_t recordBytes)
{
  Section sec{(bytes + recordBytes - 1) / recordBytes * recordBytes, recordBytes};
  bytes = sec.offset + count * recordBytes;
  return sec;
}

// Copies the leaf records of O to the next free place of their section of `blobs` and returns the index of the first one, in units of
// the record size from the start of `blobs`: what the leaf references of O's tree move by (append_tree).  The rebased first record of
// every leaf must stay in bits 0..25.
size_t place_leaf_records(std::vector<uint8_t>& blobs, Section& sec, const Accel& O, const char* tooMany)
{
  if (!O.traceable()) return 0; // nothing to place (append_tree: no tree either)
  const size_t n = O.blobs.size() / sec.recordBytes, base = sec.base() + sec.used;
  if (base + n >= LEAF_RECORD_LIMIT) RT_THROW(RTC_ERROR_INVALID_OPERATION, tooMany);
  if (n) memcpy(blobs.data() + sec.offset + sec.used * sec.recordBytes, O.blobs.data(), n * sec.recordBytes);
  sec.used += n;
  return base;
}

// Copies the tree of O (its nodes of type Node) behind `dst`; child references move by indexBase + the nodes already there (indexBase:
// where `dst` starts in the uploaded node buffer, in nodes of this type), leaf references by leafBase.  Returns the rebased root,
// REF_EMPTY for an accel with nothing to trace, and keeps `deepest`, the depth of the deepest tree placed.
template <class Node>
uint32_t append_tree(std::vector<Node>& dst, size_t indexBase, const Accel& O, const std::vector<Node>& nodes, size_t leafBase, const char* tooMany, uint32_t& deepest)
{
  if (!O.traceable()) return REF_EMPTY;
  const size_t nodeBase = indexBase + dst.size();
  if (nodeBase + nodes.size() >= (size_t)REF_LEAF) RT_THROW(RTC_ERROR_INVALID_OPERATION, tooMany);
  auto rebase = [&](uint32_t ref) -> uint32_t {
    if (ref == REF_EMPTY) return ref;
    if (ref & REF_LEAF) return ref + (uint32_t)leafBase;
    return ref + (uint32_t)nodeBase;
  };
  for (Node n : nodes) {
    for (uint32_t& c : n.child) c = rebase(c);
    dst.push_back(n);
  }
  deepest = std::max(deepest, O.maxDepth);
  return rebase(O.root);
}
const char* const TOO_MANY_NODES = "too many instanced nodes for the 31-bit node reference";

// The InstanceRecords, at the start of `blobs` in the top-level tree's leaf order, and the InstanceSteps of the moving instances, in
// record order from index firstStep (64-byte units) on.  rootOf / pad0Of hold one word per distinct scene: what its instances' records
// carry in `root` and, where given, in pad[0].  world2local is the inverse of step 0 (all zero for a singular transform: never hit);
// a moving instance has pad[1] = (segments << 24) | index of its first step.
void write_instance_records(const std::vector<PlacedInstance>& placed, const DistinctScenes& ds, const std::vector<uint32_t>& order,
                            const std::vector<uint32_t>& rootOf, const std::vector<uint32_t>* pad0Of, size_t firstStep, const char* tooManySteps, std::vector<uint8_t>& blobs)
{
  for (size_t i = 0; i < order.size(); i++) {
    const Geometry* g = placed[order[i]].geom;
    InstanceRecord rec;
    memset(&rec, 0, sizeof(rec));
    if (!invert_affine(g->local2world[0].data(), rec.world2local)) memset(rec.world2local, 0, sizeof(rec.world2local)); // singular: never hit
    rec.geomID = placed[order[i]].geomID;
    rec.root = rootOf[ds.of[order[i]]];
    if (pad0Of) rec.pad[0] = (*pad0Of)[ds.of[order[i]]];
    if (g->local2world.size() > 1) {
      if (firstStep >= INSTANCE_FIRST_STEP_LIMIT) RT_THROW(RTC_ERROR_INVALID_OPERATION, tooManySteps);
      rec.pad[1] = ((uint32_t)(g->local2world.size() - 1) << 24) | (uint32_t)firstStep;
      for (const Geometry::Xfm& x : g->local2world) {
        InstanceStep st;
        memset(&st, 0, sizeof(st));
        memcpy(st.local2world, x.data(), sizeof(st.local2world));
        memcpy(blobs.data() + firstStep++ * sizeof(InstanceStep), &st, sizeof(st));
      }
    }
    memcpy(blobs.data() + i * sizeof(InstanceRecord), &rec, sizeof(rec));
  }
}

// ---- instances of mesh scenes ----------------------------------------------------------------------------------------------------------

// What build_instance_accel places and how, decided from the device's config and from what the instanced scenes hold.
struct MeshInstances
{
  std::vector<PlacedInstance> placed; // in geomID order
  bool pluecker = false;      // the ONE arithmetic of every accel below this scene
  bool anyQuads = false;      // an instanced scene has a traceable quad accel
  bool anyMotion = false;     // an instance has more than one time step
  bool anyMeshMotion = false; // an instanced scene has a traceable motion-blur accel
  bool anyLinear = false;     // ... built under mb_bounds=linear (kinds 26..29): its nodes are QNodeMB8s
  bool anyHair = false;       // inst_hair=1: an instanced scene has a traceable curve or line accel (the kinds ACCEL_INSTMESHMB_* with Accel::instHair)
  bool anyHairMB = false;     // inst_hair_mb=1: ... a traceable motion-blur curve or line accel (implies anyHair; Accel::instHair == 2)
  bool topLinear = false;     // inst_bounds=linear and anyMotion: the top-level tree is made of QNodeMB8s (kinds ACCEL_INSTTOP_LINEAR_*)
  uint32_t pendingMax = 0;    // most trees of one instanced scene, minus one
  bool intersectFilter = false, occludedFilter = false; // inst_filters=1: an enabled geometry of a placed instance's scene has such a filter
};

// Instances are examined in geomID order.  The instanced scenes were committed before; what this commit sees of them is their committed
// accels.  A host-only device takes quads in an instanced scene only when its config names inst_accel= (Device::inst_quads_enabled), as
// it takes quad meshes at all only with quad_accel=; instances with time steps under the same rule (Device::inst_motion_enabled);
// motion-blur meshes below an instance only when it names inst_accel= and one of tri_accel_mb= / quad_accel_mb=
// (Device::inst_mesh_motion_enabled).
// Linear node bounds below an instance (inst_mb_bounds=linear, Device::inst_mb_bounds; on a host-only device only where motion-blur
// meshes below an instance are taken at all): an instanced scene whose motion-blur accels were built under mb_bounds=linear is placed
// only then; without the key it is refused as before.  One device has one mb_bounds and an instance cannot name a scene of another
// device (Geometry::setInstancedScene), so the motion-blur trees below one top scene are all of one node type.
// Time-dependent top-level boxes (inst_bounds=linear, Device::inst_top_linear_enabled): a top scene with a moving instance among those
// placed here gets the kinds ACCEL_INSTTOP_LINEAR_*; one without keeps its kind and bytes.  Moving meshes below the instances of such a
// top scene must come as QNodeMB8 trees (mb_bounds=linear,inst_mb_bounds=linear), so that one node type serves every motion-blur tree
// of the kernel's TOPMB form; otherwise the commit is refused with a message that names the three keys.
// Line segments and flat curves below an instance (inst_hair=1, Device::inst_hair_lines_enabled / inst_hair_curves_enabled): an instanced
// scene may enable such geometries with one time step, alone or beside its meshes; its curve and line accels join the agreement in
// arithmetic (their robust / fast traversal).  A top scene with any such tree below it is of the kinds ACCEL_INSTMESHMB_*, over swept
// boxes only: beside a linear kind, and beside geometry filters below the instances (the hair form of the kernel has no exclusion scan),
// the commit is refused.  Without the key every refusal is what it was.
// The same with time steps (inst_hair_mb=1 beside inst_hair=1, Device::inst_hair_mb_lines_enabled / inst_hair_mb_curves_enabled): the
// scene's motion-blur curve and line accels are two further trees under the same rules, swept boxes only - built under mb_bounds=linear
// they hold QNodeMB8s and the commit is refused.  Without that key moving hair below an instance is refused as before.
// Subdivision scenes below an instance: an instanced scene that enables a subdivision mesh is left to build_instance_subdiv_accel when
// the device takes such scenes (Device::inst_subdiv_enabled); otherwise it is refused here with the message of the config, as before.
MeshInstances classify_mesh_instances(const Scene* s)
{
  MeshInstances c;
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
  const bool linearOk = meshMotionOk && s->device->inst_mb_bounds == "linear";
  // inst_filters=1: the meshes of an instanced scene may carry filter functions; what THIS commit sees of them is recorded below, for the
  // scenes of the instances that are placed (as Scene::commit records triIntersectFilter / triOccludedFilter of its own meshes)
  const bool filtersOk = s->device->inst_filters;
  const bool hairLinesOk = s->device->inst_hair_lines_enabled(), hairCurvesOk = s->device->inst_hair_curves_enabled();
  const bool hairLinesMBOk = s->device->inst_hair_mb_lines_enabled(), hairCurvesMBOk = s->device->inst_hair_mb_curves_enabled(); // inst_hair_mb=1
  auto at_instance = [](const char* text, unsigned gid) { return std::string(text) + " (instance " + std::to_string(gid) + ")"; };
  unsigned hairGeom = 0, filterGeom = 0; // the first instance whose scene holds hair / a geometry filter: named by the refusals behind the loop
  unsigned hairLinearGeom = 0;           // ... holds a moving-hair tree of QNodeMB8s
  bool anyFilter = false, anyHairLinear = false;
  // inst_bounds=linear: will this top scene get the time-dependent top level?  Known before the scenes are examined, so that the refusal of
  // moving meshes below it has its own text from the first instance on (a moving instance of an empty scene is not placed and does not count)
  bool wantTopLinear = false;
  if (s->device->inst_top_linear_enabled())
    for (const Geometry* g : s->geometries)
      if (g && g->enabled && g->type == RTC_GEOMETRY_TYPE_INSTANCE && g->local2world.size() > 1 && g->instScene && !(subdivOk && is_subdivision_scene(g->instScene))) {
        const Scene* o = g->instScene;
        wantTopLinear |= o->triAccel.traceable() || o->quadAccel.traceable() || o->triMBAccel.traceable() || o->quadMBAccel.traceable();
      }
  const char* const topLinearNeedsLinear = "inst_bounds=linear: a scene with moving instances takes instanced scenes with motion blur meshes only when their accels hold "
                                           "time-dependent nodes (use mb_bounds=linear,inst_mb_bounds=linear beside inst_bounds=linear, or inst_bounds=swept)";
  bool haveKind = false, anySwept = false; // anySwept: a traceable motion-blur accel of the kinds 10..13 below this scene
  unsigned kindGeom = 0; // the instance whose scene fixed the arithmetic, and the accels that scene has: for the refusal below
  std::string kindNames;
  for (unsigned gid = 0; gid < s->geometries.size(); gid++) {
    Geometry* g = s->geometries[gid];
    if (!g || !g->enabled || g->type != RTC_GEOMETRY_TYPE_INSTANCE) continue;
    if (g->timeSteps != 1 && !s->device->inst_motion_enabled()) RT_THROW(RTC_ERROR_INVALID_OPERATION, "instances with more than one time step are not supported");
    Scene* o = g->instScene;
    if (!o) RT_THROW(RTC_ERROR_INVALID_OPERATION, "instance without an instanced scene");
    if (o->modified) RT_THROW(RTC_ERROR_INVALID_OPERATION, "instanced scene got not committed");
    // round_curves=1: the tube leaf runs at the top level only, whatever the inst_* keys take (asked before a subdivision scene is passed on)
    for (const Geometry* og : o->geometries)
      if (og && og->enabled && og->isRoundCurve())
        RT_THROW(RTC_ERROR_INVALID_OPERATION, at_instance("round Bezier and B-spline curves inside an instanced scene are not supported", gid));
    if (subdivOk && is_subdivision_scene(o)) continue; // build_instance_subdiv_accel places it
    // without inst_mb_bounds=linear the instanced scenes' trees are copied behind the top-level tree as QNode8s: time-dependent nodes
    // have no place there
    if (!linearOk && wantTopLinear && (o->triMBAccel.nodesAreMB() || o->quadMBAccel.nodesAreMB()))
      RT_THROW(RTC_ERROR_INVALID_OPERATION, topLinearNeedsLinear);
    if (!linearOk && (o->triMBAccel.nodesAreMB() || o->quadMBAccel.nodesAreMB()))
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "an instanced scene with a motion blur accel built under mb_bounds=linear is not supported (instance accels hold swept node boxes: use mb_bounds=swept)");
    for (Geometry* og : o->geometries) {
      if (!og || !og->enabled) continue;
      if (og->isFlatCubicCurve() ? hairCurvesOk : (og->type == RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE && hairLinesOk)) { // inst_hair=1
        if (og->timeSteps != 1 && !(og->isFlatCubicCurve() ? hairCurvesMBOk : hairLinesMBOk))
          RT_THROW(RTC_ERROR_INVALID_OPERATION, at_instance("motion blur of line segments and flat curves inside an instanced scene is not supported", gid));
        if (!filtersOk && (og->intersectFilter || og->occludedFilter)) RT_THROW(RTC_ERROR_INVALID_OPERATION, "geometry filter functions inside an instanced scene are not supported");
        continue;
      }
      if (og->isFlatCubicCurve()) RT_THROW(RTC_ERROR_INVALID_OPERATION, "flat Bezier and B-spline curves inside an instanced scene are not supported");
      const bool mesh = og->type == RTC_GEOMETRY_TYPE_TRIANGLE || (quadsOk && og->type == RTC_GEOMETRY_TYPE_QUAD);
      if (!mesh || (og->timeSteps != 1 && !meshMotionOk)) RT_THROW(RTC_ERROR_INVALID_OPERATION, only);
      if (!filtersOk && (og->intersectFilter || og->occludedFilter)) RT_THROW(RTC_ERROR_INVALID_OPERATION, "geometry filter functions inside an instanced scene are not supported");
    }
    for (const Accel* oa : o->accels())
      if (oa != &o->triAccel && !(quadsOk && oa == &o->quadAccel) && !(meshMotionOk && (oa == &o->triMBAccel || oa == &o->quadMBAccel)) &&
          !(hairCurvesOk && oa == &o->curveAccel) && !(hairLinesOk && oa == &o->lineAccel) && !(hairCurvesMBOk && oa == &o->curveMBAccel) &&
          !(hairLinesMBOk && oa == &o->lineMBAccel) && oa->kind != ACCEL_NONE)
        RT_THROW(RTC_ERROR_INVALID_OPERATION, only);
    if (!filtersOk && (o->triIntersectFilter || o->triOccludedFilter)) RT_THROW(RTC_ERROR_INVALID_OPERATION, "geometry filter functions inside an instanced scene are not supported");
    const bool tris = o->triAccel.traceable(), quads = o->quadAccel.traceable();
    const bool trisMB = o->triMBAccel.traceable(), quadsMB = o->quadMBAccel.traceable();
    const bool curves = hairCurvesOk && o->curveAccel.traceable(), lines = hairLinesOk && o->lineAccel.traceable();
    const bool curvesMB = hairCurvesMBOk && o->curveMBAccel.traceable(), linesMB = hairLinesMBOk && o->lineMBAccel.traceable();
    if (!tris && !quads && !trisMB && !quadsMB && !curves && !lines && !curvesMB && !linesMB) continue; // empty scene: nothing to hit
    std::string names; // this scene's traceable accels
    for (const char* nm : {tris ? "triangle" : "", trisMB ? "motion blur triangle" : "", quads ? "quad" : "", quadsMB ? "motion blur quad" : "", curves ? "curve" : "",
                           curvesMB ? "motion blur curve" : "", lines ? "line" : "", linesMB ? "motion blur line" : ""})
      if (*nm) names += std::string(names.empty() ? "" : ", ") + nm;
    // scenes that disagree while a motion-blur accel is involved: the message names the accels on either side
    auto disagree = [&](bool thisPl) {
      const char* const ar[2] = {"Moeller / fast", "Pluecker / robust"};
      return "the instanced scenes of one scene disagree in accel kind (Pluecker / robust and Moeller / fast): the scene of instance " + std::to_string(gid) + " has " +
             ar[thisPl] + " accels (" + names + "), the scene of instance " + std::to_string(kindGeom) + " " + ar[!thisPl] + " ones (" + kindNames + "): instances need one arithmetic";
    };
    if (trisMB || quadsMB || curves || lines || curvesMB || linesMB) {
      // one arithmetic per top scene, over all eight trees of every instanced scene
      struct { bool have, pl; const char* name; } const t[8] = {{tris, o->triAccel.kind == ACCEL_TRI_PLUECKER, "triangle"},
                                                                {trisMB, kind_row(o->triMBAccel.kind).robust, "motion blur triangle"},
                                                                {quads, o->quadAccel.kind == ACCEL_QUAD_PLUECKER, "quad"},
                                                                {quadsMB, kind_row(o->quadMBAccel.kind).robust, "motion blur quad"},
                                                                {curves, kind_row(o->curveAccel.kind).robust, "curve"},
                                                                {curvesMB, kind_row(o->curveMBAccel.kind).robust, "motion blur curve"},
                                                                {lines, kind_row(o->lineAccel.kind).robust, "line"},
                                                                {linesMB, kind_row(o->lineMBAccel.kind).robust, "motion blur line"}};
      std::string pl, mo;
      for (const auto& e : t)
        if (e.have) (e.pl ? pl : mo) += std::string((e.pl ? pl : mo).empty() ? "" : ", ") + e.name;
      if (!pl.empty() && !mo.empty())
        RT_THROW(RTC_ERROR_INVALID_OPERATION, "the accels of an instanced scene disagree in kind (Pluecker / robust: " + pl + "; Moeller / fast: " + mo + "): instances need one arithmetic");
      const bool scenePl = !pl.empty();
      if (haveKind && scenePl != c.pluecker) RT_THROW(RTC_ERROR_INVALID_OPERATION, disagree(scenePl));
      if (curves || lines || curvesMB || linesMB) {
        if (!c.anyHair) hairGeom = gid;
        c.anyHair = true;
      }
      if (curvesMB || linesMB) { // their nodes must be swept QNode8s: refused behind the loop otherwise
        c.anyHairMB = true;
        if (!anyHairLinear && ((curvesMB && o->curveMBAccel.nodesAreMB()) || (linesMB && o->lineMBAccel.nodesAreMB()))) {
          anyHairLinear = true;
          hairLinearGeom = gid;
        }
      }
      c.anyMeshMotion |= trisMB || quadsMB;
      for (const Accel* m : {trisMB ? &o->triMBAccel : nullptr, quadsMB ? &o->quadMBAccel : nullptr})
        if (m) (m->nodesAreMB() ? c.anyLinear : anySwept) = true;
    }
    c.pendingMax = std::max(c.pendingMax, (uint32_t)tris + (uint32_t)trisMB + (uint32_t)quads + (uint32_t)quadsMB + (uint32_t)curves + (uint32_t)lines + (uint32_t)curvesMB + (uint32_t)linesMB - 1u);
    // the kernel runs ONE arithmetic on both levels and in both leaves: every accel below this scene is Pluecker / robust, or every one
    // Moeller / fast
    if (tris && quads && (o->triAccel.kind == ACCEL_TRI_PLUECKER) != (o->quadAccel.kind == ACCEL_QUAD_PLUECKER))
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "the triangle and quad accels of an instanced scene disagree in kind (Pluecker / robust triangles beside Moeller / fast quads, "
                                            "as a robust scene under quad_accel=bvh8.quad4v builds them): instances need one arithmetic");
    const bool pl = tris ? o->triAccel.kind == ACCEL_TRI_PLUECKER
                  : quads ? o->quadAccel.kind == ACCEL_QUAD_PLUECKER
                  : kind_row(trisMB ? o->triMBAccel.kind : quadsMB ? o->quadMBAccel.kind : curves ? o->curveAccel.kind : curvesMB ? o->curveMBAccel.kind
                             : lines ? o->lineAccel.kind : o->lineMBAccel.kind).robust;
    if (haveKind && pl != c.pluecker) {
      if (!c.anyQuads && !quads && !c.anyMeshMotion && !c.anyHair) RT_THROW(RTC_ERROR_INVALID_OPERATION, "the instanced scenes of one scene disagree in triangle accel kind (robust and not robust)");
      if (c.anyMeshMotion || c.anyHair) RT_THROW(RTC_ERROR_INVALID_OPERATION, disagree(pl));
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "the instanced scenes of one scene disagree in accel kind (Pluecker / robust and Moeller / fast): instances need one arithmetic");
    }
    if (!haveKind) {
      kindGeom = gid;
      kindNames = names;
    }
    haveKind = true;
    c.pluecker = pl;
    c.anyQuads |= quads;
    c.anyMotion |= g->local2world.size() > 1;
    c.placed.push_back({g, gid, o, instance_world_box(g, o)});
    for (const Geometry* og : o->geometries) {
      if (!og || !og->enabled) continue;
      c.intersectFilter |= og->intersectFilter != nullptr;
      c.occludedFilter |= og->occludedFilter != nullptr;
      if ((og->intersectFilter || og->occludedFilter) && !anyFilter) {
        anyFilter = true;
        filterGeom = gid;
      }
    }
  }
  if (c.anyLinear && anySwept) RT_THROW(RTC_ERROR_UNKNOWN, "instance builder: motion blur accels of both node types below one scene");
  c.topLinear = c.anyMotion && s->device->inst_top_linear_enabled();
  if (c.topLinear && anySwept) RT_THROW(RTC_ERROR_INVALID_OPERATION, topLinearNeedsLinear);
  if (anyHairLinear)
    RT_THROW(RTC_ERROR_INVALID_OPERATION, at_instance("inst_hair_mb=1: motion blur line segments and flat curves below an instance are traced over swept boxes only; not under mb_bounds=linear", hairLinearGeom));
  if (c.anyHair && (c.topLinear || c.anyLinear))
    RT_THROW(RTC_ERROR_INVALID_OPERATION, at_instance("inst_hair=1: line segments and flat curves below an instance are traced over swept boxes only (kinds 22 / 23); not beside "
                                                      "inst_bounds=linear or inst_mb_bounds=linear trees", hairGeom));
  if (c.anyHair && anyFilter)
    RT_THROW(RTC_ERROR_INVALID_OPERATION, at_instance("inst_hair=1: geometry filter functions below the instances of a scene with instanced line segments or flat curves are not supported", filterGeom));
  return c;
}

// As long as no instanced scene has a traceable quad accel the result is the triangle-only accel (kinds ACCEL_INST_TRI_*: triangle
// trees behind the top-level tree, TriRecords, InstanceRecords, `pad` zero); otherwise it is the layout of accel.h InstanceRecord
// (kinds ACCEL_INST_PLUECKER / ACCEL_INST_MOELLER).  As soon as one enabled instance has more than one time step the kinds are
// ACCEL_INSTMB_* (chosen otherwise exactly as ACCEL_INST_*); as soon as one instanced scene has a traceable motion-blur accel they are
// ACCEL_INSTMESHMB_*, and ACCEL_INSTMESHMB_LINEAR_* as soon as one of those accels holds QNodeMB8s.  A top scene without a motion-blur
// accel below it keeps the kinds 14..21 and their arrays, whatever the config names.  A top scene with a curve or line tree below it
// (inst_hair=1) is of the kinds ACCEL_INSTMESHMB_* too, even when nothing below it moves.  Under inst_bounds=linear a top scene with a moving
// instance is of the kinds ACCEL_INSTTOP_LINEAR_*, whatever lies below its instances.
uint32_t instance_kind(const MeshInstances& c)
{
  if (c.topLinear) return c.pluecker ? ACCEL_INSTTOP_LINEAR_PLUECKER : ACCEL_INSTTOP_LINEAR_MOELLER;
  if (c.anyLinear) return c.pluecker ? ACCEL_INSTMESHMB_LINEAR_PLUECKER : ACCEL_INSTMESHMB_LINEAR_MOELLER;
  if (c.anyMeshMotion || c.anyHair) return c.pluecker ? ACCEL_INSTMESHMB_PLUECKER : ACCEL_INSTMESHMB_MOELLER;
  if (c.anyMotion) return c.anyQuads ? (c.pluecker ? ACCEL_INSTMB_PLUECKER : ACCEL_INSTMB_MOELLER) : (c.pluecker ? ACCEL_INSTMB_TRI_PLUECKER : ACCEL_INSTMB_TRI_MOELLER);
  if (c.anyQuads) return c.pluecker ? ACCEL_INST_PLUECKER : ACCEL_INST_MOELLER;
  return c.pluecker ? ACCEL_INST_TRI_PLUECKER : ACCEL_INST_TRI_MOELLER;
}

// The top-level tree, followed in the same arrays by the trees and records of every distinct instanced scene, rebased: per scene the
// triangle, motion-blur triangle, quad and motion-blur quad tree (Scene::commit's order), whichever it has.
//   blobs : InstanceRecords | QuadRecords | InstanceSteps, and with anyMeshMotion (the general layout of accel.h InstanceRecord):
//           | one InstanceSceneRecord per scene, which holds its four roots | TriMBRecords | QuadMBRecords
//           and with anyHair: | CurveRecords from a multiple of 80 bytes | LineRecords from a multiple of 48 bytes; the scene records then
//           hold six roots, REF_EMPTY for a missing hair tree too (without anyHair the two words stay zero, the bytes what they were)
//           and with anyHairMB: | CurveMBRecords from a multiple of 160 bytes | LineMBRecords from a multiple of 80 bytes; the scene records
//           then hold eight roots (without anyHairMB words 6 and 7 stay zero and the array ends where it did)
//   nodes : with anyLinear in two sections - `A.nodes` with the top-level tree and the static trees, `A.nodesMB` with the motion-blur
//           trees, child indices counted in 144-byte units from the start of the uploaded buffer, and `A.nodeImage` the two with the
//           padding between them.  With topLinear the top-level tree leads `A.nodesMB` instead of `A.nodes`, and the general layout
//           of `blobs` is used whatever the scenes hold.
// maxDepth (launch_on reserves 7 * (maxDepth + 1) + 2 stack entries) =
//     the top-level depth
//   + 1 for the exit marker
//   + the largest number of pending-tree markers any instanced scene can have stacked at once (its tree count - 1, at most 7; in the
//     kinds 14..21: 1 as soon as any scene has quads)
//   + the deepest of all instanced trees (the trees of a scene are never stacked together: a marker is popped only when the entries
//     of the tree before it are gone).
Scene::InstanceCounts layout_mesh_instances(Scene* s, const MeshInstances& c)
{
  Accel& A = s->instAccel;
  const DistinctScenes ds = distinct_scenes(c.placed);
  std::vector<uint32_t> order;
  std::vector<QNodeMB8> topMB; // topLinear: the top-level tree, references counted from its own first node
  if (c.topLinear) topMB = build_top_level_linear(s, c.placed, A, order);
  else order = build_top_level(s, c.placed, A);
  const bool general = c.anyMeshMotion || c.topLinear || c.anyHair; // the layout of `blobs` with InstanceSceneRecords
  const bool twoSections = c.anyLinear || c.topLinear;   // QNodeMB8s behind the QNode8s

  // what the distinct scenes bring (an accel that is absent or empty is not traceable and brings nothing)
  auto records = [](const Accel& O, size_t recordBytes) { return O.traceable() ? O.blobs.size() / recordBytes : 0; };
  Scene::InstanceCounts n;
  n.steps = count_steps(c.placed);
  size_t staticNodes = A.nodes.size(), mbNodes = topMB.size();
  for (const Scene* o : ds.scenes) {
    n.quads += records(o->quadAccel, sizeof(QuadRecord));
    n.triMB += records(o->triMBAccel, sizeof(TriMBRecord));
    n.quadMB += records(o->quadMBAccel, sizeof(QuadMBRecord));
    if (c.anyHair) {
      n.curves += records(o->curveAccel, sizeof(CurveRecord));
      n.lines += records(o->lineAccel, sizeof(LineRecord));
    }
    if (c.anyHairMB) {
      n.curveMB += records(o->curveMBAccel, sizeof(CurveMBRecord));
      n.lineMB += records(o->lineMBAccel, sizeof(LineMBRecord));
    }
    for (const Accel* t : {&o->triAccel, &o->triMBAccel, &o->quadAccel, &o->quadMBAccel, c.anyHair ? &o->curveAccel : nullptr, c.anyHair ? &o->lineAccel : nullptr,
                           c.anyHairMB ? &o->curveMBAccel : nullptr, c.anyHairMB ? &o->lineMBAccel : nullptr})
      if (t && t->traceable()) { // a motion-blur tree has nodes of one type or of the other
        staticNodes += t->nodes.size();
        mbNodes += t->nodesMB.size();
      }
  }
  size_t blobBytes = 0, nodeBytes = 0;
  add_section(blobBytes, c.placed.size(), sizeof(InstanceRecord)); // (the records start the array: write_instance_records)
  Section quadSec = add_section(blobBytes, n.quads, sizeof(QuadRecord)); // quad leaves index `blobs` as one array of 64-byte records
  Section stepSec = add_section(blobBytes, n.steps, sizeof(InstanceStep));
  Section sceneSec{}, triMBSec{}, quadMBSec{}, curveSec{}, lineSec{}, curveMBSec{}, lineMBSec{};
  if (general) {
    sceneSec = add_section(blobBytes, ds.scenes.size(), sizeof(InstanceSceneRecord));
    triMBSec = add_section(blobBytes, n.triMB, sizeof(TriMBRecord));    // motion-blur triangle leaves index `blobs` as one array of 96-byte records
    quadMBSec = add_section(blobBytes, n.quadMB, sizeof(QuadMBRecord)); // motion-blur quad leaves as one of 128-byte records
    if (c.anyHair) { // (an accel without hair trees ends behind the QuadMBRecords, as it always did)
      curveSec = add_section(blobBytes, n.curves, sizeof(CurveRecord)); // curve leaves index `blobs` as one array of 80-byte records (CurveLeaf::intersect)
      lineSec = add_section(blobBytes, n.lines, sizeof(LineRecord));    // line leaves as one of 48-byte records (LineLeaf::intersect)
    }
    if (c.anyHairMB) { // (an accel without moving-hair trees ends behind the LineRecords)
      curveMBSec = add_section(blobBytes, n.curveMB, sizeof(CurveMBRecord)); // motion-blur curve leaves index `blobs` as one array of 160-byte records (CurveMBLeaf::intersect)
      lineMBSec = add_section(blobBytes, n.lineMB, sizeof(LineMBRecord));    // motion-blur line leaves as one of 80-byte records (LineMBLeaf::intersect)
    }
  }
  // the node buffer: the QNode8s, and (kinds ACCEL_INSTMESHMB_LINEAR_*, no others have any) zero padding and the QNodeMB8s from the
  // multiple of 144 bytes their references count from
  add_section(nodeBytes, staticNodes, sizeof(QNode8));
  const Section mbSec = add_section(nodeBytes, mbNodes, sizeof(QNodeMB8));
  A.blobStride = sizeof(InstanceRecord);
  A.blobs.assign(blobBytes, 0);
  if (c.topLinear) { // the top-level tree leads the second section: its references move by where that section starts, in 144-byte units
    if (mbSec.base() + topMB.size() >= (size_t)REF_LEAF)
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instanced nodes for the 31-bit node reference of the top-level tree (it follows all static nodes in one buffer, counted in 144-byte units)");
    for (QNodeMB8& n : topMB)
      for (uint32_t& ch : n.child)
        if (ch != REF_EMPTY && !(ch & REF_LEAF)) ch += (uint32_t)mbSec.base();
    A.root += (uint32_t)mbSec.base(); // an inner node always (build_top_level_linear)
    A.nodesMB = std::move(topMB);
  }

  uint32_t deepest = 0;
  auto append_static = [&](const Accel& O, size_t leafBase) { return append_tree(A.nodes, 0, O, O.nodes, leafBase, TOO_MANY_NODES, deepest); };
  // a motion-blur tree: QNodeMB8s into the second section of the node buffer, or swept QNode8s behind the others
  auto append_mb = [&](const Accel& O, size_t leafBase) {
    if (!c.anyLinear) return append_static(O, leafBase);
    return append_tree(A.nodesMB, mbSec.base(), O, O.nodesMB, leafBase,
                       "too many instanced motion blur nodes for the 31-bit node reference (they follow all other nodes in one buffer, counted in 144-byte units)", deepest);
  };
  std::vector<uint32_t> rootOf, quadRootOf; // per scene: what its instances' records carry in `root` and (kinds 16, 17, 20, 21) in pad[0]
  for (const Scene* o : ds.scenes) {
    InstanceSceneRecord sc;
    memset(&sc, 0, sizeof(sc));
    const Accel& T = o->triAccel;
    if (A.prims.size() + T.prims.size() >= LEAF_RECORD_LIMIT) RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instanced triangles for the 26-bit leaf reference");
    sc.triRoot = append_static(T, A.prims.size());
    if (T.traceable()) A.prims.insert(A.prims.end(), T.prims.begin(), T.prims.end());
    sc.triMBRoot = append_mb(o->triMBAccel, place_leaf_records(A.blobs, triMBSec, o->triMBAccel, "too many instanced motion blur triangle segments for the 26-bit leaf reference (their "
                                                                                                 "records follow the instance, quad, step and scene records in one array)"));
    sc.quadRoot = append_static(o->quadAccel, place_leaf_records(A.blobs, quadSec, o->quadAccel, "too many instances and instanced quads for the 26-bit leaf reference (quad records follow "
                                                                                                 "the instance records in one array)"));
    sc.quadMBRoot = append_mb(o->quadMBAccel, place_leaf_records(A.blobs, quadMBSec, o->quadMBAccel, "too many instanced motion blur quad segments for the 26-bit leaf reference (their records "
                                                                                                     "follow all other records in one array)"));
    if (c.anyHair) { // the curve and the line tree behind the scene's four mesh trees; both are QNode8 trees over static records
      sc.curveRoot = append_static(o->curveAccel, place_leaf_records(A.blobs, curveSec, o->curveAccel, "too many instanced curves for the 26-bit leaf reference (the curve section: their records "
                                                                                                       "follow all mesh records in one array)"));
      sc.lineRoot = append_static(o->lineAccel, place_leaf_records(A.blobs, lineSec, o->lineAccel, "too many instanced line segments for the 26-bit leaf reference (the line section: their records "
                                                                                                   "follow all other records in one array)"));
    }
    if (c.anyHairMB) { // the two moving-hair trees: swept QNode8s (classify_mesh_instances has refused QNodeMB8s) over motion-blur records
      sc.curveMBRoot = append_static(o->curveMBAccel, place_leaf_records(A.blobs, curveMBSec, o->curveMBAccel, "too many instanced motion blur curve segments for the 26-bit leaf reference (the motion "
                                                                                                               "blur curve section: their records follow all static records in one array)"));
      sc.lineMBRoot = append_static(o->lineMBAccel, place_leaf_records(A.blobs, lineMBSec, o->lineMBAccel, "too many instanced motion blur line segments for the 26-bit leaf reference (the motion blur "
                                                                                                           "line section: their records follow all other records in one array)"));
    }
    quadRootOf.push_back(sc.quadRoot);
    rootOf.push_back(general ? (uint32_t)(sceneSec.base() + sceneSec.used) : sc.triRoot); // general layout: the scene's InstanceSceneRecord, in 64-byte units
    if (general) memcpy(A.blobs.data() + sceneSec.offset + sceneSec.used++ * sizeof(sc), &sc, sizeof(sc));
  }
  write_instance_records(c.placed, ds, order, rootOf, !general && c.anyQuads ? &quadRootOf : nullptr, stepSec.base(),
                         "too many instances, instanced quads and instance time steps for the 24-bit step offset of an instance record", A.blobs);
  if (twoSections) {
    A.nodeImage.assign(nodeBytes, 0);
    if (!A.nodes.empty()) memcpy(A.nodeImage.data(), A.nodes.data(), A.nodes.size() * sizeof(QNode8));
    if (!A.nodesMB.empty()) memcpy(A.nodeImage.data() + mbSec.offset, A.nodesMB.data(), A.nodesMB.size() * sizeof(QNodeMB8));
    A.blobOffsets = {(uint32_t)A.nodesMB.size(), (uint32_t)mbSec.base()};
  }
  A.kind = instance_kind(c);
  A.instHair = c.anyHairMB ? 2u : c.anyHair ? 1u : 0u;
  A.robust = c.pluecker ? 1 : 0;
  A.maxDepth += 1u + (general ? c.pendingMax : c.anyQuads ? 1u : 0u) + deepest;
  return n;
}

// ---- instances of subdivision scenes -------------------------------------------------------------------------------------------------

// Two subdivision accels are placed: the eager default (ACCEL_GRIDSOA) and bvh4.compressed.leaf at every compression level; the kernel
// is instantiated per leaf family and level, so all instanced subdivision scenes of one top scene must agree in both (their tessellation
// levels may differ).  A host-only device takes such instances only when its config names inst_accel= and subdiv_accel=
// (Device::inst_subdiv_enabled); otherwise build_instance_accel has refused them as it always did.
struct SubdivInstances
{
  std::vector<PlacedInstance> placed; // in geomID order
  uint32_t leafKind = ACCEL_NONE;     // ACCEL_GRIDSOA or ACCEL_CBVH_LEAF, of every instanced scene
  uint32_t levels = 0;                // ACCEL_CBVH_LEAF: the compression level of every instanced scene
  bool topLinear = false;             // inst_subdiv_bounds=linear and a placed instance has more than one time step: kinds ACCEL_INSTSUBDIV_TOP_LINEAR_*
};

SubdivInstances classify_subdiv_instances(const Scene* s)
{
  SubdivInstances c;
  if (!s->device->inst_subdiv_enabled()) return c;
  bool haveKind = false;
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
    if (haveKind && (O.kind != c.leafKind || C != c.levels))
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "the instanced subdivision scenes of one scene disagree in accel kind or compression level: the scene of instance " + std::to_string(gid) + " has " +
                                            accel_name(O.kind, C) + ", the scene of instance " + std::to_string(kindGeom) + " " + accel_name(c.leafKind, c.levels) +
                                            ": the instance kernel is instantiated per leaf kind and level");
    if (!haveKind) kindGeom = gid;
    haveKind = true;
    c.leafKind = O.kind;
    c.levels = C;
    c.placed.push_back({g, gid, o, instance_world_box(g, o)});
    c.topLinear |= g->local2world.size() > 1 && s->device->inst_subdiv_top_linear_enabled();
  }
  return c;
}

// Laid out like the first accel.  One node array holds the top-level tree and behind it the rebased subdivision BVH8 of every distinct
// instanced scene; `blobs` holds the InstanceRecords, the InstanceSteps of moving instances, and - from a multiple of the blob stride
// on - the leaf blobs of all instanced scenes, so that a rebased leaf reference indexes `blobs` the way the leaf functions of the
// subdivision kernels do (GridCellLeaf::intersect, CbvhLeaf::intersect).
// With topLinear (kinds ACCEL_INSTSUBDIV_TOP_LINEAR_*) the top-level tree is made of QNodeMB8s and moves to a second section of the node
// buffer, behind the instanced trees and the padding to a multiple of 144 bytes: `A.nodes` holds the instanced trees from index 0 on,
// `A.nodesMB` the top-level tree with references counted in 144-byte units from the start of the buffer, `A.nodeImage` both as uploaded.
// `blobs` is the same apart from the `root` words of the records (the instanced trees lead the buffer).
// maxDepth = the top-level depth + 1 for the exit marker + the deepest instanced tree.
void layout_subdiv_instances(Scene* s, const SubdivInstances& c)
{
  Accel& A = s->instSubdivAccel;
  const DistinctScenes ds = distinct_scenes(c.placed);
  std::vector<uint32_t> order;
  std::vector<QNodeMB8> topMB; // topLinear: the top-level tree, references counted from its own first node
  if (c.topLinear) topMB = build_top_level_linear(s, c.placed, A, order);
  else order = build_top_level(s, c.placed, A);

  const size_t stride = ds.scenes[0]->subdivAccel.blobStride;
  size_t numBlobs = 0;
  for (const Scene* o : ds.scenes) {
    const Accel& O = o->subdivAccel;
    if (O.blobStride != stride || O.blobs.size() % stride != 0) RT_THROW(RTC_ERROR_UNKNOWN, "instance builder: blob strides");
    numBlobs += O.blobs.size() / stride;
  }
  size_t blobBytes = 0;
  add_section(blobBytes, c.placed.size(), sizeof(InstanceRecord)); // (the records start the array: write_instance_records)
  const Section stepSec = add_section(blobBytes, count_steps(c.placed), sizeof(InstanceStep));
  Section blobSec = add_section(blobBytes, numBlobs, stride);
  A.blobStride = (uint32_t)stride;
  A.blobs.assign(blobBytes, 0);

  uint32_t deepest = 0;
  std::vector<uint32_t> rootOf;
  for (const Scene* o : ds.scenes) {
    const Accel& O = o->subdivAccel;
    const size_t leafBase = place_leaf_records(A.blobs, blobSec, O, "too many instanced subdivision leaf blobs for the 26-bit leaf reference (the blobs follow the instance and step records in one array)");
    rootOf.push_back(append_tree(A.nodes, 0, O, O.nodes, leafBase, TOO_MANY_NODES, deepest));
  }
  write_instance_records(c.placed, ds, order, rootOf, nullptr, stepSec.base(),
                         "too many instances and instance time steps for the 24-bit step offset of an instance record", A.blobs);
  A.kind = c.leafKind == ACCEL_GRIDSOA ? ACCEL_INSTSUBDIV_GRID : ACCEL_INSTSUBDIV_CBVH_LEAF;
  A.cbvhLevels = c.levels;
  A.maxDepth += 1u + deepest;
  A.blobOffsets = {(uint32_t)numBlobs, (uint32_t)blobSec.base()};
  if (c.topLinear) { // the top-level tree follows all instanced trees: its references move by where its section starts, in 144-byte units
    size_t nodeBytes = 0;
    add_section(nodeBytes, A.nodes.size(), sizeof(QNode8));
    const Section mbSec = add_section(nodeBytes, topMB.size(), sizeof(QNodeMB8));
    if (mbSec.base() + topMB.size() >= (size_t)REF_LEAF)
      RT_THROW(RTC_ERROR_INVALID_OPERATION, "too many instanced nodes for the 31-bit node reference of the top-level tree (it follows all instanced nodes in one buffer, counted in 144-byte units)");
    for (QNodeMB8& n : topMB)
      for (uint32_t& ch : n.child)
        if (ch != REF_EMPTY && !(ch & REF_LEAF)) ch += (uint32_t)mbSec.base();
    A.root += (uint32_t)mbSec.base(); // an inner node always (build_top_level_linear)
    A.nodesMB = std::move(topMB);
    A.nodeImage.assign(nodeBytes, 0);
    if (!A.nodes.empty()) memcpy(A.nodeImage.data(), A.nodes.data(), A.nodes.size() * sizeof(QNode8));
    memcpy(A.nodeImage.data() + mbSec.offset, A.nodesMB.data(), A.nodesMB.size() * sizeof(QNodeMB8));
    A.kind = c.leafKind == ACCEL_GRIDSOA ? ACCEL_INSTSUBDIV_TOP_LINEAR_GRID : ACCEL_INSTSUBDIV_TOP_LINEAR_CBVH_LEAF;
    A.blobOffsets.push_back((uint32_t)A.nodesMB.size());
    A.blobOffsets.push_back((uint32_t)mbSec.base());
  }
}

} // namespace

// Instances (RTC_GEOMETRY_TYPE_INSTANCE, one level) of scenes that hold triangle and quad meshes, static or with time steps.
void build_instance_accel(Scene* s)
{
  s->instAccel.clear();
  s->instCounts = Scene::InstanceCounts();
  s->instIntersectFilter = s->instOccludedFilter = false;
  const MeshInstances c = classify_mesh_instances(s);
  s->instIntersectFilter = c.intersectFilter;
  s->instOccludedFilter = c.occludedFilter;
  if (!c.placed.empty()) s->instCounts = layout_mesh_instances(s, c);
}

// Instances of subdivision scenes: the second instance accel of a scene (accel.h InstanceRecord, kinds ACCEL_INSTSUBDIV_* and ACCEL_INSTSUBDIV_TOP_LINEAR_*).  Runs after
// build_instance_accel, which has refused instances without a committed scene.
void build_instance_subdiv_accel(Scene* s)
{
  s->instSubdivAccel.clear();
  s->instSubdivAccel.robust = 1; // the subdivision accels traverse robustly, on both levels here
  const SubdivInstances c = classify_subdiv_instances(s);
  if (!c.placed.empty()) layout_subdiv_instances(s, c);
}

} // namespace rtamd
