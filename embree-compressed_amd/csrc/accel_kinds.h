// What the host code asks of an accel kind, in ONE table: a row per AccelKind (accel.h), in enum order, beside the launchers it names.
// Host only: no kernel reads it.  A new kind costs an enum value, a row here, a launcher and a builder; a kind whose row does not say
// "yes" to a kernel form does not get it ("Adding a kind / adding a slot").
#pragma once
#include <hip/hip_runtime.h>

#include "accel.h"

namespace rtamd {

struct LaunchParams; // trace.h
struct ServiceParams;

// Enqueue traversal of one batch on `stream`.  Asynchronous; errors surface through the returned hipError_t.
hipError_t launch_trace_tri(const LaunchParams& p, hipStream_t stream);       // trace_tri.hip
hipError_t launch_trace_quad(const LaunchParams& p, hipStream_t stream);      // trace_quad.hip
hipError_t launch_trace_trimb(const LaunchParams& p, hipStream_t stream);     // trace_tri_mb.hip (swept and linear-bounds kinds)
hipError_t launch_trace_quadmb(const LaunchParams& p, hipStream_t stream);    // trace_quad_mb.hip (swept and linear-bounds kinds)
hipError_t launch_trace_grid(const LaunchParams& p, hipStream_t stream);      // trace_grid.hip
hipError_t launch_trace_cbvh_box(const LaunchParams& p, hipStream_t stream);  // trace_cbvh_box.hip
hipError_t launch_trace_cbvh_leaf(const LaunchParams& p, hipStream_t stream); // trace_cbvh_leaf.hip
hipError_t launch_trace_cbvh_grid(const LaunchParams& p, hipStream_t stream); // trace_cbvh_grid.hip
hipError_t launch_trace_cbvh_full(const LaunchParams& p, hipStream_t stream); // trace_cbvh_full.hip
hipError_t launch_trace_line(const LaunchParams& p, hipStream_t stream);      // trace_line.hip (flat linear curves; no service kernel)
hipError_t launch_trace_line_mb(const LaunchParams& p, hipStream_t stream);   // trace_line_mb.hip (flat linear curves with time steps; lane kernel only)
hipError_t launch_trace_curve(const LaunchParams& p, hipStream_t stream);     // trace_curve.hip (flat Bezier / B-spline curves; lane kernel only, no service kernel)
hipError_t launch_trace_round_curve(const LaunchParams& p, hipStream_t stream); // trace_round_curve.hip (round Bezier / B-spline curves: launch_trace_curve diverts to it when LaunchParams::roundCurves is set)
hipError_t launch_trace_curve_mb(const LaunchParams& p, hipStream_t stream);  // trace_curve_mb.hip (flat Bezier / B-spline curves with time steps; lane kernel only)
hipError_t launch_trace_instance(const LaunchParams& p, hipStream_t stream);  // trace_instance.hip
hipError_t launch_trace_instance_mesh_mb(const LaunchParams& p, hipStream_t stream); // trace_instance_mesh_mb.hip
hipError_t launch_trace_instance_hair(const LaunchParams& p, hipStream_t stream);    // trace_instance_hair.hip (launch_trace_instance_mesh_mb diverts to it when LaunchParams::instHair is set)
hipError_t launch_trace_instance_hair_mb(const LaunchParams& p, hipStream_t stream); // trace_instance_hair_mb.hip (... when LaunchParams::instHair is 2)
hipError_t launch_trace_instance_subdiv(const LaunchParams& p, hipStream_t stream);  // trace_instance_subdiv.hip
hipError_t launch_trace_instance_mesh_mb_linear(const LaunchParams& p, hipStream_t stream); // trace_instance_mesh_mb_linear.hip
hipError_t launch_trace_instance_top_linear(const LaunchParams& p, hipStream_t stream); // trace_instance_top_linear.hip (closest hit, any hit and its own EXCL form)
hipError_t launch_trace_instance_subdiv_top_linear(const LaunchParams& p, hipStream_t stream); // trace_instance_subdiv_top_linear.hip (no EXCL form: filters stay refused)
// start the service kernel for base.accel.kind (and base.cbvhLevels); hipErrorInvalidValue: no service kernel for this level
hipError_t launch_service_tri(const ServiceParams& s, hipStream_t stream);       // trace_tri.hip
hipError_t launch_service_quad(const ServiceParams& s, hipStream_t stream);      // trace_quad.hip
hipError_t launch_service_grid(const ServiceParams& s, hipStream_t stream);      // trace_grid.hip
hipError_t launch_service_cbvh_box(const ServiceParams& s, hipStream_t stream);  // trace_cbvh_box.hip  (one unit per cBVH mode:
hipError_t launch_service_cbvh_leaf(const ServiceParams& s, hipStream_t stream); // trace_cbvh_leaf.hip  trace_cbvh.hip.h
hipError_t launch_service_cbvh_grid(const ServiceParams& s, hipStream_t stream); // trace_cbvh_grid.hip  instantiated for
hipError_t launch_service_cbvh_full(const ServiceParams& s, hipStream_t stream); // trace_cbvh_full.hip  that mode)

// what `nodes` holds: QNode8[]; QNodeMB8[] (mb_bounds=linear: 144-byte stride, Accel::nodesMB); or the two sections QNode8[] | padding |
// QNodeMB8[] of the linear instance kinds (Accel::nodeImage)
enum KindNodes : uint8_t { NODES_Q8, NODES_MB8, NODES_TWO_SECTION };
// two-level kinds: what lies below the instances (Scene::instAccel / Scene::instSubdivAccel)
enum KindInst : uint8_t { INST_NONE, INST_MESH, INST_SUBDIV };
// leaf kernels that always run 8 lanes per ray and so fit four waves per SIMD (grid sizing in launch_on): never, always, or in the quad
// form of the cBVH blob walk only (launch_on knows the form: LaunchParams::cbvhLaneForm)
enum KindOct : uint8_t { OCT_NEVER, OCT_ALWAYS, OCT_QUAD_FORM };

struct KindRow
{
  AccelKind kind;        // the row's own kind (checked against its place below)
  hipError_t (*trace)(const LaunchParams&, hipStream_t);  // launch_trace calls it; nullptr: nothing to trace
  hipError_t (*serve)(const ServiceParams&, hipStream_t); // the kind's service kernel for small calls (trace_service.hip.h); nullptr: it has
                                                          // none, the combiner traces such calls with the batch kernels
  bool robust;           // node test: 1 robust arithmetic (Pluecker / ROBUST kinds, every subdivision accel), 0 the fast test
  KindNodes nodes;
  KindInst inst;
  bool instGeneral;      // instance kinds: `blobs` has the general layout (InstanceSceneRecords, see InstanceRecord)
  bool pool, poolPays;   // has a ray-pool form (trace_pool.hip.h; 0: lane kernel only), and it is the faster one for very large batches (launch_on)
  bool levelFree;        // the service kernel does not depend on the scene's compression level
  bool cull;             // may take the root cull pre-pass (trace_cull.hip.h): the pre-pass decodes a QNode8 root outside any instance and
                         // launch_cull takes its node test from `robust`
  KindOct octOnly;
  uint8_t octLeaf;       // default of LaunchParams::octLeaf: triangle leaves and cBVH blobs 16, grid cells 24 (measured optima)
  bool primsInPrims;     // the primitives are the TriRecords in `prims` (rtcamdGetSceneStats); 0: records of blobStride bytes in `blobs`
};

// clang-format off
inline constexpr KindRow ACCEL_KINDS[] = {
  // kind                                  trace                                    serve                 robust nodes              inst    general pool pays levelFree cull octOnly  octLeaf inPrims
  {ACCEL_NONE,                            nullptr,                                 nullptr,                  0, NODES_Q8,          INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_TRI_PLUECKER,                    launch_trace_tri,                        launch_service_tri,       1, NODES_Q8,          INST_NONE,   0, 1, 1, 1, 1, OCT_NEVER,     16, 1},
  {ACCEL_TRI_MOELLER,                     launch_trace_tri,                        launch_service_tri,       0, NODES_Q8,          INST_NONE,   0, 1, 1, 1, 1, OCT_NEVER,     16, 1},
  {ACCEL_CBVH_BOX,                        launch_trace_cbvh_box,                   launch_service_cbvh_box,  1, NODES_Q8,          INST_NONE,   0, 1, 0, 0, 1, OCT_QUAD_FORM, 16, 0},
  {ACCEL_CBVH_LEAF,                       launch_trace_cbvh_leaf,                  launch_service_cbvh_leaf, 1, NODES_Q8,          INST_NONE,   0, 1, 0, 0, 1, OCT_QUAD_FORM, 16, 0},
  {ACCEL_CBVH_GRID,                       launch_trace_cbvh_grid,                  launch_service_cbvh_grid, 1, NODES_Q8,          INST_NONE,   0, 1, 1, 0, 1, OCT_NEVER,     16, 0},
  {ACCEL_GRIDSOA,                         launch_trace_grid,                       launch_service_grid,      1, NODES_Q8,          INST_NONE,   0, 1, 0, 1, 1, OCT_ALWAYS,    24, 0},
  {ACCEL_CBVH_FULL,                       launch_trace_cbvh_full,                  launch_service_cbvh_full, 1, NODES_Q8,          INST_NONE,   0, 1, 0, 0, 1, OCT_QUAD_FORM, 16, 0},
  {ACCEL_QUAD_PLUECKER,                   launch_trace_quad,                       launch_service_quad,      1, NODES_Q8,          INST_NONE,   0, 1, 0, 1, 1, OCT_NEVER,     16, 0},
  {ACCEL_QUAD_MOELLER,                    launch_trace_quad,                       launch_service_quad,      0, NODES_Q8,          INST_NONE,   0, 1, 0, 1, 1, OCT_NEVER,     16, 0},
  // the motion-blur leaves exist in the lane kernel only, under swept and under linear bounds
  {ACCEL_TRIMB_PLUECKER,                  launch_trace_trimb,                      nullptr,                  1, NODES_Q8,          INST_NONE,   0, 0, 0, 0, 1, OCT_NEVER,     16, 0},
  {ACCEL_TRIMB_MOELLER,                   launch_trace_trimb,                      nullptr,                  0, NODES_Q8,          INST_NONE,   0, 0, 0, 0, 1, OCT_NEVER,     16, 0},
  {ACCEL_QUADMB_PLUECKER,                 launch_trace_quadmb,                     nullptr,                  1, NODES_Q8,          INST_NONE,   0, 0, 0, 0, 1, OCT_NEVER,     16, 0},
  {ACCEL_QUADMB_MOELLER,                  launch_trace_quadmb,                     nullptr,                  0, NODES_Q8,          INST_NONE,   0, 0, 0, 0, 1, OCT_NEVER,     16, 0},
  // the two-level kernels are lane-per-ray kernels of their own: no pool form, no service kernel, no root cull pre-pass
  {ACCEL_INST_TRI_PLUECKER,               launch_trace_instance,                   nullptr,                  1, NODES_Q8,          INST_MESH,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INST_TRI_MOELLER,                launch_trace_instance,                   nullptr,                  0, NODES_Q8,          INST_MESH,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INST_PLUECKER,                   launch_trace_instance,                   nullptr,                  1, NODES_Q8,          INST_MESH,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INST_MOELLER,                    launch_trace_instance,                   nullptr,                  0, NODES_Q8,          INST_MESH,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTMB_TRI_PLUECKER,             launch_trace_instance,                   nullptr,                  1, NODES_Q8,          INST_MESH,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTMB_TRI_MOELLER,              launch_trace_instance,                   nullptr,                  0, NODES_Q8,          INST_MESH,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTMB_PLUECKER,                 launch_trace_instance,                   nullptr,                  1, NODES_Q8,          INST_MESH,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTMB_MOELLER,                  launch_trace_instance,                   nullptr,                  0, NODES_Q8,          INST_MESH,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTMESHMB_PLUECKER,             launch_trace_instance_mesh_mb,           nullptr,                  1, NODES_Q8,          INST_MESH,   1, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTMESHMB_MOELLER,              launch_trace_instance_mesh_mb,           nullptr,                  0, NODES_Q8,          INST_MESH,   1, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTSUBDIV_GRID,                 launch_trace_instance_subdiv,            nullptr,                  1, NODES_Q8,          INST_SUBDIV, 0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTSUBDIV_CBVH_LEAF,            launch_trace_instance_subdiv,            nullptr,                  1, NODES_Q8,          INST_SUBDIV, 0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  // mb_bounds=linear: no pre-pass either - a root of time-dependent boxes would have to be culled per ray time
  {ACCEL_TRIMB_LINEAR_PLUECKER,           launch_trace_trimb,                      nullptr,                  1, NODES_MB8,         INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_TRIMB_LINEAR_MOELLER,            launch_trace_trimb,                      nullptr,                  0, NODES_MB8,         INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_QUADMB_LINEAR_PLUECKER,          launch_trace_quadmb,                     nullptr,                  1, NODES_MB8,         INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_QUADMB_LINEAR_MOELLER,           launch_trace_quadmb,                     nullptr,                  0, NODES_MB8,         INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTMESHMB_LINEAR_PLUECKER,      launch_trace_instance_mesh_mb_linear,    nullptr,                  1, NODES_TWO_SECTION, INST_MESH,   1, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTMESHMB_LINEAR_MOELLER,       launch_trace_instance_mesh_mb_linear,    nullptr,                  0, NODES_TWO_SECTION, INST_MESH,   1, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTTOP_LINEAR_PLUECKER,         launch_trace_instance_top_linear,        nullptr,                  1, NODES_TWO_SECTION, INST_MESH,   1, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTTOP_LINEAR_MOELLER,          launch_trace_instance_top_linear,        nullptr,                  0, NODES_TWO_SECTION, INST_MESH,   1, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTSUBDIV_TOP_LINEAR_GRID,      launch_trace_instance_subdiv_top_linear, nullptr,                  1, NODES_TWO_SECTION, INST_SUBDIV, 0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_INSTSUBDIV_TOP_LINEAR_CBVH_LEAF, launch_trace_instance_subdiv_top_linear, nullptr,                  1, NODES_TWO_SECTION, INST_SUBDIV, 0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  // line segments: lane and pool kernels, no service kernel.  No pre-pass on the line and curve accels, static or moving: nobody has run it on them
  {ACCEL_LINE_ROBUST,                     launch_trace_line,                       nullptr,                  1, NODES_Q8,          INST_NONE,   0, 1, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_LINE_FAST,                       launch_trace_line,                       nullptr,                  0, NODES_Q8,          INST_NONE,   0, 1, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_LINEMB_ROBUST,                   launch_trace_line_mb,                    nullptr,                  1, NODES_Q8,          INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_LINEMB_FAST,                     launch_trace_line_mb,                    nullptr,                  0, NODES_Q8,          INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_LINEMB_LINEAR_ROBUST,            launch_trace_line_mb,                    nullptr,                  1, NODES_MB8,         INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_LINEMB_LINEAR_FAST,              launch_trace_line_mb,                    nullptr,                  0, NODES_MB8,         INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  // the ribbon leaf exists in the lane kernel only (lane and octet form); so does the tube leaf of the round curves, which shares these two
  // kinds (Accel::roundCurves, octet form only)
  {ACCEL_CURVE_ROBUST,                    launch_trace_curve,                      nullptr,                  1, NODES_Q8,          INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_CURVE_FAST,                      launch_trace_curve,                      nullptr,                  0, NODES_Q8,          INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_CURVEMB_ROBUST,                  launch_trace_curve_mb,                   nullptr,                  1, NODES_Q8,          INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_CURVEMB_FAST,                    launch_trace_curve_mb,                   nullptr,                  0, NODES_Q8,          INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_CURVEMB_LINEAR_ROBUST,           launch_trace_curve_mb,                   nullptr,                  1, NODES_MB8,         INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
  {ACCEL_CURVEMB_LINEAR_FAST,             launch_trace_curve_mb,                   nullptr,                  0, NODES_MB8,         INST_NONE,   0, 0, 0, 0, 0, OCT_NEVER,     16, 0},
};
// clang-format on
static_assert(sizeof(ACCEL_KINDS) / sizeof(ACCEL_KINDS[0]) == NUM_ACCEL_KINDS, "every AccelKind needs a row in ACCEL_KINDS");
constexpr bool accel_kinds_in_enum_order(uint32_t k = 0) { return k == NUM_ACCEL_KINDS || (ACCEL_KINDS[k].kind == k && accel_kinds_in_enum_order(k + 1)); }
static_assert(accel_kinds_in_enum_order(), "the rows of ACCEL_KINDS stand in enum order");

// the row of a kind; a value outside the enum reads as ACCEL_NONE, which is launched nowhere
inline const KindRow& kind_row(uint32_t kind) { return ACCEL_KINDS[kind < NUM_ACCEL_KINDS ? kind : (uint32_t)ACCEL_NONE]; }

} // namespace rtamd
