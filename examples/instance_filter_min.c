/* Filter functions on an instanced mesh (device config inst_filters=1): an alpha-tested card - a quad mesh of two unit quads, a "leaf"
 * at z = 0 (primID 0) whose left half (x < 0.5 in the card's own space) is cut out by the geometry's intersection filter, and an opaque
 * backing at z = 1 (primID 1) - committed once and placed twice by RTC_GEOMETRY_TYPE_INSTANCE geometries, at x = 0 and x = 10.
 * The filter gets the card's user data (the alpha threshold) as geometryUserPtr and finds the instance in context->instID[0] and in
 * the hit's instID[0]; ray.org is the WORLD-space origin, so the card-space x is org_x minus the instance's offset, which the
 * example keeps in a table by instance geomID.  A context filter - the application's own context struct, derived from
 * RTCIntersectContext - counts every candidate that the geometry's filter let through.
 *
 *   cc -std=c99 -I include examples/instance_filter_min.c -L embree-compressed_amd/lib -lembree3 -lm -o instance_filter_min
 */
#include <embree3/rtcore.h>
#include <math.h>
#include <stdio.h>

struct CardData { float alphaEdge; unsigned calls; };
struct CountingContext { struct RTCIntersectContext context; unsigned accepted; unsigned wrongInstance; }; /* RTCIntersectContext first */
static float g_offset[2]; /* world x of instance k, by its geomID */

static int fail(const char* what)
{
  printf("instance_filter_min: FAILED (%s)\n", what);
  return 1;
}

/* RTCRayN / RTCHitN are structure-of-arrays blobs of width N: component c of lane i is word c * N + i (ray: org_x = 0; hit: primID = 5,
 * instID[0] = 7).  N = 1 for every callback of this library. */
static float ray_org_x(const struct RTCFilterFunctionNArguments* a, unsigned i) { return ((const float*)a->ray)[0 * a->N + i]; }
static unsigned hit_primID(const struct RTCFilterFunctionNArguments* a, unsigned i) { return ((const unsigned*)a->hit)[5 * a->N + i]; }
static unsigned hit_instID(const struct RTCFilterFunctionNArguments* a, unsigned i) { return ((const unsigned*)a->hit)[7 * a->N + i]; }

/* the card's intersection filter */
static void alpha_test(const struct RTCFilterFunctionNArguments* args)
{
  struct CardData* card = (struct CardData*)args->geometryUserPtr;
  const unsigned inst = args->context->instID[0];
  const float x = ray_org_x(args, 0) - g_offset[inst < 2 ? inst : 0];
  if (!args->valid[0]) return;
  card->calls++;
  if (hit_primID(args, 0) == 0 && x < card->alphaEdge) args->valid[0] = 0; /* cut out: the ray goes on */
}

/* the context filter: runs after the geometry's, on the candidates it left valid */
static void count_accepted(const struct RTCFilterFunctionNArguments* args)
{
  struct CountingContext* mine = (struct CountingContext*)args->context;
  if (!args->valid[0]) return;
  mine->accepted++;
  if (hit_instID(args, 0) != args->context->instID[0]) mine->wrongInstance++;
}

static void init_ray(struct RTCRayHit* rh, float x, float y, unsigned id)
{
  rh->ray.org_x = x; rh->ray.org_y = y; rh->ray.org_z = -1.f;
  rh->ray.dir_x = 0.f; rh->ray.dir_y = 0.f; rh->ray.dir_z = 1.f;
  rh->ray.tnear = 0.f; rh->ray.tfar = INFINITY;
  rh->ray.time = 0.f;
  rh->ray.mask = 0xFFFFFFFFu; rh->ray.id = id; rh->ray.flags = 0;
  rh->hit.geomID = RTC_INVALID_GEOMETRY_ID;
  rh->hit.primID = RTC_INVALID_GEOMETRY_ID;
  rh->hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
}

int main(void)
{
  static const float verts[8][3] = {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f}, {1.f, 1.f, 0.f}, {0.f, 1.f, 0.f},
                                    {0.f, 0.f, 1.f}, {1.f, 0.f, 1.f}, {1.f, 1.f, 1.f}, {0.f, 1.f, 1.f}};
  /* without inst_filters=1 the commit of the top scene below is refused: a geometry filter inside an instanced scene */
  RTCDevice device = rtcNewDevice("inst_filters=1");
  struct CardData card = {0.5f, 0};
  struct CountingContext ctx;
  RTCGeometry mesh;
  RTCScene object, scene;
  unsigned instIDs[2], cardID;
  float* v;
  unsigned* idx;
  int k;
  if (!device) return fail("rtcNewDevice");

  mesh = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_QUAD);
  v = (float*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT3, 3 * sizeof(float), 8);
  idx = (unsigned*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT4, 4 * sizeof(unsigned), 2);
  if (!v || !idx) return fail("quad buffers");
  for (k = 0; k < 8; k++) {
    v[3 * k + 0] = verts[k][0];
    v[3 * k + 1] = verts[k][1];
    v[3 * k + 2] = verts[k][2];
    idx[k] = (unsigned)k;
  }
  rtcSetGeometryUserData(mesh, &card);
  rtcSetGeometryIntersectFilterFunction(mesh, alpha_test);
  rtcCommitGeometry(mesh);
  object = rtcNewScene(device);
  cardID = rtcAttachGeometry(object, mesh);
  rtcReleaseGeometry(mesh);
  rtcCommitScene(object);

  scene = rtcNewScene(device);
  for (k = 0; k < 2; k++) {
    const float xfm[12] = {1.f, 0.f, 0.f, 10.f * (float)k, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    RTCGeometry inst = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_INSTANCE);
    rtcSetGeometryInstancedScene(inst, object);
    rtcSetGeometryTransform(inst, 0, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
    rtcCommitGeometry(inst);
    instIDs[k] = rtcAttachGeometry(scene, inst);
    rtcReleaseGeometry(inst);
    if (instIDs[k] > 1) return fail("instance IDs");
    g_offset[instIDs[k]] = 10.f * (float)k;
  }
  rtcReleaseScene(object); /* the instances hold it */
  rtcCommitScene(scene);
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("commit");

  rtcInitIntersectContext(&ctx.context);
  ctx.context.filter = count_accepted;
  ctx.accepted = ctx.wrongInstance = 0;
  for (k = 0; k < 2; k++) {
    struct RTCRayHit rh;
    /* through the cut-out half of the leaf: the filter rejects the leaf, the ray ends on the backing */
    init_ray(&rh, 10.f * (float)k + 0.25f, 0.25f, (unsigned)(2 * k));
    rtcIntersect1(scene, &ctx.context, &rh);
    if (rh.hit.geomID != cardID || rh.hit.primID != 1 || rh.hit.instID[0] != instIDs[k]) return fail("ids behind the cut-out");
    if (rh.ray.tfar != 2.f) return fail("distance behind the cut-out");
    /* through the other half: the leaf itself */
    init_ray(&rh, 10.f * (float)k + 0.75f, 0.25f, (unsigned)(2 * k + 1));
    rtcIntersect1(scene, &ctx.context, &rh);
    if (rh.hit.geomID != cardID || rh.hit.primID != 0 || rh.hit.instID[0] != instIDs[k]) return fail("ids on the leaf");
    if (rh.ray.tfar != 1.f) return fail("distance on the leaf");
    printf("instance %u: x = 0.25 passes the leaf and ends at t = 2, x = 0.75 ends on it at t = 1\n", instIDs[k]);
  }
  /* per instance: leaf (rejected) + backing, then leaf: three calls of the geometry's filter, two candidates it let through */
  if (card.calls != 6) return fail("calls of the geometry filter");
  if (ctx.accepted != 4 || ctx.wrongInstance != 0) return fail("calls of the context filter");
  if (ctx.context.instID[0] != RTC_INVALID_GEOMETRY_ID) return fail("the context's instID after the calls");
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("trace");
  rtcReleaseScene(scene);
  rtcReleaseDevice(device);
  printf("instance_filter_min: ok\n");
  return 0;
}
