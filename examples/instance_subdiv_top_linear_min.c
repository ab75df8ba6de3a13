/* A fast-moving instance of a displaced subdivision mesh under time-dependent top-level boxes (device config
 * inst_subdiv_bounds=linear): a cube - six quads, Catmull-Clark, pushed out along its normal by a displacement function - committed
 * once in a scene of its own and placed by ONE RTC_GEOMETRY_TYPE_INSTANCE geometry with two time steps that carry it 64 units along x
 * over the shutter, beside a static instance of the same scene.  The box of the mover swept over the shutter is 66 units long; under
 * inst_subdiv_bounds=linear the top-level tree keeps its box at time 0 and at time 1 and a ray is tested against the box at ITS time, so
 * it pays for the interpolated transform, its inverse and the instanced tree only where the mover is then.  The same scene is built on
 * a device without the key (swept boxes, the default) and on one with it, the same rays are traced on both, and every record must be
 * equal byte for byte: only the work differs.  The scene statistics name the accel kinds 24 / 25 (swept) and 34 / 35 (linear).
 *
 *   cc -std=c99 -I include examples/instance_subdiv_top_linear_min.c -L embree-compressed_amd/lib -lembree3 -lm -o instance_subdiv_top_linear_min
 *   ./instance_subdiv_top_linear_min [further device config, e.g. subdiv_accel=bvh4.compressed.leaf]
 */
#include <embree3/rtcore.h>
#include <embree3/rtcore_amd.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#define NX 9
#define NT 5
#define NRAYS (NX * NT * 2)

static int fail(const char* what)
{
  printf("instance_subdiv_top_linear_min: FAILED (%s)\n", what);
  return 1;
}

/* pushes every point out along the normal, by a smooth bump over the face */
static void displace(const struct RTCDisplacementFunctionNArguments* args)
{
  unsigned i;
  for (i = 0; i < args->N; i++) {
    const float d = 0.125f * sinf(3.14159265f * args->u[i]) * sinf(3.14159265f * args->v[i]);
    args->P_x[i] += d * args->Ng_x[i];
    args->P_y[i] += d * args->Ng_y[i];
    args->P_z[i] += d * args->Ng_z[i];
  }
}

struct Built
{
  RTCDevice device;
  RTCScene scene;
  unsigned moverID, fixedID, kind;
};

static int build(const char* config, struct Built* b)
{
  static const float corners[8][3] = {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}, {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
  static const unsigned faces[24] = {0, 4, 5, 1, 1, 5, 7, 3, 3, 7, 6, 2, 2, 6, 4, 0, 4, 6, 7, 5, 0, 1, 3, 2};
  RTCGeometry mesh, mover, fixed;
  RTCScene object;
  struct RTCAMDSceneStats stats;
  float* v;
  float* level;
  unsigned* idx;
  unsigned* sizes;
  int k;
  b->device = rtcNewDevice(config);
  if (!b->device) return fail("rtcNewDevice");

  /* the instanced scene: one displaced subdivision mesh */
  mesh = rtcNewGeometry(b->device, RTC_GEOMETRY_TYPE_SUBDIVISION);
  v = (float*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT3, 3 * sizeof(float), 8);
  sizes = (unsigned*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_FACE, 0, RTC_FORMAT_UINT, sizeof(unsigned), 6);
  idx = (unsigned*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT, sizeof(unsigned), 24);
  level = (float*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_LEVEL, 0, RTC_FORMAT_FLOAT, sizeof(float), 24);
  if (!v || !sizes || !idx || !level) return fail("buffers");
  for (k = 0; k < 8; k++) {
    v[3 * k + 0] = corners[k][0];
    v[3 * k + 1] = corners[k][1];
    v[3 * k + 2] = corners[k][2];
  }
  for (k = 0; k < 6; k++) sizes[k] = 4;
  for (k = 0; k < 24; k++) {
    idx[k] = faces[k];
    level[k] = 16.f;
  }
  rtcSetGeometryDisplacementFunction(mesh, displace);
  rtcCommitGeometry(mesh);
  object = rtcNewScene(b->device);
  rtcAttachGeometry(object, mesh);
  rtcReleaseGeometry(mesh);
  rtcSetSceneLevels(object, 4, 2); /* 16 x 16 quads per face; compression level 2 for the compressed accels */
  rtcCommitScene(object);
  if (rtcGetDeviceError(b->device) != RTC_ERROR_NONE) return fail("commit of the instanced scene");

  /* the top scene: the mover, from x = 0 to x = 64 over the shutter, and a static instance at y = 8 */
  b->scene = rtcNewScene(b->device);
  mover = rtcNewGeometry(b->device, RTC_GEOMETRY_TYPE_INSTANCE);
  rtcSetGeometryInstancedScene(mover, object);
  rtcSetGeometryTimeStepCount(mover, 2);
  for (k = 0; k < 2; k++) {
    /* local-to-world of time step k, 3 x 4 row-major: the translation in the fourth column */
    const float xfm[12] = {1.f, 0.f, 0.f, 64.f * (float)k, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    rtcSetGeometryTransform(mover, (unsigned)k, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
  }
  rtcCommitGeometry(mover);
  b->moverID = rtcAttachGeometry(b->scene, mover);
  rtcReleaseGeometry(mover);
  fixed = rtcNewGeometry(b->device, RTC_GEOMETRY_TYPE_INSTANCE);
  rtcSetGeometryInstancedScene(fixed, object);
  {
    const float xfm[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 8.f, 0.f, 0.f, 1.f, 0.f};
    rtcSetGeometryTransform(fixed, 0, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
  }
  rtcCommitGeometry(fixed);
  b->fixedID = rtcAttachGeometry(b->scene, fixed);
  rtcReleaseGeometry(fixed);
  rtcReleaseScene(object); /* the instances hold it */
  rtcCommitScene(b->scene);
  if (rtcGetDeviceError(b->device) != RTC_ERROR_NONE) return fail("commit");
  stats.byteSize = sizeof(stats);
  rtcamdGetSceneStats(b->scene, &stats);
  b->kind = stats.accelKind;
  printf("'%s': accel kind %u, %u instances\n", config, stats.accelKind, (unsigned)stats.leafCount);
  return 0;
}

/* NX places along the mover's path x NT ray times, above the mover's row (y = 0) and above the static instance (y = 8) */
static void make_rays(struct RTCRayHit* rh)
{
  int ix, it, row, n = 0;
  for (row = 0; row < 2; row++)
    for (ix = 0; ix < NX; ix++)
      for (it = 0; it < NT; it++, n++) {
        rh[n].ray.org_x = 8.f * (float)ix + 0.25f; rh[n].ray.org_y = 8.f * (float)row + 0.125f; rh[n].ray.org_z = 10.f;
        rh[n].ray.dir_x = 0.f; rh[n].ray.dir_y = 0.f; rh[n].ray.dir_z = -1.f;
        rh[n].ray.tnear = 0.f; rh[n].ray.tfar = INFINITY;
        rh[n].ray.time = 0.25f * (float)it;
        rh[n].ray.mask = 0xFFFFFFFFu; rh[n].ray.id = (unsigned)n; rh[n].ray.flags = 0;
        rh[n].hit.Ng_x = rh[n].hit.Ng_y = rh[n].hit.Ng_z = rh[n].hit.u = rh[n].hit.v = 0.f;
        rh[n].hit.geomID = rh[n].hit.primID = rh[n].hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
      }
}

int main(int argc, char** argv)
{
  static struct RTCRayHit rays[2][NRAYS];
  struct Built built[2];
  struct RTCIntersectContext context;
  char config[2][256];
  int d, n, hitsMover = 0, hitsFixed = 0;
  const char* more = argc > 1 ? argv[1] : "";
  if (strlen(more) > 200) return fail("config too long");
  snprintf(config[0], sizeof(config[0]), "%s", more);
  snprintf(config[1], sizeof(config[1]), "%s%sinst_subdiv_bounds=linear", more, more[0] ? "," : "");
  for (d = 0; d < 2; d++)
    if (build(config[d], &built[d])) return 1;
  if (built[0].kind != 24 && built[0].kind != 25) return fail("accel kind without the key: 24 / 25");
  if (built[1].kind != built[0].kind + 10) return fail("accel kind: a moving subdivision instance under inst_subdiv_bounds=linear gives 34 / 35");
  if (built[0].moverID != built[1].moverID || built[0].fixedID != built[1].fixedID) return fail("geometry IDs");

  for (d = 0; d < 2; d++) {
    memset(rays[d], 0, sizeof(rays[d]));
    make_rays(rays[d]);
    rtcInitIntersectContext(&context);
    rtcIntersect1M(built[d].scene, &context, rays[d], NRAYS, sizeof(struct RTCRayHit));
    if (rtcGetDeviceError(built[d].device) != RTC_ERROR_NONE) return fail("trace");
  }
  if (memcmp(rays[0], rays[1], sizeof(rays[0])) != 0) return fail("the records under swept and under linear boxes differ");

  /* what the records say: above the mover's path a ray at x = 8 ix meets the mover only at the time it is there (64 t = 8 ix up to
   * its half width), and the static instance is met at every time by the rays of its column */
  for (n = 0; n < NRAYS; n++) {
    const struct RTCRayHit* r = &rays[1][n];
    const int row = n / (NX * NT), ix = (n / NT) % NX, it = n % NT;
    const int there = row == 0 ? 8 * ix == 16 * it : ix == 0;
    if (there) {
      if (r->hit.geomID != 0 || r->hit.instID[0] != (row == 0 ? built[1].moverID : built[1].fixedID)) return fail("a ray above an instance at its time must hit it");
      if (!(r->ray.tfar > 8.5f && r->ray.tfar < 9.6f)) return fail("distance"); /* the displaced limit surface of the +z face */
      if (row == 0) hitsMover++; else hitsFixed++;
    } else if (r->hit.geomID != RTC_INVALID_GEOMETRY_ID || r->ray.tfar != INFINITY)
      return fail("nothing is there at this time");
  }
  printf("%d rays: %d meet the mover where it is at their time, %d the static instance, records equal under both configs\n", NRAYS, hitsMover, hitsFixed);
  if (hitsMover != 5 || hitsFixed != NT) return fail("hit counts");
  { /* any hit: the mover occludes at its time only */
    struct RTCRay shadow[2];
    for (d = 0; d < 2; d++) {
      for (n = 0; n < 2; n++) {
        shadow[n] = rays[0][0].ray; /* x = 0.25, y = 0.125: where the mover is at time 0 */
        shadow[n].org_x = 0.25f; shadow[n].org_y = 0.125f; shadow[n].tfar = INFINITY;
        shadow[n].time = (float)n;
      }
      rtcOccluded1M(built[d].scene, &context, shadow, 2, sizeof(struct RTCRay));
      if (!(shadow[0].tfar < 0.f) || shadow[1].tfar != INFINITY) return fail("occluded");
    }
  }
  for (d = 0; d < 2; d++) {
    if (rtcGetDeviceError(built[d].device) != RTC_ERROR_NONE) return fail("trace");
    rtcReleaseScene(built[d].scene);
    rtcReleaseDevice(built[d].device);
  }
  printf("instance_subdiv_top_linear_min: ok\n");
  return 0;
}
