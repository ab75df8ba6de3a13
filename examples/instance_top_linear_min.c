/* A fast-moving instance under time-dependent top-level boxes (device config inst_bounds=linear): a unit quad in the plane z = 0,
 * committed once in a scene of its own and placed by ONE RTC_GEOMETRY_TYPE_INSTANCE geometry with two time steps that carry it 64
 * units along x over the shutter, beside a static instance of the same scene.  The box of the mover swept over the shutter is 65 units
 * long; under inst_bounds=linear the top-level tree keeps its box at time 0 and at time 1 and a ray is tested against the box at ITS
 * time: a ray down -z above where the quad is at time t meets it at ray.time = t and passes at ray.time = 1 - t without entering the
 * instance.  Hits are what they are under inst_bounds=swept (the default); only the work differs.  The scene statistics name the accel
 * kind 32 / 33.
 *
 *   cc -std=c99 -I include examples/instance_top_linear_min.c -L embree-compressed_amd/lib -lembree3 -o instance_top_linear_min
 */
#include <embree3/rtcore.h>
#include <embree3/rtcore_amd.h>
#include <math.h>
#include <stdio.h>

static int fail(const char* what)
{
  printf("instance_top_linear_min: FAILED (%s)\n", what);
  return 1;
}

int main(void)
{
  static const float quad[4][3] = {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f}, {1.f, 1.f, 0.f}, {0.f, 1.f, 0.f}};
  RTCDevice device = rtcNewDevice("inst_bounds=linear");
  RTCGeometry mesh, mover, fixed;
  RTCScene object, scene;
  struct RTCIntersectContext context;
  struct RTCAMDSceneStats stats;
  unsigned moverID, fixedID;
  float* v;
  unsigned* idx;
  int k;
  if (!device) return fail("rtcNewDevice");

  /* the instanced scene: one static quad */
  mesh = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_QUAD);
  v = (float*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT3, 3 * sizeof(float), 4);
  idx = (unsigned*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT4, 4 * sizeof(unsigned), 1);
  if (!v || !idx) return fail("quad buffers");
  for (k = 0; k < 4; k++) {
    v[3 * k + 0] = quad[k][0];
    v[3 * k + 1] = quad[k][1];
    v[3 * k + 2] = quad[k][2];
    idx[k] = (unsigned)k;
  }
  rtcCommitGeometry(mesh);
  object = rtcNewScene(device);
  rtcAttachGeometry(object, mesh);
  rtcReleaseGeometry(mesh);
  rtcCommitScene(object);

  /* the top scene: the mover, from x = 0 to x = 64 over the shutter, and a static instance at y = 4 */
  scene = rtcNewScene(device);
  mover = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_INSTANCE);
  rtcSetGeometryInstancedScene(mover, object);
  rtcSetGeometryTimeStepCount(mover, 2);
  for (k = 0; k < 2; k++) {
    /* local-to-world of time step k, 3 x 4 row-major: the translation in the fourth column */
    const float xfm[12] = {1.f, 0.f, 0.f, 64.f * (float)k, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    rtcSetGeometryTransform(mover, (unsigned)k, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
  }
  rtcCommitGeometry(mover);
  moverID = rtcAttachGeometry(scene, mover);
  fixed = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_INSTANCE);
  rtcSetGeometryInstancedScene(fixed, object);
  {
    const float xfm[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 4.f, 0.f, 0.f, 1.f, 0.f};
    rtcSetGeometryTransform(fixed, 0, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
  }
  rtcCommitGeometry(fixed);
  fixedID = rtcAttachGeometry(scene, fixed);
  rtcReleaseScene(object); /* the instances hold it */
  rtcCommitScene(scene);
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("commit");
  stats.byteSize = sizeof(stats);
  rtcamdGetSceneStats(scene, &stats);
  if (stats.accelKind != 32 && stats.accelKind != 33) return fail("accel kind: a moving instance under inst_bounds=linear gives 32 / 33");
  printf("accel kind %u, %u instances\n", stats.accelKind, (unsigned)stats.leafCount);

  rtcInitIntersectContext(&context);
  for (k = 0; k <= 4; k++) {
    const float at = 0.25f * (float)k; /* the ray goes down above where the quad is at time `at` */
    int pass;
    for (pass = 0; pass < 2; pass++) {
      const float time = pass ? 1.f - at : at;
      struct RTCRayHit rh;
      rh.ray.org_x = 64.f * at + 0.25f; rh.ray.org_y = 0.5f; rh.ray.org_z = 3.f;
      rh.ray.dir_x = 0.f; rh.ray.dir_y = 0.f; rh.ray.dir_z = -1.f;
      rh.ray.tnear = 0.f; rh.ray.tfar = INFINITY;
      rh.ray.time = time;
      rh.ray.mask = 0xFFFFFFFFu; rh.ray.id = (unsigned)k; rh.ray.flags = 0;
      rh.hit.geomID = RTC_INVALID_GEOMETRY_ID;
      rh.hit.primID = RTC_INVALID_GEOMETRY_ID;
      rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
      rtcIntersect1(scene, &context, &rh);
      if (time == at) { /* (k = 2: both passes are at time 0.5) */
        if (rh.hit.geomID != 0 || rh.hit.instID[0] != moverID || rh.ray.tfar != 3.f) return fail("the mover at the ray's time");
        if (fabsf(rh.hit.u - 0.25f) > 1e-6f || fabsf(rh.hit.v - 0.5f) > 1e-6f) return fail("u, v");
      } else if (rh.hit.geomID != RTC_INVALID_GEOMETRY_ID || rh.ray.tfar != INFINITY)
        return fail("the mover is elsewhere at this time");
    }
    printf("x = %5.2f: the quad is there at time %.2f only\n", 64.f * at + 0.25f, at);
  }
  { /* the static instance is where it is at every time */
    struct RTCRay shadow;
    shadow.org_x = 0.5f; shadow.org_y = 4.5f; shadow.org_z = 3.f;
    shadow.dir_x = 0.f; shadow.dir_y = 0.f; shadow.dir_z = -1.f;
    shadow.tnear = 0.f; shadow.tfar = INFINITY;
    shadow.time = 0.7f;
    shadow.mask = 0xFFFFFFFFu; shadow.id = 0; shadow.flags = 0;
    rtcOccluded1(scene, &context, &shadow);
    if (shadow.tfar >= 0.f) return fail("static instance not occluding");
  }
  (void)fixedID;
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("trace");
  rtcReleaseGeometry(mover);
  rtcReleaseGeometry(fixed);
  rtcReleaseScene(scene);
  rtcReleaseDevice(device);
  printf("instance_top_linear_min: ok\n");
  return 0;
}
