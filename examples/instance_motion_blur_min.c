/* Instance motion blur: a unit quad in the plane z = 0 over [0, 1] x [0, 1], committed once in a scene of its own and placed by ONE
 * RTC_GEOMETRY_TYPE_INSTANCE geometry with two time steps: at time 0 the instance is moved to z = 1, at time 1 to z = 3.  A ray along
 * +z from z = -1 with ray.time = 0, 0.5, 1 sees the instance under the interpolated transform and meets the quad at t = 2, 3, 4.
 * The hit's Ng is in the instance's LOCAL space; rtcamdGetGeometryWorld2Local gives the world-to-local matrix of the ray's time, whose
 * transposed linear part takes Ng to world space.
 *
 *   cc -std=c99 -I include examples/instance_motion_blur_min.c -L embree-compressed_amd/lib -lembree3 -o instance_motion_blur_min
 */
#include <embree3/rtcore.h>
#include <embree3/rtcore_amd.h>
#include <math.h>
#include <stdio.h>

static int fail(const char* what)
{
  printf("instance_motion_blur_min: FAILED (%s)\n", what);
  return 1;
}

int main(void)
{
  static const float quad[4][3] = {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f}, {1.f, 1.f, 0.f}, {0.f, 1.f, 0.f}};
  RTCDevice device = rtcNewDevice(NULL);
  RTCGeometry mesh, inst;
  RTCScene object, scene;
  struct RTCIntersectContext context;
  unsigned instID;
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

  /* the top scene: one instance with two time steps */
  scene = rtcNewScene(device);
  inst = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_INSTANCE);
  rtcSetGeometryInstancedScene(inst, object);
  rtcSetGeometryTimeStepCount(inst, 2);
  for (k = 0; k < 2; k++) {
    /* local-to-world of time step k, 3 x 4 row-major: the translation in the fourth column */
    const float xfm[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 1.f + 2.f * (float)k};
    rtcSetGeometryTransform(inst, (unsigned)k, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
  }
  rtcCommitGeometry(inst);
  instID = rtcAttachGeometry(scene, inst);
  rtcReleaseScene(object); /* the instance holds it */
  rtcCommitScene(scene);
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("commit");

  rtcInitIntersectContext(&context);
  for (k = 0; k < 3; k++) {
    const float time = 0.5f * (float)k;
    struct RTCRayHit rh;
    struct RTCRay shadow;
    float w2l[12], nx, ny, nz;
    rh.ray.org_x = 0.25f; rh.ray.org_y = 0.5f; rh.ray.org_z = -1.f;
    rh.ray.dir_x = 0.f; rh.ray.dir_y = 0.f; rh.ray.dir_z = 1.f;
    rh.ray.tnear = 0.f; rh.ray.tfar = INFINITY;
    rh.ray.time = time;
    rh.ray.mask = 0xFFFFFFFFu; rh.ray.id = (unsigned)k; rh.ray.flags = 0;
    rh.hit.geomID = RTC_INVALID_GEOMETRY_ID;
    rh.hit.primID = RTC_INVALID_GEOMETRY_ID;
    rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
    shadow = rh.ray;
    rtcIntersect1(scene, &context, &rh);
    if (rh.hit.geomID != 0 || rh.hit.primID != 0 || rh.hit.instID[0] != instID) return fail("ids");
    if (rh.ray.tfar != 2.f + (float)k) return fail("distance"); /* the plane is at z = 1 + 2 time */
    if (fabsf(rh.hit.u - 0.25f) > 1e-6f || fabsf(rh.hit.v - 0.5f) > 1e-6f) return fail("u, v");
    /* the world-to-local matrix of this ray's time (3 x 4 row-major): a translation by -(1 + 2 time) along z */
    rtcamdGetGeometryWorld2Local(inst, time, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, w2l);
    if (w2l[0] != 1.f || w2l[5] != 1.f || w2l[10] != 1.f || w2l[11] != -(1.f + 2.f * time)) return fail("world2local");
    /* Ng to world space: the transposed linear part of world2local applied to the local Ng */
    nx = w2l[0] * rh.hit.Ng_x + w2l[4] * rh.hit.Ng_y + w2l[8] * rh.hit.Ng_z;
    ny = w2l[1] * rh.hit.Ng_x + w2l[5] * rh.hit.Ng_y + w2l[9] * rh.hit.Ng_z;
    nz = w2l[2] * rh.hit.Ng_x + w2l[6] * rh.hit.Ng_y + w2l[10] * rh.hit.Ng_z;
    if (nx != 0.f || ny != 0.f || nz == 0.f) return fail("normal");
    shadow.tfar = 1.5f + (float)k;
    rtcOccluded1(scene, &context, &shadow);
    if (shadow.tfar < 0.f) return fail("occluded too early");
    shadow.tfar = 2.5f + (float)k;
    rtcOccluded1(scene, &context, &shadow);
    if (shadow.tfar >= 0.f) return fail("not occluded");
    printf("time %.1f: quad at t = %.1f\n", time, rh.ray.tfar);
  }
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("trace");
  rtcReleaseGeometry(inst);
  rtcReleaseScene(scene);
  rtcReleaseDevice(device);
  printf("instance_motion_blur_min: ok\n");
  return 0;
}
