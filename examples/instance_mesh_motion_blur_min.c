/* A moving mesh below instances: one triangle in the plane z = 0 that moves along z over two time steps - to z = 2 at time 1 - committed
 * once in a scene of its own (vertex motion blur: rtcSetGeometryTimeStepCount and one vertex buffer per step), and placed twice in the
 * top scene: by a static instance that lifts it by 1 along z, and by an instance with two time steps of its own (z + 1 at time 0, z + 3
 * at time 1) next to it at x + 100.  A ray's time passes into the instanced scene unchanged, so a ray along +z from z = -1 at
 * time = k / 8 meets the triangle of the first instance at t = 2 + 2 time and that of the second at t = 2 + 4 time.
 *
 *   cc -std=c99 -I include examples/instance_mesh_motion_blur_min.c -L embree-compressed_amd/lib -lembree3 -o instance_mesh_motion_blur_min
 */
#include <embree3/rtcore.h>
#include <math.h>
#include <stdio.h>

static int fail(const char* what)
{
  printf("instance_mesh_motion_blur_min: FAILED (%s)\n", what);
  return 1;
}

int main(void)
{
  static const float tri[3][3] = {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}};
  RTCDevice device = rtcNewDevice(NULL);
  RTCGeometry mesh, inst;
  RTCScene object, scene;
  struct RTCIntersectContext context;
  unsigned instID[2];
  unsigned* idx;
  int i, k, step;
  if (!device) return fail("rtcNewDevice");

  /* the instanced scene: one triangle with two time steps */
  mesh = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_TRIANGLE);
  rtcSetGeometryTimeStepCount(mesh, 2);
  for (step = 0; step < 2; step++) {
    float* v = (float*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_VERTEX, (unsigned)step, RTC_FORMAT_FLOAT3, 3 * sizeof(float), 3);
    if (!v) return fail("vertex buffer");
    for (k = 0; k < 3; k++) {
      v[3 * k + 0] = tri[k][0];
      v[3 * k + 1] = tri[k][1];
      v[3 * k + 2] = tri[k][2] + 2.f * (float)step;
    }
  }
  idx = (unsigned*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT3, 3 * sizeof(unsigned), 1);
  if (!idx) return fail("index buffer");
  idx[0] = 0; idx[1] = 1; idx[2] = 2;
  rtcCommitGeometry(mesh);
  object = rtcNewScene(device);
  rtcAttachGeometry(object, mesh);
  rtcReleaseGeometry(mesh);
  rtcCommitScene(object);

  /* the top scene: a static instance, and a moving one at x + 100 */
  scene = rtcNewScene(device);
  for (i = 0; i < 2; i++) {
    inst = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_INSTANCE);
    rtcSetGeometryInstancedScene(inst, object);
    rtcSetGeometryTimeStepCount(inst, i == 0 ? 1u : 2u);
    for (step = 0; step <= i; step++) {
      /* local-to-world of this time step, 3 x 4 row-major: the translation in the fourth column */
      const float xfm[12] = {1.f, 0.f, 0.f, 100.f * (float)i, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 1.f + 2.f * (float)step};
      rtcSetGeometryTransform(inst, (unsigned)step, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
    }
    rtcCommitGeometry(inst);
    instID[i] = rtcAttachGeometry(scene, inst);
    rtcReleaseGeometry(inst);
  }
  rtcReleaseScene(object); /* the instances hold it */
  rtcCommitScene(scene);
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("commit");

  rtcInitIntersectContext(&context);
  for (k = 0; k <= 8; k += 2) {
    const float time = (float)k / 8.f;
    for (i = 0; i < 2; i++) {
      /* the triangle is at z = 2 time in its scene; instance 0 adds 1, instance 1 adds 1 + 2 time */
      const float want = i == 0 ? 2.f + 2.f * time : 2.f + 4.f * time;
      struct RTCRayHit rh;
      struct RTCRay shadow;
      rh.ray.org_x = 0.25f + 100.f * (float)i; rh.ray.org_y = 0.5f; rh.ray.org_z = -1.f;
      rh.ray.dir_x = 0.f; rh.ray.dir_y = 0.f; rh.ray.dir_z = 1.f;
      rh.ray.tnear = 0.f; rh.ray.tfar = INFINITY;
      rh.ray.time = time;
      rh.ray.mask = 0xFFFFFFFFu; rh.ray.id = (unsigned)(2 * k + i); rh.ray.flags = 0;
      rh.hit.geomID = RTC_INVALID_GEOMETRY_ID;
      rh.hit.primID = RTC_INVALID_GEOMETRY_ID;
      rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
      shadow = rh.ray;
      rtcIntersect1(scene, &context, &rh);
      if (rh.hit.geomID != 0 || rh.hit.primID != 0 || rh.hit.instID[0] != instID[i]) return fail("ids");
      if (rh.ray.tfar != want) return fail("distance");
      if (fabsf(rh.hit.u - 0.25f) > 1e-6f || fabsf(rh.hit.v - 0.5f) > 1e-6f) return fail("u, v");
      if (rh.hit.Ng_x != 0.f || rh.hit.Ng_y != 0.f || rh.hit.Ng_z == 0.f) return fail("normal"); /* Ng is in the instance's local space */
      shadow.tfar = want - 0.5f;
      rtcOccluded1(scene, &context, &shadow);
      if (shadow.tfar < 0.f) return fail("occluded too early");
      shadow.tfar = want + 0.5f;
      rtcOccluded1(scene, &context, &shadow);
      if (shadow.tfar >= 0.f) return fail("not occluded");
      printf("time %.2f, instance %d: triangle at t = %.2f\n", time, i, rh.ray.tfar);
    }
  }
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("trace");
  rtcReleaseScene(scene);
  rtcReleaseDevice(device);
  printf("instance_mesh_motion_blur_min: ok\n");
  return 0;
}
