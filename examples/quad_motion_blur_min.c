/* Motion blur on a quad mesh through the embree3 API: one unit quad that moves from z = 0 (time 0) to z = 2 (time 1) while it
 * slides by 0.5 along x; rays along +z from z = -1 at three times meet it at distance 1 + 2 * time, on its first triangle
 * (v0, v1, v3) or on its second (v2, v1, v3), and report the quad's own u / v on both.
 *
 *   cc -std=c99 -I include examples/quad_motion_blur_min.c -L embree-compressed_amd/lib -lembree3 -o quad_motion_blur_min
 */
#include <embree3/rtcore.h>
#include <math.h>
#include <stdio.h>

static int fail(const char* what)
{
  printf("quad_motion_blur_min: FAILED (%s)\n", what);
  return 1;
}

int main(void)
{
  static const float corners[4][2] = {{0.f, 0.f}, {1.f, 0.f}, {1.f, 1.f}, {0.f, 1.f}};
  static const float times[3] = {0.f, 0.25f, 1.f};
  /* where the rays meet the quad, in the quad's own parametrisation: u + v < 1 is the first triangle, u + v > 1 the second */
  static const float uv[2][2] = {{0.25f, 0.5f}, {0.75f, 0.625f}};
  RTCDevice device = rtcNewDevice(NULL);
  RTCGeometry geom;
  RTCScene scene;
  struct RTCIntersectContext context;
  unsigned* idx;
  int step, i, k;
  if (!device) return fail("rtcNewDevice");

  geom = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_QUAD);
  rtcSetGeometryTimeStepCount(geom, 2);
  for (step = 0; step < 2; step++) { /* vertex buffer slot = time step */
    float* v = (float*)rtcSetNewGeometryBuffer(geom, RTC_BUFFER_TYPE_VERTEX, (unsigned)step, RTC_FORMAT_FLOAT3, 3 * sizeof(float), 4);
    if (!v) return fail("vertex buffer");
    for (i = 0; i < 4; i++) {
      v[3 * i + 0] = corners[i][0] + (step ? 0.5f : 0.f);
      v[3 * i + 1] = corners[i][1];
      v[3 * i + 2] = step ? 2.f : 0.f;
    }
  }
  idx = (unsigned*)rtcSetNewGeometryBuffer(geom, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT4, 4 * sizeof(unsigned), 1);
  if (!idx) return fail("index buffer");
  idx[0] = 0; idx[1] = 1; idx[2] = 2; idx[3] = 3;
  rtcCommitGeometry(geom);

  scene = rtcNewScene(device);
  rtcAttachGeometry(scene, geom);
  rtcReleaseGeometry(geom);
  rtcCommitScene(scene);
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("commit");

  rtcInitIntersectContext(&context);
  for (i = 0; i < 3; i++) {
    for (k = 0; k < 2; k++) {
      struct RTCRayHit rh;
      struct RTCRay shadow;
      const float expect = 1.f + 2.f * times[i];
      rh.ray.org_x = uv[k][0] + 0.5f * times[i]; /* the quad has moved by 0.5 * time along x */
      rh.ray.org_y = uv[k][1];
      rh.ray.org_z = -1.f;
      rh.ray.dir_x = 0.f; rh.ray.dir_y = 0.f; rh.ray.dir_z = 1.f;
      rh.ray.tnear = 0.f; rh.ray.tfar = INFINITY;
      rh.ray.time = times[i];
      rh.ray.mask = 0xFFFFFFFFu; rh.ray.id = (unsigned)(2 * i + k); rh.ray.flags = 0;
      rh.hit.geomID = RTC_INVALID_GEOMETRY_ID;
      rh.hit.primID = RTC_INVALID_GEOMETRY_ID;
      rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
      shadow = rh.ray;
      rtcIntersect1(scene, &context, &rh);
      if (rh.hit.geomID != 0 || rh.hit.primID != 0) return fail("ids");
      if (fabsf(rh.ray.tfar - expect) > 1e-5f) return fail("distance");
      if (fabsf(rh.hit.u - uv[k][0]) > 1e-5f || fabsf(rh.hit.v - uv[k][1]) > 1e-5f) return fail("u / v");
      printf("time %.2f, %s triangle: hit at t = %.4f, u = %.3f, v = %.3f\n", times[i], k ? "second" : "first", rh.ray.tfar, rh.hit.u, rh.hit.v);
      /* a shadow ray that ends in front of the quad at this time is not occluded, one that reaches it is */
      shadow.tfar = expect - 0.5f;
      rtcOccluded1(scene, &context, &shadow);
      if (shadow.tfar < 0.f) return fail("occluded too early");
      shadow.tfar = expect + 0.5f;
      rtcOccluded1(scene, &context, &shadow);
      if (shadow.tfar >= 0.f) return fail("not occluded");
    }
  }
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("trace");
  rtcReleaseScene(scene);
  rtcReleaseDevice(device);
  printf("quad_motion_blur_min: ok\n");
  return 0;
}
