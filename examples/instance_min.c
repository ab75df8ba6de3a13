/* Instancing through the embree3 API: one mesh - a unit square of two triangles in the plane z = 0 - committed once in its own scene
 * and placed 16 times on a 4 x 4 grid by RTC_GEOMETRY_TYPE_INSTANCE geometries: instance (i, j) is scaled by 2 and moved to
 * (4 i, 4 j, 1 + i + 4 j).  A ray along +z from z = -1 through the middle of cell (i, j) meets it at distance 2 + i + 4 j; the hit
 * names the mesh (geomID 0) and, in instID[0], the instance.
 *
 *   cc -std=c99 -I include examples/instance_min.c -L embree-compressed_amd/lib -lembree3 -o instance_min
 */
#include <embree3/rtcore.h>
#include <math.h>
#include <stdio.h>

static int fail(const char* what)
{
  printf("instance_min: FAILED (%s)\n", what);
  return 1;
}

int main(void)
{
  static const float corners[4][3] = {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f}, {1.f, 1.f, 0.f}, {0.f, 1.f, 0.f}};
  RTCDevice device = rtcNewDevice(NULL);
  RTCGeometry mesh;
  RTCScene object, scene;
  struct RTCIntersectContext context;
  unsigned instIDs[16];
  float* v;
  unsigned* idx;
  int i, j, k;
  if (!device) return fail("rtcNewDevice");

  /* the instanced scene: static triangle meshes only */
  mesh = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_TRIANGLE);
  v = (float*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT3, 3 * sizeof(float), 4);
  idx = (unsigned*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT3, 3 * sizeof(unsigned), 2);
  if (!v || !idx) return fail("buffers");
  for (k = 0; k < 4; k++) {
    v[3 * k + 0] = corners[k][0];
    v[3 * k + 1] = corners[k][1];
    v[3 * k + 2] = corners[k][2];
  }
  idx[0] = 0; idx[1] = 1; idx[2] = 2;
  idx[3] = 0; idx[4] = 2; idx[5] = 3;
  rtcCommitGeometry(mesh);
  object = rtcNewScene(device);
  rtcAttachGeometry(object, mesh);
  rtcReleaseGeometry(mesh);
  rtcCommitScene(object);

  /* the top scene: 16 instances of it */
  scene = rtcNewScene(device);
  for (j = 0; j < 4; j++) {
    for (i = 0; i < 4; i++) {
      /* local-to-world, 3 x 4 row-major: scale 2, then the translation in the fourth column */
      const float xfm[12] = {2.f, 0.f, 0.f, 4.f * (float)i, 0.f, 2.f, 0.f, 4.f * (float)j, 0.f, 0.f, 2.f, 1.f + (float)i + 4.f * (float)j};
      RTCGeometry inst = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_INSTANCE);
      rtcSetGeometryInstancedScene(inst, object);
      rtcSetGeometryTransform(inst, 0, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
      rtcCommitGeometry(inst);
      instIDs[4 * j + i] = rtcAttachGeometry(scene, inst);
      rtcReleaseGeometry(inst);
    }
  }
  rtcReleaseScene(object); /* the instances hold it */
  rtcCommitScene(scene);
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("commit");

  rtcInitIntersectContext(&context);
  for (j = 0; j < 4; j++) {
    for (i = 0; i < 4; i++) {
      struct RTCRayHit rh;
      struct RTCRay shadow;
      const float expect = 2.f + (float)i + 4.f * (float)j;
      rh.ray.org_x = 4.f * (float)i + 0.5f; rh.ray.org_y = 4.f * (float)j + 1.5f; rh.ray.org_z = -1.f;
      rh.ray.dir_x = 0.f; rh.ray.dir_y = 0.f; rh.ray.dir_z = 1.f;
      rh.ray.tnear = 0.f; rh.ray.tfar = INFINITY;
      rh.ray.time = 0.f;
      rh.ray.mask = 0xFFFFFFFFu; rh.ray.id = (unsigned)(4 * j + i); rh.ray.flags = 0;
      rh.hit.geomID = RTC_INVALID_GEOMETRY_ID;
      rh.hit.primID = RTC_INVALID_GEOMETRY_ID;
      rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
      shadow = rh.ray;
      rtcIntersect1(scene, &context, &rh);
      if (rh.hit.geomID != 0 || rh.hit.primID != 1) return fail("ids"); /* world (0.5, 1.5) is local (0.25, 0.75): the second triangle */
      if (rh.hit.instID[0] != instIDs[4 * j + i]) return fail("instID");
      if (fabsf(rh.ray.tfar - expect) > 1e-5f) return fail("distance");
      /* Ng is the normal in the instance's own space: along z */
      if (rh.hit.Ng_x != 0.f || rh.hit.Ng_y != 0.f || rh.hit.Ng_z == 0.f) return fail("normal");
      printf("instance %2u: hit at t = %.4f\n", rh.hit.instID[0], rh.ray.tfar);
      shadow.tfar = expect - 0.5f;
      rtcOccluded1(scene, &context, &shadow);
      if (shadow.tfar < 0.f) return fail("occluded too early");
      shadow.tfar = expect + 0.5f;
      rtcOccluded1(scene, &context, &shadow);
      if (shadow.tfar >= 0.f) return fail("not occluded");
    }
  }
  { /* between the instances nothing is hit */
    struct RTCRayHit rh;
    rh.ray.org_x = 3.f; rh.ray.org_y = 3.f; rh.ray.org_z = -1.f;
    rh.ray.dir_x = 0.f; rh.ray.dir_y = 0.f; rh.ray.dir_z = 1.f;
    rh.ray.tnear = 0.f; rh.ray.tfar = INFINITY; rh.ray.time = 0.f;
    rh.ray.mask = 0xFFFFFFFFu; rh.ray.id = 99; rh.ray.flags = 0;
    rh.hit.geomID = rh.hit.primID = rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
    rtcIntersect1(scene, &context, &rh);
    if (rh.hit.geomID != RTC_INVALID_GEOMETRY_ID || rh.hit.instID[0] != RTC_INVALID_GEOMETRY_ID) return fail("miss");
  }
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("trace");
  rtcReleaseScene(scene);
  rtcReleaseDevice(device);
  printf("instance_min: ok\n");
  return 0;
}
