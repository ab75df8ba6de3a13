/* Instances of a subdivision mesh through the embree3 API: a cube - six quads, Catmull-Clark - committed once in its own scene at
 * tessellation level 4 and placed three times by RTC_GEOMETRY_TYPE_INSTANCE geometries: instance k is scaled by s = 1, 2, 1/2 and moved
 * to x = 8 k.  A ray along +z from z = -10 through the middle of instance k meets the limit surface of the cube's -z face at
 * t = 10 - s h, with the same local height h for all three; the hit names the mesh (geomID 0), the face (primID) and, in instID[0], the
 * instance.  An instanced scene holds either subdivision meshes only, as here, or triangle and quad meshes; a top scene may place both.
 *
 *   cc -std=c99 -I include examples/instance_subdiv_min.c -L embree-compressed_amd/lib -lembree3 -lm -o instance_subdiv_min
 *   ./instance_subdiv_min [device config, e.g. subdiv_accel=bvh4.compressed.leaf]
 */
#include <embree3/rtcore.h>
#include <math.h>
#include <stdio.h>

static int fail(const char* what)
{
  printf("instance_subdiv_min: FAILED (%s)\n", what);
  return 1;
}

static void init_ray(struct RTCRayHit* rh, float x, float y, unsigned id)
{
  rh->ray.org_x = x; rh->ray.org_y = y; rh->ray.org_z = -10.f;
  rh->ray.dir_x = 0.f; rh->ray.dir_y = 0.f; rh->ray.dir_z = 1.f;
  rh->ray.tnear = 0.f; rh->ray.tfar = INFINITY; rh->ray.time = 0.f;
  rh->ray.mask = 0xFFFFFFFFu; rh->ray.id = id; rh->ray.flags = 0;
  rh->hit.geomID = rh->hit.primID = rh->hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
}

int main(int argc, char** argv)
{
  static const float corners[8][3] = {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}, {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
  static const unsigned faces[24] = {0, 4, 5, 1, 1, 5, 7, 3, 3, 7, 6, 2, 2, 6, 4, 0, 4, 6, 7, 5, 0, 1, 3, 2};
  static const float scales[3] = {1.f, 2.f, 0.5f};
  RTCDevice device = rtcNewDevice(argc > 1 ? argv[1] : NULL);
  RTCGeometry mesh;
  RTCScene object, scene;
  struct RTCIntersectContext context;
  unsigned instIDs[3];
  float heights[3];
  float* v;
  float* level;
  unsigned* idx;
  unsigned* sizes;
  int k;
  if (!device) return fail("rtcNewDevice");

  /* the instanced scene: subdivision meshes only */
  mesh = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_SUBDIVISION);
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
  rtcCommitGeometry(mesh);
  object = rtcNewScene(device);
  rtcAttachGeometry(object, mesh);
  rtcReleaseGeometry(mesh);
  rtcSetSceneLevels(object, 4, 2); /* 16 x 16 quads per face; compression level 2 for the compressed accels */
  rtcCommitScene(object);
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("commit of the instanced scene");

  /* the top scene: three instances of it */
  scene = rtcNewScene(device);
  for (k = 0; k < 3; k++) {
    /* local-to-world, 3 x 4 row-major: the scale, then the translation in the fourth column */
    const float s = scales[k];
    const float xfm[12] = {s, 0.f, 0.f, 8.f * (float)k, 0.f, s, 0.f, 0.f, 0.f, 0.f, s, 0.f};
    RTCGeometry inst = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_INSTANCE);
    rtcSetGeometryInstancedScene(inst, object);
    rtcSetGeometryTransform(inst, 0, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
    rtcCommitGeometry(inst);
    instIDs[k] = rtcAttachGeometry(scene, inst);
    rtcReleaseGeometry(inst);
  }
  rtcReleaseScene(object); /* the instances hold it */
  rtcCommitScene(scene);
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("commit");

  rtcInitIntersectContext(&context);
  for (k = 0; k < 3; k++) {
    struct RTCRayHit rh;
    struct RTCRay shadow;
    /* a little off the middle of the face, the same local point in every instance */
    init_ray(&rh, 8.f * (float)k + 0.125f * scales[k], 0.0625f * scales[k], (unsigned)k);
    shadow = rh.ray;
    rtcIntersect1(scene, &context, &rh);
    printf("instance %u: instID %u geomID %u primID %u t = %.5f\n", (unsigned)k, rh.hit.instID[0], rh.hit.geomID, rh.hit.primID, rh.ray.tfar);
    if (rh.hit.instID[0] != instIDs[k]) return fail("instID");
    if (rh.hit.geomID != 0 || rh.hit.primID != 3) return fail("ids"); /* face 3 (vertices 2 6 4 0) lies in z = -1 */
    heights[k] = (10.f - rh.ray.tfar) / scales[k];
    if (!(heights[k] > 0.4f && heights[k] < 1.001f)) return fail("distance"); /* the limit surface lies inside the cube */
    shadow.tfar = rh.ray.tfar - 0.25f * scales[k];
    rtcOccluded1(scene, &context, &shadow);
    if (shadow.tfar < 0.f) return fail("occluded too early");
    shadow.tfar = INFINITY;
    rtcOccluded1(scene, &context, &shadow);
    if (shadow.tfar >= 0.f) return fail("not occluded");
  }
  for (k = 1; k < 3; k++)
    if (fabsf(heights[k] - heights[0]) > 0.05f) return fail("the instances disagree in the local height"); /* (the compressed accels quantize heights) */
  { /* between the instances nothing is hit */
    struct RTCRayHit rh;
    init_ray(&rh, 4.f, 0.f, 99);
    rtcIntersect1(scene, &context, &rh);
    if (rh.hit.geomID != RTC_INVALID_GEOMETRY_ID || rh.hit.instID[0] != RTC_INVALID_GEOMETRY_ID) return fail("miss");
  }
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("trace");
  rtcReleaseScene(scene);
  rtcReleaseDevice(device);
  printf("instance_subdiv_min: ok\n");
  return 0;
}
