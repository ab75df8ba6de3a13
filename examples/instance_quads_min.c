/* Instancing a scene that holds a quad mesh beside a triangle mesh: a unit quad in the plane z = 0 over [0, 1] x [0, 1] (geomID 0) and
 * a triangle in the plane z = 1 over x in [2, 3] (geomID 1), committed once in one scene and placed three times by
 * RTC_GEOMETRY_TYPE_INSTANCE geometries: instance k is moved to (10 k, 0, k).  A ray along +z from z = -1 meets the quad of instance
 * k at distance 1 + k and its triangle at 2 + k; the hit names the mesh (geomID), the primitive and, in instID[0], the instance.
 *
 *   cc -std=c99 -I include examples/instance_quads_min.c -L embree-compressed_amd/lib -lembree3 -o instance_quads_min
 */
#include <embree3/rtcore.h>
#include <math.h>
#include <stdio.h>

static int fail(const char* what)
{
  printf("instance_quads_min: FAILED (%s)\n", what);
  return 1;
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
  static const float quad[4][3] = {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f}, {1.f, 1.f, 0.f}, {0.f, 1.f, 0.f}};
  static const float tri[3][3] = {{2.f, 0.f, 1.f}, {3.f, 0.f, 1.f}, {2.f, 1.f, 1.f}};
  RTCDevice device = rtcNewDevice(NULL);
  RTCGeometry mesh;
  RTCScene object, scene;
  struct RTCIntersectContext context;
  unsigned instIDs[3], quadID, triID;
  float* v;
  unsigned* idx;
  int k;
  if (!device) return fail("rtcNewDevice");

  /* the instanced scene: a static quad mesh and a static triangle mesh */
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
  quadID = rtcAttachGeometry(object, mesh);
  rtcReleaseGeometry(mesh);
  mesh = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_TRIANGLE);
  v = (float*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT3, 3 * sizeof(float), 3);
  idx = (unsigned*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT3, 3 * sizeof(unsigned), 1);
  if (!v || !idx) return fail("triangle buffers");
  for (k = 0; k < 3; k++) {
    v[3 * k + 0] = tri[k][0];
    v[3 * k + 1] = tri[k][1];
    v[3 * k + 2] = tri[k][2];
    idx[k] = (unsigned)k;
  }
  rtcCommitGeometry(mesh);
  triID = rtcAttachGeometry(object, mesh);
  rtcReleaseGeometry(mesh);
  rtcCommitScene(object);
  if (quadID != 0 || triID != 1) return fail("geometry IDs");

  /* the top scene: three instances of it */
  scene = rtcNewScene(device);
  for (k = 0; k < 3; k++) {
    /* local-to-world, 3 x 4 row-major: the translation in the fourth column */
    const float xfm[12] = {1.f, 0.f, 0.f, 10.f * (float)k, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, (float)k};
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
    /* the quad, on either side of its v1 - v3 diagonal: u = x, v = y in the quad's own parametrisation on both */
    init_ray(&rh, 10.f * (float)k + 0.25f, 0.25f, (unsigned)(3 * k));
    rtcIntersect1(scene, &context, &rh);
    if (rh.hit.geomID != quadID || rh.hit.primID != 0 || rh.hit.instID[0] != instIDs[k]) return fail("quad ids");
    if (rh.ray.tfar != 1.f + (float)k) return fail("quad distance");
    if (fabsf(rh.hit.u - 0.25f) > 1e-6f || fabsf(rh.hit.v - 0.25f) > 1e-6f) return fail("quad u, v (triangle A)");
    init_ray(&rh, 10.f * (float)k + 0.75f, 0.5f, (unsigned)(3 * k + 1));
    shadow = rh.ray;
    rtcIntersect1(scene, &context, &rh);
    if (rh.hit.geomID != quadID || rh.hit.primID != 0 || rh.hit.instID[0] != instIDs[k]) return fail("quad ids (triangle B)");
    if (rh.ray.tfar != 1.f + (float)k) return fail("quad distance (triangle B)");
    if (fabsf(rh.hit.u - 0.75f) > 1e-6f || fabsf(rh.hit.v - 0.5f) > 1e-6f) return fail("quad u, v (triangle B)");
    if (rh.hit.Ng_x != 0.f || rh.hit.Ng_y != 0.f || rh.hit.Ng_z == 0.f) return fail("normal"); /* in the instance's own space: along z */
    shadow.tfar = 0.5f + (float)k;
    rtcOccluded1(scene, &context, &shadow);
    if (shadow.tfar < 0.f) return fail("occluded too early");
    shadow.tfar = 1.5f + (float)k;
    rtcOccluded1(scene, &context, &shadow);
    if (shadow.tfar >= 0.f) return fail("not occluded");
    /* the triangle of the same instance */
    init_ray(&rh, 10.f * (float)k + 2.25f, 0.25f, (unsigned)(3 * k + 2));
    rtcIntersect1(scene, &context, &rh);
    if (rh.hit.geomID != triID || rh.hit.primID != 0 || rh.hit.instID[0] != instIDs[k]) return fail("triangle ids");
    if (rh.ray.tfar != 2.f + (float)k) return fail("triangle distance");
    printf("instance %u: quad at t = %.1f, triangle at t = %.1f\n", instIDs[k], 1.f + (float)k, rh.ray.tfar);
  }
  { /* between the instances nothing is hit */
    struct RTCRayHit rh;
    init_ray(&rh, 5.f, 0.5f, 99);
    rtcIntersect1(scene, &context, &rh);
    if (rh.hit.geomID != RTC_INVALID_GEOMETRY_ID || rh.hit.instID[0] != RTC_INVALID_GEOMETRY_ID) return fail("miss");
  }
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("trace");
  rtcReleaseScene(scene);
  rtcReleaseDevice(device);
  printf("instance_quads_min: ok\n");
  return 0;
}
