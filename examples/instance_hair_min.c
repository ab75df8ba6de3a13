/* Fur on a body, placed many times: ONE scene holds a quad "scalp" (the square [0, 4] x [0, 4] in the plane z = 0, geomID 0) and a tuft
 * of 16 flat Bezier curves rooted on it that bend towards -z (geomID 1).  The device is created with "inst_hair=1", which lets an
 * instanced scene hold line segments and flat curves beside its meshes.  Four RTC_GEOMETRY_TYPE_INSTANCE geometries place the scene:
 * instance 0 as it is, instance 1 moved to x = 16, instance 2 moved to x = 32 and scaled by 2, instance 3 with two time steps, moving
 * from x = 64 to x = 65 over the shutter.  A 32 x 32 grid of rays along +z is shot at every instance - laid over the instance where it
 * is (at time 0.5 for the moving one), so that all four grids are the same rays in the instanced scene's own space - and the hits are
 * counted per instance: so many on hair, so many on the scalp, the same numbers for every instance.
 *
 *   cc -std=c99 -I include examples/instance_hair_min.c -L embree-compressed_amd/lib -lembree3 -lm -o instance_hair_min
 */
#include <embree3/rtcore.h>
#include <math.h>
#include <stdio.h>

#define GRID 32
#define HAIRS 16

static int fail(const char* what)
{
  printf("instance_hair_min: FAILED (%s)\n", what);
  return 1;
}

int main(void)
{
  static const float scalp[4][3] = {{0.f, 0.f, 0.f}, {4.f, 0.f, 0.f}, {4.f, 4.f, 0.f}, {0.f, 4.f, 0.f}};
  /* where the instances are at the time their rays are shot, and their scale */
  static const float place[4] = {0.f, 16.f, 32.f, 64.5f}, scale[4] = {1.f, 1.f, 2.f, 1.f};
  static struct RTCRayHit rays[GRID * GRID];
  RTCDevice device = rtcNewDevice("inst_hair=1");
  RTCGeometry geom;
  RTCScene object, scene;
  struct RTCIntersectContext context;
  unsigned scalpID, hairID, instIDs[4];
  unsigned onHair[4], onScalp[4];
  float* v;
  unsigned* idx;
  int i, k;
  if (!device) return fail("rtcNewDevice");

  /* the instanced scene: the scalp ... */
  geom = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_QUAD);
  v = (float*)rtcSetNewGeometryBuffer(geom, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT3, 3 * sizeof(float), 4);
  idx = (unsigned*)rtcSetNewGeometryBuffer(geom, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT4, 4 * sizeof(unsigned), 1);
  if (!v || !idx) return fail("quad buffers");
  for (k = 0; k < 4; k++) {
    v[3 * k + 0] = scalp[k][0];
    v[3 * k + 1] = scalp[k][1];
    v[3 * k + 2] = scalp[k][2];
    idx[k] = (unsigned)k;
  }
  rtcCommitGeometry(geom);
  object = rtcNewScene(device);
  scalpID = rtcAttachGeometry(object, geom);
  rtcReleaseGeometry(geom);
  /* ... and the tuft: hair h is rooted at (0.5 + h % 4, 0.5 + h / 4, 0); four control points (x, y, z, radius) each */
  geom = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE);
  v = (float*)rtcSetNewGeometryBuffer(geom, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT4, 4 * sizeof(float), 4 * HAIRS);
  idx = (unsigned*)rtcSetNewGeometryBuffer(geom, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT, sizeof(unsigned), HAIRS);
  if (!v || !idx) return fail("curve buffers");
  for (k = 0; k < HAIRS; k++) {
    const float x = 0.5f + (float)(k % 4), y = 0.5f + (float)(k / 4);
    const float cp[4][4] = {{x, y, 0.f, 0.125f}, {x + 0.25f, y, -0.5f, 0.09375f}, {x + 0.25f, y + 0.25f, -1.f, 0.0625f}, {x, y + 0.375f, -1.5f, 0.03125f}};
    for (i = 0; i < 16; i++) v[16 * k + i] = cp[i / 4][i % 4];
    idx[k] = (unsigned)(4 * k);
  }
  rtcSetGeometryTessellationRate(geom, 8.f);
  rtcCommitGeometry(geom);
  hairID = rtcAttachGeometry(object, geom);
  rtcReleaseGeometry(geom);
  rtcCommitScene(object);
  if (scalpID != 0 || hairID != 1) return fail("geometry IDs");

  /* the top scene: four instances, the last one moving */
  scene = rtcNewScene(device);
  for (k = 0; k < 4; k++) {
    /* local-to-world, 3 x 4 row-major: the translation in the fourth column */
    const float s = scale[k];
    float xfm[12] = {s, 0.f, 0.f, place[k], 0.f, s, 0.f, 0.f, 0.f, 0.f, s, 0.f};
    geom = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_INSTANCE);
    rtcSetGeometryInstancedScene(geom, object);
    if (k == 3) {
      rtcSetGeometryTimeStepCount(geom, 2);
      xfm[3] = 64.f;
      rtcSetGeometryTransform(geom, 0, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
      xfm[3] = 65.f;
      rtcSetGeometryTransform(geom, 1, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
    } else
      rtcSetGeometryTransform(geom, 0, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
    rtcCommitGeometry(geom);
    instIDs[k] = rtcAttachGeometry(scene, geom);
    rtcReleaseGeometry(geom);
  }
  rtcReleaseScene(object); /* the instances hold it */
  rtcCommitScene(scene);
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("commit");

  rtcInitIntersectContext(&context);
  for (k = 0; k < 4; k++) {
    onHair[k] = onScalp[k] = 0;
    for (i = 0; i < GRID * GRID; i++) {
      struct RTCRayHit* rh = &rays[i];
      /* the grid in the instanced scene's space: cell centres of [0, 4] x [0, 4], from z = -4 */
      const float lx = ((float)(i % GRID) + 0.5f) * (4.f / GRID), ly = ((float)(i / GRID) + 0.5f) * (4.f / GRID);
      rh->ray.org_x = place[k] + scale[k] * lx; rh->ray.org_y = scale[k] * ly; rh->ray.org_z = scale[k] * -4.f;
      rh->ray.dir_x = 0.f; rh->ray.dir_y = 0.f; rh->ray.dir_z = 1.f;
      rh->ray.tnear = 0.f; rh->ray.tfar = INFINITY;
      rh->ray.time = 0.5f;
      rh->ray.mask = 0xFFFFFFFFu; rh->ray.id = (unsigned)i; rh->ray.flags = 0;
      rh->hit.geomID = rh->hit.primID = rh->hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
    }
    rtcIntersect1M(scene, &context, rays, GRID * GRID, sizeof(rays[0]));
    for (i = 0; i < GRID * GRID; i++) {
      const struct RTCRayHit* rh = &rays[i];
      if (rh->hit.geomID == RTC_INVALID_GEOMETRY_ID) return fail("a ray over the scalp missed"); /* the scalp lies behind every hair */
      if (rh->hit.instID[0] != instIDs[k]) return fail("instID");
      if (rh->hit.geomID == hairID) {
        if (!(rh->ray.tfar < scale[k] * 4.f) || rh->hit.primID >= HAIRS) return fail("hair hit"); /* in front of the scalp */
        onHair[k]++;
      } else {
        if (rh->hit.geomID != scalpID || rh->ray.tfar != scale[k] * 4.f) return fail("scalp hit");
        onScalp[k]++;
      }
    }
    printf("instance %u%s: %u rays end on hair, %u on the scalp\n", instIDs[k], k == 3 ? " (moving, time 0.5)" : k == 2 ? " (scaled by 2)" : "", onHair[k], onScalp[k]);
    if (onHair[k] == 0 || onHair[k] != onHair[0] || onScalp[k] != onScalp[0]) return fail("the instances disagree");
  }
  { /* a shadow ray that ends in front of the tuft is free, one that reaches it is not; between the instances nothing is hit */
    struct RTCRay shadow = rays[0].ray;
    struct RTCRayHit rh = rays[0];
    shadow.org_x = 0.5f; shadow.org_y = 0.5f; shadow.org_z = -4.f; /* over the root of hair 0 */
    shadow.tfar = 2.f;
    rtcOccluded1(scene, &context, &shadow);
    if (shadow.tfar < 0.f) return fail("occluded too early");
    shadow.tfar = 5.f;
    rtcOccluded1(scene, &context, &shadow);
    if (shadow.tfar >= 0.f) return fail("not occluded");
    rh.ray.org_x = 10.f; rh.ray.org_y = 0.5f; rh.ray.org_z = -4.f;
    rh.ray.tfar = INFINITY;
    rh.hit.geomID = rh.hit.primID = rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
    rtcIntersect1(scene, &context, &rh);
    if (rh.hit.geomID != RTC_INVALID_GEOMETRY_ID || rh.hit.instID[0] != RTC_INVALID_GEOMETRY_ID) return fail("miss");
  }
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("trace");
  rtcReleaseScene(scene);
  rtcReleaseDevice(device);
  printf("instance_hair_min: ok\n");
  return 0;
}
