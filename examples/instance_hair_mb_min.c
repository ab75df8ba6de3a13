/* Fur that sways over the shutter, placed many times: ONE scene holds a quad "scalp" (the square [0, 4] x [0, 4] in the plane z = 0,
 * geomID 0) and a tuft of 16 flat B-spline curves with TWO time steps rooted on it (geomID 1): at time 0 every hair leans towards +x,
 * at time 1 towards +y.  The device is created with "inst_hair=1,inst_hair_mb=1": the first key lets an instanced scene hold line
 * segments and flat curves beside its meshes, the second lets them have time steps.  Four RTC_GEOMETRY_TYPE_INSTANCE geometries place
 * the scene: instance 0 as it is, instance 1 moved to x = 16, instance 2 moved to x = 32 and scaled by 2, instance 3 with two transform
 * steps, moving from x = 64 to x = 65 over the shutter.  At the times 0, 0.5 and 1 a 32 x 32 grid of rays along +z is shot at every
 * instance - laid over the instance where it is at that time, so that all four grids are the same rays in the instanced scene's own
 * space - and the hits are counted per instance: so many on hair, so many on the scalp, the same numbers for every instance.  A probe
 * ray over the place where hair 0 is at time 0 ends on that hair at time 0 and on the scalp at time 1.
 *
 *   cc -std=c99 -I include examples/instance_hair_mb_min.c -L embree-compressed_amd/lib -lembree3 -lm -o instance_hair_mb_min
 */
#include <embree3/rtcore.h>
#include <math.h>
#include <stdio.h>

#define GRID 32
#define HAIRS 16

static int fail(const char* what)
{
  printf("instance_hair_mb_min: FAILED (%s)\n", what);
  return 1;
}

int main(void)
{
  static const float scalp[4][3] = {{0.f, 0.f, 0.f}, {4.f, 0.f, 0.f}, {4.f, 4.f, 0.f}, {0.f, 4.f, 0.f}};
  static const float times[3] = {0.f, 0.5f, 1.f};
  static const float scale[4] = {1.f, 1.f, 2.f, 1.f};
  static struct RTCRayHit rays[GRID * GRID];
  RTCDevice device = rtcNewDevice("inst_hair=1,inst_hair_mb=1");
  RTCGeometry geom;
  RTCScene object, scene;
  struct RTCIntersectContext context;
  unsigned scalpID, hairID, instIDs[4];
  unsigned onHair[4], onScalp[4];
  float* v;
  unsigned* idx;
  int i, k, step, t;
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
  /* ... and the tuft: hair h is rooted at (0.5 + h % 4, 0.5 + h / 4, 0); four B-spline control points (x, y, z, radius) per hair and time
   * step.  The curve runs from (p0 + 4 p1 + p2) / 6 to (p1 + 4 p2 + p3) / 6: from just above the root to half a unit beside it, one unit up */
  geom = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_FLAT_BSPLINE_CURVE);
  rtcSetGeometryTimeStepCount(geom, 2);
  idx = (unsigned*)rtcSetNewGeometryBuffer(geom, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT, sizeof(unsigned), HAIRS);
  if (!idx) return fail("curve index buffer");
  for (step = 0; step < 2; step++) {
    v = (float*)rtcSetNewGeometryBuffer(geom, RTC_BUFFER_TYPE_VERTEX, (unsigned)step, RTC_FORMAT_FLOAT4, 4 * sizeof(float), 4 * HAIRS);
    if (!v) return fail("curve vertex buffer");
    for (k = 0; k < HAIRS; k++) {
      const float x = 0.5f + (float)(k % 4), y = 0.5f + (float)(k / 4);
      const float lx = step == 0 ? 0.5f : 0.f, ly = step == 0 ? 0.f : 0.5f; /* the lean */
      const float cp[4][4] = {{x, y, 0.5f, 0.125f}, {x, y, 0.f, 0.125f}, {x + lx, y + ly, -1.f, 0.125f}, {x + 2.f * lx, y + 2.f * ly, -2.f, 0.125f}};
      for (i = 0; i < 16; i++) v[16 * k + i] = cp[i / 4][i % 4];
      idx[k] = (unsigned)(4 * k);
    }
  }
  rtcSetGeometryTessellationRate(geom, 8.f);
  rtcCommitGeometry(geom);
  hairID = rtcAttachGeometry(object, geom);
  rtcReleaseGeometry(geom);
  rtcCommitScene(object);
  if (scalpID != 0 || hairID != 1) return fail("geometry IDs");
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("commit of the instanced scene");

  /* the top scene: four instances, the last one moving */
  scene = rtcNewScene(device);
  for (k = 0; k < 4; k++) {
    /* local-to-world, 3 x 4 row-major: the translation in the fourth column */
    const float s = scale[k];
    float xfm[12] = {s, 0.f, 0.f, 16.f * (float)k, 0.f, s, 0.f, 0.f, 0.f, 0.f, s, 0.f};
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
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("commit"); /* (without inst_hair_mb=1: refused here) */

  rtcInitIntersectContext(&context);
  for (t = 0; t < 3; t++) {
    for (k = 0; k < 4; k++) {
      const float place = k == 3 ? 64.f + times[t] : 16.f * (float)k; /* where the instance is at this time */
      onHair[k] = onScalp[k] = 0;
      for (i = 0; i < GRID * GRID; i++) {
        struct RTCRayHit* rh = &rays[i];
        /* the grid in the instanced scene's space: cell centres of [0, 4] x [0, 4], from z = -4 */
        const float lx = ((float)(i % GRID) + 0.5f) * (4.f / GRID), ly = ((float)(i / GRID) + 0.5f) * (4.f / GRID);
        rh->ray.org_x = place + scale[k] * lx; rh->ray.org_y = scale[k] * ly; rh->ray.org_z = scale[k] * -4.f;
        rh->ray.dir_x = 0.f; rh->ray.dir_y = 0.f; rh->ray.dir_z = 1.f;
        rh->ray.tnear = 0.f; rh->ray.tfar = INFINITY;
        rh->ray.time = times[t];
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
      printf("time %.1f, instance %u%s: %u rays end on hair, %u on the scalp\n", times[t], instIDs[k], k == 3 ? " (moving)" : k == 2 ? " (scaled by 2)" : "", onHair[k], onScalp[k]);
      if (onHair[k] == 0 || onHair[k] != onHair[0] || onScalp[k] != onScalp[0]) return fail("the instances disagree");
    }
  }
  for (k = 0; k < 4; k++) { /* the probe: 0.4 beside the root of hair 0 in x - under the hair at time 0, beside it at time 1 */
    for (t = 0; t < 3; t += 2) {
      const float place = k == 3 ? 64.f + times[t] : 16.f * (float)k;
      struct RTCRayHit rh = rays[0];
      struct RTCRay shadow;
      rh.ray.org_x = place + scale[k] * 0.9f; rh.ray.org_y = scale[k] * 0.5f; rh.ray.org_z = scale[k] * -4.f;
      rh.ray.tfar = INFINITY;
      rh.ray.time = times[t];
      rh.hit.geomID = rh.hit.primID = rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
      shadow = rh.ray;
      shadow.tfar = scale[k] * 3.5f; /* ends between the hair and the scalp */
      rtcIntersect1(scene, &context, &rh);
      rtcOccluded1(scene, &context, &shadow);
      if (rh.hit.instID[0] != instIDs[k]) return fail("probe instID");
      if (t == 0 && (rh.hit.geomID != hairID || rh.hit.primID != 0 || !(shadow.tfar < 0.f))) return fail("probe at time 0");
      if (t == 2 && (rh.hit.geomID != scalpID || rh.ray.tfar != scale[k] * 4.f || shadow.tfar < 0.f)) return fail("probe at time 1");
    }
  }
  if (rtcGetDeviceError(device) != RTC_ERROR_NONE) return fail("trace");
  rtcReleaseScene(scene);
  rtcReleaseDevice(device);
  printf("instance_hair_mb_min: ok\n");
  return 0;
}
