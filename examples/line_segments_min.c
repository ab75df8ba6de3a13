/*
 * Line segments through the plain C API: a small tuft of three strands (RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE: FLOAT4 vertices x, y, z,
 * radius; one UINT per segment, the index of its first vertex) beside one triangle.  Rays along +z with known answers go through
 * rtcIntersect1, rtcOccluded1 and one rtcIntersect1M stream: a hit on a segment reports the depth of the point on the segment's AXIS
 * (the curve is flat: a ribbon that faces the ray), u along the segment, v = 0 and Ng = v1 - v0, not normalised.  rtcInterpolate gives
 * the point on the axis and the interpolated radius.
 *
 * An application should try the geometry type: RTC_DEVICE_PROPERTY_CURVE_GEOMETRY_SUPPORTED speaks for all five curve types, and the
 * round Bezier and B-spline ones are taken only on a device created with round_curves=1 (round_curve_min.c): it is 0 here.
 *
 * C99 on purpose:
 *   gcc -std=c99 -Iinclude examples/line_segments_min.c -Lembree-compressed_amd/lib -lembree3 -lm \
 *       -Wl,-rpath,$PWD/embree-compressed_amd/lib -o /tmp/line_segments_min
 * argv[1]: device config (e.g. "line_accel=bvh8.line4i"); argv[2] = "robust": RTC_SCENE_FLAG_ROBUST (robust traversal)
 */
#include <embree3/rtcore.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_errors = 0;
static void error_handler(void* user, enum RTCError code, const char* str)
{
  (void)user;
  if (code == RTC_ERROR_NONE) return;
  fprintf(stderr, "embree error %d: %s\n", (int)code, str ? str : "");
  g_errors++;
}

/* three strands along y at x = -1, 0, 1: two segments each, thinner towards the tip */
static const float strands[9][4] = {{-1.f, 0.f, 0.f, 0.125f}, {-1.f, 1.f, 0.f, 0.125f}, {-1.f, 2.f, 0.f, 0.0625f},
                                    {0.f, 0.f, 0.f, 0.125f},  {0.f, 1.f, 0.f, 0.125f},  {0.f, 2.f, 0.f, 0.0625f},
                                    {1.f, 0.f, 0.f, 0.125f},  {1.f, 1.f, 0.f, 0.125f},  {1.f, 2.f, 0.f, 0.0625f}};
static const unsigned first_vertex[6] = {0, 1, 3, 4, 6, 7};

struct Case { float x, y; int geom; unsigned prim; float u; };

static int run(const char* cfg, int robust)
{
  RTCDevice dev = rtcNewDevice(cfg);
  if (!dev) { fprintf(stderr, "rtcNewDevice failed: error %d\n", (int)rtcGetDeviceError(NULL)); return 2; }
  rtcSetDeviceErrorFunction(dev, error_handler, NULL);
  RTCScene scene = rtcNewScene(dev);
  if (robust) rtcSetSceneFlags(scene, RTC_SCENE_FLAG_ROBUST);

  RTCGeometry tri = rtcNewGeometry(dev, RTC_GEOMETRY_TYPE_TRIANGLE);
  float* tv = (float*)rtcSetNewGeometryBuffer(tri, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT3, 3 * sizeof(float), 3);
  const float pos[3][3] = {{2, 0, 0}, {3, 0, 0}, {2, 1, 0}};
  memcpy(tv, pos, sizeof(pos));
  unsigned* ti = (unsigned*)rtcSetNewGeometryBuffer(tri, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT3, 3 * sizeof(unsigned), 1);
  ti[0] = 0; ti[1] = 1; ti[2] = 2;
  rtcCommitGeometry(tri);
  const unsigned triID = rtcAttachGeometry(scene, tri);

  RTCGeometry tuft = rtcNewGeometry(dev, RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE);
  if (!tuft) { fprintf(stderr, "this library does not take RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE\n"); return 2; }
  rtcSetSharedGeometryBuffer(tuft, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT4, strands, 0, 4 * sizeof(float), 9);
  unsigned* li = (unsigned*)rtcSetNewGeometryBuffer(tuft, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT, sizeof(unsigned), 6);
  memcpy(li, first_vertex, sizeof(first_vertex));
  rtcCommitGeometry(tuft);
  const unsigned tuftID = rtcAttachGeometry(scene, tuft);
  rtcCommitScene(scene);

  /* x, y of a ray from z = -4 along +z; geometry (-1: a miss), primID and u of its hit */
  const struct Case cases[] = {{0.f, 0.5f, 1, 2, 0.5f},          /* the middle strand's lower segment, on its axis */
                               {-1.f, 1.5f, 1, 1, 0.5f},         /* the left strand's tip segment */
                               {1.0625f, 0.25f, 1, 4, 0.25f},    /* 1/16 beside the right strand's axis: inside the radius 1/8 */
                               {1.25f, 0.25f, -1, 0, 0.f},       /* 1/4 beside it: outside */
                               {0.09375f, 1.75f, -1, 0, 0.f},    /* the tip segment at u = 3/4 has radius 5/64 < 6/64 */
                               {0.0625f, 1.75f, 1, 3, 0.75f},    /* ... > 4/64 */
                               {0.5f, 0.5f, -1, 0, 0.f},         /* between two strands */
                               {2.25f, 0.25f, 0, 0, 0.f}};       /* the triangle */
  enum { N = sizeof(cases) / sizeof(cases[0]) };
  struct RTCRayHit* stream = NULL;
  if (posix_memalign((void**)&stream, 16, sizeof(struct RTCRayHit) * N)) return 2;
  struct RTCIntersectContext ctx;
  rtcInitIntersectContext(&ctx);
  int bad = 0, onLines = 0;
  for (int pass = 0; pass < 2; pass++) { /* 0: rtcIntersect1 / rtcOccluded1 per ray, 1: the same rays as one rtcIntersect1M stream */
    if (pass == 1) rtcIntersect1M(scene, &ctx, stream, N, sizeof(struct RTCRayHit));
    for (int i = 0; i < (int)N; i++) {
      const struct Case c = cases[i];
      struct RTCRayHit rh;
      if (pass == 0) {
        memset(&rh, 0, sizeof(rh));
        rh.ray.org_x = c.x; rh.ray.org_y = c.y; rh.ray.org_z = -4.f;
        rh.ray.dir_z = 1.f;
        rh.ray.tnear = 0.f; rh.ray.tfar = INFINITY; rh.ray.mask = 0xFFFFFFFFu;
        rh.hit.geomID = rh.hit.primID = rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
        stream[i] = rh;
        rtcIntersect1(scene, &ctx, &rh);
      } else
        rh = stream[i];
      const unsigned wantGeom = c.geom < 0 ? RTC_INVALID_GEOMETRY_ID : (c.geom == 0 ? triID : tuftID);
      if (rh.hit.geomID != wantGeom) { fprintf(stderr, "ray %d: geomID %u, expected %u\n", i, rh.hit.geomID, wantGeom); bad++; continue; }
      if (c.geom < 0) { if (rh.ray.tfar != INFINITY) bad++; continue; }
      if (fabsf(rh.ray.tfar - 4.f) > 1e-6f) { fprintf(stderr, "ray %d: t %g\n", i, rh.ray.tfar); bad++; }
      if (c.geom == 0) continue;
      onLines++;
      /* the depth of the axis point (4, not 4 - radius), u along the segment, v = 0, Ng = v1 - v0 = (0, 1, 0) */
      if (rh.hit.primID != c.prim || fabsf(rh.hit.u - c.u) > 1e-6f || rh.hit.v != 0.f || rh.hit.Ng_x != 0.f || rh.hit.Ng_y != 1.f || rh.hit.Ng_z != 0.f) {
        fprintf(stderr, "ray %d: primID %u u %g v %g Ng %g %g %g\n", i, rh.hit.primID, rh.hit.u, rh.hit.v, rh.hit.Ng_x, rh.hit.Ng_y, rh.hit.Ng_z);
        bad++;
      }
      if (pass == 1) continue;
      /* the point on the axis and the radius there */
      float P[4], du[4], dv[4];
      rtcInterpolate1(tuft, rh.hit.primID, rh.hit.u, rh.hit.v, RTC_BUFFER_TYPE_VERTEX, 0, P, du, dv, 4);
      const float* a = strands[first_vertex[c.prim]];
      const float* b = strands[first_vertex[c.prim] + 1];
      for (int k = 0; k < 4; k++)
        if (fabsf(P[k] - ((1.f - c.u) * a[k] + c.u * b[k])) > 1e-6f || du[k] != b[k] - a[k] || dv[k] != 0.f) bad++;
      /* a shadow ray back through the segment is occluded, one that stops short is not */
      struct RTCRay sh;
      memset(&sh, 0, sizeof(sh));
      sh.org_x = c.x; sh.org_y = c.y; sh.org_z = 4.f; sh.dir_z = -1.f; sh.tnear = 0.f; sh.tfar = INFINITY; sh.mask = 0xFFFFFFFFu;
      rtcOccluded1(scene, &ctx, &sh);
      if (sh.tfar != -INFINITY) bad++;
      sh.tfar = 3.5f;
      rtcOccluded1(scene, &ctx, &sh);
      if (sh.tfar != 3.5f) bad++;
    }
  }
  free(stream);
  rtcReleaseGeometry(tri);
  rtcReleaseGeometry(tuft);
  rtcReleaseScene(scene);
  rtcReleaseDevice(dev);
  printf("line_segments_min (%s%s): %d rays, %d hits on segments, %d bad\n", cfg, robust ? " robust" : "", 2 * (int)N, onLines, bad);
  return bad;
}

int main(int argc, char** argv)
{
  int bad = 0;
  if (argc > 1) bad = run(argv[1], argc > 2 && strcmp(argv[2], "robust") == 0);
  else {
    bad += run("", 0);                       /* fast traversal */
    bad += run("", 1);                       /* robust traversal */
    bad += run("line_accel=bvh8.line4i", 0);
  }
  if (bad || g_errors) { printf("line_segments_min: FAILED (%d bad, %d errors)\n", bad, g_errors); return 1; }
  printf("line_segments_min: ok\n");
  return 0;
}
