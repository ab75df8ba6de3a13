/*
 * Motion blur on line segments through the plain C API: a tuft of three strands (RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE) with TWO time
 * steps - rtcSetGeometryTimeStepCount(geometry, 2) and one FLOAT4 vertex buffer (x, y, z, radius) per step in the vertex slots 0 and 1.
 * Over the shutter the tuft moves by 8 along x and its strands get twice as thick; a ray sees it where it is at ray.time, with the
 * radius interpolated like a coordinate.  Rays along +z with known answers go through rtcIntersect1, rtcOccluded1 and one
 * rtcIntersect1M stream; rtcInterpolate reads one time step's buffer by its slot.
 *
 * C99 on purpose:
 *   gcc -std=c99 -Iinclude examples/line_motion_blur_min.c -Lembree-compressed_amd/lib -lembree3 -lm \
 *       -Wl,-rpath,$PWD/embree-compressed_amd/lib -o /tmp/line_motion_blur_min
 * argv[1]: device config (e.g. "mb_bounds=linear": time-dependent node boxes, the better choice for fast movers; or
 * "line_accel_mb=bvh8.line4imb"); argv[2] = "robust": RTC_SCENE_FLAG_ROBUST (robust traversal)
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

/* three strands along y at x = -1, 0, 1, two segments each; step 1: moved by 8 along x, radii doubled */
static float step0[9][4] = {{-1.f, 0.f, 0.f, 0.125f}, {-1.f, 1.f, 0.f, 0.125f}, {-1.f, 2.f, 0.f, 0.0625f},
                            {0.f, 0.f, 0.f, 0.125f},  {0.f, 1.f, 0.f, 0.125f},  {0.f, 2.f, 0.f, 0.0625f},
                            {1.f, 0.f, 0.f, 0.125f},  {1.f, 1.f, 0.f, 0.125f},  {1.f, 2.f, 0.f, 0.0625f}};
static float step1[9][4];
static const unsigned first_vertex[6] = {0, 1, 3, 4, 6, 7};

struct Case { float x, y, time; int hit; unsigned prim; float u; };

static int run(const char* cfg, int robust)
{
  RTCDevice dev = rtcNewDevice(cfg);
  if (!dev) { fprintf(stderr, "rtcNewDevice failed: error %d\n", (int)rtcGetDeviceError(NULL)); return 2; }
  rtcSetDeviceErrorFunction(dev, error_handler, NULL);
  RTCScene scene = rtcNewScene(dev);
  if (robust) rtcSetSceneFlags(scene, RTC_SCENE_FLAG_ROBUST);

  for (int i = 0; i < 9; i++) {
    step1[i][0] = step0[i][0] + 8.f; step1[i][1] = step0[i][1]; step1[i][2] = step0[i][2];
    step1[i][3] = 2.f * step0[i][3];
  }
  RTCGeometry tuft = rtcNewGeometry(dev, RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE);
  if (!tuft) { fprintf(stderr, "this library does not take RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE\n"); return 2; }
  rtcSetGeometryTimeStepCount(tuft, 2);
  rtcSetSharedGeometryBuffer(tuft, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT4, step0, 0, 4 * sizeof(float), 9);
  rtcSetSharedGeometryBuffer(tuft, RTC_BUFFER_TYPE_VERTEX, 1, RTC_FORMAT_FLOAT4, step1, 0, 4 * sizeof(float), 9);
  unsigned* li = (unsigned*)rtcSetNewGeometryBuffer(tuft, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT, sizeof(unsigned), 6);
  memcpy(li, first_vertex, sizeof(first_vertex));
  rtcCommitGeometry(tuft);
  const unsigned tuftID = rtcAttachGeometry(scene, tuft);
  rtcCommitScene(scene);
  if (g_errors) return 2; /* e.g. a library without motion blur on line segments refuses the commit */

  /* x, y and time of a ray from z = -4 along +z; whether it hits, and primID and u of the hit */
  const struct Case cases[] = {{0.f, 0.5f, 0.f, 1, 2, 0.5f},        /* the middle strand where it is at time 0 ... */
                               {4.f, 0.5f, 0.5f, 1, 2, 0.5f},       /* ... at time 1/2 */
                               {8.f, 0.5f, 1.f, 1, 2, 0.5f},        /* ... at time 1 */
                               {8.f, 0.5f, 0.f, 0, 0, 0.f},         /* and not where it is at another time */
                               {0.f, 0.5f, 1.f, 0, 0, 0.f},
                               {1.f, 1.5f, 0.25f, 1, 1, 0.5f},      /* the left strand's tip at time 1/4: x = -1 + 2 */
                               {5.1875f, 0.25f, 0.5f, 1, 4, 0.25f}, /* 3/16 beside the right strand at time 1/2: the radius is 3/16 there */
                               {5.25f, 0.25f, 0.5f, 0, 0, 0.f},     /* 1/4 beside it: outside */
                               {5.1875f, 0.25f, 0.f, 0, 0, 0.f}};   /* and the strand is not there at time 0 */
  enum { N = sizeof(cases) / sizeof(cases[0]) };
  struct RTCRayHit* stream = NULL;
  if (posix_memalign((void**)&stream, 16, sizeof(struct RTCRayHit) * N)) return 2;
  struct RTCIntersectContext ctx;
  rtcInitIntersectContext(&ctx);
  int bad = 0, hits = 0;
  for (int pass = 0; pass < 2; pass++) { /* 0: rtcIntersect1 / rtcOccluded1 per ray, 1: the same rays as one rtcIntersect1M stream */
    if (pass == 1) rtcIntersect1M(scene, &ctx, stream, N, sizeof(struct RTCRayHit));
    for (int i = 0; i < (int)N; i++) {
      const struct Case c = cases[i];
      struct RTCRayHit rh;
      if (pass == 0) {
        memset(&rh, 0, sizeof(rh));
        rh.ray.org_x = c.x; rh.ray.org_y = c.y; rh.ray.org_z = -4.f;
        rh.ray.dir_z = 1.f;
        rh.ray.time = c.time;
        rh.ray.tnear = 0.f; rh.ray.tfar = INFINITY; rh.ray.mask = 0xFFFFFFFFu;
        rh.hit.geomID = rh.hit.primID = rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
        stream[i] = rh;
        rtcIntersect1(scene, &ctx, &rh);
      } else
        rh = stream[i];
      const unsigned wantGeom = c.hit ? tuftID : RTC_INVALID_GEOMETRY_ID;
      if (rh.hit.geomID != wantGeom) { fprintf(stderr, "ray %d: geomID %u, expected %u\n", i, rh.hit.geomID, wantGeom); bad++; continue; }
      if (!c.hit) { if (rh.ray.tfar != INFINITY) bad++; continue; }
      hits++;
      /* the depth of the axis point, u along the segment, v = 0, Ng = v1 - v0 = (0, 1, 0) at every time */
      if (fabsf(rh.ray.tfar - 4.f) > 1e-6f || rh.hit.primID != c.prim || fabsf(rh.hit.u - c.u) > 1e-6f || rh.hit.v != 0.f || rh.hit.Ng_x != 0.f ||
          rh.hit.Ng_y != 1.f || rh.hit.Ng_z != 0.f) {
        fprintf(stderr, "ray %d: t %g primID %u u %g v %g Ng %g %g %g\n", i, rh.ray.tfar, rh.hit.primID, rh.hit.u, rh.hit.v, rh.hit.Ng_x, rh.hit.Ng_y, rh.hit.Ng_z);
        bad++;
      }
      if (pass == 1) continue;
      /* the hit point's place and radius at the ray's time: rtcInterpolate per time step (buffer slot), then the lerp over time */
      float P0[4], P1[4];
      rtcInterpolate0(tuft, rh.hit.primID, rh.hit.u, rh.hit.v, RTC_BUFFER_TYPE_VERTEX, 0, P0, 4);
      rtcInterpolate0(tuft, rh.hit.primID, rh.hit.u, rh.hit.v, RTC_BUFFER_TYPE_VERTEX, 1, P1, 4);
      const float px = (1.f - c.time) * P0[0] + c.time * P1[0], pr = (1.f - c.time) * P0[3] + c.time * P1[3];
      if (fabsf(px - c.x) > pr + 1e-6f || P1[0] - P0[0] != 8.f || P1[3] != 2.f * P0[3]) bad++;
      /* a shadow ray back through the segment is occluded at that time, and not at another */
      struct RTCRay sh;
      memset(&sh, 0, sizeof(sh));
      sh.org_x = c.x; sh.org_y = c.y; sh.org_z = 4.f; sh.dir_z = -1.f; sh.tnear = 0.f; sh.tfar = INFINITY; sh.mask = 0xFFFFFFFFu;
      sh.time = c.time;
      rtcOccluded1(scene, &ctx, &sh);
      if (sh.tfar != -INFINITY) bad++;
      sh.tfar = INFINITY;
      sh.time = c.time < 0.5f ? c.time + 0.5f : c.time - 0.5f;
      rtcOccluded1(scene, &ctx, &sh);
      if (sh.tfar != INFINITY) bad++;
    }
  }
  free(stream);
  rtcReleaseGeometry(tuft);
  rtcReleaseScene(scene);
  rtcReleaseDevice(dev);
  printf("line_motion_blur_min (%s%s): %d rays, %d hits, %d bad\n", cfg, robust ? " robust" : "", 2 * (int)N, hits, bad);
  return bad;
}

int main(int argc, char** argv)
{
  int bad = 0;
  if (argc > 1) bad = run(argv[1], argc > 2 && strcmp(argv[2], "robust") == 0);
  else {
    bad += run("", 0);                 /* fast traversal, node boxes swept over the shutter */
    bad += run("", 1);                 /* robust traversal */
    bad += run("mb_bounds=linear", 0); /* time-dependent node boxes */
    bad += run("line_accel_mb=bvh8.line4imb", 0);
  }
  if (bad || g_errors) { printf("line_motion_blur_min: FAILED (%d bad, %d errors)\n", bad, g_errors); return 1; }
  printf("line_motion_blur_min: ok\n");
  return 0;
}
