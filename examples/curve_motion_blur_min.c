/*
 * Motion blur on flat cubic curves through the plain C API: one ribbon (RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE) with TWO time steps -
 * rtcSetGeometryTimeStepCount(geometry, 2) and one FLOAT4 vertex buffer (x, y, z, radius) of four control points per step in the vertex
 * slots 0 and 1.  The ribbon lies along x (its point at u is (-1.5 + 3 u, 0, 0)); over the shutter it moves by 8 along x and gets twice
 * as wide.  A ray sees it where it is at ray.time, with the radius interpolated like a coordinate.  Rays along +z with known answers go
 * through rtcIntersect1, rtcOccluded1 and one rtcIntersect1M stream; rtcInterpolate reads one time step's buffer by its slot.
 *
 * C99 on purpose:
 *   gcc -std=c99 -Iinclude examples/curve_motion_blur_min.c -Lembree-compressed_amd/lib -lembree3 -lm \
 *       -Wl,-rpath,$PWD/embree-compressed_amd/lib -o /tmp/curve_motion_blur_min
 * argv[1]: device config (e.g. "mb_bounds=linear": time-dependent node boxes, the better choice for fast movers; or
 * "hair_accel_mb=bvh8.bezier1imb"); argv[2] = "robust": RTC_SCENE_FLAG_ROBUST (robust traversal)
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

/* four equally spaced collinear control points, radius 1/4; step 1: moved by 8 along x, radius 1/2 (one float of padding behind each
 * buffer: a shared FLOAT4 buffer is read in 16-byte units) */
static float step0[5][4] = {{-1.5f, 0.f, 0.f, 0.25f}, {-0.5f, 0.f, 0.f, 0.25f}, {0.5f, 0.f, 0.f, 0.25f}, {1.5f, 0.f, 0.f, 0.25f}, {0.f, 0.f, 0.f, 0.f}};
static float step1[5][4];

struct Case { float x, y, time; int hit; float u, v; };

static int run(const char* cfg, int robust)
{
  RTCDevice dev = rtcNewDevice(cfg);
  if (!dev) { fprintf(stderr, "rtcNewDevice failed: error %d\n", (int)rtcGetDeviceError(NULL)); return 2; }
  rtcSetDeviceErrorFunction(dev, error_handler, NULL);
  RTCScene scene = rtcNewScene(dev);
  if (robust) rtcSetSceneFlags(scene, RTC_SCENE_FLAG_ROBUST);

  for (int i = 0; i < 4; i++) {
    step1[i][0] = step0[i][0] + 8.f; step1[i][1] = step0[i][1]; step1[i][2] = step0[i][2];
    step1[i][3] = 2.f * step0[i][3];
  }
  RTCGeometry ribbon = rtcNewGeometry(dev, RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE);
  if (!ribbon) { fprintf(stderr, "this library does not take RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE\n"); return 2; }
  rtcSetGeometryTimeStepCount(ribbon, 2);
  rtcSetSharedGeometryBuffer(ribbon, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT4, step0, 0, 4 * sizeof(float), 4);
  rtcSetSharedGeometryBuffer(ribbon, RTC_BUFFER_TYPE_VERTEX, 1, RTC_FORMAT_FLOAT4, step1, 0, 4 * sizeof(float), 4);
  unsigned* ci = (unsigned*)rtcSetNewGeometryBuffer(ribbon, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT, sizeof(unsigned), 1);
  ci[0] = 0;
  rtcCommitGeometry(ribbon);
  const unsigned ribbonID = rtcAttachGeometry(scene, ribbon);
  rtcCommitScene(scene);
  if (g_errors) return 2; /* e.g. a library without motion blur on flat cubic curves refuses the commit */

  /* x, y and time of a ray from z = -4 along +z; whether it hits, and u and v of the hit */
  const struct Case cases[] = {{0.f, 0.f, 0.f, 1, 0.5f, 0.f},         /* the ribbon's middle where it is at time 0 ... */
                               {4.f, 0.f, 0.5f, 1, 0.5f, 0.f},        /* ... at time 1/2 */
                               {8.f, 0.f, 1.f, 1, 0.5f, 0.f},         /* ... at time 1 */
                               {8.f, 0.f, 0.f, 0, 0.f, 0.f},          /* and not where it is at another time */
                               {0.f, 0.f, 1.f, 0, 0.f, 0.f},
                               {0.f, 0.f, 0.5f, 0, 0.f, 0.f},
                               {4.375f, 0.f, 0.5f, 1, 0.625f, 0.f},   /* u along the ribbon at time 1/2: x runs from 2.5 to 5.5 */
                               {4.f, 0.375f, 0.5f, 1, 0.5f, 1.f},     /* on the edge at time 1/2: the radius is 3/8 there */
                               {4.f, 0.4375f, 0.5f, 0, 0.f, 0.f},     /* beyond it */
                               {8.f, 0.4375f, 1.f, 1, 0.5f, 0.875f},  /* but inside the radius 1/2 of time 1 */
                               {0.f, 0.375f, 0.f, 0, 0.f, 0.f}};      /* and outside the radius 1/4 of time 0 */
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
      const unsigned wantGeom = c.hit ? ribbonID : RTC_INVALID_GEOMETRY_ID;
      if (rh.hit.geomID != wantGeom) { fprintf(stderr, "ray %d: geomID %u, expected %u\n", i, rh.hit.geomID, wantGeom); bad++; continue; }
      if (!c.hit) { if (rh.ray.tfar != INFINITY) bad++; continue; }
      hits++;
      /* the ribbon faces the ray: t is its depth; u along the curve, v across it; Ng = the curve's derivative (3, 0, 0) at every time */
      if (fabsf(rh.ray.tfar - 4.f) > 1e-6f || rh.hit.primID != 0 || fabsf(rh.hit.u - c.u) > 1e-6f || fabsf(rh.hit.v - c.v) > 1e-6f || rh.hit.Ng_x != 3.f ||
          rh.hit.Ng_y != 0.f || rh.hit.Ng_z != 0.f) {
        fprintf(stderr, "ray %d: t %g primID %u u %g v %g Ng %g %g %g\n", i, rh.ray.tfar, rh.hit.primID, rh.hit.u, rh.hit.v, rh.hit.Ng_x, rh.hit.Ng_y, rh.hit.Ng_z);
        bad++;
      }
      if (pass == 1) continue;
      /* the hit point's place and radius at the ray's time: rtcInterpolate per time step (buffer slot), then the lerp over time */
      float P0[4], P1[4];
      rtcInterpolate0(ribbon, rh.hit.primID, rh.hit.u, rh.hit.v, RTC_BUFFER_TYPE_VERTEX, 0, P0, 4);
      rtcInterpolate0(ribbon, rh.hit.primID, rh.hit.u, rh.hit.v, RTC_BUFFER_TYPE_VERTEX, 1, P1, 4);
      const float px = (1.f - c.time) * P0[0] + c.time * P1[0], pr = (1.f - c.time) * P0[3] + c.time * P1[3];
      if (fabsf(px - c.x) > 1e-5f || fabsf(c.y) > pr + 1e-6f || fabsf(P1[0] - P0[0] - 8.f) > 1e-5f || fabsf(P1[3] - 2.f * P0[3]) > 1e-6f) bad++;
      /* a shadow ray back through the ribbon is occluded at that time, and not at another */
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
  rtcReleaseGeometry(ribbon);
  rtcReleaseScene(scene);
  rtcReleaseDevice(dev);
  printf("curve_motion_blur_min (%s%s): %d rays, %d hits, %d bad\n", cfg, robust ? " robust" : "", 2 * (int)N, hits, bad);
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
    bad += run("hair_accel_mb=bvh8.bezier1imb", 0);
  }
  if (bad || g_errors) { printf("curve_motion_blur_min: FAILED (%d bad, %d errors)\n", bad, g_errors); return 1; }
  printf("curve_motion_blur_min: ok\n");
  return 0;
}
