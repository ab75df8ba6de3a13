/*
 * Flat cubic curves (ribbon hair) through the plain C API: one Bezier strand (RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE) and one B-spline strand
 * (RTC_GEOMETRY_TYPE_FLAT_BSPLINE_CURVE), each FLOAT4 vertices x, y, z, radius and one UINT per curve, the index of the first of its four
 * control points.  Both strands are straight with equally spaced control points, so the answers are known in closed form: the Bezier
 * strand runs from x = -1.5 to 1.5 at y = 0, the B-spline strand - whose curve spans the middle third of its control polygon - from
 * x = -1 to 1 at y = 10.  Rays along +z go through rtcIntersect1, rtcOccluded1 and one rtcIntersect1M stream: a hit reports the depth of
 * the ribbon (it faces the ray), u along the curve, v in [-1, 1] across it and Ng = the curve's derivative at u, not normalised.
 * rtcInterpolate evaluates the geometry's own basis on the user's control points.
 *
 * An application should try the geometry type: RTC_DEVICE_PROPERTY_CURVE_GEOMETRY_SUPPORTED speaks for the round
 * curve types as well, which this library takes only on a device created with round_curves=1 (round_curve_min.c): it is 0 here.
 *
 * C99 on purpose:
 *   gcc -std=c99 -Iinclude examples/curve_hair_min.c -Lembree-compressed_amd/lib -lembree3 -lm \
 *       -Wl,-rpath,$PWD/embree-compressed_amd/lib -o /tmp/curve_hair_min
 * argv[1]: device config (e.g. "hair_accel=bvh4.bezier1v"); argv[2] = "robust": RTC_SCENE_FLAG_ROBUST (robust traversal)
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

static const float bezier_cp[4][4] = {{-1.5f, 0.f, 0.f, 0.25f}, {-0.5f, 0.f, 0.f, 0.25f}, {0.5f, 0.f, 0.f, 0.25f}, {1.5f, 0.f, 0.f, 0.25f}};
static const float bspline_cp[4][4] = {{-3.f, 10.f, 0.f, 0.25f}, {-1.f, 10.f, 0.f, 0.25f}, {1.f, 10.f, 0.f, 0.25f}, {3.f, 10.f, 0.f, 0.25f}};

/* x, y of a ray from z = -4 along +z; strand (0 Bezier, 1 B-spline, -1: a miss), u, v and dP/du.x of its hit */
struct Case { float x, y; int strand; float u, v, ngx; };

static int run(const char* cfg, int robust)
{
  RTCDevice dev = rtcNewDevice(cfg);
  if (!dev) { fprintf(stderr, "rtcNewDevice failed: error %d\n", (int)rtcGetDeviceError(NULL)); return 2; }
  rtcSetDeviceErrorFunction(dev, error_handler, NULL);
  RTCScene scene = rtcNewScene(dev);
  if (robust) rtcSetSceneFlags(scene, RTC_SCENE_FLAG_ROBUST);

  RTCGeometry strand[2];
  unsigned id[2];
  for (int s = 0; s < 2; s++) {
    strand[s] = rtcNewGeometry(dev, s == 0 ? RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE : RTC_GEOMETRY_TYPE_FLAT_BSPLINE_CURVE);
    if (!strand[s]) { fprintf(stderr, "this library does not take the flat cubic curve types\n"); return 2; }
    rtcSetSharedGeometryBuffer(strand[s], RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT4, s == 0 ? bezier_cp : bspline_cp, 0, 4 * sizeof(float), 4);
    unsigned* ci = (unsigned*)rtcSetNewGeometryBuffer(strand[s], RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT, sizeof(unsigned), 1);
    ci[0] = 0;
    rtcSetGeometryTessellationRate(strand[s], 8.f); /* ribbon quads per curve (default 4, at most 16) */
    rtcCommitGeometry(strand[s]);
    id[s] = rtcAttachGeometry(scene, strand[s]);
  }
  rtcCommitScene(scene);

  const struct Case cases[] = {{0.f, 0.f, 0, 0.5f, 0.f, 3.f},              /* the middle of the Bezier strand */
                               {-0.75f, 0.125f, 0, 0.25f, 0.5f, 3.f},      /* a quarter along it, halfway to its upper edge */
                               {1.125f, -0.25f, 0, 0.875f, -1.f, 3.f},     /* on its lower edge */
                               {1.75f, 0.f, -1, 0.f, 0.f, 0.f},            /* past its end */
                               {0.f, 0.5f, -1, 0.f, 0.f, 0.f},             /* beside it */
                               {0.f, 10.f, 1, 0.5f, 0.f, 2.f},             /* the middle of the B-spline strand */
                               {0.5f, 10.125f, 1, 0.75f, 0.5f, 2.f},
                               {2.f, 10.f, -1, 0.f, 0.f, 0.f}};            /* inside its control polygon, past the end of the curve */
  enum { N = sizeof(cases) / sizeof(cases[0]) };
  struct RTCRayHit* stream = NULL;
  if (posix_memalign((void**)&stream, 16, sizeof(struct RTCRayHit) * N)) return 2;
  struct RTCIntersectContext ctx;
  rtcInitIntersectContext(&ctx);
  int bad = 0, onCurves = 0;
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
      const unsigned wantGeom = c.strand < 0 ? RTC_INVALID_GEOMETRY_ID : id[c.strand];
      if (rh.hit.geomID != wantGeom) { fprintf(stderr, "ray %d: geomID %u, expected %u\n", i, rh.hit.geomID, wantGeom); bad++; continue; }
      if (c.strand < 0) { if (rh.ray.tfar != INFINITY) bad++; continue; }
      onCurves++;
      if (pass == 0)
        printf("ray %d: strand %d t %.6f u %.6f v %.6f Ng %.6f %.6f %.6f (expected t 4 u %g v %g Ng %g 0 0)\n", i, c.strand, rh.ray.tfar, rh.hit.u, rh.hit.v,
               rh.hit.Ng_x, rh.hit.Ng_y, rh.hit.Ng_z, c.u, c.v, c.ngx);
      /* the Bezier strand's numbers are dyadic and exact; the B-spline strand goes through 1/6 and 2/3 at commit */
      const float tol = c.strand == 0 ? 0.f : 1e-5f;
      if (rh.hit.primID != 0 || fabsf(rh.ray.tfar - 4.f) > tol || fabsf(rh.hit.u - c.u) > tol || fabsf(rh.hit.v - c.v) > tol || fabsf(rh.hit.Ng_x - c.ngx) > tol ||
          fabsf(rh.hit.Ng_y) > tol || fabsf(rh.hit.Ng_z) > tol) {
        fprintf(stderr, "ray %d: primID %u t %g u %g v %g Ng %g %g %g\n", i, rh.hit.primID, rh.ray.tfar, rh.hit.u, rh.hit.v, rh.hit.Ng_x, rh.hit.Ng_y, rh.hit.Ng_z);
        bad++;
      }
      if (pass == 1) continue;
      /* the point on the curve and the radius there: the geometry's own basis on the user's control points */
      float P[4], du[4], dv[4];
      rtcInterpolate1(strand[c.strand], rh.hit.primID, rh.hit.u, rh.hit.v, RTC_BUFFER_TYPE_VERTEX, 0, P, du, dv, 4);
      const float wantP[4] = {c.x, c.strand == 0 ? 0.f : 10.f, 0.f, 0.25f};
      for (int k = 0; k < 4; k++)
        if (fabsf(P[k] - wantP[k]) > 1e-5f || fabsf(du[k] - (k == 0 ? c.ngx : 0.f)) > 1e-5f) bad++;
      /* a shadow ray back through the ribbon is occluded, one that stops short is not */
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
  rtcReleaseGeometry(strand[0]);
  rtcReleaseGeometry(strand[1]);
  rtcReleaseScene(scene);
  rtcReleaseDevice(dev);
  printf("curve_hair_min (%s%s): %d rays, %d hits on curves, %d bad\n", cfg, robust ? " robust" : "", 2 * (int)N, onCurves, bad);
  return bad;
}

int main(int argc, char** argv)
{
  int bad = 0;
  if (argc > 1) bad = run(argv[1], argc > 2 && strcmp(argv[2], "robust") == 0);
  else {
    bad += run("", 0);                          /* fast traversal */
    bad += run("", 1);                          /* robust traversal */
    bad += run("hair_accel=bvh4.bezier1v", 0);
  }
  if (bad || g_errors) { printf("curve_hair_min: FAILED (%d bad, %d errors)\n", bad, g_errors); return 1; }
  printf("curve_hair_min: ok\n");
  return 0;
}
