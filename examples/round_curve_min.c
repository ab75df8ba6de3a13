/*
 * Round cubic curves (tubes) through the plain C API, on a device created with round_curves=1: a straight Bezier tube
 * (RTC_GEOMETRY_TYPE_ROUND_BEZIER_CURVE) of radius 0.25 from x = -1.5 to 1.5 at y = 0, a tapered one at y = 10 whose radius grows from
 * 0.1 to 0.4, and a straight B-spline tube (RTC_GEOMETRY_TYPE_ROUND_BSPLINE_CURVE) at y = 20, whose curve spans the middle third of its
 * control polygon, x = -1 to 1.  Buffers as for the flat curves: FLOAT4 vertices x, y, z, radius and one UINT per curve, the index of the
 * first of its four control points.  The surface of a curve P(u), r(u) is the set of points at distance r(u) from P(u) in the plane
 * normal to P'(u); there are no end caps, and a ray that starts inside hits where it leaves.  A hit reports t, u along the curve, v = 0
 * and an Ng that points away from the axis (not normalised).
 *
 * With the key, RTC_DEVICE_PROPERTY_CURVE_GEOMETRY_SUPPORTED answers 1: all five curve types are taken.
 *
 * C99 on purpose:
 *   gcc -std=c99 -Iinclude examples/round_curve_min.c -Lembree-compressed_amd/lib -lembree3 -lm \
 *       -Wl,-rpath,$PWD/embree-compressed_amd/lib -o /tmp/round_curve_min
 * argv[1]: further device config, appended to "round_curves=1"; argv[2] = "robust": RTC_SCENE_FLAG_ROBUST (robust traversal)
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

static const float tubes[3][4][4] = {
  {{-1.5f, 0.f, 0.f, 0.25f}, {-0.5f, 0.f, 0.f, 0.25f}, {0.5f, 0.f, 0.f, 0.25f}, {1.5f, 0.f, 0.f, 0.25f}},
  {{-1.5f, 10.f, 0.f, 0.1f}, {-0.5f, 10.f, 0.f, 0.2f}, {0.5f, 10.f, 0.f, 0.3f}, {1.5f, 10.f, 0.f, 0.4f}},
  {{-3.f, 20.f, 0.f, 0.25f}, {-1.f, 20.f, 0.f, 0.25f}, {1.f, 20.f, 0.f, 0.25f}, {3.f, 20.f, 0.f, 0.25f}}};

/* a ray, its tnear, and the answer: tube (-1: a miss), t and u */
struct Case { float ox, oy, oz, dx, dy, dz, tnear; int tube; float t, u; };

int main(int argc, char** argv)
{
  char cfg[512];
  snprintf(cfg, sizeof(cfg), "round_curves=1%s%s", argc > 1 && argv[1][0] ? "," : "", argc > 1 ? argv[1] : "");
  const int robust = argc > 2 && strcmp(argv[2], "robust") == 0;
  RTCDevice dev = rtcNewDevice(cfg);
  if (!dev) { fprintf(stderr, "rtcNewDevice failed: error %d\n", (int)rtcGetDeviceError(NULL)); return 2; }
  rtcSetDeviceErrorFunction(dev, error_handler, NULL);
  const long supported = (long)rtcGetDeviceProperty(dev, RTC_DEVICE_PROPERTY_CURVE_GEOMETRY_SUPPORTED);
  printf("RTC_DEVICE_PROPERTY_CURVE_GEOMETRY_SUPPORTED = %ld\n", supported);
  RTCScene scene = rtcNewScene(dev);
  if (robust) rtcSetSceneFlags(scene, RTC_SCENE_FLAG_ROBUST);
  unsigned id[3];
  for (int s = 0; s < 3; s++) {
    RTCGeometry g = rtcNewGeometry(dev, s == 2 ? RTC_GEOMETRY_TYPE_ROUND_BSPLINE_CURVE : RTC_GEOMETRY_TYPE_ROUND_BEZIER_CURVE);
    if (!g) { fprintf(stderr, "this device does not take the round curve types\n"); return 2; }
    rtcSetSharedGeometryBuffer(g, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT4, tubes[s], 0, 4 * sizeof(float), 4);
    unsigned* ci = (unsigned*)rtcSetNewGeometryBuffer(g, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT, sizeof(unsigned), 1);
    ci[0] = 0;
    rtcCommitGeometry(g);
    id[s] = rtcAttachGeometry(scene, g);
    rtcReleaseGeometry(g);
  }
  rtcCommitScene(scene);

  static const struct Case cases[] = {
    {0.f, 0.f, -4.f, 0.f, 0.f, 1.f, 0.f, 0, 3.75f, 0.5f},            /* the front of the straight tube */
    {0.f, 0.f, -4.f, 0.f, 0.f, 1.f, 3.8f, 0, 4.25f, 0.5f},           /* tnear behind the front: its back */
    {0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0, 0.25f, 0.5f},             /* from inside: where the ray leaves */
    {0.f, 0.2f, -4.f, 0.f, 0.f, 1.f, 0.f, 0, 3.85f, 0.5f},           /* off the axis: sqrt(0.25^2 - 0.2^2) = 0.15 */
    {-4.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, -1, 0.f, 0.f},              /* along the axis: no end caps */
    {0.f, 0.26f, -4.f, 0.f, 0.f, 1.f, 0.f, -1, 0.f, 0.f},            /* past the tube */
    {0.75f, 10.f, -4.f, 0.f, 0.f, 1.f, 0.f, 1, 3.675f, 0.75f},       /* the tapered tube: r(0.75) = 0.325 */
    {-0.75f, 10.f, -4.f, 0.f, 0.f, 1.f, 0.f, 1, 3.825f, 0.25f},      /* ... r(0.25) = 0.175 */
    {0.5f, 20.f, -4.f, 0.f, 0.f, 1.f, 0.f, 2, 3.75f, 0.75f},         /* the B-spline tube: x = -1 + 2 u */
    {1.25f, 20.f, -4.f, 0.f, 0.f, 1.f, 0.f, -1, 0.f, 0.f}};          /* beyond its end at x = 1, inside its control polygon */
  const int n = (int)(sizeof(cases) / sizeof(cases[0]));
  int bad = 0;
  struct RTCIntersectContext ctx;
  for (int i = 0; i < n; i++) {
    const struct Case* c = &cases[i];
    struct RTCRayHit rh;
    memset(&rh, 0, sizeof(rh));
    rh.ray.org_x = c->ox; rh.ray.org_y = c->oy; rh.ray.org_z = c->oz;
    rh.ray.dir_x = c->dx; rh.ray.dir_y = c->dy; rh.ray.dir_z = c->dz;
    rh.ray.tnear = c->tnear; rh.ray.tfar = INFINITY; rh.ray.mask = 0xFFFFFFFFu;
    rh.hit.geomID = rh.hit.primID = rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
    struct RTCRay shadow = rh.ray;
    rtcInitIntersectContext(&ctx);
    rtcIntersect1(scene, &ctx, &rh);
    rtcInitIntersectContext(&ctx);
    rtcOccluded1(scene, &ctx, &shadow);
    int ok;
    if (c->tube < 0) ok = rh.hit.geomID == RTC_INVALID_GEOMETRY_ID && shadow.tfar == INFINITY;
    else {
      const float away = rh.hit.Ng_x * 0.f + rh.hit.Ng_y * (c->oy - tubes[c->tube][0][1]) + rh.hit.Ng_z * ((c->oz + rh.ray.tfar * c->dz) - 0.f);
      ok = rh.hit.geomID == id[c->tube] && rh.hit.primID == 0 && fabsf(rh.ray.tfar - c->t) <= 1e-4f * c->t && fabsf(rh.hit.u - c->u) <= 1e-4f &&
           rh.hit.v == 0.f && away > 0.f && shadow.tfar == -INFINITY;
    }
    printf("ray %d: %s t %g u %g%s\n", i, rh.hit.geomID == RTC_INVALID_GEOMETRY_ID ? "miss" : "hit", rh.ray.tfar, rh.hit.u, ok ? "" : "   <-- unexpected");
    bad += !ok;
  }
  rtcReleaseScene(scene);
  rtcReleaseDevice(dev);
  if (bad || g_errors || supported != 1) { printf("round_curve_min: %d unexpected answers, %d errors\n", bad, g_errors); return 1; }
  printf("round_curve_min: ok (%d rays)\n", n);
  return 0;
}
