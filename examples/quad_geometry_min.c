/*
 * Quad meshes through the plain C API: one unit quad (0,0,0) (1,0,0) (1,1,0) (0,1,0) as RTC_GEOMETRY_TYPE_QUAD with a UINT4 index
 * buffer and a vertex-attribute buffer.  Rays along +z through both halves of the quad (triangle A = v0 v1 v3 where x+y < 1,
 * triangle B = v2 v1 v3 beyond the diagonal) go through rtcIntersect1, rtcOccluded1 and one rtcIntersect1M stream; every hit must
 * report t = 1, the quad's own parametrisation u = x, v = y on either half, and an Ng along z of one sign.  rtcInterpolate of the
 * attribute is checked against the bilinear-by-halves closed form of QuadMesh::interpolate.
 *
 * C99 on purpose:
 *   gcc -std=c99 -Iinclude examples/quad_geometry_min.c -Lembree-compressed_amd/lib -lembree3 -lm \
 *       -Wl,-rpath,$PWD/embree-compressed_amd/lib -o /tmp/quad_geometry_min
 * argv[1]: device config (e.g. "quad_accel=bvh8.quad4v"); argv[2] = "robust": RTC_SCENE_FLAG_ROBUST (the Pluecker quads)
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

static const float attrib[4][2] = {{0.f, 10.f}, {1.f, 20.f}, {3.f, 40.f}, {2.f, 30.f}};

static int run(const char* cfg, int robust)
{
  RTCDevice dev = rtcNewDevice(cfg);
  if (!dev) { fprintf(stderr, "rtcNewDevice failed: error %d\n", (int)rtcGetDeviceError(NULL)); return 2; }
  rtcSetDeviceErrorFunction(dev, error_handler, NULL);
  RTCScene scene = rtcNewScene(dev);
  if (robust) rtcSetSceneFlags(scene, RTC_SCENE_FLAG_ROBUST);
  RTCGeometry mesh = rtcNewGeometry(dev, RTC_GEOMETRY_TYPE_QUAD);
  float* v = (float*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT3, 3 * sizeof(float), 4);
  const float pos[4][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}};
  memcpy(v, pos, sizeof(pos));
  unsigned* q = (unsigned*)rtcSetNewGeometryBuffer(mesh, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT4, 4 * sizeof(unsigned), 1);
  q[0] = 0; q[1] = 1; q[2] = 2; q[3] = 3;
  rtcSetGeometryVertexAttributeCount(mesh, 1);
  rtcSetSharedGeometryBuffer(mesh, RTC_BUFFER_TYPE_VERTEX_ATTRIBUTE, 0, RTC_FORMAT_FLOAT2, attrib, 0, 2 * sizeof(float), 4);
  rtcCommitGeometry(mesh);
  const unsigned gid = rtcAttachGeometry(scene, mesh);
  rtcCommitScene(scene);

  enum { N = 16 };
  struct RTCRayHit* stream = NULL;
  if (posix_memalign((void**)&stream, 16, sizeof(struct RTCRayHit) * N)) return 2;
  struct RTCIntersectContext ctx;
  rtcInitIntersectContext(&ctx);
  int bad = 0, halfA = 0, halfB = 0;
  float ngz = 0.f;
  for (int i = 0; i < N; i++) {
    const float x = 0.05f + 0.9f * (float)((i * 7) % N) / (float)N, y = 0.05f + 0.9f * (float)i / (float)N;
    struct RTCRayHit rh;
    memset(&rh, 0, sizeof(rh));
    rh.ray.org_x = x; rh.ray.org_y = y; rh.ray.org_z = -1.f;
    rh.ray.dir_z = 1.f;
    rh.ray.tnear = 0.f; rh.ray.tfar = INFINITY; rh.ray.mask = 0xFFFFFFFFu;
    rh.hit.geomID = rh.hit.primID = rh.hit.instID[0] = RTC_INVALID_GEOMETRY_ID;
    stream[i] = rh;
    rtcIntersect1(scene, &ctx, &rh);
    if (rh.hit.geomID != gid || rh.hit.primID != 0 || fabsf(rh.ray.tfar - 1.f) > 1e-6f) { bad++; continue; }
    if (fabsf(rh.hit.u - x) > 2e-6f || fabsf(rh.hit.v - y) > 2e-6f) { fprintf(stderr, "ray %d: u,v %g %g for %g %g\n", i, rh.hit.u, rh.hit.v, x, y); bad++; }
    if (rh.hit.Ng_x != 0.f || rh.hit.Ng_y != 0.f || rh.hit.Ng_z == 0.f || (ngz != 0.f && (rh.hit.Ng_z > 0.f) != (ngz > 0.f))) bad++;
    ngz = rh.hit.Ng_z;
    if (x + y < 1.f) halfA++; else halfB++;
    /* interpolate the attribute at the hit: the closed form of the half the hit lies on */
    float P[2], du[2], dv[2];
    rtcInterpolate1(mesh, 0, rh.hit.u, rh.hit.v, RTC_BUFFER_TYPE_VERTEX_ATTRIBUTE, 0, P, du, dv, 2);
    for (int k = 0; k < 2; k++) {
      const float u = rh.hit.u, w = rh.hit.v;
      const int left = u + w <= 1.f;
      const float p0 = attrib[0][k], p1 = attrib[1][k], p2 = attrib[2][k], p3 = attrib[3][k];
      const float want = left ? (1.f - u - w) * p0 + u * p1 + w * p3 : (u + w - 1.f) * p2 + (1.f - u) * p3 + (1.f - w) * p1;
      const float wdu = left ? p1 - p0 : p2 - p3, wdv = left ? p3 - p0 : p2 - p1;
      if (fabsf(P[k] - want) > 1e-4f * (1.f + fabsf(want)) || du[k] != wdu || dv[k] != wdv) {
        fprintf(stderr, "interpolate at %g %g: %g (%g) %g (%g) %g (%g)\n", u, w, P[k], want, du[k], wdu, dv[k], wdv);
        bad++;
      }
    }
    /* a shadow ray back through the quad is occluded, one that stops short is not */
    struct RTCRay sh;
    memset(&sh, 0, sizeof(sh));
    sh.org_x = x; sh.org_y = y; sh.org_z = 1.f; sh.dir_z = -1.f; sh.tnear = 0.f; sh.tfar = INFINITY; sh.mask = 0xFFFFFFFFu;
    rtcOccluded1(scene, &ctx, &sh);
    if (sh.tfar != -INFINITY) bad++;
    sh.tfar = 0.5f;
    rtcOccluded1(scene, &ctx, &sh);
    if (sh.tfar != 0.5f) bad++;
  }
  /* the same rays as one stream: identical records */
  rtcIntersect1M(scene, &ctx, stream, N, sizeof(struct RTCRayHit));
  for (int i = 0; i < N; i++) {
    struct RTCRayHit rh = stream[i];
    const float x = rh.ray.org_x, y = rh.ray.org_y;
    if (rh.hit.geomID != gid || fabsf(rh.ray.tfar - 1.f) > 1e-6f || fabsf(rh.hit.u - x) > 2e-6f || fabsf(rh.hit.v - y) > 2e-6f) bad++;
  }
  free(stream);
  rtcReleaseGeometry(mesh);
  rtcReleaseScene(scene);
  rtcReleaseDevice(dev);
  if (halfA == 0 || halfB == 0) { fprintf(stderr, "rays did not cover both halves (%d, %d)\n", halfA, halfB); bad++; }
  printf("quad_geometry_min (%s%s): %d rays, %d on triangle A, %d on triangle B, %d bad\n", cfg, robust ? " robust" : "", N, halfA, halfB, bad);
  return bad;
}

int main(int argc, char** argv)
{
  int bad = 0;
  if (argc > 1) bad = run(argv[1], argc > 2 && strcmp(argv[2], "robust") == 0);
  else {
    bad += run("", 0);       /* Moeller quads, fast traversal */
    bad += run("", 1);       /* Pluecker quads, robust traversal */
    bad += run("quad_accel=bvh8.quad4v", 1);
  }
  if (bad || g_errors) { printf("quad_geometry_min: FAILED (%d bad, %d errors)\n", bad, g_errors); return 1; }
  printf("quad_geometry_min: ok\n");
  return 0;
}
