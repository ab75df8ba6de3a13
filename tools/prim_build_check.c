/* Stand-alone check of the primitive builders (csrc/rt_prim_build.cpp) and the commit sequence (csrc/rt_scene.cpp), meant for a sanitizer
 * build of the host code on the CPU; it is not loaded into python and needs no GPU:
 *   make -C embree-compressed_amd OUT=lib_asan HOSTEXTRA="-fsanitize=address,undefined -fno-omit-frame-pointer"
 *   /opt/rocm/lib/llvm/bin/clang -std=c99 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I include tools/prim_build_check.c \
 *      -L embree-compressed_amd/lib_asan -lembree3 -Wl,-rpath,$PWD/embree-compressed_amd/lib_asan -lm -o tools/prim_build_check && tools/prim_build_check
 * (the clang that hipcc drives: the library needs the sanitizer runtime of the compiler that built it)
 * Through the public C API, on host-only devices, it commits generated scenes of each of the seven types - triangles, quads, flat curves
 * and line segments, static and with time steps, swept and under mb_bounds=linear - at 1, 5, 29 and 300 primitives, with a NaN vertex, an
 * index that reaches past the vertex buffer and a geometry without primitives, then all seven in one scene, which is committed again
 * after a geometry was disabled; it checks the kind and the record count and reads every byte of every exported array. */
#include <embree3/rtcore.h>
#include <embree3/rtcore_amd.h>
#include <math.h>
#include <stdio.h>

#define CFG "gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,line_accel_mb=default,hair_accel=default"

enum { TRI, TRIMB, QUAD, QUADMB, CURVE, LINE, LINEMB, NUM_TYPES };
static const char* const names[NUM_TYPES] = {"triangles", "motion blur triangles", "quads", "motion blur quads", "curves", "lines", "motion blur lines"};
/* kinds of a default scene: fast, robust, and under mb_bounds=linear fast, robust */
static const unsigned kinds[NUM_TYPES][4] = {{2, 1, 2, 1}, {11, 10, 27, 26}, {9, 8, 9, 8}, {13, 12, 29, 28}, {43, 42, 43, 42}, {37, 36, 37, 36}, {39, 38, 41, 40}};

static int failed = 0;

static void check(int ok, const char* what, const char* name)
{
  if (!ok) {
    printf("prim_build_check: FAILED (%s, %s)\n", what, name);
    failed = 1;
  }
}

/* n primitives of a type, primitive i around (i % 17, i / 17, z0); bad: primitive 1 gets a NaN and the last an index past the buffer.
 * Returns the number of records the accel must hold. */
static unsigned add(RTCDevice device, RTCScene scene, int type, unsigned n, float z0, int bad)
{
  const int mesh = type <= QUADMB, moving = type == TRIMB || type == QUADMB || type == LINEMB;
  const unsigned k = type <= TRIMB ? 3u : (type <= QUADMB ? 4u : (type == CURVE ? 4u : 2u)); /* points per primitive */
  const unsigned steps = moving ? 3u : 1u, w = mesh ? 3u : 4u;
  const enum RTCGeometryType gtype = type <= TRIMB ? RTC_GEOMETRY_TYPE_TRIANGLE : (type <= QUADMB ? RTC_GEOMETRY_TYPE_QUAD : (type == CURVE ? RTC_GEOMETRY_TYPE_FLAT_BEZIER_CURVE : RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE));
  RTCGeometry g = rtcNewGeometry(device, gtype);
  unsigned* idx;
  unsigned step, i, j, valid = n;
  if (moving) rtcSetGeometryTimeStepCount(g, steps);
  for (step = 0; step < steps; step++) {
    float* v = (float*)rtcSetNewGeometryBuffer(g, RTC_BUFFER_TYPE_VERTEX, step, mesh ? RTC_FORMAT_FLOAT3 : RTC_FORMAT_FLOAT4, w * sizeof(float), (size_t)n * k);
    for (i = 0; i < n; i++)
      for (j = 0; j < k; j++) {
        float* p = v + (size_t)w * (i * k + j);
        p[0] = (float)(i % 17u) + 0.3f * (float)(j & 1u) + 0.125f * (float)step;
        p[1] = (float)(i / 17u) + 0.3f * (float)(j >> 1);
        p[2] = z0 + 0.0625f * (float)((i * 7u + j) % 5u);
        if (!mesh) p[3] = 0.02f + 0.01f * (float)j;
      }
    if (bad && n > 1) v[w * k] = NAN;
  }
  idx = (unsigned*)rtcSetNewGeometryBuffer(g, RTC_BUFFER_TYPE_INDEX, 0, mesh ? (k == 3 ? RTC_FORMAT_UINT3 : RTC_FORMAT_UINT4) : RTC_FORMAT_UINT, (mesh ? k : 1u) * sizeof(unsigned), n);
  for (i = 0; i < n; i++) {
    if (mesh) for (j = 0; j < k; j++) idx[i * k + j] = i * k + j;
    else idx[i] = i * k;
  }
  if (bad && n > 1) valid--;
  if (bad && n > 2) {
    if (mesh) idx[(n - 1) * k + 1] = n * k;
    else idx[n - 1] = (n - 1) * k + 1;
    valid--;
  }
  rtcCommitGeometry(g);
  rtcAttachGeometry(scene, g);
  rtcReleaseGeometry(g);
  return valid * (steps > 1 ? steps - 1 : 1u);
}

/* checks the kind and the record count of the accel the inspection calls describe, and reads all it exports */
static void inspect(RTCDevice device, RTCScene scene, unsigned kind, unsigned records, const char* name)
{
  struct RTCAMDSceneStats st;
  unsigned a, sum = 0;
  size_t total = 0;
  check(rtcGetDeviceError(device) == RTC_ERROR_NONE, "commit", name);
  st.byteSize = sizeof(st);
  rtcamdGetSceneStats(scene, &st);
  check(st.accelKind == kind, "accel kind", name);
  check(st.primCount == records, "record count", name);
  for (a = 0; a < 4; a++) {
    size_t bytes = 0, b;
    const unsigned char* p = (const unsigned char*)rtcamdGetAccelData(scene, a, &bytes);
    for (b = 0; p && b < bytes; b++) sum += p[b];
    total += bytes;
  }
  check(records == 0 || total > 0, "no accel data", name);
  printf("%s: kind %u, %u records, %zu bytes read, byte sum %u\n", name, (unsigned)st.accelKind, records, total, sum);
}

int main(void)
{
  static const unsigned sizes[4] = {1, 5, 29, 300};
  int linear, robust, type, k;
  for (linear = 0; linear < 2; linear++) {
    RTCDevice device = rtcNewDevice(linear ? CFG ",mb_bounds=linear" : CFG);
    RTCScene all;
    unsigned records;
    check(device != NULL, "rtcNewDevice", "device");
    if (!device) return 1;
    for (type = 0; type < NUM_TYPES; type++)
      for (k = 0; k < 4; k++)
        for (robust = 0; robust < 2; robust++) {
          RTCScene scene = rtcNewScene(device);
          if (robust) rtcSetSceneFlags(scene, RTC_SCENE_FLAG_ROBUST);
          add(device, scene, type, 0, 5.f, 0); /* a geometry without primitives takes geomID 0 */
          records = add(device, scene, type, sizes[k], 0.f, 1);
          rtcCommitScene(scene);
          inspect(device, scene, records ? kinds[type][2 * linear + robust] : 0u, records, names[type]);
          rtcReleaseScene(scene);
        }
    /* all seven types (geomID = type): the inspection calls describe the triangles, and after they were disabled the next type */
    all = rtcNewScene(device);
    for (type = 0; type < NUM_TYPES; type++) records = add(device, all, type, 40u + (unsigned)type, (float)type, 1);
    rtcCommitScene(all);
    inspect(device, all, kinds[TRI][0], 38, "all seven types");
    rtcDisableGeometry(rtcGetGeometry(all, TRI));
    rtcCommitGeometry(rtcGetGeometry(all, TRI));
    rtcCommitScene(all);
    inspect(device, all, kinds[TRIMB][2 * linear], 39 * 2, "all seven types, triangles disabled");
    rtcReleaseScene(all);
    rtcReleaseDevice(device);
  }
  if (!failed) printf("prim_build_check: ok\n");
  return failed;
}
