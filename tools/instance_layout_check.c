/* Stand-alone check of the offsets the instance builders compute (csrc/rt_instance_build.cpp), meant for a sanitizer build of the host
 * code on the CPU; it is not loaded into python and needs no GPU:
 *   make -C embree-compressed_amd OUT=lib_asan HOSTEXTRA="-fsanitize=address,undefined -fno-omit-frame-pointer"
 *   /opt/rocm/lib/llvm/bin/clang -std=c99 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I include tools/instance_layout_check.c \
 *      -L embree-compressed_amd/lib_asan -lembree3 -Wl,-rpath,$PWD/embree-compressed_amd/lib_asan -o tools/instance_layout_check && tools/instance_layout_check
 * (the clang that hipcc drives: the library needs the sanitizer runtime of the compiler that built it)
 * Through the public C API, on host-only devices, it commits one tiny generated scene per layout family of the instance accels - kinds
 * 15, 19, 23, 31 and 25 - each with two distinct instanced scenes, one of them shared, and a moving instance where the kind has steps,
 * checks the kind and reads every byte of every exported array (rtcamdGetAccelData 0..3 and 16..19).  A write or read past a section
 * of `blobs` or of the node buffer stops the sanitizer build. */
#include <embree3/rtcore.h>
#include <embree3/rtcore_amd.h>
#include <stdio.h>

#define FULL "gpu=none,quad_accel=default,quad_accel_mb=default,tri_accel_mb=default,inst_accel=default"

static int failed = 0;

static void check(int ok, const char* what)
{
  if (!ok) {
    printf("instance_layout_check: FAILED (%s)\n", what);
    failed = 1;
  }
}

/* n x n cells over [0, n]^2 at height z0, lifted by 0.5 per time step: two triangles or one quad per cell */
static void add_mesh(RTCDevice device, RTCScene scene, int quads, unsigned steps, int n, float z0)
{
  RTCGeometry g = rtcNewGeometry(device, quads ? RTC_GEOMETRY_TYPE_QUAD : RTC_GEOMETRY_TYPE_TRIANGLE);
  unsigned* idx;
  unsigned step;
  int x, y, k = 0;
  rtcSetGeometryTimeStepCount(g, steps);
  for (step = 0; step < steps; step++) {
    float* v = (float*)rtcSetNewGeometryBuffer(g, RTC_BUFFER_TYPE_VERTEX, step, RTC_FORMAT_FLOAT3, 3 * sizeof(float), (size_t)((n + 1) * (n + 1)));
    for (y = 0; y <= n; y++)
      for (x = 0; x <= n; x++) {
        float* p = v + 3 * (y * (n + 1) + x);
        p[0] = (float)x; p[1] = (float)y; p[2] = z0 + 0.125f * (float)((x * 3 + y * 5) % 7) + 0.5f * (float)step;
      }
  }
  idx = (unsigned*)rtcSetNewGeometryBuffer(g, RTC_BUFFER_TYPE_INDEX, 0, quads ? RTC_FORMAT_UINT4 : RTC_FORMAT_UINT3, (quads ? 4 : 3) * sizeof(unsigned),
                                           (size_t)(quads ? n * n : 2 * n * n));
  for (y = 0; y < n; y++)
    for (x = 0; x < n; x++) {
      const unsigned a = (unsigned)(y * (n + 1) + x), b = a + 1, c = a + (unsigned)n + 2, d = a + (unsigned)n + 1;
      if (quads) { idx[k++] = a; idx[k++] = b; idx[k++] = c; idx[k++] = d; }
      else { idx[k++] = a; idx[k++] = b; idx[k++] = c; idx[k++] = a; idx[k++] = c; idx[k++] = d; }
    }
  rtcCommitGeometry(g);
  rtcAttachGeometry(scene, g);
  rtcReleaseGeometry(g);
}

/* a cube as a subdivision mesh */
static void add_cube(RTCDevice device, RTCScene scene)
{
  static const float verts[8][3] = {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}, {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
  static const unsigned faces[24] = {0, 4, 5, 1, 1, 5, 7, 3, 3, 7, 6, 2, 2, 6, 4, 0, 4, 6, 7, 5, 0, 1, 3, 2};
  RTCGeometry g = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_SUBDIVISION);
  float* v = (float*)rtcSetNewGeometryBuffer(g, RTC_BUFFER_TYPE_VERTEX, 0, RTC_FORMAT_FLOAT3, 3 * sizeof(float), 8);
  unsigned* fs = (unsigned*)rtcSetNewGeometryBuffer(g, RTC_BUFFER_TYPE_FACE, 0, RTC_FORMAT_UINT, sizeof(unsigned), 6);
  unsigned* fi = (unsigned*)rtcSetNewGeometryBuffer(g, RTC_BUFFER_TYPE_INDEX, 0, RTC_FORMAT_UINT, sizeof(unsigned), 24);
  int i;
  for (i = 0; i < 24; i++) v[i] = verts[i / 3][i % 3];
  for (i = 0; i < 6; i++) fs[i] = 4;
  for (i = 0; i < 24; i++) fi[i] = faces[i];
  rtcCommitGeometry(g);
  rtcAttachGeometry(scene, g);
  rtcReleaseGeometry(g);
}

static void add_instance(RTCDevice device, RTCScene top, RTCScene object, float x, unsigned steps)
{
  RTCGeometry inst = rtcNewGeometry(device, RTC_GEOMETRY_TYPE_INSTANCE);
  unsigned step;
  rtcSetGeometryInstancedScene(inst, object);
  rtcSetGeometryTimeStepCount(inst, steps);
  for (step = 0; step < steps; step++) {
    const float xfm[12] = {1.f, 0.f, 0.f, x, 0.f, 2.f, 0.f, (float)step, 0.f, 0.f, 0.5f, 0.25f * (float)step};
    rtcSetGeometryTransform(inst, step, RTC_FORMAT_FLOAT3X4_ROW_MAJOR, xfm);
  }
  rtcCommitGeometry(inst);
  rtcAttachGeometry(top, inst);
  rtcReleaseGeometry(inst);
}

/* family: the kind expected; the two instanced scenes are a (used by instances 0, 2 and 4) and b (instances 1 and 3) */
static void run(const char* cfg, unsigned family)
{
  RTCDevice device = rtcNewDevice(cfg);
  RTCScene a, b, top;
  struct RTCAMDSceneStats st;
  unsigned kind, sum = 0;
  size_t total = 0;
  int i;
  const unsigned moving = family == 15 ? 1u : 3u; /* time steps of instance 2 */
  check(device != NULL, "rtcNewDevice");
  if (!device) return;
  a = rtcNewScene(device);
  b = rtcNewScene(device);
  if (family == 25) {
    add_cube(device, a);
    add_cube(device, b);
    rtcSetSceneLevels(a, 2, 1);
    rtcSetSceneLevels(b, 3, 1);
  } else {
    add_mesh(device, a, 0, 1, 5, 0.f);
    if (family == 23 || family == 31) { /* all four trees in a, a motion-blur tree alone in b */
      add_mesh(device, a, 0, 2, 4, 1.f);
      add_mesh(device, a, 1, 1, 3, 2.f);
      add_mesh(device, a, 1, 3, 6, 3.f);
      add_mesh(device, b, 1, 2, 7, 0.f);
    } else
      add_mesh(device, b, 0, 1, 3, 0.f);
  }
  rtcCommitScene(a);
  rtcCommitScene(b);
  top = rtcNewScene(device);
  for (i = 0; i < 5; i++) add_instance(device, top, i % 2 ? b : a, 20.f * (float)i, i == 2 ? moving : 1u);
  rtcCommitScene(top);
  check(rtcGetDeviceError(device) == RTC_ERROR_NONE, "commit");
  st.byteSize = sizeof(st);
  rtcamdGetSceneStats(top, &st);
  check(st.accelKind == family, "accel kind");
  for (kind = 0; kind < 20; kind = kind == 3 ? 16 : kind + 1) {
    size_t bytes = 0, k;
    const unsigned char* p = (const unsigned char*)rtcamdGetAccelData(top, kind, &bytes);
    for (k = 0; p && k < bytes; k++) sum += p[k];
    total += bytes;
  }
  check(total > 0, "no accel data");
  printf("kind %u: %zu bytes read, byte sum %u\n", st.accelKind, total, sum);
  rtcReleaseScene(top);
  rtcReleaseScene(a);
  rtcReleaseScene(b);
  rtcReleaseDevice(device);
}

int main(void)
{
  run("gpu=none,inst_accel=default", 15);
  run("gpu=none,inst_accel=default", 19);
  run(FULL, 23);
  run(FULL ",mb_bounds=linear,inst_mb_bounds=linear", 31);
  run("gpu=none,inst_accel=default,subdiv_accel=bvh4.compressed.leaf", 25);
  if (!failed) printf("instance_layout_check: ok\n");
  return failed;
}
