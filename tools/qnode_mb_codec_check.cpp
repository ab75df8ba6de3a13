// Stand-alone check of the QNodeMB8 codec (csrc/bvh8_builder.cpp quantize_node_mb / dequantize_child_mb), meant for a sanitizer build on
// the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off -I include -I embree-compressed_amd/csrc \
//       -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/qnode_mb_codec_check.cpp embree-compressed_amd/csrc/bvh8_builder.cpp -lpthread -o qnode_mb_codec_check && ./qnode_mb_codec_check
// Random nodes of 1..8 children whose end boxes move, sit far from the origin, or are flat: every decoded box must hold the
// interpolated end boxes at every tested time, at t = 0 and t = 1 with at least one and less than two grid steps to spare, and times
// outside [0, 1] (and NaN) must decode like the nearer end.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "bvh8_builder.h"

using namespace rtamd;

static float scale_of(uint8_t e)
{
  uint32_t bits = uint32_t(e) << 23;
  float f;
  memcpy(&f, &bits, 4);
  return f;
}

int main()
{
  std::mt19937 rng(12345);
  std::uniform_real_distribution<float> u01(0.f, 1.f);
  size_t checks = 0;
  for (int iter = 0; iter < 20000; iter++) {
    const int n = 1 + (int)(rng() % 8);
    const float centre = iter % 5 == 0 ? 0.f : std::ldexp(u01(rng) - 0.5f, (int)(rng() % 24) - 4); // up to +-2^18
    const float size = std::ldexp(0.5f + u01(rng), (int)(rng() % 16) - 10);
    const float speed = iter % 3 == 0 ? 0.f : 16.f * u01(rng);
    const bool flat = iter % 7 == 0;
    Box3 b0[8], b1[8];
    uint32_t refs[8];
    for (int i = 0; i < n; i++) {
      refs[i] = REF_LEAF | (uint32_t)i;
      for (int a = 0; a < 3; a++) {
        const float lo = centre + size * (u01(rng) - 0.5f), ext = (flat && a == 1) ? 0.f : size * 0.3f * u01(rng);
        const float move = speed * size * (u01(rng) - 0.5f);
        b0[i].lo[a] = lo; b0[i].hi[a] = lo + ext;
        b1[i].lo[a] = lo + move; b1[i].hi[a] = lo + move + ext * (0.5f + u01(rng));
      }
    }
    QNodeMB8 q;
    quantize_node_mb(b0, b1, refs, n, q);
    for (int i = 0; i < 8; i++)
      if ((q.child[i] == REF_EMPTY) != (i >= n)) { printf("FAIL child refs, iteration %d\n", iter); return 1; }
    const float times[] = {0.f, 1.f, 0.5f, 0.25f, 0.1f, 0.9f, u01(rng), u01(rng), 1e-30f, 0.99999994f};
    for (int i = 0; i < n; i++) {
      for (float t : times) {
        const Box3 d = dequantize_child_mb(q, i, t);
        for (int a = 0; a < 3; a++) {
          const double s = scale_of(q.exp[a]);
          const double lo = (1.0 - (double)t) * b0[i].lo[a] + (double)t * b1[i].lo[a], hi = (1.0 - (double)t) * b0[i].hi[a] + (double)t * b1[i].hi[a];
          checks++;
          if (!(s > 0.0) || !((double)d.lo[a] <= lo - 0.5 * s) || !((double)d.hi[a] >= hi + 0.5 * s)) {
            printf("FAIL containment, iteration %d child %d axis %d t %a: [%a, %a] vs [%a, %a], step %a\n", iter, i, a, t, d.lo[a], d.hi[a], lo, hi, s);
            return 1;
          }
          if ((t == 0.f || t == 1.f) && (!(lo - (double)d.lo[a] < 2.0 * s) || !((double)d.hi[a] - hi < 2.0 * s) || !(lo - (double)d.lo[a] >= s) || !((double)d.hi[a] - hi >= s))) {
            printf("FAIL padding, iteration %d child %d axis %d t %g\n", iter, i, a, t);
            return 1;
          }
        }
      }
      const Box3 e0 = dequantize_child_mb(q, i, 0.f), e1 = dequantize_child_mb(q, i, 1.f);
      const Box3 below = dequantize_child_mb(q, i, -3.f), above = dequantize_child_mb(q, i, 7.5f), nan = dequantize_child_mb(q, i, std::nanf(""));
      if (memcmp(&below, &e0, sizeof(Box3)) || memcmp(&above, &e1, sizeof(Box3)) || memcmp(&nan, &e0, sizeof(Box3))) { printf("FAIL clamp, iteration %d\n", iter); return 1; }
    }
  }
  printf("qnode_mb_codec_check: ok (%zu plane pairs)\n", checks);
  return 0;
}
