// Stand-alone check of the exclusion lists of the host filter loop (csrc/rt_excl_list.h: flatten, deviceBytes and the device image), meant
// for a sanitizer build on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I embree-compressed_amd/csrc tools/excl_list_check.cpp -o excl_list_check && ./excl_list_check
// Lists of the three key forms - (geomID, primID), + bits of t, + bits of t and the instance's geomID (two words per entry, the form of
// filters below an instance) - are filled for a few rays, flattened for random subsets of active rays in random order, and laid out into a
// heap block of exactly deviceBytes() bytes, which the program then reads the way the kernels do: offsets by the ray's index in the
// compacted batch, pairs by entry, t and instance as one 8-byte word at entry e.  Any write or read outside the block is the sanitizer's
// to report; the contents are compared with the lists.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "rt_excl_list.h"

using namespace rtamd;

static int fail(const char* what, int form, unsigned round)
{
  printf("excl_list_check: FAILED (%s; form %d, round %u)\n", what, form, round);
  return 1;
}

int main()
{
  std::mt19937 rng(4711);
  size_t entriesChecked = 0;
  for (int form = 0; form < 3; form++) {
    for (unsigned round = 0; round < 200; round++) {
      const uint32_t M = 1u + rng() % 9u;
      ExclListHost L;
      L.keyedByT = form >= 1;
      L.withInst = form == 2;
      L.perRay.resize(M);
      for (uint32_t i = 0; i < M; i++) {
        const uint32_t n = rng() % 5u; // rays without entries among them
        for (uint32_t e = 0; e < n; e++) L.perRay[i].push_back(ExclListHost::Rejected{(uint32_t)(rng() % 7u), (uint32_t)(rng() % 100u), (uint32_t)rng(), (uint32_t)(rng() % 3u)});
      }
      // the active rays of a round: a subset, in ascending order as the loop keeps them, or (every other round) shuffled
      std::vector<uint32_t> act;
      for (uint32_t i = 0; i < M; i++)
        if (rng() % 4u) act.push_back(i);
      if (round & 1u) std::shuffle(act.begin(), act.end(), rng);
      L.flatten(act);
      const size_t words = L.withInst ? 2 : L.keyedByT ? 1 : 0;
      if (L.off.size() != act.size() + 1) return fail("offset count", form, round);
      if (L.tbits.size() != L.pairs.size() * words) return fail("words per entry", form, round);
      const size_t bytes = L.deviceBytes();
      if (bytes % 16 != 0) return fail("deviceBytes not a multiple of 16", form, round);
      if (bytes < L.off.size() * 4 + L.pairs.size() * 8 + L.tbits.size() * 4) return fail("deviceBytes too small", form, round);
      char* D = (char*)malloc(bytes ? bytes : 1); // malloc: 16-byte aligned, as the device allocation is
      L.image(D);
      const uint32_t* off = (const uint32_t*)D;
      const ExclListHost::Pair* pairs = (const ExclListHost::Pair*)(D + ExclListHost::a16(L.offBytes()));
      const char* dT = (const char*)pairs + ExclListHost::a16(L.pairBytes());
      if (((uintptr_t)dT & 15) != 0 || ((uintptr_t)pairs & 15) != 0) return fail("array alignment", form, round);
      if (off[0] != 0) return fail("first offset", form, round);
      for (size_t k = 0; k < act.size(); k++) {
        const std::vector<ExclListHost::Rejected>& want = L.perRay[act[k]];
        if (off[k + 1] - off[k] != want.size()) return fail("entries of a ray", form, round);
        for (uint32_t e = off[k]; e < off[k + 1]; e++) {
          const ExclListHost::Rejected& w = want[e - off[k]];
          if (pairs[e].x != w.geomID || pairs[e].y != w.primID) return fail("pair", form, round);
          if (words == 1 && ((const uint32_t*)dT)[e] != w.tbits) return fail("t", form, round);
          if (words == 2) {
            uint64_t both; // the kernel's one 8-byte load
            memcpy(&both, dT + (size_t)e * 8, 8);
            if ((uint32_t)both != w.tbits || (uint32_t)(both >> 32) != w.instID) return fail("t and instance", form, round);
          }
          entriesChecked++;
        }
      }
      if (off[act.size()] != L.pairs.size()) return fail("last offset", form, round);
      free(D);
    }
  }
  printf("excl_list_check: ok (%zu entries read back)\n", entriesChecked);
  return 0;
}
