// The exclusion lists of the host filter loop (rt_filter.cpp) in their host form: what the callbacks rejected, per ray, and the flattened
// arrays a re-trace uploads.  Plain C++ without HIP, so that tools/excl_list_check.cpp can run it under a sanitizer.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rtamd {

struct ExclListHost
{
  struct Rejected { uint32_t geomID, primID, tbits, instID; };
  struct Pair { uint32_t x, y; }; // the layout of a device uint2
  bool keyedByT = false; // grid cells and quads: a candidate is (geomID, primID, bits of t); triangles: (geomID, primID)
  bool withInst = false; // candidates below an instance (always keyed by t): the instance's geomID beside t, two words per entry in `tbits`
  std::vector<std::vector<Rejected>> perRay; // by ray of the batch
  std::vector<uint32_t> off, tbits;
  std::vector<Pair> pairs;
  static size_t a16(size_t n) { return (n + 15) & ~(size_t)15; }

  // the lists of the rays act[0..], in that order: off[k] .. off[k + 1] are the entries of ray act[k] (LaunchParams::exclOffsets is
  // indexed by the ray's index in the compacted batch); entry e is pairs[e] and tbits[e] or, withInst, tbits[2e] = bits of t and
  // tbits[2e + 1] = instance geomID (trace.h)
  void flatten(const std::vector<uint32_t>& act)
  {
    off.assign(act.size() + 1, 0);
    pairs.clear();
    tbits.clear();
    for (size_t k = 0; k < act.size(); k++) {
      off[k] = (uint32_t)pairs.size();
      for (const Rejected& e : perRay[act[k]]) {
        pairs.push_back(Pair{e.geomID, e.primID});
        if (keyedByT || withInst) tbits.push_back(e.tbits);
        if (withInst) tbits.push_back(e.instID);
      }
    }
    off[act.size()] = (uint32_t)pairs.size();
  }
  // three arrays, each from a multiple of 16 bytes on (the two-word entries of `tbits` are read as 8-byte words)
  size_t offBytes() const { return off.size() * 4; }
  size_t pairBytes() const { return pairs.size() * sizeof(Pair); }
  size_t tBytes() const { return tbits.size() * 4; }
  size_t deviceBytes() const { return a16(offBytes()) + a16(pairBytes()) + a16(tBytes()); }
  // the image of deviceBytes() bytes that upload() (rt_filter.cpp) leaves on the device
  void image(char* D) const
  {
    char* dPairs = D + a16(offBytes());
    char* dT = dPairs + a16(pairBytes());
    for (size_t i = 0; i < off.size(); i++) ((uint32_t*)D)[i] = off[i];
    for (size_t i = 0; i < pairs.size(); i++) ((Pair*)dPairs)[i] = pairs[i];
    for (size_t i = 0; i < tbits.size(); i++) ((uint32_t*)dT)[i] = tbits[i];
  }
};

} // namespace rtamd
