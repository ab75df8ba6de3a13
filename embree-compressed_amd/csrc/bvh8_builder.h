// Host builder: binned-SAH binary tree collapsed into 8-wide nodes, then quantized into QNode8 records.
//
// This is new code, not a restatement: the reference's builders (kernels/builders/*, bvh_builder_sah.cpp)
// are outside the hot path and tree shape does not change which hit is closest.
// What is kept from the reference are the leaf-size conventions of BVHNBuilderSAH<8,...,Triangle4v>
// (bvh_builder_sah.cpp:651-658: SAH block size 4, leaves of up to 7 blocks) and of the subdiv builders
// (bvh_builder_subdiv.cpp:845-851: exactly one primitive per leaf).
#pragma once
#include <functional>

#include "accel.h"
#include "rt_common.h"

namespace rtamd {

struct BuildPrim
{
  Box3 box;
  uint32_t id; // index into the caller's primitive list
};

struct BuildSettings
{
  uint32_t blockSize = 4;    // SAH cost counts ceil(n/blockSize) intersections
  uint32_t minLeaf = 4;      // never split at or below this size
  uint32_t maxLeaf = 28;     // always split above this size
  float travCost = 1.0f;
  float intCost = 1.0f;
  unsigned threads = 1;      // host threads for the upper levels of the binary tree (subtrees above 64 k primitives)
};

struct BuildResult
{
  std::vector<QNode8> nodes;
  uint32_t root = REF_EMPTY;
  uint32_t maxDepth = 0;
  size_t leafCount = 0;
};

// makeLeaf(prims, begin, end) -> leaf reference (REF_LEAF | payload); prims[begin,end) is the final
// leaf order (the builder permutes the array in place).
using MakeLeafFn = std::function<uint32_t(const BuildPrim* prims, size_t begin, size_t end)>;

BuildResult build_bvh8(std::vector<BuildPrim>& prims, const BuildSettings& settings, const MakeLeafFn& makeLeaf);

// Quantize the boxes of up to 8 children into one node; exported for the unit tests of the codec.
void quantize_node(const Box3* childBoxes, const uint32_t* childRefs, int n, QNode8& out);
// Decode child i of a node with exactly the arithmetic the kernels use.
Box3 dequantize_child(const QNode8& node, int i);


// ---- time-dependent nodes (mb_bounds=linear, accel.h QNodeMB8) ----------------------------------------------------------------------
// The same binned-SAH build and collapse over the boxes the caller put into `prims` (for the motion-blur accels: every record's box at
// the midpoint of its time segment); the boxes stored in the nodes do not come from `prims` but from linearBounds(prims, begin, end,
// b0, b1), called once per child of every node with the child's final, contiguous range of `prims`: two boxes, at time 0 and at time 1,
// whose linear interpolation holds everything below the child at every time the records below are valid.
struct BuildResultMB
{
  std::vector<QNodeMB8> nodes;
  uint32_t root = REF_EMPTY;
  uint32_t maxDepth = 0;
  size_t leafCount = 0;
};
using LinearBoundsFn = std::function<void(const BuildPrim* prims, size_t begin, size_t end, Box3& b0, Box3& b1)>;
BuildResultMB build_bvh8_mb(std::vector<BuildPrim>& prims, const BuildSettings& settings, const MakeLeafFn& makeLeaf, const LinearBoundsFn& linearBounds);

// Quantize the end boxes (time 0, time 1) of up to 8 children into one node, every plane at least one and less than two grid steps
// outside its box (the guarantee and its argument: accel.h QNodeMB8); exported for the unit tests of the codec.
void quantize_node_mb(const Box3* childBoxes0, const Box3* childBoxes1, const uint32_t* childRefs, int n, QNodeMB8& out);
// Decode child i of a node at ray time t with exactly the arithmetic the kernels use.
Box3 dequantize_child_mb(const QNodeMB8& node, int i, float t);

} // namespace rtamd
