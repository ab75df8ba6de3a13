// What the two units of the subdivision two-level kernel share: trace_instance_subdiv.hip (where the kernel is described; swept top-level
// boxes, kinds 24 / 25) and trace_instance_subdiv_top_linear.hip (its TOPMB form, kinds 34 / 35).  The kernel's text itself is
// trace_instance_subdiv_body.hip.h, included inside the braces of each unit's __global__ function.
#pragma once
#include <type_traits>
#include "trace_grid.hip.h"
#include "trace_cbvh.hip.h"
#include "trace_mb.hip.h"
#include "instance_xfm.h"

namespace rtamd {
namespace dev {

// Waves per SIMD the register allocator is asked for: the bound of the same leaf's top-level lane kernel (Leaf::MIN_WAVES: 3, cBVH from
// C = 4 on 2), one wave less for a closest-hit kernel that spills more than that twin (tools/kernel_resources.sh; the table is in
// docs/experiments.md, "Subdivision meshes below an instance").  The cBVH kernels compile without scratch at their twins' bounds.  The
// eager closest-hit kernel needs 36 bytes of scratch at 3 waves (168 VGPRs) where its twin has none - the lane kernel tests cells 8
// lanes per ray and does not hold GridCellLeaf::intersect with its 40 cell words at all; the ray-pool kernel, which does, takes 186
// VGPRs: 2 waves.
template <typename Leaf> struct inst_subdiv_waves
{
  static constexpr int closest = Leaf::MIN_WAVES, any = Leaf::MIN_WAVES;
};
template <> struct inst_subdiv_waves<GridCellLeaf>
{
  static constexpr int closest = GridCellLeaf::MIN_WAVES - 1, any = GridCellLeaf::MIN_WAVES;
};
template <typename Leaf, bool OCCLUDED> constexpr int inst_subdiv_min_waves() { return OCCLUDED ? inst_subdiv_waves<Leaf>::any : inst_subdiv_waves<Leaf>::closest; }

} // namespace dev
} // namespace rtamd
