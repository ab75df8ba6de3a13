// What the two units of the subdivision two-level kernel share: trace_instance_subdiv.hip (where the kernel is described; swept top-level
// boxes, kinds 24 / 25) and trace_instance_subdiv_top_linear.hip (its TOPMB form, kinds 34 / 35) - the two leaves' headers and the form of
// a kernel.  The kernel's text is trace_instance_body.hip.h, the launcher launch_instance_pair, the wave bound instance_min_waves
// (trace_instance.hip.h), as for the mesh family.
#pragma once
#include "trace_instance.hip.h"
#include "trace_grid.hip.h"
#include "trace_cbvh.hip.h"

namespace rtamd {
namespace dev {

template <typename Leaf> constexpr InstanceForm instance_subdiv_form(bool occluded, bool vec, bool topmb)
{
  InstanceForm f;
  f.OCCLUDED = occluded; f.VEC = vec;
  f.SUBDIV = f.XFMB = true; // every instantiation takes instances with transform time steps
  f.GRID = std::is_same<Leaf, GridCellLeaf>::value;
  f.NODEMB = f.TOPMB = topmb; // time-dependent nodes at top level or nowhere
  return f;
}

} // namespace dev
} // namespace rtamd
