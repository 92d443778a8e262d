// lbvh.h -- device LBVH builder entry (see lbvh.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/vkrt.h"
#include "dev_buffer.h"
#include "device_scene.h"

namespace vkrt {

// Device-side collapse of the binary tree into the 8-wide compressed layout (wide_collapse.hip).  bin: the BVH2 over T triangles, one per
// leaf (k_emit with leaf size 1): node i = radix-tree node i, whose parents (k_hierarchy) come with it; its records in sorted (leaf) order.
// A tree deeper than the level budget leaves `out` empty: the caller collapses it on the host instead.
int collapse_wide8_device(uint32_t T, const TreeBuffers& bin, const int* parentInternal, const int* parentLeaf, hipStream_t stream, BuiltTree& out,
                          std::string& err);

// What the device build makes of the scene: the binary layout always, the wide one when asked for and the collapse fits its level budget
// (otherwise the caller collapses `tree` on the host).
struct LbvhResult
{
  BuiltTree tree;  // BVH2, 64 B per node
  BuiltTree wide;  // wide8, or empty
  uint32_t triCount = 0;    // triangle SLOTS = references (leaves) of the tree
  uint32_t uniqueTris = 0;  // instanced triangles (== triCount without pre-splitting)
  std::string error;
};

struct LbvhParams
{
  bool wide = false;          // collapse into the wide layout as well (the binary tree then keeps one triangle per leaf)
  bool ploc = false;          // cluster (ploc.hip) instead of the Morton radix tree
  unsigned splitPercent = 0;  // budget of extra references for triangle pre-splitting, in percent of the triangle count (0 = off)
};

// Binary hierarchy over the Morton-sorted triangles by parallel locally-ordered clustering (ploc.hip): fills the same arrays as
// k_hierarchy + k_fit of lbvh.hip (children, parents, boxes; range[i] = (0, triangles below i - 1)); node 0 is the root.
int ploc_cluster_device(uint32_t T, const unsigned* order, const float* triBox, hipStream_t stream, int2* children, int2* range, int* parentInternal,
                        int* parentLeaf, float* nodeBox, std::string& err);

// sc must already hold the uploaded positions / indices / instances and the watertight / dissolve settings of the build.
int build_lbvh_device(const DevScene& sc, uint32_t instCount, const std::vector<vkrt_prim_mesh>& pm, const std::vector<vkrt_node>& nodes,
                      const LbvhParams& p, hipStream_t stream, LbvhResult& out);

// What triangle pre-splitting makes of the scene for a budget of splitPercent % (vkrt_debug_split_references): the flattening and the
// pre-split stage of build_lbvh_device and nothing after them, downloaded into host arrays -- the priorities [triangles] and the scale D
// (either may be null; zeros when the budget rounds to 0 splits), and the references in emission order, refTri [refCount] and
// refBox [6 x refCount]; the identity list with the whole-triangle boxes when nothing was split.  A capacity below triangles + budget
// is VKRT_ERR_INVALID_ARGUMENT and writes nothing.  No tree is built or touched.
int split_references_device(const DevScene& sc, uint32_t instCount, const std::vector<vkrt_prim_mesh>& pm, const std::vector<vkrt_node>& nodes,
                            unsigned splitPercent, hipStream_t stream, float* prio, float* scale, uint32_t* refTri, float* refBox, uint64_t capacity,
                            uint32_t* refCount, std::string& err);

}  // namespace vkrt
