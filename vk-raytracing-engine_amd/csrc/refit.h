// refit.h -- moving instances without a rebuild (refit.hip): instance-record uploads and the refit of a built tree.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "dev_buffer.h"
#include "device_scene.h"

namespace vkrt {

// Scratch of the refit, owned by the scene and valid for one build (allocated at the first refit after a build, freed by the next build):
// the tree's nodes grouped by depth level (derived from the node words on the device), one exact float box and one SAH term per node.
struct RefitScratch
{
  DevBuf mem;                    // one allocation for everything below
  float* box = nullptr;          // [nodeCap][6]: lo.xyz, hi.xyz of every node reached from the root
  float* cost = nullptr;         // [nodeCap]: SAH terms of the node (0 for array entries that are not part of the tree)
  uint32_t* list = nullptr;      // [nodeCap]: node ids, level after level (root first)
  uint32_t* words = nullptr;     // [0] list tail, [1] bad references seen while deriving the levels, [2] SAH cost of the last refit (float bits)
  uint32_t nodeCap = 0;          // node array entries
  std::vector<uint32_t> levelStart;  // host copy: level L = list[levelStart[L], levelStart[L + 1])
};

// Node records [first, first + count) of the instance table, enqueued on `stream` (the records travel as kernel arguments: nothing is
// staged on the host, so the caller may reuse its array at once and no host synchronisation is needed).
hipError_t upload_instances(DevInstance* table, uint32_t first, uint32_t count, const DevInstance* src, hipStream_t stream);

// First refit after a build: allocate the scratch and derive the level lists (synchronises `stream` once per level).
int refit_prepare(const DevScene& sc, uint32_t nodeCap, hipStream_t stream, RefitScratch& rs, std::string& err);

// The refit itself, enqueued on `stream` without host synchronisation or allocation: triangle records from the current instance
// table, then the node boxes level by level from the deepest to the root, then the SAH cost into rs.words[2].
int refit_enqueue(const DevScene& sc, uint32_t instCount, const RefitScratch& rs, hipStream_t stream, std::string& err);

}  // namespace vkrt
