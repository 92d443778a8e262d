// node_update.h -- moving instances from device memory (node_update.hip): the device side of vkrt_scene_update_node_transforms and of
// vkrt_scene_set_instance_visibility.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_scene.h"

namespace vkrt {

// New transforms from device memory, one launch on `stream`, no allocation, no host synchronisation.  matrices: [count][16] floats,
// column-major, 16-byte aligned.  indices == nullptr: entry k moves node first + k (the caller has checked the range); else entry k moves
// node indices[k], and an index >= nodeCount skips its entry.  Each record keeps its primMesh, its visibility bits 0-15 and its pad; o2w,
// w2o and the mirrored bit are instance_record.h's of the new matrix, bit for bit what make_instance writes on the host.
hipError_t launch_node_transforms(DevInstance* table, uint32_t nodeCount, uint32_t first, uint32_t count, const float* matrices, const uint32_t* indices,
                                  hipStream_t stream);

// The visibility words of records [first, first + count): (old & VKRT_VIS_MIRRORED) | words[k], words[k] = mask | flags << 8.  The words
// travel as kernel arguments of launches on `stream` (like upload_instances' records: nothing staged, no synchronisation); everything else
// of a record stays, so a transform that the host copy has not seen stays too.
hipError_t launch_instance_visibility(DevInstance* table, uint32_t first, uint32_t count, const uint32_t* words, hipStream_t stream);

}  // namespace vkrt
