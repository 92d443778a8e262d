// node_update.hip -- moving instances from device memory: the device side of vkrt_scene_update_node_transforms and of
// vkrt_scene_set_instance_visibility (include/vkrt.h).
//
// vkrt_scene_update_nodes makes its 96-B instance records on the host and sends them as kernel arguments (refit.hip k_rf_instances): right
// for a host that owns the transforms, a round trip for a caller whose simulation, crowd system or policy has just written them on the
// device.  Here the record is made where the matrix is:
//   k_nu_transforms  one lane per entry: the matrix as four 16-B loads, the last quad of the old record (primMesh, visibility), the
//                    binary64 inverse and determinant of instance_record.h -- the functions make_instance runs on the host, so the record
//                    is bit for bit the host's --, six 16-B stores.  A lane touches its own record only: no LDS, no atomics, no scratch
//   k_nu_visibility  one lane per record: the visibility word alone, (old & VKRT_VIS_MIRRORED) | mask | flags << 8, from words that travel
//                    as kernel arguments.  The transform of the record is not read or written, so the call no longer needs the host to
//                    know it
// Pure streaming; the binary64 arithmetic (27 multiplies, one division) hides under it.  What the compiler makes of k_nu_transforms
// (gfx950, -O3): the three rows that are read as 12-B loads, five full 16-B stores, and of the last quad only what changes -- w2o[8] as
// a dword and the upper half of the visibility word as a short -- so the old record is not loaded at all: 48 B read, 86 B written.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>

#include "instance_record.h"
#include "node_update.h"

namespace vkrt {

constexpr uint32_t kVisPerLaunch = 1000;  // 8 + 1000 x 4 B of kernel arguments (limit 4 KiB)

// (outside the anonymous namespace: tools/kernel_resources.py reads the kernel's name off its demangled signature)
struct VisBatch
{
  uint32_t first, count;
  uint32_t word[kVisPerLaunch];
};

namespace {

constexpr unsigned kBlock = 256;
static_assert(sizeof(DevInstance) == 6 * sizeof(uint4), "a record is six quads");

__global__ __launch_bounds__(kBlock) void k_nu_transforms(uint32_t first, uint32_t count, uint32_t nodeCount, const float4* __restrict__ matrices,
                                                          const uint32_t* __restrict__ indices, uint4* table)
{
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= count)
    return;
  const uint32_t node = indices ? indices[k] : first + k;
  if(node >= nodeCount)
    return;  // (a sparse entry that names no node; a dense range was checked on the host)
  const float4 c0 = matrices[4 * (size_t)k], c1 = matrices[4 * (size_t)k + 1], c2 = matrices[4 * (size_t)k + 2], c3 = matrices[4 * (size_t)k + 3];
  uint4* rec = table + 6 * (size_t)node;
  const uint4 old = rec[5];  // (w2o[8], primMesh, vis, pad): integer words stay integer words
  const float M[16] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
  float o2w[12], w2o[9];
  vkrt_instance_rows(M, o2w);
  vkrt_invert3x3_rows(o2w, w2o);
  const uint32_t vis = (old.z & 0xffffu) | vkrt_mirrored_bit(o2w);
  rec[0] = make_uint4(__float_as_uint(o2w[0]), __float_as_uint(o2w[1]), __float_as_uint(o2w[2]), __float_as_uint(o2w[3]));
  rec[1] = make_uint4(__float_as_uint(o2w[4]), __float_as_uint(o2w[5]), __float_as_uint(o2w[6]), __float_as_uint(o2w[7]));
  rec[2] = make_uint4(__float_as_uint(o2w[8]), __float_as_uint(o2w[9]), __float_as_uint(o2w[10]), __float_as_uint(o2w[11]));
  rec[3] = make_uint4(__float_as_uint(w2o[0]), __float_as_uint(w2o[1]), __float_as_uint(w2o[2]), __float_as_uint(w2o[3]));
  rec[4] = make_uint4(__float_as_uint(w2o[4]), __float_as_uint(w2o[5]), __float_as_uint(w2o[6]), __float_as_uint(w2o[7]));
  rec[5] = make_uint4(__float_as_uint(w2o[8]), old.y, vis, old.w);
}

__global__ __launch_bounds__(kBlock) void k_nu_visibility(VisBatch b, DevInstance* table)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= b.count)
    return;
  uint32_t* vis = &table[b.first + i].vis;
  *vis = (*vis & VKRT_VIS_MIRRORED) | b.word[i];
}

}  // namespace

hipError_t launch_node_transforms(DevInstance* table, uint32_t nodeCount, uint32_t first, uint32_t count, const float* matrices, const uint32_t* indices,
                                  hipStream_t stream)
{
  if(count == 0)
    return hipSuccess;
  hipLaunchKernelGGL(k_nu_transforms, dim3((count - 1) / kBlock + 1), dim3(kBlock), 0, stream, first, count, nodeCount, (const float4*)matrices, indices,
                     (uint4*)table);
  return hipGetLastError();
}

hipError_t launch_instance_visibility(DevInstance* table, uint32_t first, uint32_t count, const uint32_t* words, hipStream_t stream)
{
  for(uint32_t done = 0; done < count; done += kVisPerLaunch)
  {
    VisBatch b;
    b.first = first + done;
    b.count = std::min(kVisPerLaunch, count - done);
    memcpy(b.word, words + done, (size_t)b.count * sizeof(uint32_t));
    hipLaunchKernelGGL(k_nu_visibility, dim3((b.count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, b, table);
  }
  return hipGetLastError();
}

}  // namespace vkrt
