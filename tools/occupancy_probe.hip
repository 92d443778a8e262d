// occupancy_probe.hip -- what the HIP runtime says about the residency of the two product traversal kernels: one-wave workgroups per
// CU (hipOccupancyMaxActiveBlocksPerMultiprocessor) against the dynamic LDS size, for the sizes the stacks of wide8 trees ask for and
// for a sweep from which the LDS allocation granule can be read (the count changes only where the charge crosses a granule).
// The kernels are those of a csrc/ directory, compiled into the probe with the flags csrc/Makefile gives wf_traverse.hip:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -mllvm -amdgpu-sched-strategy=max-memory-clause \
//         -fno-slp-vectorize -I vk-raytracing-engine_amd/csrc -I include -o tools/build/occupancy_probe tools/occupancy_probe.hip
// (-I <a checkout of the parent's csrc> gives the parent's side.)  Launches nothing; prints one JSON object.
#include "wf_traverse.hip"

#include <cstdio>

template <typename K>
static void report(const char* name, K kernel, bool last)
{
  hipFuncAttributes a{};
  hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(kernel));
  printf(" \"%s\": {\"attr_error\": %d, \"vgprs\": %d, \"static_lds_bytes\": %zu, \"scratch_bytes\": %zu,\n", name, (int)e, a.numRegs, a.sharedSizeBytes,
         a.localSizeBytes);
  // wide8 trees: stackCap = 2 * (depth + 1) words per lane, 64 lanes
  printf("  \"workgroups_per_cu_by_wide_depth\": {");
  for(int depth = 4; depth <= 14; depth++)
  {
    int n = -1;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 64, (size_t)(2 * (depth + 1)) * 64 * 4);
    printf("\"%d\": %d%s", depth, e == hipSuccess ? n : -(int)e, depth < 14 ? ", " : "");
  }
  printf("},\n  \"sweep\": {\"step_bytes\": 64, \"note\": \"[dynamic LDS bytes, workgroups per CU] where the count changes\", \"changes\": [");
  int prev = -2;
  bool first = true;
  for(size_t dyn = 0; dyn <= 40960; dyn += 64)
  {
    int n = -1;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 64, dyn);
    if(e != hipSuccess) n = -(int)e;
    if(n != prev)
    {
      printf("%s[%zu, %d]", first ? "" : ", ", dyn, n);
      first = false;
      prev = n;
    }
  }
  printf("]}}%s\n", last ? "" : ",");
}

int main()
{
  hipDeviceProp_t prop{};
  if(hipGetDeviceProperties(&prop, 0) != hipSuccess)
  {
    fprintf(stderr, "no device\n");
    return 1;
  }
  printf("{\"device\": \"%s\", \"arch\": \"%s\", \"cus\": %d, \"lds_bytes_per_cu\": %zu, \"lds_bytes_per_workgroup\": %zu,\n", prop.name, prop.gcnArchName,
         prop.multiProcessorCount, prop.maxSharedMemoryPerMultiProcessor, prop.sharedMemPerBlock);
  report("k_wf_traverse<false, true, 64, 0>", k_wf_traverse<false, true, 64, 0>, false);
  report("k_wf_traverse_camera<false, 0>", k_wf_traverse_camera<false, 0>, true);
  printf("}\n");
  return 0;
}
