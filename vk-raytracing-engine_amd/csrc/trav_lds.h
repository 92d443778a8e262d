// trav_lds.h -- what a traversal wave of the frame kernels (wf_traverse.hip) is charged in LDS, and how many of them a CU then holds.
// api_accel.cpp takes the stack size from travStackCap when a tree is installed and decides nothing else: every depth runs the same kernels
// on the same block, and the depth alone makes the charge.  travLdsPlan states that charge for the checks: tests/test_six_waves_isa.py
// compiles this header alone, for the CPU (no HIP type), and holds the kernels' static block and the measured granule to it.
//
// A wave of k_wf_traverse / k_wf_traverse_camera takes its stack columns (stackCap words for each of 64 lanes, dynamic) and the block its
// lanes share results through (traverse_share.h: 64 x (u64 key, slot, u, v), static).  gfx950 hands LDS out in granules of 1280 B (320
// dwords: 160 KiB / 128; the runtime's occupancy query does not show it, the frame time does: profiles/r12_experiments.md #174), so six waves per SIMD --
// 24 per CU -- fit only while a wave's charge is at most five granules, 6400 B <= 163840 / 24.  With the result block at exactly one
// granule that leaves four for the stack: stackCap <= 20, a wide8 tree of depth <= 9.  A deeper tree is charged a sixth granule and runs
// at five waves per SIMD as before (21 per CU by LDS); nothing else changes for it.
#pragma once
#include <cstddef>
#include <cstdint>

#define VKRT_LDS_BYTES_PER_CU 163840u
#define VKRT_LDS_GRANULE_BYTES 1280u
#define VKRT_SIMDS_PER_CU 4u
#define VKRT_SHARE_LDS_WORDS_SIX 320  // the frame kernels' result block without the donor plane (traverse_wide8_share<..., DONOR_LDS = false>)

// Words of LDS stack per lane for a tree of `maxDepth` levels below the root.  wide8 (layout 1): at most one pending group per level,
// uint2 entries, plus `postponeRoom` reserved entries for parked triangle groups when triangles are postponed; BVH2: one word per level.
inline uint32_t travStackCap(uint32_t layout, uint32_t maxDepth, bool postpone, uint32_t postponeRoom)
{
  if(layout != 1u)
    return maxDepth + 2u;
  return 2u * (maxDepth + 1u) + (postpone ? 2u * postponeRoom : 0u);
}

struct TravLds
{
  size_t dynamicBytes;  // the stack columns of one wave (the launch's dynamic LDS size)
  size_t staticBytes;   // the result block
  size_t chargedBytes;  // their sum, rounded up to the allocation granule
  uint32_t wavesPerCu;  // one-wave workgroups a CU holds by LDS alone
  uint32_t wavesPerSimd;  // ... per SIMD, capped at the six the product kernels' registers allow
};

inline TravLds travLdsPlan(uint32_t stackCap)
{
  TravLds p;
  p.dynamicBytes = (size_t)stackCap * 64u * sizeof(uint32_t);
  p.staticBytes = (size_t)VKRT_SHARE_LDS_WORDS_SIX * sizeof(uint32_t);
  p.chargedBytes = (p.dynamicBytes + p.staticBytes + VKRT_LDS_GRANULE_BYTES - 1u) / VKRT_LDS_GRANULE_BYTES * VKRT_LDS_GRANULE_BYTES;
  p.wavesPerCu = (uint32_t)(VKRT_LDS_BYTES_PER_CU / p.chargedBytes);
  p.wavesPerSimd = p.wavesPerCu / VKRT_SIMDS_PER_CU < 6u ? p.wavesPerCu / VKRT_SIMDS_PER_CU : 6u;
  return p;
}
