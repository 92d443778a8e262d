// refit.hip -- moving instances without a rebuild: the device side of vkrt_scene_update_nodes and vkrt_accel_refit (include/vkrt.h).
//
// The Vulkan interface that vkrt_accel_build stands in for refits a built acceleration structure in place
// (VK_BUILD_ACCELERATION_STRUCTURE_ALLOW_UPDATE_BIT_KHR + VK_BUILD_ACCELERATION_STRUCTURE_MODE_UPDATE_KHR): same topology, new boxes.
// Here the topology of either layout lives entirely in words a refit never writes -- wide8: imask, childBase, triBase, meta bytes
// (bvh_host.h); BVH2: child0 / child1 (device_scene.h) -- so one refit serves every builder, with or without pre-split references:
//   k_rf_tris    one lane per triangle SLOT: the record's instance word + its shading record's vertex indices -> the 9 geometry floats,
//                written with the helpers k_flatten uses (tri_prep.h), so they are bit for bit those of a fresh build; id words untouched
//   k_rf_w8 /    one launch per depth level, deepest first: a node's slot boxes from its children's exact float boxes (scratch) or from
//   k_rf_b2      vkrt_tri_bounds of its leaf records, re-encoded with the collapse's quantisation (wide_node.h) / stored as floats (BVH2)
//   k_rf_finish  the SAH cost of the refitted tree, reduced in a fixed order into one device word
// Level launches rather than a bottom-up walk with arrival counters: a node's children are finished by the kernel boundary before it
// is read, with no cross-workgroup hand-off inside a launch (L1 is per CU and not refreshed by other CUs' stores).  The levels are
// derived once per build from the node words (k_rf_expand), at the first refit.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/vkrt.h"
#include "refit.h"
#include "tri_prep.h"
#include "wide_node.h"

namespace vkrt {

namespace {

constexpr uint32_t kInstancesPerLaunch = 40;  // 8 + 40 x 96 B of kernel arguments (limit 4 KiB)
constexpr int kMaxLevels = 64;                // the LDS traversal stack bounds any tree the builders accept to fewer levels than this

struct InstanceBatch
{
  uint32_t first, count;
  DevInstance rec[kInstancesPerLaunch];
};

__global__ void k_rf_instances(InstanceBatch b, DevInstance* table)
{
  const uint32_t i = threadIdx.x;
  if(i < b.count)
    table[b.first + i] = b.rec[i];
}

__device__ inline float rfArea(const float* lo, const float* hi)
{
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  return 2.f * (dx * dy + dy * dz + dz * dx);
}

// the box a builder starts from for the triangle of one record (tri_prep.h), re-derived from the record's geometry floats
__device__ inline void recordBounds(const float4* __restrict__ tris, uint32_t slot, int watertight, float lo[3], float hi[3])
{
  const float4 a = tris[3 * (size_t)slot + 0], b = tris[3 * (size_t)slot + 1], c = tris[3 * (size_t)slot + 2];
  const float p0[3] = {a.x, a.y, a.z}, r1[3] = {a.w, b.x, b.y}, r2[3] = {b.z, b.w, c.x};
  float e1[3], e2[3];
  for(int k = 0; k < 3; k++)
  {
    e1[k] = watertight ? r1[k] - p0[k] : r1[k];
    e2[k] = watertight ? r2[k] - p0[k] : r2[k];
  }
  vkrt_tri_bounds(p0, r1, r2, e1, e2, watertight, lo, hi);  // (p1 / p2 are read only when watertight, where r1 / r2 are them)
}

__global__ void k_rf_tris(uint32_t T, const float* __restrict__ positions, const DevInstance* __restrict__ instances, uint32_t instCount,
                          const uint4* __restrict__ shade, float4* tris, int watertight)
{
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if(s >= T)
    return;
  const float4 c = tris[3 * (size_t)s + 2];
  const uint32_t inst = __float_as_uint(c.z);
  if(inst >= instCount)
    return;
  const uint4 ix = shade[s];  // absolute vertex indices of the slot's triangle (indices[firstIndex + 3 prim + k] + vertexOffset)
  const uint32_t ii[3] = {ix.x, ix.y, ix.z};
  float o2w[12];
  for(int k = 0; k < 12; k++) o2w[k] = instances[inst].o2w[k];
  float p[3][3];
#pragma unroll
  for(int k = 0; k < 3; k++)
  {
    const float q[3] = {positions[3 * (size_t)ii[k]], positions[3 * (size_t)ii[k] + 1], positions[3 * (size_t)ii[k] + 2]};
    vkrt_xform_point(o2w, q, p[k]);
  }
  float g[9], e1[3], e2[3];
  vkrt_tri_record(p[0], p[1], p[2], watertight, g, e1, e2);
  tris[3 * (size_t)s + 0] = make_float4(g[0], g[1], g[2], g[3]);
  tris[3 * (size_t)s + 1] = make_float4(g[4], g[5], g[6], g[7]);
  tris[3 * (size_t)s + 2] = make_float4(g[8], c.y, c.z, c.w);
}

// level L -> level L + 1: every internal child of the level's nodes is appended to the list (order inside a level does not matter)
__global__ void k_rf_expand(uint32_t layout, const uint4* __restrict__ nodes, uint32_t* list, uint32_t start, uint32_t count, uint32_t nodeCap,
                            uint32_t* words)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if(t >= count)
    return;
  const uint32_t n = list[start + t];
  uint32_t child[8];
  int nc = 0;
  if(layout == 1u)
  {
    const uint4 a = nodes[(size_t)n * VKRT_WNODE_QUADS], b = nodes[(size_t)n * VKRT_WNODE_QUADS + 1];
    const uint32_t imask = a.w >> 24;
    for(int s = 0; s < 8; s++)
      if((imask >> s) & 1u) child[nc++] = b.x + (uint32_t)__popc(imask & ((1u << s) - 1u));
  }
  else
  {
    const uint4 q3 = nodes[(size_t)n * VKRT_NODE_QUADS + 3];
    if((int)q3.x >= 0) child[nc++] = q3.x;
    if((int)q3.y >= 0) child[nc++] = q3.y;
  }
  for(int k = 0; k < nc; k++)
  {
    const uint32_t pos = child[k] < nodeCap ? atomicAdd(&words[0], 1u) : nodeCap;
    if(pos < nodeCap)
      list[pos] = child[k];
    else
      atomicAdd(&words[1], 1u);
  }
}

__global__ void k_rf_w8(const uint32_t* __restrict__ list, uint32_t start, uint32_t count, uint4* nodes, const float4* __restrict__ tris, uint32_t T,
                        int watertight, float* box, float* cost)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if(t >= count)
    return;
  const uint32_t n = list[start + t];
  uint4* nd = nodes + (size_t)n * VKRT_WNODE_QUADS;
  const uint4 a = nd[0], b = nd[1];
  const uint32_t imask = a.w >> 24, childBase = b.x, triBase = b.y;
  float slo[8][3], shi[8][3];
  uint32_t slotMask = 0, cnt[8];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for(int s = 0; s < 8; s++)
  {
    const uint32_t meta = ((s < 4 ? b.z : b.w) >> (8 * (s & 3))) & 255u;
    cnt[s] = 0;
    for(int q = 0; q < 3; q++) { slo[s][q] = INFINITY; shi[s][q] = -INFINITY; }
    if(meta == 0u)
      continue;
    slotMask |= 1u << s;
    if((imask >> s) & 1u)
    {  // internal child: its exact box, finished by the previous (deeper) level's launch
      const float* cb = box + 6 * (size_t)(childBase + (uint32_t)__popc(imask & ((1u << s) - 1u)));
      for(int q = 0; q < 3; q++) { slo[s][q] = cb[q]; shi[s][q] = cb[3 + q]; }
    }
    else
    {  // leaf: the union of its records' boxes (a pre-split reference gets its whole triangle's box: looser, still conservative)
      cnt[s] = (uint32_t)__popc(meta >> 5);
      for(uint32_t k = 0; k < cnt[s]; k++)
      {
        const uint32_t slot = triBase + (meta & 31u) + k;
        if(slot >= T)
          continue;
        float tl[3], th[3];
        recordBounds(tris, slot, watertight, tl, th);
        for(int q = 0; q < 3; q++) { slo[s][q] = fminf(slo[s][q], tl[q]); shi[s][q] = fmaxf(shi[s][q], th[q]); }
      }
    }
    for(int q = 0; q < 3; q++) { lo[q] = fminf(lo[q], slo[s][q]); hi[q] = fmaxf(hi[q], shi[s][q]); }
  }
  uint32_t eb[3];
  uint16_t qlo[3][8], qhi[3][8];
  vkrt_wnode_quantise(lo, hi, slotMask, slo, shi, eb, qlo, qhi);
  uint32_t w[VKRT_WNODE_DWORDS];
  vkrt_wnode_store_planes(w, qlo, qhi);
  nd[0] = make_uint4(__float_as_uint(lo[0]), __float_as_uint(lo[1]), __float_as_uint(lo[2]), eb[0] | (eb[1] << 8) | (eb[2] << 16) | (imask << 24));
  for(int k = 2; k < VKRT_WNODE_QUADS; k++) nd[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
  for(int q = 0; q < 3; q++) { box[6 * (size_t)n + q] = lo[q]; box[6 * (size_t)n + 3 + q] = hi[q]; }
  // the SAH terms of the node as k_w8_write accumulates them (traversal 1, intersection 1)
  double sah = (double)rfArea(lo, hi);
  for(int s = 0; s < 8; s++)
    if(cnt[s]) sah += (double)rfArea(slo[s], shi[s]) * cnt[s];
  cost[n] = (float)sah;
}

__global__ void k_rf_b2(const uint32_t* __restrict__ list, uint32_t start, uint32_t count, float4* nodes, const float4* __restrict__ tris, uint32_t T,
                        int watertight, float* box, float* cost)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if(t >= count)
    return;
  const uint32_t n = list[start + t];
  float4* nd = nodes + (size_t)n * VKRT_NODE_QUADS;
  const float4 q3 = nd[3];
  const int ref[2] = {__float_as_int(q3.x), __float_as_int(q3.y)};
  float bx[2][6];
  double leaf = 0.0;
  for(int c = 0; c < 2; c++)
  {
    float* lo = bx[c];
    float* hi = bx[c] + 3;
    for(int q = 0; q < 3; q++) { lo[q] = INFINITY; hi[q] = -INFINITY; }
    if(ref[c] >= 0)
    {
      const float* cb = box + 6 * (size_t)ref[c];
      for(int q = 0; q < 6; q++) bx[c][q] = cb[q];
    }
    else
    {  // leaf: ~(first slot << 3 | count - 1)
      const uint32_t code = ~(uint32_t)ref[c], first = code >> 3, cnt = (code & 7u) + 1u;
      for(uint32_t k = 0; k < cnt; k++)
      {
        if(first + k >= T)
          continue;
        float tl[3], th[3];
        recordBounds(tris, first + k, watertight, tl, th);
        for(int q = 0; q < 3; q++) { lo[q] = fminf(lo[q], tl[q]); hi[q] = fmaxf(hi[q], th[q]); }
      }
      leaf += (double)rfArea(lo, hi) * cnt;
    }
  }
  nd[0] = make_float4(bx[0][0], bx[0][1], bx[0][2], bx[0][3]);
  nd[1] = make_float4(bx[0][4], bx[0][5], bx[1][0], bx[1][1]);
  nd[2] = make_float4(bx[1][2], bx[1][3], bx[1][4], bx[1][5]);
  float lo[3], hi[3];
  for(int q = 0; q < 3; q++) { lo[q] = fminf(bx[0][q], bx[1][q]); hi[q] = fmaxf(bx[0][3 + q], bx[1][3 + q]); }
  for(int q = 0; q < 3; q++) { box[6 * (size_t)n + q] = lo[q]; box[6 * (size_t)n + 3 + q] = hi[q]; }
  cost[n] = (float)((double)rfArea(lo, hi) + leaf);
}

// SAH cost = sum of the node terms / area of the root's box, summed in the order of k_w8_finish (wide_collapse.hip)
__global__ __launch_bounds__(1024) void k_rf_finish(uint32_t nodeCap, const float* __restrict__ cost, const float* __restrict__ box, uint32_t* words)
{
  __shared__ double part[1024];
  double s = 0;
  for(uint32_t k = threadIdx.x; k < nodeCap; k += 1024) s += (double)cost[k];
  part[threadIdx.x] = s;
  __syncthreads();
  for(uint32_t off = 512; off > 0; off >>= 1)
  {
    if(threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if(threadIdx.x == 0)
  {
    const float ra = fmaxf(rfArea(box, box + 3), 1e-30f);
    words[2] = __float_as_uint((float)(part[0] / (double)ra));
  }
}

}  // namespace

hipError_t upload_instances(DevInstance* table, uint32_t first, uint32_t count, const DevInstance* src, hipStream_t stream)
{
  for(uint32_t done = 0; done < count; done += kInstancesPerLaunch)
  {
    InstanceBatch b;
    b.first = first + done;
    b.count = std::min(kInstancesPerLaunch, count - done);
    memcpy(b.rec, src + done, (size_t)b.count * sizeof(DevInstance));
    hipLaunchKernelGGL(k_rf_instances, dim3(1), dim3(64), 0, stream, b, table);
  }
  return hipGetLastError();
}

int refit_prepare(const DevScene& sc, uint32_t nodeCap, hipStream_t stream, RefitScratch& rs, std::string& err)
{
  rs = RefitScratch{};
  rs.nodeCap = nodeCap;
  const size_t boxBytes = (size_t)nodeCap * 24, costBytes = (size_t)nodeCap * 4, listBytes = (size_t)nodeCap * 4;
  VKRT_TRY(err, rs.mem.alloc(boxBytes + costBytes + listBytes + 16));
  rs.box = rs.mem.get<float>();
  rs.cost = rs.box + (size_t)nodeCap * 6;
  rs.list = (uint32_t*)(rs.cost + nodeCap);
  rs.words = rs.list + nodeCap;
  VKRT_TRY(err, hipMemsetAsync(rs.cost, 0, costBytes + listBytes + 16, stream));
  rs.levelStart.assign(1, 0u);
  if(sc.rootRef != 0 || nodeCap == 0)
    return VKRT_OK;  // no nodes (an empty scene, or a BVH2 whose root is a leaf): the refit rewrites triangle records only
  const uint32_t one = 1;  // list[0] = node 0 (zeroed above), tail = 1
  VKRT_TRY(err, hipMemcpyAsync(rs.words, &one, 4, hipMemcpyHostToDevice, stream));
  rs.levelStart.push_back(1u);
  const unsigned B = 256;
  for(int lvl = 0;; lvl++)
  {
    if(lvl >= kMaxLevels)
    {
      err = "tree deeper than the refit's level budget";
      return VKRT_ERR_UNSUPPORTED;
    }
    const uint32_t start = rs.levelStart[(size_t)lvl], count = rs.levelStart[(size_t)lvl + 1] - start;
    hipLaunchKernelGGL(k_rf_expand, dim3((count + B - 1) / B), dim3(B), 0, stream, sc.layout, (const uint4*)sc.nodes, rs.list, start, count, nodeCap,
                       rs.words);
    VKRT_TRY(err, hipGetLastError());
    uint32_t w[2];
    VKRT_TRY(err, hipMemcpyAsync(w, rs.words, 8, hipMemcpyDeviceToHost, stream));
    VKRT_TRY(err, hipStreamSynchronize(stream));
    if(w[1] != 0u)
    {
      err = "node words reference " + std::to_string(w[1]) + " children outside the node array";
      return VKRT_ERR_HIP;
    }
    if(w[0] == start + count)
      break;
    rs.levelStart.push_back(w[0]);
  }
  return VKRT_OK;
}

int refit_enqueue(const DevScene& sc, uint32_t instCount, const RefitScratch& rs, hipStream_t stream, std::string& err)
{
  const unsigned B = 256;
  const int wt = sc.watertight ? 1 : 0;
  if(sc.triCount)
    hipLaunchKernelGGL(k_rf_tris, dim3((sc.triCount + B - 1) / B), dim3(B), 0, stream, sc.triCount, sc.positions, sc.instances, instCount,
                       sc.triShade, (float4*)sc.tris, wt);
  const int levels = (int)rs.levelStart.size() - 1;
  for(int lvl = levels - 1; lvl >= 0; lvl--)
  {
    const uint32_t start = rs.levelStart[(size_t)lvl], count = rs.levelStart[(size_t)lvl + 1] - start;
    if(sc.layout == 1u)
      hipLaunchKernelGGL(k_rf_w8, dim3((count + B - 1) / B), dim3(B), 0, stream, (const uint32_t*)rs.list, start, count, (uint4*)sc.nodes, sc.tris,
                         sc.triCount, wt, rs.box, rs.cost);
    else
      hipLaunchKernelGGL(k_rf_b2, dim3((count + B - 1) / B), dim3(B), 0, stream, (const uint32_t*)rs.list, start, count, (float4*)sc.nodes, sc.tris,
                         sc.triCount, wt, rs.box, rs.cost);
  }
  if(levels > 0)
    hipLaunchKernelGGL(k_rf_finish, dim3(1), dim3(1024), 0, stream, rs.nodeCap, (const float*)rs.cost, (const float*)rs.box, rs.words);
  VKRT_TRY(err, hipGetLastError());
  return VKRT_OK;
}

}  // namespace vkrt
