// vertex_record.h -- what skin.hip, morph.hip and vertex_update.hip share: the vector types of a vertex's words, the captured pose of a
// vertex range (a skin's bind pose, a morph's base shape) with its layout, loads and stores, and the stores of a live vertex.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "device_scene.h"

namespace vkrt {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f3 __attribute__((ext_vector_type(3)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f3u __attribute__((ext_vector_type(3), aligned(4)));  // the scene's own vec3 positions, and a morph's deltas

static_assert(VKRT_VERTEX_QUADS == 3, "the vertex kernels read and write the three float4 of a vertex record");

// device_math.h normalize3, guarded: a zero or overflowing length leaves the vector as it is
__device__ __forceinline__ f3 normalizeGuarded(f3 a)
{
  const float d = (a.x * a.x + a.y * a.y) + a.z * a.z;
  if(d > 0.0f && d < __builtin_inff())
  {
    const float inv = 1.0f / sqrtf(d);
    return a * inv;
  }
  return a;
}

// The captured pose of `count` vertices, 40 B each: the words of their vertexPN records without the uv.  Every array starts 16-byte
// aligned when the allocation does.
struct Pose
{
  float4* pn = nullptr;   // position.xyz, normal.x
  float4* tan = nullptr;  // tangent.xyzw
  float2* nyz = nullptr;  // normal.yz
  Pose at(size_t vertex) const { return Pose{pn + vertex, tan + vertex, nyz + vertex}; }
};

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
inline size_t pose_bytes(uint32_t count) { return 2 * (size_t)count * 16 + align16((size_t)count * 8); }
// the pose at the start of `mem`; returns the first byte behind it
inline char* pose_carve(char* mem, uint32_t count, Pose& out)
{
  out.pn = (float4*)mem;
  out.tan = out.pn + count;
  out.nyz = (float2*)(out.tan + count);
  return mem + pose_bytes(count);
}

struct PoseVertex
{
  f3 p, n, t;
  float tw;  // the tangent's handedness, carried as captured
};

__device__ __forceinline__ PoseVertex pose_load(const Pose& b, uint32_t i)
{
  const float4 b0 = b.pn[i];
  const float2 b1 = b.nyz[i];
  const float4 b2 = b.tan[i];
  return PoseVertex{{b0.x, b0.y, b0.z}, {b0.w, b1.x, b1.y}, {b2.x, b2.y, b2.z}, b2.w};
}

__device__ __forceinline__ void pose_store(const Pose& b, uint32_t i, const PoseVertex& m)
{
  b.pn[i] = make_float4(m.p.x, m.p.y, m.p.z, m.n.x);
  b.nyz[i] = make_float2(m.n.y, m.n.z);
  b.tan[i] = make_float4(m.t.x, m.t.y, m.t.z, m.tw);
}

// Live vertex v: the vec3 position as a three-dword store, quad 0 and the tangent as four-dword stores, normal.yz as a two-dword
// store that leaves the uv words beside it alone.
__device__ __forceinline__ void live_store(float* positions, float4* vertexPN, size_t v, const PoseVertex& m)
{
  float* rec = (float*)(vertexPN + VKRT_VERTEX_QUADS * v);  // 48 B, 16-byte aligned
  *(f3u*)(positions + 3 * v) = m.p;
  *(f4*)rec = f4{m.p.x, m.p.y, m.p.z, m.n.x};        // quad 0 = position.xyz, normal.x
  *(f2*)(rec + 4) = f2{m.n.y, m.n.z};                // quad 1 = normal.yz, uv (kept)
  *(f4*)(rec + 8) = f4{m.t.x, m.t.y, m.t.z, m.tw};   // quad 2 = tangent
}

}  // namespace vkrt
