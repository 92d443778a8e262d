// dev_buffer.h -- host-side owners of device memory, the built-tree record every builder fills, and the one mapping of HIP errors to
// vkrt return codes.  No device code.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/vkrt.h"
#include "device_scene.h"

namespace vkrt {

// hipError_t -> vkrt return code; a failure also leaves "<what>: <HIP's message>" in err
inline int hip_status(hipError_t e, const char* what, std::string& err)
{
  if(e == hipSuccess)
    return VKRT_OK;
  err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? VKRT_ERR_OUT_OF_MEMORY : VKRT_ERR_HIP;
}

// return the code of a failed HIP call from the enclosing function, its message in err
#define VKRT_TRY(err, expr)                                                         \
  do                                                                                \
  {                                                                                 \
    if(const int rc_ = vkrt::hip_status((expr), #expr, err); rc_ != VKRT_OK)        \
      return rc_;                                                                   \
  } while(0)

// One hipMalloc, freed by the destructor or when another DevBuf is moved over it.
class DevBuf
{
public:
  hipError_t alloc(size_t bytes)
  {
    p_.reset();
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes);
    p_.reset(e == hipSuccess ? q : nullptr);
    return e;
  }
  template <typename T = void>
  T* get() const { return (T*)p_.get(); }

private:
  struct Free { void operator()(void* p) const { (void)hipFree(p); } };
  std::unique_ptr<void, Free> p_;
};

// The staging buffer of a scene's host-sourced data: vertex update arrays, joint matrices, morph weights, the texels of a texture
// update.  One rule makes one buffer enough for all of them: a call that stages waits for its stream before it returns, so at the next put() nothing reads the buffer
// any more, and it may be overwritten, or freed to grow.  It only grows.
class StageBuf
{
public:
  struct Part
  {
    const float* src;   // host array, or NULL: no part
    size_t floats;
    const float** dev;  // where the part lies on the device (left alone without a part)
  };
  // The parts back to back, in the order given, copied on `stream`.  The caller orders them so that each starts aligned for its reader
  // (16-byte elements first), and synchronises `stream` before it returns.
  hipError_t put(std::initializer_list<Part> parts, hipStream_t stream)
  {
    size_t bytes = 0;
    for(const Part& p : parts)
      bytes += p.src ? p.floats * sizeof(float) : 0;
    if(const hipError_t e = reserve(bytes); e != hipSuccess)
      return e;
    float* at = buf_.get<float>();
    for(const Part& p : parts)
      if(p.src)
      {
        if(const hipError_t e = hipMemcpyAsync(at, p.src, p.floats * sizeof(float), hipMemcpyHostToDevice, stream); e != hipSuccess)
          return e;
        *p.dev = at;
        at += p.floats;
      }
    return hipSuccess;
  }
  // One part of any type: `bytes` from src to the start of the buffer (256-byte aligned), copied on `stream`; the same rule for the caller.
  hipError_t putBytes(const void* src, size_t bytes, const void** dev, hipStream_t stream)
  {
    if(const hipError_t e = reserve(bytes); e != hipSuccess)
      return e;
    *dev = buf_.get();
    return hipMemcpyAsync(buf_.get(), src, bytes, hipMemcpyHostToDevice, stream);
  }

private:
  hipError_t reserve(size_t bytes)
  {
    if(bytes <= bytes_)
      return hipSuccess;
    bytes_ = 0;
    if(const hipError_t e = buf_.alloc(bytes); e != hipSuccess)
      return e;
    bytes_ = bytes;
    return hipSuccess;
  }
  DevBuf buf_;
  size_t bytes_ = 0;
};

// One event / one stream, destroyed by the destructor or when another owner is moved over it.
class DevEvent
{
public:
  hipError_t create(unsigned flags = hipEventDefault)
  {
    hipEvent_t e = nullptr;
    const hipError_t rc = hipEventCreateWithFlags(&e, flags);
    p_.reset(rc == hipSuccess ? e : nullptr);
    return rc;
  }
  hipEvent_t get() const { return p_.get(); }

private:
  struct Destroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
  std::unique_ptr<std::remove_pointer_t<hipEvent_t>, Destroy> p_;
};
class DevStream
{
public:
  hipError_t create(unsigned flags)
  {
    hipStream_t q = nullptr;
    const hipError_t rc = hipStreamCreateWithFlags(&q, flags);
    p_.reset(rc == hipSuccess ? q : nullptr);
    return rc;
  }
  hipStream_t get() const { return p_.get(); }

private:
  struct Destroy { void operator()(hipStream_t q) const { (void)hipStreamDestroy(q); } };
  std::unique_ptr<std::remove_pointer_t<hipStream_t>, Destroy> p_;
};

// Typed allocations of at least 16 bytes, all freed when the arena goes: the scratch of one build, the tables of one scene.
struct DevArena
{
  std::vector<DevBuf> bufs;
  template <typename T>
  hipError_t alloc(T** p, size_t count)
  {
    bufs.emplace_back();
    const hipError_t e = bufs.back().alloc(std::max<size_t>(count * sizeof(T), 16));
    *p = bufs.back().get<T>();
    return e;
  }
};

// The tree's device buffers: nodes, then 48-B triangle and 16-B shading records (vertex indices + material) in the tree's slot order.
struct TreeBuffers
{
  DevBuf nodes, tris, triShade;
};

// What a builder produced: the buffers and what vkrt_accel_info reports about them.  An empty record (no node buffer) is no tree.
struct BuiltTree
{
  uint32_t layout = 0;  // 0 = BVH2, 1 = wide8
  int32_t rootRef = VKRT_TRAV_DONE;
  uint32_t maxDepth = 0, nodeCount = 0;
  float sahCost = 0;
  uint64_t nodeBytes = 0, triangleBytes = 0;
  TreeBuffers buf;
};

}  // namespace vkrt
