// api_denoise.cpp -- image-space passes that never touch a scene (include/vkrt.h): the diffuse denoiser (denoise.hip) and vkrt_post.
#include "scene_state.h"

using namespace vkrt;

extern "C" {

struct vkrt_denoiser
{
  int device = 0;
  uint32_t width = 0, height = 0;
  vkrt::DevBuf mem;             // one allocation: 8 planes of float4 per pixel
  float4* colour[3] = {};       // colour history / temporal result / ping-pong of the a-trous passes (roles rotate per call)
  float4* geom[2] = {};         // (position.xyz, oct normal) of the current and the previous call
  float4* mom[2] = {};          // (m1, m2, history length, 0)
  float4* rec = nullptr;        // guide record of the current call
  int hist = 0;                 // colour[hist] holds the colour history
  int cur = 0;                  // geom[cur] / mom[cur] are written by the next call
  bool hasHistory = false;
  float prevViewProj[16] = {};
};

int vkrt_denoiser_create(int device, uint32_t width, uint32_t height, vkrt_denoiser** out)
{
  if(!out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = nullptr;
  if(width == 0 || height == 0 || (uint64_t)width * height > 0x7FFFFFFFull / 4u)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "denoiser size %ux%u out of range", width, height);
  const int ndev = vkrt_device_count();
  if(ndev <= 0)
    return fail(VKRT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  if(device < 0 || device >= ndev)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "device %d outside [0,%d)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  vkrt_denoiser* dn = new vkrt_denoiser();
  dn->device = device;
  dn->width = width;
  dn->height = height;
  const size_t plane = (size_t)width * height * sizeof(float4);
  const hipError_t e = dn->mem.alloc(8 * plane);
  if(e != hipSuccess)
  {
    delete dn;
    return fail(e == hipErrorOutOfMemory ? VKRT_ERR_OUT_OF_MEMORY : VKRT_ERR_HIP, "vkrt_denoiser_create: hipMalloc: %s", hipGetErrorString(e));
  }
  float4* base = dn->mem.get<float4>();
  const size_t n = (size_t)width * height;
  for(int k = 0; k < 3; k++) dn->colour[k] = base + k * n;
  dn->geom[0] = base + 3 * n; dn->geom[1] = base + 4 * n;
  dn->mom[0] = base + 5 * n; dn->mom[1] = base + 6 * n;
  dn->rec = base + 7 * n;
  *out = dn;
  return VKRT_OK;
}

void vkrt_denoiser_destroy(vkrt_denoiser* dn)
{
  if(!dn)
    return;
  (void)hipSetDevice(dn->device);
  delete dn;
}

int vkrt_denoiser_reset(vkrt_denoiser* dn)
{
  if(!dn)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL denoiser");
  dn->hasHistory = false;
  return VKRT_OK;
}

namespace {
// vkrt_denoise_diffuse (prevPosition NULL) and vkrt_denoise_diffuse_motion: one call sequence, the temporal kernel differs
int denoiseImpl(vkrt_denoiser* dn, const vkrt_denoise_settings* settings, const GlobalUniforms* cam, const vkrt_gbuffer* g, const vkrt_nrd_planes* nrd,
                const float* prevPosition, float* out, void* hip_stream)
{
  vkrt_denoise_settings st{sizeof(vkrt_denoise_settings), 5, 32};
  if(settings)
  {
    if(settings->struct_size < sizeof(vkrt_denoise_settings))
      return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_denoise_settings.struct_size %u < %zu", settings->struct_size, sizeof(vkrt_denoise_settings));
    st = *settings;
    if(st.atrous_iterations < 0 || st.atrous_iterations > 5)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "atrous_iterations %d outside [0,5]", st.atrous_iterations);
    if(st.max_history < 1 || st.max_history > 255)
      return fail(VKRT_ERR_INVALID_ARGUMENT, "max_history %d outside [1,255]", st.max_history);
  }
  if(!cam || !g || !nrd || !out)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(!g->color || !g->position || !g->normal || !g->roughMetal)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL G-buffer plane");
  if(!nrd->viewZ || !nrd->diffRadianceHitDist)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL NRD plane (viewZ / diffRadianceHitDist)");
  if(!dn)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL denoiser");
  HIP_TRY(hipSetDevice(dn->device));
  hipStream_t stream = (hipStream_t)hip_stream;
  const int K = st.atrous_iterations;
  // colour roles: h = history (read by the temporal taps), a = temporal result, b = variance output; a-trous iteration 0 writes the
  // new history over the old one (read only by the temporal stage), then the passes alternate between the two others
  const int h = dn->hist, a = (h + 1) % 3, b = (h + 2) % 3;
  DenoiseParams D;
  memset(&D, 0, sizeof D);
  D.W = dn->width; D.H = dn->height;
  D.color = (const float4*)g->color; D.position = (const float4*)g->position; D.normal = (const float4*)g->normal;
  D.rough = (const float2*)g->roughMetal; D.viewZ = nrd->viewZ; D.radHitD = (const float4*)nrd->diffRadianceHitDist;
  D.histColor = dn->colour[h];
  D.geomPrev = dn->geom[dn->cur ^ 1]; D.geomCur = dn->geom[dn->cur];
  D.momPrev = dn->mom[dn->cur ^ 1]; D.momCur = dn->mom[dn->cur];
  D.rec = dn->rec;
  D.colorOut = dn->colour[a]; D.colorVar = dn->colour[b];
  D.out = K == 0 ? out : nullptr;
  memcpy(D.curViewProj, cam->viewProj.m, sizeof D.curViewProj);
  memcpy(D.prevViewProj, dn->prevViewProj, sizeof D.prevViewProj);
  D.useHistory = dn->hasHistory ? 1 : 0;
  D.maxHistory = st.max_history;
  D.prevPosition = (const float4*)prevPosition;
  HIP_TRY(vkrt_launch_denoise_temporal(D, K > 0, stream));
  int in = b;
  for(int i = 0; i < K; i++)
  {
    const int dst = i == 0 ? h : (in == h ? a : (in == a ? b : a));
    DenoiseAtrous A;
    A.W = dn->width; A.H = dn->height; A.step = 1 << i;
    A.rec = dn->rec; A.in = dn->colour[in]; A.outBuf = dn->colour[dst];
    A.out = i == K - 1 ? out : nullptr;
    A.color = D.color; A.position = D.position; A.normal = D.normal; A.rough = D.rough;
    HIP_TRY(vkrt_launch_denoise_atrous(A, stream));
    in = dst;
  }
  if(K == 0)
    dn->hist = a;  // the temporal result is the history
  memcpy(dn->prevViewProj, cam->viewProj.m, sizeof dn->prevViewProj);
  dn->cur ^= 1;
  dn->hasHistory = true;
  return VKRT_OK;
}
}  // namespace

int vkrt_denoise_diffuse(vkrt_denoiser* dn, const vkrt_denoise_settings* settings, const GlobalUniforms* cam, const vkrt_gbuffer* g,
                         const vkrt_nrd_planes* nrd, float* out, void* hip_stream)
{
  return denoiseImpl(dn, settings, cam, g, nrd, nullptr, out, hip_stream);
}

int vkrt_denoise_diffuse_motion(vkrt_denoiser* dn, const vkrt_denoise_settings* settings, const GlobalUniforms* cam, const vkrt_gbuffer* g,
                                const vkrt_nrd_planes* nrd, const float* prevPosition, float* out, void* hip_stream)
{
  if(!prevPosition)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_denoise_diffuse_motion: prev_position_rgba32f is NULL");
  if(((uintptr_t)prevPosition & 15u) != 0u)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_denoise_diffuse_motion: prev_position_rgba32f is not 16-byte aligned");
  return denoiseImpl(dn, settings, cam, g, nrd, prevPosition, out, hip_stream);
}

int vkrt_post(int device, const PushConstantPost* pc, uint32_t n, const float* mainImg, const float* rtImg, float* out, void* hip_stream)
{
  if(!pc || !mainImg || !out || (pc->rtMode == 0 && !rtImg))
    return fail(VKRT_ERR_INVALID_ARGUMENT, "NULL argument");
  if(vkrt_device_count() <= 0)
    return fail(VKRT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  HIP_TRY(hipSetDevice(device));
  if(n == 0)
    return VKRT_OK;
  HIP_TRY(vkrt_launch_post(pc->rtMode, pc->viewAccumulated, pc->useGI, n, mainImg, rtImg, out, (hipStream_t)hip_stream));
  return VKRT_OK;
}

}  // extern "C"
