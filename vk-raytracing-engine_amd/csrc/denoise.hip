// denoise.hip -- spatio-temporal variance-guided filter (SVGF: Schied et al., HPG 2017) for the diffuse GI term of the hybrid mode.
// It stands where the reference's commented-out NRD.Denoise call sits (main.cpp:565-602) and consumes the planes that
// vkrt_gbuffer_raycast_nrd / vkrt_hybrid_trace_nrd write.  Three stages, one thread per pixel in 16x16 tiles:
//   k_dn_temporal  decode + demodulate the GI radiance, reproject the history with the previous camera, blend colour and moments,
//                  write the per-pixel guide record (viewZ, dviewZ/dx, dviewZ/dy, oct normal) every later tap reads;
//                  k_dn_motion_temporal is the same stage with the caller's previous-position plane (moving / deforming geometry)
//   k_dn_variance  variance from the temporal moments (7x7 spatial estimate while the history is short)
//   k_dn_atrous    one edge-avoiding a-trous iteration (5x5 B3 kernel, step 2^i); iteration 0 feeds the colour history, the last
//                  one remodulates and writes out.xyz
// Every formula and its operation order is restated in tests/np_denoise.py; DESIGN.md section "Denoiser" lists them.
// Built with the library's -ffp-contract=off -fno-fast-math: no fused multiply-adds, correctly rounded / and sqrtf.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "kernels.h"

#define DN_TILE 16
#define DN_INVALID 0x80008000u  // normal word of a pixel without geometry (the oct encoding never produces -32768)

namespace {

__device__ __forceinline__ bool dnGeomValid(float4 pos, float4 nrm)  // k_hybrid's `shaded` test (hybrid.hip:320)
{
  return !(pos.x == 0.0f && pos.y == 0.0f && pos.z == 0.0f && nrm.x == 0.0f && nrm.y == 0.0f && nrm.z == 0.0f);
}

__device__ __forceinline__ float dnMinAbs(float a, float b) { return fabsf(a) <= fabsf(b) ? a : b; }
__device__ __forceinline__ float dnSign(float v) { return v >= 0.0f ? 1.0f : -1.0f; }

// Octahedral unit vector in two snorm16 halves (x low, y high)
__device__ __forceinline__ uint32_t dnOctEncode(float nx, float ny, float nz)
{
  float s = (fabsf(nx) + fabsf(ny)) + fabsf(nz);
  if(!(s > 0.0f))
    s = 1.0f;
  float vx = nx / s, vy = ny / s;
  if(!(nz >= 0.0f))
  {
    const float wx = (1.0f - fabsf(vy)) * dnSign(vx), wy = (1.0f - fabsf(vx)) * dnSign(vy);
    vx = wx; vy = wy;
  }
  const int qx = (int)rintf(fminf(fmaxf(vx, -1.0f), 1.0f) * 32767.0f);
  const int qy = (int)rintf(fminf(fmaxf(vy, -1.0f), 1.0f) * 32767.0f);
  return ((uint32_t)qx & 0xFFFFu) | (((uint32_t)qy & 0xFFFFu) << 16);
}

__device__ __forceinline__ float3 dnOctDecode(uint32_t bits)
{
  float x = (float)(int)(int16_t)(bits & 0xFFFFu) * (1.0f / 32767.0f);
  float y = (float)(int)(int16_t)(bits >> 16) * (1.0f / 32767.0f);
  const float z = (1.0f - fabsf(x)) - fabsf(y);
  const float t = fmaxf(-z, 0.0f);
  x = x + (x >= 0.0f ? -t : t);
  y = y + (y >= 0.0f ? -t : t);
  const float r = 1.0f / sqrtf((x * x + y * y) + z * z);
  return make_float3(x * r, y * r, z * r);
}

__device__ __forceinline__ float dnDot(float3 a, float3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float dnLum(float r, float g, float b) { return (0.25f * r + 0.5f * g) + 0.25f * b; }

// w_n = max(0, dot)^128 as seven squarings
__device__ __forceinline__ float dnPow128(float d)
{
  d = fmaxf(d, 0.0f);
#pragma unroll
  for(int k = 0; k < 7; k++)
    d = d * d;
  return d;
}

// Demodulation factor: the curWeight k_hybrid multiplied in (hybrid.hip:398) -- the G-buffer albedo on the diffuse branch, 1 on the
// specular one (metal * (1 - rough) >= 0.8) and where the albedo is black (max < 1e-3); channels floored at 1e-3.
__device__ __forceinline__ float3 dnAlbedo(float4 c, float4 p, float4 n, float2 rm)
{
  const float ratio = rm.y * (1.0f - rm.x);
  const float amax = fmaxf(fmaxf(c.w, p.w), n.w);
  if(!(ratio < 0.8f) || !(amax >= 1e-3f))
    return make_float3(1.0f, 1.0f, 1.0f);
  return make_float3(fmaxf(c.w, 1e-3f), fmaxf(p.w, 1e-3f), fmaxf(n.w, 1e-3f));
}

// Continuous pixel coordinate of world point X under viewProj M (column-major), primaryDir's pixel-centre convention:
// ndc = 2 (x + 0.5) / W - 1.  false: X is not in front of the camera.
__device__ __forceinline__ bool dnProject(const float* M, float X, float Y, float Z, uint32_t W, uint32_t H, float& px, float& py)
{
  const float cx = ((M[0] * X + M[4] * Y) + M[8] * Z) + M[12];
  const float cy = ((M[1] * X + M[5] * Y) + M[9] * Z) + M[13];
  const float cw = ((M[3] * X + M[7] * Y) + M[11] * Z) + M[15];
  if(!(cw > 0.0f))
    return false;
  px = ((cx / cw) * 0.5f + 0.5f) * (float)W - 0.5f;
  py = ((cy / cw) * 0.5f + 0.5f) * (float)H - 0.5f;
  return true;
}

// Exponent of the depth weight of a tap at pixel offset (ox, oy): |zq - zp| / (sigma_z |grad z . offset| + 1e-3 |zp|), sigma_z = 1
__device__ __forceinline__ float dnEz(float zp, float gx, float gy, float zq, float ox, float oy)
{
  return fabsf(zq - zp) / (1.0f * fabsf(gx * ox + gy * oy) + 1e-3f * fabsf(zp));
}

__device__ __forceinline__ bool dnPixel(uint32_t W, uint32_t H, uint32_t& x, uint32_t& y)
{
  x = blockIdx.x * DN_TILE + threadIdx.x;
  y = blockIdx.y * DN_TILE + threadIdx.y;
  return x < W && y < H;
}

__device__ __forceinline__ bool dnValidAt(const DenoiseParams& D, uint32_t q)
{
  return dnGeomValid(D.position[q], D.normal[q]);
}

}  // namespace

// The temporal stage.  MOTION (vkrt_denoise_diffuse_motion): the history is looked up where the pixel's surface point was one call ago,
// Xp = prevPosition[p].xyz -- projected under prevViewProj and held against geomPrev in the plane test -- instead of where it is now;
// prevPosition[p].w == 0 marks a surface that did not exist then (no history).  Everything else is the one code of both kernels.
template <bool MOTION>
__device__ __forceinline__ void dnTemporal(const DenoiseParams& D)
{
  uint32_t x, y;
  if(!dnPixel(D.W, D.H, x, y))
    return;
  const uint32_t p = y * D.W + x;
  const float4 pos = D.position[p], nrm = D.normal[p];
  if(!dnGeomValid(pos, nrm))
  {
    D.rec[p] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(DN_INVALID));
    D.geomCur[p] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(DN_INVALID));
    D.momCur[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  // guide record: viewZ and its screen-space gradient.  Of the two one-sided differences the one of smaller magnitude: on a smooth
  // surface that is the central difference to first order, at a depth discontinuity it is the slope of the pixel's own surface (a
  // central difference there spans the step and lets the depth weight pass taps across it).  One-sided next to a pixel without geometry.
  const float z = D.viewZ[p];
  const bool vl = x > 0 && dnValidAt(D, p - 1), vr = x + 1 < D.W && dnValidAt(D, p + 1);
  const bool vu = y > 0 && dnValidAt(D, p - D.W), vd = y + 1 < D.H && dnValidAt(D, p + D.W);
  const float zl = vl ? D.viewZ[p - 1] : 0.0f, zr = vr ? D.viewZ[p + 1] : 0.0f;
  const float zu = vu ? D.viewZ[p - D.W] : 0.0f, zd = vd ? D.viewZ[p + D.W] : 0.0f;
  const float gx = (vl && vr) ? dnMinAbs(zr - z, z - zl) : vr ? zr - z : vl ? z - zl : 0.0f;
  const float gy = (vu && vd) ? dnMinAbs(zd - z, z - zu) : vd ? zd - z : vu ? z - zu : 0.0f;
  const uint32_t oct = dnOctEncode(nrm.x, nrm.y, nrm.z);
  D.rec[p] = make_float4(z, gx, gy, __uint_as_float(oct));
  D.geomCur[p] = make_float4(pos.x, pos.y, pos.z, __uint_as_float(oct));

  // current sample: YCoCg -> linear (clamped at 0), demodulated
  const float4 c4 = D.color[p];
  const float2 rm = D.rough[p];
  const float3 f = dnAlbedo(c4, pos, nrm, rm);
  const float4 r = D.radHitD[p];
  const float t = r.x - r.z;
  const float cr = fmaxf(t + r.y, 0.0f) / f.x, cg = fmaxf(r.x + r.z, 0.0f) / f.y, cb = fmaxf(t - r.y, 0.0f) / f.z;
  const float Y = dnLum(cr, cg, cb);

  // history: bilinear taps around the reprojected position that pass the plane-distance and normal tests
  float sw = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, h1 = 0.0f, h2 = 0.0f, maxLen = 0.0f;
  float pxPrev, pyPrev, pxCur, pyCur;
  float4 Xp = pos;
  bool existed = true;
  if(MOTION)
  {
    Xp = D.prevPosition[p];
    existed = !(Xp.w == 0.0f);
  }
  if(D.useHistory && existed && dnProject(D.prevViewProj, Xp.x, Xp.y, Xp.z, D.W, D.H, pxPrev, pyPrev) &&
     dnProject(D.curViewProj, pos.x, pos.y, pos.z, D.W, D.H, pxCur, pyCur))
  {
    // q = p + screen-space motion: an unchanged camera lands exactly on the pixel (no rounding blur of the history)
    const float qx = (float)x + (pxPrev - pxCur), qy = (float)y + (pyPrev - pyCur);
    if(qx > -1.0f && qx < (float)D.W && qy > -1.0f && qy < (float)D.H)
    {
      const float x0 = floorf(qx), y0 = floorf(qy);
      const float fx = qx - x0, fy = qy - y0;
      const float3 N = make_float3(nrm.x, nrm.y, nrm.z);
      const float tol = 0.01f * fabsf(z);
      for(int j = 0; j < 2; j++)
        for(int i = 0; i < 2; i++)
        {
          const float w = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
          const int tx = (int)x0 + i, ty = (int)y0 + j;
          if(!(w > 0.0f) || tx < 0 || ty < 0 || tx >= (int)D.W || ty >= (int)D.H)
            continue;
          const uint32_t q = (uint32_t)ty * D.W + (uint32_t)tx;
          const float4 g = D.geomPrev[q];
          const uint32_t gn = __float_as_uint(g.w);
          if(gn == DN_INVALID)
            continue;
          const float3 d = make_float3(g.x - Xp.x, g.y - Xp.y, g.z - Xp.z);
          if(!(fabsf(dnDot(N, d)) <= tol) || !(dnDot(N, dnOctDecode(gn)) >= 0.9f))
            continue;
          const float4 m = D.momPrev[q];
          const float4 h = D.histColor[q];
          sw = sw + w;
          hr = hr + w * h.x; hg = hg + w * h.y; hb = hb + w * h.z;
          h1 = h1 + w * m.x; h2 = h2 + w * m.y;
          maxLen = fmaxf(maxLen, m.z);
        }
    }
  }
  float len = 1.0f, orr = cr, og = cg, ob = cb, m1 = Y, m2 = Y * Y;
  if(sw > 0.0f)
  {
    len = fminf(maxLen, (float)(D.maxHistory - 1)) + 1.0f;
    const float a = 1.0f / len;
    orr = (hr / sw) * (1.0f - a) + cr * a;
    og = (hg / sw) * (1.0f - a) + cg * a;
    ob = (hb / sw) * (1.0f - a) + cb * a;
    m1 = (h1 / sw) * (1.0f - a) + Y * a;
    m2 = (h2 / sw) * (1.0f - a) + (Y * Y) * a;
  }
  D.momCur[p] = make_float4(m1, m2, len, 0.0f);
  D.colorOut[p] = make_float4(orr, og, ob, 0.0f);
  if(D.out)  // temporal stage only (no a-trous iteration): remodulate here
  {
    D.out[4 * (size_t)p + 0] = orr * f.x;
    D.out[4 * (size_t)p + 1] = og * f.y;
    D.out[4 * (size_t)p + 2] = ob * f.z;
  }
}

__global__ __launch_bounds__(256) void k_dn_temporal(const DenoiseParams D) { dnTemporal<false>(D); }
__global__ __launch_bounds__(256) void k_dn_motion_temporal(const DenoiseParams D) { dnTemporal<true>(D); }

__global__ __launch_bounds__(256) void k_dn_variance(const DenoiseParams D)
{
  uint32_t x, y;
  if(!dnPixel(D.W, D.H, x, y))
    return;
  const uint32_t p = y * D.W + x;
  const float4 rp = D.rec[p];
  if(__float_as_uint(rp.w) == DN_INVALID)
    return;
  const float4 m = D.momCur[p];
  float var;
  if(m.z >= 4.0f)
    var = fmaxf(m.y - m.x * m.x, 0.0f);
  else
  {  // short history: moments of the 7x7 neighbourhood, weighted by the depth and normal terms
    const float3 Np = dnOctDecode(__float_as_uint(rp.w));
    float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
    for(int dy = -3; dy <= 3; dy++)
      for(int dx = -3; dx <= 3; dx++)
      {
        const int qx = (int)x + dx, qy = (int)y + dy;
        if(qx < 0 || qy < 0 || qx >= (int)D.W || qy >= (int)D.H)
          continue;
        const uint32_t q = (uint32_t)qy * D.W + (uint32_t)qx;
        const float4 rq = D.rec[q];
        if(__float_as_uint(rq.w) == DN_INVALID)
          continue;
        const float w = expf(-dnEz(rp.x, rp.y, rp.z, rq.x, (float)dx, (float)dy)) * dnPow128(dnDot(Np, dnOctDecode(__float_as_uint(rq.w))));
        const float4 mq = D.momCur[q];
        s1 = s1 + w * mq.x;
        s2 = s2 + w * mq.y;
        sw = sw + w;
      }
    const float sws = sw > 0.0f ? sw : 1.0f;  // sw > 0 at a pixel with geometry (its own tap); the guard mirrors the restatement
    const float a = s1 / sws, b = s2 / sws;
    var = fmaxf(b - a * a, 0.0f) * (4.0f / m.z);
  }
  const float4 c = D.colorOut[p];
  D.colorVar[p] = make_float4(c.x, c.y, c.z, var);
}

// Address of tap (qx, qy), clamped into the image: every load of a tap is issued unconditionally (both planes cover the whole image;
// what a clamped address or a pixel without geometry holds is never used -- the tap's `ok` selects it away), so the loads of a row
// are independent of each other and of any test.
__device__ __forceinline__ uint32_t dnClampedIndex(const DenoiseAtrous& A, int qx, int qy, bool& inside)
{
  inside = qx >= 0 && qy >= 0 && qx < (int)A.W && qy < (int)A.H;
  return (uint32_t)min(max(qy, 0), (int)A.H - 1) * A.W + (uint32_t)min(max(qx, 0), (int)A.W - 1);
}

// One tap of k_dn_atrous from its loaded record rq and colour cq; a tap outside the image or without geometry leaves the sums
// unchanged through selects.
__device__ __forceinline__ void dnAtrousTap(float4 rq, float4 cq, bool inside, float h, float ox, float oy, float4 rp, float3 Np, float Yp,
                                            float invL, float& sr, float& sg, float& sb, float& sv, float& sw)
{
  const bool ok = inside && __float_as_uint(rq.w) != DN_INVALID;
  // w_z * w_l as one exponential: exp(-(|dz| / den_z + |dY| / den_l))
  const float e = dnEz(rp.x, rp.y, rp.z, rq.x, ox, oy) + fabsf(Yp - dnLum(cq.x, cq.y, cq.z)) * invL;
  const float wn = dnPow128(dnDot(Np, dnOctDecode(__float_as_uint(rq.w))));
  const float w = (h * wn) * expf(-e);
  sr = ok ? sr + w * cq.x : sr;
  sg = ok ? sg + w * cq.y : sg;
  sb = ok ? sb + w * cq.z : sb;
  sv = ok ? sv + (w * w) * cq.w : sv;
  sw = ok ? sw + w : sw;
}

__global__ __launch_bounds__(256) void k_dn_atrous(const DenoiseAtrous A)
{
  uint32_t ux, uy;
  if(!dnPixel(A.W, A.H, ux, uy))
    return;
  const int x = (int)ux, y = (int)uy;
  const uint32_t p = uy * A.W + ux;
  const float4 rp = A.rec[p];
  if(__float_as_uint(rp.w) == DN_INVALID)
    return;
  const float3 Np = dnOctDecode(__float_as_uint(rp.w));
  // 3x3 Gaussian (1/4, 1/2, 1/4)^2 of the variance around p, over the pixels with geometry (row by row, dx inner); loads first
  uint32_t gq[9];
  bool gin[9];
#pragma unroll
  for(int k = 0; k < 9; k++)
    gq[k] = dnClampedIndex(A, x + k % 3 - 1, y + k / 3 - 1, gin[k]);
  uint32_t gw[9];
  float gvq[9];
#pragma unroll
  for(int k = 0; k < 9; k++)
  {
    gw[k] = __float_as_uint(A.rec[gq[k]].w);
    gvq[k] = A.in[gq[k]].w;
  }
  float gv = 0.0f, gk = 0.0f;
#pragma unroll
  for(int k = 0; k < 9; k++)
  {
    const float kk = (k % 3 == 1 ? 0.5f : 0.25f) * (k / 3 == 1 ? 0.5f : 0.25f);
    const bool ok = gin[k] && gw[k] != DN_INVALID;
    gv = ok ? gv + kk * gvq[k] : gv;
    gk = ok ? gk + kk : gk;
  }
  const float4 cp = A.in[p];
  const float Yp = dnLum(cp.x, cp.y, cp.z);
  const float invL = 1.0f / (4.0f * sqrtf(gv / (gk > 0.0f ? gk : 1.0f)) + 1e-10f);  // sigma_l = 4 (gk > 0: p itself has geometry)
  const int s = A.step;
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, sw = 0.0f;
  // rows in a loop (its ten loads in flight together), the five taps of a row unrolled with their B3 weights as constants
#pragma unroll 1
  for(int dy = -2; dy <= 2; dy++)
  {
    const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
    float4 rq[5], cq[5];
    bool in[5];
#pragma unroll
    for(int k = 0; k < 5; k++)
    {
      const uint32_t q = dnClampedIndex(A, x + (k - 2) * s, y + dy * s, in[k]);
      rq[k] = A.rec[q];
      cq[k] = A.in[q];
    }
#pragma unroll
    for(int k = 0; k < 5; k++)
    {
      const float hx = k == 2 ? 0.375f : (k == 1 || k == 3) ? 0.25f : 0.0625f;
      dnAtrousTap(rq[k], cq[k], in[k], hx * hy, (float)((k - 2) * s), (float)(dy * s), rp, Np, Yp, invL, sr, sg, sb, sv, sw);
    }
  }
  // sw > 0 holds at a pixel with geometry (its own tap: w_z = w_n = w_l = 1 up to rounding); the guard mirrors the restatement
  const float sws = sw > 0.0f ? sw : 1.0f;
  const float orr = sr / sws, og = sg / sws, ob = sb / sws;
  A.outBuf[p] = make_float4(orr, og, ob, sv / (sws * sws));
  if(A.out)  // last iteration: remodulate into the caller's plane (.w untouched)
  {
    const float3 f = dnAlbedo(A.color[p], A.position[p], A.normal[p], A.rough[p]);
    A.out[4 * (size_t)p + 0] = orr * f.x;
    A.out[4 * (size_t)p + 1] = og * f.y;
    A.out[4 * (size_t)p + 2] = ob * f.z;
  }
}

static dim3 dnGrid(uint32_t W, uint32_t H) { return dim3((W + DN_TILE - 1) / DN_TILE, (H + DN_TILE - 1) / DN_TILE); }

hipError_t vkrt_launch_denoise_temporal(const DenoiseParams& D, bool variance, hipStream_t stream)
{
  if(D.prevPosition)
    hipLaunchKernelGGL(k_dn_motion_temporal, dnGrid(D.W, D.H), dim3(DN_TILE, DN_TILE), 0, stream, D);
  else
    hipLaunchKernelGGL(k_dn_temporal, dnGrid(D.W, D.H), dim3(DN_TILE, DN_TILE), 0, stream, D);
  if(variance)
    hipLaunchKernelGGL(k_dn_variance, dnGrid(D.W, D.H), dim3(DN_TILE, DN_TILE), 0, stream, D);
  return hipGetLastError();
}

hipError_t vkrt_launch_denoise_atrous(const DenoiseAtrous& A, hipStream_t stream)
{
  hipLaunchKernelGGL(k_dn_atrous, dnGrid(A.W, A.H), dim3(DN_TILE, DN_TILE), 0, stream, A);
  return hipGetLastError();
}
