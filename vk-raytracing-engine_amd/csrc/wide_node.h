// Layout of one 8-wide BVH node, shared by the two encoders (bvh_host.cpp, wide_collapse.hip) and the node test (traverse_wide.h).
//
// 80 B = 5 x float4.  Words 0..7 (bvh_host.h): origin, grid exponents | imask, childBase, triBase, eight meta bytes.  Words 8..19: the
// child boxes as 8-bit grid coordinates, four children per dword: lo.x[0..3] lo.x[4..7] lo.y.. lo.z.. hi.x.. hi.y.. hi.z..
// (A 128-B variant with binary16 planes fed to v_fma_mix_f32 saved 48 VALU instructions per node test and was 13-15 % slower: eight
// 16-B loads per lane instead of five; profiles/r03_experiments.md #95.  It lives in the history, not here.)
#pragma once
#include <cstdint>
#include <math.h>

#define VKRT_WNODE_QUADS 5
#define VKRT_WNODE_QMAX 255
#define VKRT_WNODE_DWORDS (4 * VKRT_WNODE_QUADS)
#define VKRT_WNODE_BYTES (16 * VKRT_WNODE_QUADS)
#define VKRT_WNODE_MIN_ALLOC VKRT_WNODE_BYTES

#if defined(__HIPCC__)
#define VKRT_WN_HD __host__ __device__ inline
#else
#define VKRT_WN_HD inline
#endif

// words 8.. of a node from the grid coordinates of its eight child slots (empty slots: 0)
VKRT_WN_HD void vkrt_wnode_store_planes(uint32_t* n, const uint16_t qlo[3][8], const uint16_t qhi[3][8])
{
  for(int p = 0; p < 6; p++)
  {
    const uint16_t* q = p < 3 ? qlo[p] : qhi[p - 3];
    for(int w = 0; w < 2; w++)
      n[8 + 2 * p + w] = (uint32_t)q[4 * w] | ((uint32_t)q[4 * w + 1] << 8) | ((uint32_t)q[4 * w + 2] << 16) | ((uint32_t)q[4 * w + 3] << 24);
  }
}

// The grid of one node and the 8-bit planes of its occupied slots (slotMask bit s; empty slots stay 0): origin = lo, per axis the
// smallest power-of-two cell with which every slot's hi fits QMAX cells, slot boxes rounded outwards -- floor / ceil verified in double,
// so a decoded box always contains the float box it came from.  eb = biased exponents (e + 127).  Shared by the device collapse
// (k_w8_write, wide_collapse.hip) and the refit (refit.hip): a refit of an unmoved scene re-encodes every node bit for bit.
VKRT_WN_HD void vkrt_wnode_quantise(const float lo[3], const float hi[3], uint32_t slotMask, const float slo[8][3], const float shi[8][3], uint32_t eb[3],
                                    uint16_t qlo[3][8], uint16_t qhi[3][8])
{
  const int QMAX = VKRT_WNODE_QMAX;
  for(int q = 0; q < 3; q++)
  {
    const double ext = (double)hi[q] - (double)lo[q];
    int e = -126;
    if(ext > 0)
    {
      int ex;
      const double m = frexp(ext / (double)QMAX, &ex);  // ext / QMAX = m 2^ex, m in [0.5, 1): ceil(log2) = ex, or ex - 1 for an exact power of two
      e = m == 0.5 ? ex - 1 : ex;
    }
    e = e < -126 ? -126 : (e > 126 ? 126 : e);
    for(;;)
    {  // make sure every child's hi really fits (ceil may need one more cell)
      const double sc = ldexp(1.0, e);
      bool ok = true;
      for(int s = 0; s < 8; s++)
        if(((slotMask >> s) & 1u) && ceil(((double)shi[s][q] - (double)lo[q]) / sc) > (double)QMAX) ok = false;
      if(ok || e >= 126) break;
      e++;
    }
    eb[q] = (uint32_t)(e + 127);
  }
  for(int q = 0; q < 3; q++)
    for(int s = 0; s < 8; s++) { qlo[q][s] = 0; qhi[q][s] = 0; }
  for(int s = 0; s < 8; s++)
  {
    if(!((slotMask >> s) & 1u))
      continue;
    for(int q = 0; q < 3; q++)
    {
      const double sc = ldexp(1.0, (int)eb[q] - 127), o = (double)lo[q];
      int ql = (int)floor(((double)slo[s][q] - o) / sc);
      ql = ql < 0 ? 0 : (ql > QMAX ? QMAX : ql);
      while(ql > 0 && o + ql * sc > (double)slo[s][q]) ql--;
      int qh = (int)ceil(((double)shi[s][q] - o) / sc);
      qh = qh < 0 ? 0 : (qh > QMAX ? QMAX : qh);
      while(qh < QMAX && o + qh * sc < (double)shi[s][q]) qh++;
      qlo[q][s] = (uint16_t)ql;
      qhi[q][s] = (uint16_t)qh;
    }
  }
}
