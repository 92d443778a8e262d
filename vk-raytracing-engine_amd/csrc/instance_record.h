// instance_record.h -- the arithmetic of one instance record (scene_records.h DevInstance), once, for the host (make_instance in
// scene_pack.cpp, invert3x3_rows in bvh_host.cpp) and for the device (k_nu_transforms in node_update.hip): a record that
// vkrt_scene_update_node_transforms makes from a matrix in device memory is bit for bit the one vkrt_scene_update_nodes makes from the
// same matrix on the host.  Fixed-width integers and floats only, no HIP type: host-only code includes it (tests compile it with g++).
//
// Every operation below is IEEE binary64 or binary32 in source order (the translation units that include this are built with
// -ffp-contract=off; binary64 division is correctly rounded on either side), so the two sides agree on every finite result, on
// infinities, on zeros and on the NaN that a singular matrix makes (0 x inf: 0xffc00000 after rounding, on an x86 host and on gfx950
// alike; tests/test_gpu_node_update.py has a zero scale in its ranges).  One corner is left open: an inverse entry whose binary32 value
// is subnormal (a matrix with entries near 1e38) may differ between the two sides, which round such values under different denormal
// modes.  Nothing reads a record that extreme as a transform.
#pragma once
#include <stdint.h>
#include "scene_records.h"

#if defined(__HIPCC__)
#define VKRT_IR_HD __host__ __device__ inline
#else
#define VKRT_IR_HD inline
#endif

// o2w: the upper three rows of the column-major object->world matrix M (vkrt_node.worldMatrix), row-major 3x4
VKRT_IR_HD void vkrt_instance_rows(const float M[16], float o2w[12])
{
  for(int r = 0; r < 3; r++)
    for(int c = 0; c < 4; c++)
      o2w[r * 4 + c] = M[c * 4 + r];
}

// w2o: cofactor inverse of the upper-left 3x3 of o2w in double, fixed operation order
VKRT_IR_HD void vkrt_invert3x3_rows(const float o2w[12], float w2o[9])
{
  const double a = o2w[0], b = o2w[1], c = o2w[2];
  const double d = o2w[4], e = o2w[5], f = o2w[6];
  const double g = o2w[8], h = o2w[9], i = o2w[10];
  const double A = e * i - f * h;
  const double B = -(d * i - f * g);
  const double C = d * h - e * g;
  const double det = a * A + b * B + c * C;
  const double inv = 1.0 / det;
  w2o[0] = (float)(A * inv);
  w2o[1] = (float)(-(b * i - c * h) * inv);
  w2o[2] = (float)((b * f - c * e) * inv);
  w2o[3] = (float)(B * inv);
  w2o[4] = (float)((a * i - c * g) * inv);
  w2o[5] = (float)(-(a * f - c * d) * inv);
  w2o[6] = (float)(C * inv);
  w2o[7] = (float)(-(a * h - b * g) * inv);
  w2o[8] = (float)((a * e - b * d) * inv);
}

// VKRT_VIS_MIRRORED or 0: a mirroring transform turns the world-space winding around (traverse.h query_rejects); decided in double on
// the rows
VKRT_IR_HD uint32_t vkrt_mirrored_bit(const float m[12])
{
  const double det = (double)m[0] * ((double)m[5] * m[10] - (double)m[6] * m[9]) - (double)m[1] * ((double)m[4] * m[10] - (double)m[6] * m[8]) +
                     (double)m[2] * ((double)m[4] * m[9] - (double)m[5] * m[8]);
  return det < 0.0 ? VKRT_VIS_MIRRORED : 0u;
}
