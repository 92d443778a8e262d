// scene_options.h -- the one table of the scene options of include/vkrt.h (vkrt_option 1..18): environment name, default and legal
// values per option.  vkrt_scene's initial values, vkrt_scene_set_option's range check and the environment hooks all read it.
// No HIP type: tests/test_scene_options.py compiles it with g++.
#pragma once
#include <cstdlib>
#include <cstring>
#include "../../include/vkrt.h"
#include "wf_schedule.h"  // VKRT_WF_MAX_LANES

namespace vkrt {

struct OptionRow
{
  const char* env;       // process-wide test hook documented in include/vkrt.h, read once per scene handle
  const char* zeroWord;  // non-NULL: the hook is string-valued, and this word alone sets the option (to 0)
  int def;
  enum Rule { BOOL, RANGE, TRAV_BLOCK, MASK } rule;
  int lo, hi;  // RANGE: clamped to [lo, hi]; MASK: v & hi
};

constexpr int kOptionLast = VKRT_OPT_ALPHA_TEST;
// row = option id; row 0 is no option
constexpr OptionRow kOptions[kOptionLast + 1] = {
    {nullptr, nullptr, 0, OptionRow::BOOL, 0, 0},
    {"VKRT_MODE", "mega", 1, OptionRow::BOOL, 0, 0},
    {"VKRT_BVH", "bvh2", 1, OptionRow::BOOL, 0, 0},
    {"VKRT_WF_SUBFRAMES", nullptr, 3, OptionRow::RANGE, 1, VKRT_WF_MAX_LANES},
    {"VKRT_WF_TRAV_BLOCK", nullptr, 64, OptionRow::TRAV_BLOCK, 0, 0},  // 64, 128 or 256; anything else is 64
    {"VKRT_WF_SHARE", nullptr, 16, OptionRow::RANGE, 0, 64},
    {"VKRT_TRI_THRESHOLD", nullptr, 32, OptionRow::RANGE, 0, 65},
    {"VKRT_WF_SHARE_PERIOD", nullptr, 0, OptionRow::RANGE, 0, 255},
    {"VKRT_WF_SHARE_FLAGS", nullptr, 25, OptionRow::MASK, 0, 31},
    {"VKRT_GBUFFER_MIPS", nullptr, 1, OptionRow::BOOL, 0, 0},
    {"VKRT_WATERTIGHT", nullptr, 0, OptionRow::BOOL, 0, 0},
    {"VKRT_SKIP_DEAD_SHADOW_RAYS", nullptr, 0, OptionRow::BOOL, 0, 0},
    {"VKRT_ANYHIT_DISSOLVE", nullptr, 0, OptionRow::BOOL, 0, 0},
    {"VKRT_WF_FRAMES_IN_FLIGHT", nullptr, 3, OptionRow::RANGE, 1, VKRT_WF_MAX_LANES},
    {"VKRT_SPLIT_BUDGET", nullptr, -1, OptionRow::RANGE, -1, 100},  // -1 = automatic: vkrt_accel_build decides per scene
    {"VKRT_WF_SAMPLE_SYNC", nullptr, 1, OptionRow::BOOL, 0, 0},     // sample-synchronous schedule of the wavefront path tracer (wavefront.hip)
    {"VKRT_WF_CAMERA_ROUNDS", nullptr, 1, OptionRow::BOOL, 0, 0},   // ... whose camera rays are traced from the pixel grid (wavefront.hip)
    {"VKRT_WF_TRI_LEND", nullptr, 1, OptionRow::BOOL, 0, 0},        // triangle steps of the sharing wave lend pending triangles (traverse_share.h)
    {"VKRT_ALPHA_TEST", nullptr, 0, OptionRow::BOOL, 0, 0},
};

inline bool is_option(int option) { return option >= 1 && option <= kOptionLast; }

// the nearest legal value; vkrt_scene_set_option refuses a value this would change
inline int clamp_option(int option, int v)
{
  if(!is_option(option))
    return v;
  const OptionRow& r = kOptions[option];
  switch(r.rule)
  {
    case OptionRow::BOOL: return v ? 1 : 0;
    case OptionRow::RANGE: return v < r.lo ? r.lo : v > r.hi ? r.hi : v;
    case OptionRow::TRAV_BLOCK: return v == 256 ? 256 : v == 128 ? 128 : 64;
    case OptionRow::MASK: return v & r.hi;
  }
  return v;
}

// Initial option values of a scene handle: the defaults, then the environment hooks
inline void initial_options(int opt[kOptionLast + 1])
{
  opt[0] = 0;
  for(int o = 1; o <= kOptionLast; o++)
  {
    const OptionRow& r = kOptions[o];
    opt[o] = r.def;
    const char* e = getenv(r.env);
    if(e && r.zeroWord)
      opt[o] = strcmp(e, r.zeroWord) ? opt[o] : 0;
    else if(e)
      opt[o] = clamp_option(o, atoi(e));
  }
}

}  // namespace vkrt
