// wf_schedule.h -- the host-side schedule of a wavefront frame call: which launches it turns into, in what host order, on which lane and
// behind which event, and how much the caller keeps for it (frame groups, pool events, timing events).  wavefront.hip issues what this
// header enumerates and api_frames.cpp allocates what it says.  No HIP type: tests/test_wf_schedule.py compiles it alone, for the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#define VKRT_WF_MAX_LANES 8       // internal streams (and record-stream sets) a call can use
#define VKRT_FRAMES_PER_BATCH 32  // a longer call is rendered as batches of this many frames, one launcher call each (bounds the event pool)

// the integers of one launcher call
struct WfCall
{
  int samples, depth;             // PushConstantRay
  bool sampleSync, cameraRounds;  // VKRT_FLAG_SAMPLE_SYNC / VKRT_FLAG_CAMERA_ROUNDS as the caller set them
  uint32_t tileCount;             // 8x8 tiles of the shard
  int frames;                     // progressive frames of the launcher call (one batch of vkrt_pathtrace_frames); below 1 counts as 1
  int inFlight, subframes;        // VKRT_OPT_WF_FRAMES_IN_FLIGHT, VKRT_OPT_WF_SUBFRAMES
  int groups;                     // frame groups of the working set (WfBuffers::groups)
  int lanes;                      // internal streams the caller has (WfAsync::count; 0 = none: everything on the caller's stream)
  bool timed;                     // per-kernel timing: wants the kernels one after another
};

// ---- rounds and steps of a frame --------------------------------------------------------------------------------------------------
// A sample takes at most depth + 1 rounds: its first closest-hit ray, then one round per further segment (the shadow ray of segment k
// travels with the closest-hit ray of segment k + 1), then the shadow ray of its last segment.  A degenerate frame (no samples or no
// depth) has no rounds: its begin item stores the pixels.
inline int wfRounds(int samples, int depth) { return (samples <= 0 || depth <= 0) ? 0 : samples * (depth + 1); }
// Timing events (two per traversal launch) a timed call of `frames` frames asks for.  Kept numerically for compatibility -- the number of
// launches vkrt_last_trace_timing reports for a long call follows from it: it dates from frames of 2 * samples * depth rounds, is an upper
// bound of 2 * wfRounds * frames only while frames <= 8, and a call that needs more times its first launches only (WfTiming::capacity).
inline size_t wfTimingEvents(int samples, int depth, uint32_t frames)
{
  return std::min<size_t>(8192, (size_t)2 * (2 * (size_t)samples * depth) * std::min<uint32_t>(frames, 8u));
}
// camera rounds: the first round of every sample runs the two camera kernels and the frame has no init launch at all
inline bool wfCameraRounds(const WfCall& c) { return c.cameraRounds && wfRounds(c.samples, c.depth) > 0; }
// Steps = the launches of a frame between its begin and its blend: the rounds, and in the sample-synchronous schedule one sample init in
// front of the first round of every sample but the first (whose camera rays the begin item made) -- unless the frame runs camera rounds.
inline int wfSteps(const WfCall& c)
{
  const int rounds = wfRounds(c.samples, c.depth);
  return rounds + ((c.sampleSync && !wfCameraRounds(c) && rounds > 0) ? c.samples - 1 : 0);
}
struct WfStep
{
  enum Kind { ROUND, CAMERA_ROUND, SAMPLE_INIT } kind;
  int round;   // ROUND / CAMERA_ROUND: the round; SAMPLE_INIT: the round it stands in front of
  int sample;  // CAMERA_ROUND / SAMPLE_INIT: the sample that starts; ROUND: -1
};
inline WfStep wfStep(const WfCall& c, int i)
{
  const int perSample = c.depth + 1;
  if(wfCameraRounds(c))
    return i % perSample == 0 ? WfStep{WfStep::CAMERA_ROUND, i, i / perSample} : WfStep{WfStep::ROUND, i, -1};
  if(!c.sampleSync)
    return {WfStep::ROUND, i, -1};
  // sample init + depth + 1 rounds per sample; i + 1: as if sample 0 had an init of its own at step -1
  const int s = (i + 1) / (perSample + 1), k = (i + 1) % (perSample + 1);
  return k == 0 ? WfStep{WfStep::SAMPLE_INIT, s * perSample, s} : WfStep{WfStep::ROUND, s * perSample + k - 1, -1};
}

// ---- lanes ------------------------------------------------------------------------------------------------------------------------
// A call's work is dealt to F x S lanes, each with its own record streams and its own HIP stream, so that kernels of different lanes
// overlap.  Frames in flight keep every launch at full size, sub-frames cut it into S pieces -- and what overlaps well on this device
// is few, large launches (profiles/r04_experiments.md #110: two or three full-size lanes reach 0.96-0.97 of linear on a 4K / 8 shard,
// three third-size lanes 0.90, four quarter-size lanes 0.77): a call of several frames runs F of them in flight, one lane each (frame k
// belongs to group k % F and is staged, see BLEND below); a single frame is split into S tile ranges.  Per-kernel timing wants the
// kernels one after another; tiny frames are not worth splitting.
struct WfLanes
{
  int F, S;  // frame groups x tile ranges; lane q = g * S + j.  F > 1: the frames are staged (BLEND below) and S = 1
  uint32_t tileCount;
  int frames;
  // tile range j = [tileFirst(j), tileFirst(j + 1))
  uint32_t tileFirst(int j) const { return (uint32_t)((uint64_t)tileCount * j / S); }
  // lane q renders the frames g, g + F, g + 2 F, ... of the call: that many
  int framesOf(int q) const { return (frames - q / S + F - 1) / F; }
};
// frames a call of `frames` frames keeps in flight when the option allows `want`: as many turns of `want` as the call needs, the frames
// dealt evenly over them (4 frames, want 3 -> two turns of 2, not 3 + 1: measured 30.8 against 31.5 ms per frame on a 4K / 8 shard)
inline int wfBalancedInFlight(int frames, int want)
{
  want = std::max(1, std::min(want, frames));
  const int turns = (frames + want - 1) / want;
  return (frames + turns - 1) / turns;
}
inline WfLanes wfLanes(const WfCall& c)
{
  const bool single = c.timed || c.lanes <= 0;
  const int avail = std::min(VKRT_WF_MAX_LANES, c.lanes), frames = std::max(c.frames, 1);
  int F = (single || wfSteps(c) == 0) ? 1 : std::min(wfBalancedInFlight(frames, c.inFlight), c.groups);
  F = std::max(1, std::min(F, avail));
  int S = (single || F > 1) ? 1 : std::max(1, std::min(std::min(VKRT_WF_MAX_LANES, c.subframes), avail));
  S = (int)std::min<uint32_t>((uint32_t)S, std::max(1u, c.tileCount / 256u));
  return {F, S, c.tileCount, frames};
}

// ---- what the caller keeps ------------------------------------------------------------------------------------------------------------
// Frame groups the working set is allocated for: the option, but never more than the call has frames.  This is not the balanced number
// wfLanes uses and may exceed it (4 frames, option 3: 3 groups, 2 in flight).  The extra group is slack, kept because the size of the
// working set (vkrt_wf_state_bytes) is observable and because a later call with other frame counts finds it allocated.
inline int wfGroupsWanted(int inFlight, uint32_t frames) { return std::max(1, (int)std::min<uint32_t>((uint32_t)std::max(inFlight, 1), frames)); }
// Pool events a launcher call of `frames` frames can use: one per blend that another blend waits for -- every frame but the last (a
// staged call has S = 1).  The batches of a long call use the same events again: each batch is joined before the next is enqueued.
inline int wfPoolEvents(int frames) { return std::max(frames, 1) - 1; }

// ---- frame parameters -------------------------------------------------------------------------------------------------------------------
// the parameters of frame k of a call whose frame 0 has P (progressive frames of an unchanged camera: main.cpp:503-508,
// hello_vulkan.cpp:1501-1521): frame index and seed move on.  Params = TraceParams (a template only to keep HIP types out of here)
template <class Params>
inline Params wfFrameParams(const Params& P, uint32_t k, uint32_t seedStep)
{
  Params Q = P;
  Q.pc.frame += (int)k;
  Q.seed += k * seedStep;
  return Q;
}

// ---- items ------------------------------------------------------------------------------------------------------------------------------
// The launches of a call in host enqueue order.  Every (frame, tile range) is BEGIN, STEP 0 .. steps - 1 and, when the call is staged, BLEND,
// all on one lane.  The items of the lanes are dealt round-robin -- item i of every lane before item i + 1 of any: enqueueing one lane's
// hundreds of launches after the other's makes the later lanes start milliseconds late (profiles/r03_experiments.md #106).
// BLEND: a frame in flight writes its pixel values into its group's staging plane, and a blend kernel at its end applies
// raytrace.rgen:136-141 in frame order, so the image is what single-frame calls would have left, bit for bit.  The blend of frame k goes
// behind the blend of frame k - 1 (another lane) through a pool event that frame k - 1 records and nothing else ever does, so no record
// call replaces one that still has a wait to come.  A wait refers to the record calls made BEFORE it: a lane whose blend would wait for
// a record that has not been enumerated yet is skipped for a turn.
struct WfItem
{
  enum Kind { BEGIN, STEP, BLEND } kind;
  int lane, frame, range;  // q, k, j
  int step;                // STEP: which (wfStep)
  int wait, record;        // BLEND: index in the event pool to wait on first / to record afterwards, -1 = none
};
// visit(const WfItem&) -> bool, false = stop.  Returns whether every item was visited: always, unless a visit stops (the blends follow
// frame order, so some lane can always move: tests/test_wf_schedule.py).
template <class Visit>
inline bool wfForEachItem(const WfCall& c, const WfLanes& l, Visit&& visit)
{
  const int steps = wfSteps(c), items = steps + 1 + (l.F > 1 ? 1 : 0);
  int cursor[VKRT_WF_MAX_LANES] = {}, remaining = l.frames * l.S * items;  // items a lane has been dealt; items still to deal
  for(bool dealt = true; dealt && remaining > 0;)
  {
    dealt = false;
    for(int q = 0; q < l.F * l.S; q++)
    {
      const int it = cursor[q] % items, k = q / l.S + cursor[q] / items * l.F;
      if(k >= l.frames)
        continue;  // the lane is through
      WfItem item{it == 0 ? WfItem::BEGIN : it <= steps ? WfItem::STEP : WfItem::BLEND, q, k, q % l.S, it - 1, -1, -1};
      if(item.kind == WfItem::BLEND)  // F > 1, so S = 1: the lane is the group, the pool index the frame
      {
        if(k > 0 && cursor[(k - 1) % l.F] < ((k - 1) / l.F + 1) * items)
          continue;  // the blend of frame k - 1 is still to come
        item.wait = k - 1;  // (frame 0: none)
        item.record = k + 1 < l.frames ? k : -1;
      }
      if(!visit(item))
        return false;
      cursor[q]++; remaining--;
      dealt = true;
    }
  }
  return remaining == 0;
}
