// traverse_share.h -- wide8 traversal of 64 rays by one wave with work sharing between the lanes.
//
// Measured on the bench workload (profiles/r01_experiments.md #17, #25): the traversal kernel is VALU-issue bound and
// its node steps run with 47 % of the lanes busy, because a wave lasts as long as its longest walk while the other
// lanes sit idle.  Handing whole rays to other waves does not pay on gfx950 (#13, #21, #28: the walk loses its
// co-resident neighbours and becomes memory-bound).  Here the idle lanes stay in the wave and take over PART of a
// busy lane's walk instead: a lane with pending node groups on its stack gives the oldest one (the largest, farthest
// subtree) to an idle lane, which continues that ray from there.
//
// A ray's result lives in LDS (`res`, indexed by the ray's home lane) so that every lane working on the ray prunes
// against the same bound and publishes improvements to it
// ballot... (see publish step: one LDS 64-bit atomic minimum on (t, triangle id), then the winner stores its payload).  The result is the same as in traverse_wide.h:
// closest = smallest t in (tmin, tmax), ties -> smallest triangle id; any = exists (order-independent definitions).
#pragma once
#include "trav_lds.h"
#include "traverse_wide.h"

// per-wave LDS block: 64 x (u64 key, slot, u, v, donor lane by rank)
#define VKRT_SHARE_LDS_WORDS 384
// ... and without the donor plane (traverse_wide8_share<..., DONOR_LDS = false>): VKRT_SHARE_LDS_WORDS_SIX = 320 words, 1280 B, one LDS
// allocation granule of gfx950, so that the frame kernels' waves of a tree of wide depth <= 9 are charged 6400 B and 24 of them fit a
// CU (trav_lds.h, which the host shares)
struct ShareRes
{
  unsigned long long* key;  // closest: float bits of the best t << 32 | triangle id of the best hit (tie rule); initial tmax << 32 | ~0
  int* slot;                // triangle slot of the best hit, -1 = none
  float* u;
  float* v;
  int* donor;               // scratch of a sharing step: lane of the r-th donor
};
// The lanes of the sharing wave talk to each other through LDS (res.*, donor[]).  They run in lockstep, but the HIP memory
// model does not know that: order every cross-lane write before the reads that depend on it with a wavefront-scope
// release / acquire pair around a wave barrier (no instruction beyond the s_waitcnt the accesses need anyway; it stops
// the compiler from caching or reordering the LDS accesses).
VKRT_DEV void shareSync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// number of set bits of a wave mask below this lane (v_mbcnt: two instructions, no per-lane mask register)
VKRT_DEV unsigned laneRank(unsigned long long mask)
{
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}
// A cursor into a lane's stack column is the LDS address of an entry: 32 bits, in bytes, the lane's column folded in once -- the
// operand ds_read_b64 / ds_write_b64 take as it is.  (As entry indices the cursors cost a shift-add per access, and the parked end
// a subtraction before it: four to six instructions of every iteration, profiles/r11_experiments.md #158.)
typedef unsigned vkrt_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) vkrt_u32x2* ShareStk;
VKRT_DEV uint2 stkLoad(ShareStk p)
{
  const vkrt_u32x2 e = *p;
  return make_uint2(e.x, e.y);
}
VKRT_DEV void stkStore(ShareStk p, uint2 e)
{
  vkrt_u32x2 w;
  w.x = e.x; w.y = e.y;
  *p = w;
}
VKRT_DEV ShareRes shareRes(int* lds320)
{
  ShareRes r;
  r.key = (unsigned long long*)lds320; r.slot = lds320 + 128; r.u = (float*)(lds320 + 192); r.v = (float*)(lds320 + 256); r.donor = lds320 + 320;
  return r;
}

// The match of a sharing or lending step without a plane of its own (DONOR_LDS = false): every lane names a slot -- the r-th giver
// slot r, the lanes that give nothing the slots behind the givers' in lane order, so no two name the same -- and ds_permute_b32 leaves
// its lane number in that slot's lane; lane r then holds what donor[r] held, and the r-th taker fetches it with ds_bpermute_b32.  Both
// go through the LDS crossbar without touching LDS memory.  All 64 lanes must be here (the slot's lane has to receive).
VKRT_DEV int laneOfRank(bool gives, unsigned giveRank, unsigned long long giveMask, unsigned takeRank, int lane)
{
  const unsigned slot = gives ? giveRank : (unsigned)__popcll(giveMask) + (unsigned)lane - giveRank;
  const int byRank = __builtin_amdgcn_ds_permute((int)(slot << 2), lane);
  return __builtin_amdgcn_ds_bpermute((int)(takeRank << 2), byRank);
}

// Must be called by all 64 lanes of a one-wave workgroup (lanes without a ray pass valid = false and only help).
// stk: this lane's stack column (stride 64 entries), res: the wave's ShareRes block: VKRT_SHARE_LDS_WORDS of them with DONOR_LDS,
// VKRT_SHARE_LDS_WORDS_SIX without (res.donor is not used then: closest-hit walks match in registers, laneOfRank; any-hit walks,
// which never write u / v and whose lending step is not entered by every lane, keep the match in the u plane).
template <bool COUNT, bool ANYHIT, int TM = 0, bool DONOR_LDS = true>
VKRT_DEV void traverse_wide8_share(const DevScene& sc, bool valid, f3 o, f3 d, float tmin, float tmax, uint2* stk, ShareRes res, RayHit& hit,
                                   TravCount& tc, uint32_t raySeed = 0u)
{
  // (the `[isa: ...]` comments name the regions tools/isa_blocks.py --loops-json attributes instructions to: each holds to the next one)
  TriRay<(TM & VKRT_TM_WATERTIGHT) != 0> tr;  // [isa: prologue_epilogue]
  tr.set(d);
  const float4* __restrict__ nodes = sc.nodes;
  const float4* __restrict__ tris = sc.tris;
  const int stride = 64;
  const int lane = (int)lane_id();
  // (used only where DONOR_LDS || ANYHIT.  Without the donor plane an any-hit walk keeps its matches in the u plane, as ints: that
  //  holds only while NO any-hit path stores u or v -- publish and the lending step below store the slot alone -- and every access
  //  is fenced by shareSync.  An any-hit stage that wants u / v published needs a plane of its own again.)
  int* const donor = DONOR_LDS ? res.donor : (int*)res.u;
  const ShareStk stkBase = (ShareStk)stk, stkCap = stkBase + (int)(sc.stackCap >> 1) * stride;  // the lane's column: [stkBase, stkCap)
  const unsigned shareMin = sc.shareMinIdle;
  bool farFirst = ANYHIT && anyhit_far_first(sc, o, d, tmax);  // child order of this lane's ray (traverse.h)

  res.key[lane] = ((unsigned long long)__float_as_uint(tmax) << 32) | 0xffffffffull;
  res.slot[lane] = -1; res.u[lane] = 0.0f; res.v[lane] = 0.0f;
  shareSync();  // adopting lanes read res.*[owner] of other lanes

  int owner = lane;  // home lane of the ray this lane is working on
  // where every step of the walk looks first: the ray's key (closest) or slot (any) in res, as an address kept beside `owner`
  unsigned long long* ownerKey = res.key + lane;
  int* ownerSlot = res.slot + lane;
  f3 id = mk3(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
  bool px = !(id.x < 0.0f), py = !(id.y < 0.0f), pz = !(id.z < 0.0f);
  unsigned oct4 = ((px ? 1u : 0u) | (py ? 2u : 0u) | (pz ? 4u : 0u)) * 0x01010101u;  // octinv in every byte (w8_test_children)
  uint2 G = make_uint2(0u, (valid && sc.rootRef != VKRT_TRAV_DONE) ? 0x80000000u : 0u);
  uint2 T = make_uint2(0u, 0u);
  ShareStk sp = stkBase, sb = stkBase, top = stkCap;  // node groups live in [sb, sp), parked triangle groups in [top, stkCap)
  // Step bound (termination safety net): one count for the wave, kept by the scalar unit with the loop counter, instead of one per
  // lane that every adoption had to reset.  Every iteration either finishes a busy lane or takes at least one lane one node test or
  // one triangle test further (when no lane has node work left the triangle step is taken), and the 64 rays of a wave have at most
  // nodes + triangles tests each: at most 2 x 64 x (nodes + triangles) + 64 iterations, which 64 x stepLimit =
  // 64 x (4 x (nodes + triangles) + 64) covers twice.  Looser than the per-lane count, finite; a wave that reaches it faults.
  bool busy = G.y != 0u;
  const unsigned iterLimit = sc.stepLimit > 0x03ffffffu ? 0xffffffffu : sc.stepLimit * 64u;
  // triangle lending (the triangle step below); launch-uniform.  Not built where the watertight test and the dissolve stage meet: a borrower
  // holds a second ray, seed and bound beside its own, and with both stages that is more than the 96 registers of five waves per SIMD
  const bool lendOn = (TM & (VKRT_TM_WATERTIGHT | VKRT_TM_DISSOLVE)) != (VKRT_TM_WATERTIGHT | VKRT_TM_DISSOLVE) && (sc.shareFlags & VKRT_SHARE_TRI_LEND) != 0u;

  for(unsigned iter = 0;; iter++)  // [isa: bookkeeping]
  {
    const unsigned long long busyMask = __ballot(busy);
    if(busyMask == 0ull || iter >= iterLimit)  // (one exit: a lane that leaves with work in its hands has met the bound)
      break;
    // ---- work sharing (every 4th step): idle lanes adopt the oldest pending node group of busy lanes ---------------------
    // [isa: sharing_step]
    if((iter & sc.sharePeriodMask) == sc.sharePeriodMask && (unsigned)__popcll(~busyMask) >= shareMin)
    {
      // donors: lanes with a pending group on their stack give the oldest one (largest, farthest subtree); with shareFlags bit 0
      // a lane whose stack is empty but whose current group still has two or more pending children gives the farthest of them;
      // with shareFlags bit 4 (round 4) a lane that has no node work to give gives TRIANGLES: a parked triangle group whole, or the
      // upper half (by position in the node's triangle block) of two or more pending triangles.  A ray grazing a plane of thin strips
      // comes out of ONE node test with up to 24 triangles to test, one per step, while the rest of the wave has long finished: on
      // Sponza-like drapery half of all steps were such triangle-only steps at 16 % lane efficiency (profiles/r04_experiments.md
      // #113, #116).  (A second matching round, so that lanes giving node work can give triangles in the same step, costs more per
      // step than it saves: -2.7 % on the uniform scene, #116b.)
      const bool giveStack = busy && sp > sb;
      const bool giveChild = (sc.shareFlags & 1u) != 0u && busy && !giveStack && (G.y & 0xff000000u & ((G.y & 0xff000000u) - 1u)) != 0u;
      const bool mayTris = (sc.shareFlags & 16u) != 0u && busy && !giveStack && !giveChild;
      const bool giveParked = mayTris && top < stkCap;
      const bool giveTris = mayTris && !giveParked && (T.y & (T.y - 1u)) != 0u;
      const bool wants = giveStack || giveChild || giveParked || giveTris;
      const unsigned long long donorMask = __ballot(wants), idleMask = ~busyMask;
      if(donorMask != 0ull)
      {
        const unsigned n = min((unsigned)__popcll(donorMask), (unsigned)__popcll(idleMask));
        const unsigned giveRank = laneRank(donorMask), takeRank = laneRank(idleMask);
        const bool gives = wants && giveRank < n;
        const bool takes = !busy && takeRank < n;
        uint2 e = make_uint2(0u, 0u);
        if(gives)
        {
          if(giveStack)
          {
            e = stkLoad(sb);
            sb += stride;
          }
          else if(giveChild)
          {
            const unsigned top = G.y & 0xff000000u;
            // the child this lane would visit LAST: the lowest pending bit in front-to-back order, the highest with farFirst
            const unsigned low = farFirst ? (0x80000000u >> (unsigned)__clz((int)top)) : (top & (0u - top));
            e = make_uint2(G.x, low | (G.y & 0xffu));
            G.y &= ~low;
          }
          else if(giveParked)
          {
            e = stkLoad(top);
            e.x |= 0x80000000u;  // bit 31 of the base marks the entry as a triangle group
            top += stride;
          }
          else
          {
            // the triangles above the middle of the span of pending positions
            const unsigned lo = (unsigned)__ffs((int)T.y) - 1u, hi = 31u - (unsigned)__clz((int)T.y);
            const unsigned upper = T.y & ~((1u << ((lo + hi + 1u) >> 1)) - 1u);
            e = make_uint2(T.x | 0x80000000u, upper);
            T.y &= ~upper;
          }
          if(DONOR_LDS || ANYHIT)
            donor[giveRank] = lane;  // r-th donor feeds the r-th idle lane
        }
        int src = lane;
        if(DONOR_LDS || ANYHIT)
        {
          shareSync();
          if(takes) src = donor[takeRank];
        }
        else
        {
          const int giver = laneOfRank(wants, giveRank, donorMask, takeRank, lane);
          if(takes) src = giver;
        }
        const unsigned ex = (unsigned)__shfl((int)e.x, src), ey = (unsigned)__shfl((int)e.y, src);
        const float ox = __shfl(o.x, src), oy = __shfl(o.y, src), oz = __shfl(o.z, src);
        const float dx = __shfl(d.x, src), dy = __shfl(d.y, src), dz = __shfl(d.z, src);
        const float ix = __shfl(id.x, src), iy = __shfl(id.y, src), iz = __shfl(id.z, src);
        const float tm = __shfl(tmax, src);
        const int ow = __shfl(owner, src);
        const unsigned o4 = (unsigned)__shfl((int)oct4, src);  // (the taker keeps the donor's octant word instead of building it again)
        if(TM & VKRT_TM_DISSOLVE)
        {
          const uint32_t sd = (uint32_t)__shfl((int)raySeed, src);  // the any-hit stage decides per (ray seed, triangle)
          if(takes) raySeed = sd;
        }
        if(takes)
        {
          o = mk3(ox, oy, oz); d = mk3(dx, dy, dz); id = mk3(ix, iy, iz); tmax = tm;
          tr.set(d);  // (watertight: the adopted ray's shear constants, recomputed rather than shuffled)
          farFirst = ANYHIT && anyhit_far_first(sc, o, d, tmax);
          px = !(id.x < 0.0f); py = !(id.y < 0.0f); pz = !(id.z < 0.0f);
          oct4 = o4;
          if(ex & 0x80000000u)  // a triangle group of the donor's ray: nothing to walk, only to test
          {
            G = make_uint2(0u, 0u);
            T = make_uint2(ex & 0x7fffffffu, ey);
          }
          else
          {
            G = make_uint2(ex, ey);
            T = make_uint2(0u, 0u);
          }
          sp = stkBase; sb = stkBase; top = stkCap;
          owner = ow;
          ownerKey = res.key + ow; ownerSlot = res.slot + ow;
          busy = true;
        }
      }
    }
    // ---- one step of every busy lane's walk (same step as w8run) -----------------------------------------------------
    // [isa: bookkeeping]
    shareSync();  // results published in the previous step are visible to every lane of the ray
    if(busy || lendOn)  // (with triangle lending the lanes without work walk along, empty-handed, to borrow)
    {
      float bt = tmax;
      int bg = -1;
      bool finished = false;
      bool occluded = false;  // any-hit walks: this lane found an occluder in this step
      if(ANYHIT)
        finished = busy && __hip_atomic_load(ownerSlot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) >= 0;  // somebody already found an occluder for this ray
      else
      {
        const unsigned long long k = __hip_atomic_load(ownerKey, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        bt = __uint_as_float((unsigned)(k >> 32));
        bg = (int)(unsigned)k;
      }
      // (laneOfRank below needs all 64 lanes at its call: the sharing step above stands outside this block; the lending step inside it
      //  is reached by every lane of a closest-hit walk because `finished` is still false here for !ANYHIT and lendOn, which gates
      //  the lending, lets the lanes without work in.  An any-hit walk does leave lanes behind here, and matches through LDS.)
      if(!finished)
      {
        // A candidate hit lives only between the tests of one site and its publication right behind them (kept across the whole
        // step, its six registers were re-initialised on every level of the nested control flow: 20 v_mov_b32 per iteration).
        struct Cand
        {
          bool found;
          float t, u, v;
          int slot, gid;
        };
        auto testOne = [&](Cand& cd) {  // [isa: triangle_test]
          const unsigned i = (unsigned)__ffs((int)T.y) - 1u;
          T.y &= T.y - 1u;
          const unsigned s = T.x + i;
          const float4* __restrict__ tp = tris + (size_t)s * VKRT_TRI_QUADS;
          const float4 a = tp[0];
          const float4 b = tp[1];
          const float4 c = tp[2];
          if(COUNT)
          {
            tc.tris++;
            if(lane == __ffsll((long long)__ballot(1)) - 1) tc.waveTriSteps++;
          }
          float t, u, v;
          bool ccw;  // (an adopting lane holds the donor's ray: facing is judged with the donor's direction)
          if(tr.hit(o, d, a, b, c, t, u, v, ccw) && t > tmin)
          {
            if(ANYHIT)
            {
              if(t < tmax && !cd.found && !query_rejects<TM>(sc, c, ccw) && !anyhit_ignores<TM>(sc, s, c.y, raySeed, VKRT_HOOK_UV(TM, u, v)))
              {
                cd.found = true; cd.t = t; cd.slot = (int)s;
              }
            }
            else
            {
              const int gid = tri_gid<TM>(c.y);
              const float rt = cd.found ? cd.t : bt;
              const int rg = cd.found ? cd.gid : bg;
              if((t < rt || (t == rt && gid < rg)) && !query_rejects<TM>(sc, c, ccw) && !anyhit_ignores<TM>(sc, s, c.y, raySeed, VKRT_HOOK_UV(TM, u, v)))
              {
                cd.found = true; cd.t = t; cd.u = u; cd.v = v; cd.slot = (int)s; cd.gid = gid;
              }
            }
          }
        };
        // [isa: bookkeeping]
        // publish an improvement: LDS atomic minimum on (t, id), the winner leaves its payload.  Called where the candidate was found,
        // by the lanes that found one: the lanes of a site run it in lockstep, and the sequences of two sites never interleave.
        auto publish = [&](const Cand& cd) {
          if(!cd.found)
            return;
          if(ANYHIT)
          {
            __hip_atomic_store(ownerSlot, cd.slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            occluded = true;
          }
          else
          {
            // (t bits, triangle id) is unique per candidate, so "the minimum is mine" identifies exactly one winner among the
            // lanes publishing for this ray in this step; it alone writes the payload.  Keys only decrease.
            const unsigned long long mine = ((unsigned long long)__float_as_uint(cd.t) << 32) | (unsigned)cd.gid;
            __hip_atomic_fetch_min(ownerKey, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            shareSync();  // every lane's minimum has been applied before anyone checks who won
            if(__hip_atomic_load(ownerKey, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) == mine)
            {
              res.slot[owner] = cd.slot; res.u[owner] = cd.u; res.v[owner] = cd.v;
            }
            bt = cd.t; bg = cd.gid;  // (the ray's best is at least this good now)
          }
        };
        // test a whole group out on the spot (rare: a parked group in the way of a node push, or no room to park)
        auto flushT = [&]() {
          Cand cd = {false, 0.0f, 0.0f, 0.0f, -1, 0};
          while(T.y != 0u && !(ANYHIT && cd.found))
            testOne(cd);
          publish(cd);
        };
        if(G.y & 0xff000000u)
        {
          // closest-hit walks go front to back; any-hit walks take the FARTHEST pending child first (farFirst): see anyhit_far_first
          const unsigned bitIdx = farFirst ? (unsigned)__ffs((int)(G.y & 0xff000000u)) - 1u : 31u - (unsigned)__clz((int)G.y);
          const unsigned slot = (bitIdx - 24u) ^ (oct4 & 7u);
          const unsigned child = G.x + (unsigned)__popc(G.y & 0xffu & ((1u << slot) - 1u));
          G.y &= ~(1u << bitIdx);
          if(G.y & 0xff000000u)
          {
            bool full = sp >= top;  // (one comparison on the way every push takes; the rare block makes its own)
            if(__builtin_expect(full && top < stkCap - VKRT_W8_POSTPONE_ROOM * stride, 0))
            {
              // a triangle group parked beyond its reserved room sits where this node group has to go: test it out now
              const uint2 keep = T;
              T = stkLoad(top);
              top += stride;
              flushT();
              T = keep;
              full = sp >= top;
            }
            if(!full)
            {
              stkStore(sp, G);
              sp += stride;
            }
            else
              VKRT_TRAV_FAULT(sc);
          }
          uint2 Tn;
          w8_test_children<COUNT, (TM & VKRT_TM_FILTER) != 0>(nodes, child, o, id, oct4, px, py, pz, tmin, bt, G, Tn, tc, query_node_masks<TM>(sc),
                                                              query_cull_mask<TM>(sc));
          if(Tn.y != 0u)
          {
            if(T.y != 0u)
            {
              if(__builtin_expect(top > stkCap - VKRT_W8_MAX_POSTPONED * stride && sp < top, 1))
              {
                top -= stride;
                stkStore(top, T);
              }
              else
              {
                if(!occluded)
                  flushT();
                T.y = 0u;
              }
            }
            T = Tn;
          }
        }
        if((G.y & 0xff000000u) == 0u && sp > sb)
        {
          sp -= stride;
          G = stkLoad(sp);
        }
        if(T.y == 0u && top < stkCap)
        {
          T = stkLoad(top);
          top += stride;
        }
        // triangle step: with triThreshold > 1 the wave tests triangles only when that many of 64 walking lanes hold a pending group
        // (the share of the lanes still busy, so that the thin tail of a wave is not left waiting for a count it cannot reach), or
        // none of them has node work left.  1 = every iteration (experiment #57); default 32: with eight parked groups per lane the
        // triangle step runs at 45 % instead of 29 % lane efficiency for 1.5 % more node visits (profiles/r04_experiments.md #118)
        const unsigned long long hasTMask = __ballot(T.y != 0u);  // one vote for the triangle step and for the lending below
        bool triStep = true;
        if(sc.triThreshold > 1u)
          triStep = (unsigned)__popcll(hasTMask) * 64u >= sc.triThreshold * (unsigned)__popcll(busyMask) ||
                    __ballot((G.y & 0xff000000u) != 0u) == 0ull;
        // triangle lending (VKRT_OPT_WF_TRI_LEND): in a triangle step a walking lane that holds no pending triangle sits the test out while
        // its neighbour, which came out of one node test with several, tests them one per step.  Here a lane with two or more pending
        // triangles lends its LAST one (the highest position, so its own order of testing is untouched) to such a free lane: the r-th
        // lender feeds the r-th free lane, matched by rank among the ballots like donors and idle lanes above (res.donor[] is free between
        // sharing steps).  The borrower tests that triangle in this step with the lender's ray (origin, direction, home lane, the lender's
        // view of the ray's bound and tie id and, in the dissolve modes, the seed come by shuffle) and publishes to the ray's home lane as
        // any lane working on the ray does; nothing of its own walk changes.  Lanes without work walk along empty-handed so that they can
        // borrow too: two of three free lanes of a triangle step are such lanes.  The result is the minimum over (t, id) / "exists" whoever
        // tests.  Bench frame: 42.7 M -> 30.3 M triangle wave-steps, lane efficiency 0.40 -> 0.57 (profiles/r09_experiments.md #148-#153).
        bool lentStep = false;  // [isa: lending]
        if(lendOn && triStep)  // (launch-uniform; triStep is the same in every lane that is here)
        {
          const bool tests = T.y != 0u && !occluded;
          const unsigned rest1 = T.y & (T.y - 1u);
          const bool multi = rest1 != 0u && !occluded, isFree = T.y == 0u && !occluded;
          // (a closest-hit walk has no `occluded`: its free lanes are the lanes here that hold no triangle)
          const unsigned long long lendMask = __ballot(multi), freeMask = ANYHIT ? __ballot(isFree) : (__ballot(true) & ~hasTMask);
          const unsigned n = min((unsigned)__popcll(lendMask), (unsigned)__popcll(freeMask));
          if(n != 0u)
          {
            lentStep = true;
            const unsigned lendRank = laneRank(lendMask), freeRank = laneRank(freeMask);
            const bool borrows = isFree && freeRank < n;
            unsigned s = 0u, ls = 0u;
            if(multi && lendRank < n)
            {
              const unsigned hi = 31u - (unsigned)__clz((int)T.y);
              T.y &= ~(1u << hi);
              ls = T.x + hi;
              if(DONOR_LDS || ANYHIT)
                donor[lendRank] = lane;  // r-th lender feeds the r-th free lane
            }
            if(tests)
            {
              s = T.x + (unsigned)__ffs((int)T.y) - 1u;
              T.y &= T.y - 1u;
            }
            int src = lane;
            if(DONOR_LDS || ANYHIT)
            {
              shareSync();
              if(borrows) src = donor[freeRank];
            }
            else
            {
              const int lender = laneOfRank(multi, lendRank, lendMask, freeRank, lane);  // (a closest-hit walk: all 64 lanes are here)
              if(borrows) src = lender;
            }
            const unsigned bs = (unsigned)__shfl((int)ls, src);
            const f3 ro = mk3(__shfl(o.x, src), __shfl(o.y, src), __shfl(o.z, src));
            const f3 rd = mk3(__shfl(d.x, src), __shfl(d.y, src), __shfl(d.z, src));
            const int row = __shfl(owner, src);
            // the lender's view of its ray's best hit, loaded at the top of this step: never below the ray's current one, so no candidate
            // that could still win is dropped (any-hit walks: tmax)
            const float rbt = __shfl(bt, src);
            const int rbg = ANYHIT ? 0 : __shfl(bg, src);
            uint32_t rseed = raySeed;
            if(TM & VKRT_TM_DISSOLVE)
              rseed = (uint32_t)__shfl((int)raySeed, src);
            if(tests || borrows)
            {
              if(borrows)
              {
                s = bs;
                tr.set(rd);  // (watertight: the borrowed ray's shear constants, recomputed rather than shuffled or held beside the lane's own)
              }
              const float4* __restrict__ tp = tris + (size_t)s * VKRT_TRI_QUADS;  // [isa: triangle_test]
              const float4 a = tp[0];
              const float4 b = tp[1];
              const float4 c = tp[2];
              if(COUNT)
              {
                tc.tris++;
                if(lane == __ffsll((long long)__ballot(1)) - 1) tc.waveTriSteps++;
              }
              float t, u, v;
              bool ccw;
              if(tr.hit(ro, rd, a, b, c, t, u, v, ccw) && t > tmin)
              {
                if(ANYHIT)
                {
                  if(t < rbt && !query_rejects<TM>(sc, c, ccw) && !anyhit_ignores<TM>(sc, s, c.y, rseed, VKRT_HOOK_UV(TM, u, v)))
                  {
                    __hip_atomic_store(&res.slot[row], (int)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                    if(!borrows)
                      occluded = true;  // (the lender of an occluder sees it at the top of its next step)
                  }
                }
                else
                {
                  const int gid = tri_gid<TM>(c.y);
                  if((t < rbt || (t == rbt && gid < rbg)) && !query_rejects<TM>(sc, c, ccw) && !anyhit_ignores<TM>(sc, s, c.y, rseed, VKRT_HOOK_UV(TM, u, v)))
                  {
                    const unsigned long long mine = ((unsigned long long)__float_as_uint(t) << 32) | (unsigned)gid;
                    __hip_atomic_fetch_min(&res.key[row], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                    shareSync();
                    if(__hip_atomic_load(&res.key[row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) == mine)
                    {
                      res.slot[row] = (int)s; res.u[row] = u; res.v[row] = v;
                    }
                  }
                }
              }
              if((TM & VKRT_TM_WATERTIGHT) != 0 && borrows)  // [isa: lending]
                tr.set(d);  // back to the lane's own ray
            }
          }
        }
        if(!lentStep && T.y != 0u && triStep && !occluded)  // [isa: bookkeeping]
        {
          Cand cd = {false, 0.0f, 0.0f, 0.0f, -1, 0};
          testOne(cd);
          publish(cd);
        }
        // (testing two or three triangles per lane in steps where no lane of the wave has node work left -- all loop overhead around one
        //  test -- did not pay: 4110 -> 4082 / 4078 Mrays/s on the strip scene, profiles/r04_experiments.md #116c)
        if(ANYHIT && occluded)
          finished = true;
        else if((G.y & 0xff000000u) == 0u && T.y == 0u && top == stkCap)
          finished = true;  // (sp == sb here: the refill above would have popped otherwise)
      }
      if(finished)
      {
        if(lendOn && busy)  // (not the lanes that walk along already: they would empty their hands in every iteration)
        {
          G.y = 0u; T.y = 0u; sp = stkBase; sb = stkBase; top = stkCap;  // empty-handed from here on, where the lane walks along to borrow
        }
        busy = false;  // (without lending G, T and the stack cursors are dead until the lane adopts new work)
      }
    }
  }
  if(__builtin_expect(busy, 0))  // [isa: prologue_epilogue]
    VKRT_TRAV_FAULT(sc);
  shareSync();
  // (the lane's result addresses are formed again here, from a lane number the compiler cannot tie to the prologue's: held across the
  //  loop for these four loads they cost three registers of every iteration)
  int home = lane;
  asm volatile("" : "+v"(home));
  hit.t = __uint_as_float((unsigned)(res.key[home] >> 32)); hit.u = res.u[home]; hit.v = res.v[home]; hit.slot = res.slot[home];
  if(ANYHIT)
    hit.t = tmax;
  if(ANYHIT && !DONOR_LDS)
    hit.u = 0.0f;  // (what an any-hit walk leaves there in the other layout; here the plane held the matches)
}
