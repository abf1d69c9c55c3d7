// enum_walk.hip — the walk launches of the enumeration: ALL children of a node in one vector test (the second
// generation, enum_walk_kernel<.., CHAIN = false>), and around the same test the bookkeeping that makes the chain
// the common case (the third generation, <.., CHAIN = true>).  ONE kernel text: what the generations share appears
// once, every place where they differ is an `if constexpr (CHAIN)`.
//
// Reference behaviour reproduced (fplll v5.5.0): EnumerationBase::enumerate_recursive,
// fplll/enum/enumerate_base.cpp:24-118 (centre, roundto, zig-zag order :80-92, bound test :31 / :93, node
// counting :33, the dual recursion :57-61 / :103-105) with the bounds of EnumerationDyn
// (enumerate.cpp:218-239).  Same visit set, same arithmetic per node (separate multiply / add, the reference's
// operand order), same per-level counts and candidates as enum_phase_kernel (enum_kernel.hip) — which stays the
// kernel of the split launches, of sub-solution calls and the A/B partner of these (FPHIP_WALK2=0).  The final walk
// launches of shortest-vector calls run the fifth generation (this text once more, under FPHIP_WALK5: see enum_walk5.hip
// and the macros below), FPHIP_WALK5=0 the fourth (under FPHIP_WALK4: enum_walk4.hip), closest-vector calls and
// FPHIP_WALK4=0 the third; FPHIP_WALK3=0 selects the second, its A/B partner.
//
// The second generation: what changed, and why.  enum_phase_kernel visits the children of a node one test at a
// time: the first child in its CHILD chain, every later sibling in its STEP loop, and every node's sibling sequence
// ENDS with a failing test — per counted node one successful and one failing test, 40.5 vector + 38.8 scalar /
// branch instructions, 0.81 of the vector issue port (profiles/r05_enum_pmc_summary.txt).  The siblings of a node,
// however, are a function of three wave-uniform numbers (the centre c, the parent's distance, r_kk): child j of the
// zig-zag has x_j = round(c) + z_j, dist_j = pd + (x_j - c)^2 r, and the sequence of distances is non-decreasing.  This
// kernel evaluates the 61 first candidates of a node in the 64 LANES (z = 0 sits in lane 0 of each of the four
// 16-lane rows) — one add, two multiplies, one add, one compare — and reads the number of surviving children off the
// ballot (its popcount - 3): the failing test is gone and the later siblings need no test at all (STEP: the next
// index of the stored count).  Every dist_j is the double the reference's operation sequence produces (x_j - c is
// formed as (x_0 - c) + z_j: one rounding of the same real number, see EXPAND), and a node is counted when it is
// visited, so the visit set and the counts are the reference's bit for bit.
//
//   EXPAND(k):  node at level k (column S_k, distance nd).  c = S_k[k-1]; x_0 = roundto(c), a = x_0 - c; lanes j:
//               dist_j = nd + (a + z_j)^2 r; m = ballot(dist_j <= pruning_{k-1} maxdist); m = 0: STEP(k).  Else
//               n = popcount(m) - 3 and level registers (lane k-1): c, x_0, pd = nd, st = (i = 0, n); push S_k; descend
//               into child 0 (++nodes[k-1]; its distance = dist_j of z = 0: lane 0 of every 16-lane row, handed to
//               the row by one DPP move, row_bcast0_f64 — nothing recomputed, nothing through the LDS crossbar).
//               The vector test runs around rint(c), NOT roundto(c): on a tie (a = +-0.5 exactly) the two nearest
//               integers see the same multiset of |a + z_j| over the 61 candidates, hence the same popcount and the
//               same distance of z = 0 — and z = +-1 shares that distance, so a tie has no child or at least two
//               and is never a chain link.  roundto()'s tie test therefore sits on the descent WITH siblings alone, in
//               a block of its own behind the fail, special, popcount-64 and chain exits, where x_0 is corrected (and
//               a's sign flipped: the dual column update multiplies by it) before they are stored and used.  The
//               special exits redo the expansion by hand with their own roundto (tests/test_walk_tie_model.py).
//   STEP(k):    st_k.i + 1 < st_k.n: x = x_0 + z(i) (z from a 2 KB table through the scalar cache, as a double),
//               dist = pd + (x - c)^2 r, S_k = S_{k+1} - x mu_k, EXPAND(k).  Else climb: STEP(k + 1).
//
// Rare cases leave the hot cycle through ONE bit test (smask, as in enum_phase_kernel) or a flag in st:
//   * emission levels (work donation), the children of a level-1 node (leaves: candidates are reported one by
//     one, each may lower the bound for its next sibling, :97-101);
//   * the chain of first children below a root of distance exactly 0 (is_svp: x only grows there, :80-89 — by
//     symmetry those children are the odd indices of the zig-zag over the same centre 0: flag `grow`);
//   * a node whose candidates +-30 all survive (61 children or more: they are tested one by one, the slow levels).
// A bound that shrinks (a candidate was found) re-tests the not-yet-visited siblings of the active levels and
// shortens their counts (reprune): a sibling is never visited under a bound it fails, to the granularity at which
// waves learn of a new bound — enum_phase_kernel's contract as well.
//
// The third generation (CHAIN): the chain is the common case.  Same visit set, arithmetic, counting rule and
// candidates as the second, whose EXPAND test (all children of a node in one 64-lane test) it keeps.  What changed is
// the bookkeeping around it.  Two thirds of the nodes of the flagship tree have exactly one surviving child
// (DESIGN.md section 3), and the second generation paid for sibling state on every one of them: the column push, six
// selects and a writelane for (c, x_0, pd, st) — none of it ever read back when n = 1 — and, on the way up, one
// readlane-compare-branch iteration per level.
//
// Sibling state lives in two wave-uniform 64-bit masks (SGPRs), bit l = level l:
//   P  level l has a sibling left (a hot level with i + 1 < n, or a slow level that is not exhausted).  Invariant:
//      no bit below the level of the current node is set.  STEP is therefore ONE scalar search: the lowest set bit
//      of P is the level of the next sibling; an empty P ends the task.
//   B  level l's lane registers (cs, x0s, pds, st) and its pushed column are valid: set by an expansion with n >= 2
//      and by the slow levels (zero chain, 61+ children), cleared by a chain descent.  P implies B.
// A chain descent (n = 1) counts the child, takes its distance and column and clears B: no push, no lane-register
// write.  The coefficient of a level outside B is roundto(centre) and is not stored: the three rare paths that need
// the coefficients of the path (a level-1 leaf report, the prefix of a donated task) replay the path from the task's
// root column with the walk's own operation sequence, so the bits are identical; reprune touches B levels only.
//
// Closest-vector mode (FPHIP_CVP): enum_walk_cvp.hip compiles this text a second time with
// FPHIP_CVP = 1, into kernels of another name (enum_walk_cvp_kernel).  The reference's walk with a target
// (!is_svp, enumerate_base.cpp:44 / :80 / :99) differs in what the `if constexpr (CVP)` lines say and in nothing else:
// no zero chain (the zig-zag at every node, the root included), and a leaf at distance exactly 0 is a candidate.  The
// target itself sits in the root task's column.  Without the macro the text is what it was: the kernels of the
// shortest-vector walk keep their names and their code.
//
// Build: like enum_kernel.hip (-ffp-contract=off; -structurizecfg-skip-uniform-regions, no lifetime markers).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "enum_device.h"
#include "enum_wave.h"
#include "enum_kernels.h"

#ifndef FPHIP_CVP
#define FPHIP_CVP 0
#endif
// List mode (FPHIP_LIST): enum_walk_list.hip and enum_walk_cvp_list.hip compile this text once
// more, into enum_walk_list_kernel / enum_walk_cvp_list_kernel, for calls whose radius never moves (fphip_enum_list).
// Every candidate is appended to a list on the device (ListBuf, one more kernel argument) instead of being handed to
// the host through the pinned ring, and the children of a level-1 node are tested 64 at a time.  Every line of it sits
// behind the preprocessor: without the macro the text is what it was.
#ifndef FPHIP_LIST
#define FPHIP_LIST 0
#endif
#if FPHIP_LIST && FPHIP_CVP
#define FPHIP_WALK_KERNEL enum_walk_cvp_list_kernel
#elif FPHIP_LIST
#define FPHIP_WALK_KERNEL enum_walk_list_kernel
#elif FPHIP_CVP
#define FPHIP_WALK_KERNEL enum_walk_cvp_kernel
#else
#define FPHIP_WALK_KERNEL enum_walk_kernel
#endif
#if FPHIP_LIST
#define FPHIP_LIST_PARAM , ListBuf lst
#define FPHIP_LIST_TYPE , ListBuf
#else
#define FPHIP_LIST_PARAM
#define FPHIP_LIST_TYPE
#endif
// The fourth generation (enum_walk4.hip compiles this text with FPHIP_WALK4 = 1 into enum_walk4_kernel<MU_LDS, DUAL>,
// see the header there): the third with ready pair siblings.  Every line of it sits behind the preprocessor
// (FPHIP_W4_PAIR): without the macro the text, and with it the machine code of the kernels above, is what it was
// (tests/perf/walk_isa_diff.py).
// The fifth generation (enum_walk5.hip compiles this text with FPHIP_WALK5 = 1 into enum_walk5_kernel<MU_LDS, DUAL>, see
// the header there): the fourth — FPHIP_WALK5 switches FPHIP_WALK4 on — with the pair sibling's distance taken from the
// lanes of the vector test (FPHIP_W5_PAIR) and the EXPAND loop rotated (FPHIP_W5_AHEAD); either can be switched off
// on the compiler's command line, which is how each was measured alone.  Every line of it sits behind the preprocessor
// as well.
#ifndef FPHIP_WALK5
#define FPHIP_WALK5 0
#endif
#if FPHIP_WALK5
#define FPHIP_WALK4 1
#ifndef FPHIP_W5_PAIR
#define FPHIP_W5_PAIR 1
#endif
#ifndef FPHIP_W5_AHEAD
#define FPHIP_W5_AHEAD 1
#endif
#else
#define FPHIP_W5_PAIR 0
#define FPHIP_W5_AHEAD 0
#endif
#ifndef FPHIP_WALK4
#define FPHIP_WALK4 0
#endif
#if FPHIP_WALK4
#undef FPHIP_WALK_KERNEL
#define FPHIP_WALK_KERNEL enum_walk4_kernel
#define FPHIP_W4_PAIR 1
#else
#define FPHIP_W4_PAIR 0
#endif
#if FPHIP_WALK5
#undef FPHIP_WALK_KERNEL
#define FPHIP_WALK_KERNEL enum_walk5_kernel
#endif

namespace fphip
{

// st: the sibling state of one level (lane = level; CHAIN: of one B level)
//   hot level     bits 0-6: i, the index of the current child in zig-zag order (0..59); bits 8-14: n, the number of
//                 surviving children (1..60; CHAIN: 2..60); the direction of the first step is not stored: it is
//                 c >= x_0 again
//   slow level    (st & 0x7fff) == ST_MARK (i = 100 < n = 127: "a sibling is left" for the hot test, which sends
//                 every i >= 64 to the general path); bits 17-31: iw, the index of the current child.  Levels of the
//                 zero chain, levels with 61+ surviving children — and, without CHAIN, lane Lt & 63, the task root's:
//                 the climb that reaches it ends the task
//   0             (without CHAIN) nothing left at this level
#define ST_I(s) ((s)&0x7f)
#define ST_N(s) (((s) >> 8) & 0x7f)
#define ST_MARK 0x7f64
#define ST_IS_SLOW(s) (((s)&0x7fff) == ST_MARK)
#define ST_IW(s) ((int)((unsigned)(s) >> 17))

// z(i): 0, +1, -1, +2, -2, ... (first step up), negated when the first step goes down (:80-92)
__device__ __forceinline__ int zig_of(int i, bool down)
{
  const int hh = (i + 1) >> 1;
  const int z  = (i & 1) ? hh : -hh;
  return down ? -z : z;
}

// r_kk of one level through the scalar cache (the bound of the level comes out of a lane register here)
__device__ __forceinline__ v2u r_issue(const double *tab, unsigned off)
{
  v2u q;
  asm volatile("s_load_dwordx2 %0, %1, %2" : "=s"(q) : "s"(tab), "s"(off));
  return q;
}
__device__ __forceinline__ void rp_wait(v2u &q) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(q)); }
__device__ __forceinline__ double rp_r2(const v2u &q) { return __hiloint2double((int)q.y, (int)q.x); }

#if FPHIP_WALK4
template <bool MU_LDS, bool DUAL>
#else
template <bool MU_LDS, bool DUAL, bool CHAIN>
#endif
__global__ void __launch_bounds__(FPHIP_MAX_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8)))
    FPHIP_WALK_KERNEL(DevShared *__restrict__ g, HostCtl *__restrict__ h, TaskBuf in, TaskBuf out,
                     int d, int Lmax, unsigned task_lo, unsigned task_hi,
                     const unsigned *__restrict__ idxlist, int launch_idx, int count_nodes,
                     unsigned budget, const double *__restrict__ xhi_root, double *__restrict__ gstk,
                     int Tsplit, unsigned *__restrict__ qh, const unsigned *__restrict__ rcnt, unsigned rcap,
                     unsigned long long bound_init FPHIP_LIST_PARAM)
{
  constexpr bool CVP = FPHIP_CVP != 0;  // closest-vector mode: see the header
#if FPHIP_WALK4
  constexpr bool CHAIN = true;
#endif
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (wave-uniform: the per-wave bases in SGPRs)
  constexpr unsigned MUROW8 = FPHIP_MUROW * 8u;
  const unsigned lane8 = (unsigned)lane << 3;
  const int triL = (Lmax * (Lmax + 1)) >> 1;
  // LDS: [mu rows (MU_LDS)][per-wave column stacks] — the stack layout and the split into an LDS part (slots
  // below Ts) and a global part are enum_phase_kernel's (see there)
  const double *mu_s;
  const int nw     = (int)(blockDim.x >> 6);
  const int Ts     = min(Tsplit, Lmax + 1);
  const int Tsm1   = Ts - 1;
  const int ldsRow = tri_off(Ts);
  const int ldsWave = ldsRow + FPHIP_STACK_PAD;
  double *stk;
  if constexpr (MU_LDS)
  {
    double *mu_l = smem;
    stk          = smem + triL + wave * ldsWave;
    const int nmu = (Lmax * (Lmax - 1)) >> 1;
    for (int i = threadIdx.x; i < nmu; i += blockDim.x)
      mu_l[i] = g->mu_tri[i];
    mu_s = mu_l;
  }
  else
  {
    mu_s = &g->mu_sq[0][0];
    stk  = smem + wave * ldsWave;
  }
  if constexpr (MU_LDS)
    __syncthreads();
  const __amdgpu_buffer_rsrc_t mu_b = mu_rsrc(&g->mu_sq[0][0], (unsigned)sizeof(g->mu_sq));
  char *stk_top      = (char *)stk + (((unsigned)ldsRow << 3) + lane8);
  double *gst = gstk + (size_t)(blockIdx.x * nw + wave) * (size_t)(triL - ldsRow + 1) - ldsRow;
  const double *rptab = &g->mu_sq[0][64];
  // z_j of this lane's candidate of an expansion (first step up): 0 in lane 0 of every 16-lane row (lanes 0, 16,
  // 32, 48), +1, -1, +2, -2, ... +30, -30 over the other 60 lanes — 61 distinct candidates, z = 0 four times, so that
  // the first child's distance reaches every lane by one row broadcast (row_bcast0_f64)
#if FPHIP_W5_PAIR
  // (the fifth generation: z = 0, +1, -1 in lanes 0, 1, 2 of EVERY row — the distance of either neighbour of x_0
  //  reaches every lane by one row broadcast as well — and +-2 ... +-27 over the other 52 lanes: 55 distinct candidates,
  //  the three nearest four times each; FPHIP_ZONCE masks the copies out of a ballot)
  double zz = (double)zig_of((lane & 15) < 3 ? (lane & 15) : (lane & 15) + 13 * (lane >> 4), false);
#define FPHIP_ZONCE 0xfff8fff8fff8ffffull
#else
  double zz = (lane & 15) == 0 ? 0.0 : (double)zig_of(lane - (lane >> 4), false);
#endif
  FPHIP_IN_VGPR(zz);

  unsigned long long mbits =
      rfl_u64(min(bound_init, __hip_atomic_load(&g->bound_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
  double maxdist   = __longlong_as_double((long long)mbits);
  double maxdist_v = maxdist;
  FPHIP_IN_VGPR(maxdist_v);

  // level registers (lane = level)
  double cs = 0.0, x0s = 0.0, pds = 0.0;
  int st = 0;
  unsigned long long cnt = 0;
  unsigned cnt32         = 0;
  unsigned iter          = 0;
  // steps until the next refresh event (the bound, the donation test).  A step is taken once per ~3 nodes: 24 steps
  // are the 64 failed steps of enum_phase_kernel in nodes — a wave must not run longer than that on a stale bound
  constexpr int RF = 24;
  int left               = RF - 1;

  // (bchg: the bound went down — the caller re-tests the pending siblings, see reprune)
#define FPHIP_REFRESH_BOUND(from_host, bchg)                                                      \
  do                                                                                              \
  {                                                                                               \
    unsigned long long nb_;                                                                       \
    if (from_host)                                                                                \
    {                                                                                             \
      nb_ = load_sys_u64(&h->bound_bits);                                                         \
      if (nb_ < mbits && lane == 0)                                                               \
        atomicMin(&g->bound_bits, nb_);                                                           \
      FPHIP_JOIN();                                                                               \
    }                                                                                             \
    else                                                                                          \
    {                                                                                             \
      nb_ = __hip_atomic_load(&g->bound_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        \
    }                                                                                             \
    nb_ = rfl_u64(nb_);                                                                           \
    if (nb_ < mbits)                                                                              \
    {                                                                                             \
      mbits   = nb_;                                                                              \
      maxdist = __longlong_as_double((long long)mbits);                                           \
      maxdist_v = maxdist;                                                                        \
      FPHIP_IN_VGPR(maxdist_v);                                                                   \
      bchg = true;                                                                                \
    }                                                                                             \
  } while (0)

  unsigned q = (unsigned)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * nw + wave) % FPHIP_NQ));
  const unsigned nlist = task_hi - task_lo;
  for (;;)
  {
    // ---- pull a task (the queues of enum_phase_kernel) ----------------------------------------
    unsigned t = 0, cq = 0;
    bool have = false;
    for (;;)
    {
      if (lane == 0)
        t = atomicAdd(&qh[q * FPHIP_QS], 1u);
      t  = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
      cq = rcnt ? min((unsigned)__builtin_amdgcn_readfirstlane((int)rcnt[q * FPHIP_QS]), rcap)
                : (nlist > q ? (nlist - q + FPHIP_NQ - 1u) / FPHIP_NQ : 0u);
      if (t < cq)
      {
        have = true;
        break;
      }
      bool any = false;
#pragma unroll
      for (unsigned hf = 0; hf < FPHIP_NQ / 64; ++hf)
      {
        const unsigned qq = (q + 1u + hf * 64u + (unsigned)lane) % FPHIP_NQ;
        const unsigned hd = __hip_atomic_load(&qh[qq * FPHIP_QS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned cn = rcnt ? min(rcnt[qq * FPHIP_QS], rcap)
                                 : (nlist > qq ? (nlist - qq + FPHIP_NQ - 1u) / FPHIP_NQ : 0u);
        const unsigned long long m = __builtin_amdgcn_ballot_w64(hd < cn);
        if (m != 0ull)
        {
          q   = (q + 1u + hf * 64u + (unsigned)__builtin_ctzll(m)) % FPHIP_NQ;
          any = true;
          break;
        }
      }
      if (!any)
        break;
    }
    if (!have)
    {
      if (budget != 0u && lane == 0)
        __hip_atomic_store(&g->drain[launch_idx], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      FPHIP_JOIN();
      break;
    }
    const unsigned long long pos = (unsigned long long)task_lo + q + (unsigned long long)t * FPHIP_NQ;
    const unsigned long long ti =
        rcnt ? (unsigned long long)q * rcap + (cq - 1u - t)
             : (idxlist ? (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)idxlist[pos]) : pos);
    const int Lt      = __builtin_amdgcn_readfirstlane(in.level[ti]);
    const int rid     = __builtin_amdgcn_readfirstlane(in.root[ti]);
    // (without CHAIN the task's coefficients and column are read up front; with it the column only, below: in.x is
    //  read inside path_x)
    double xpre = 0.0, col0 = 0.0;
    if constexpr (!CHAIN)
    {
      const int tl = here_lane(lane);
      xpre         = in.x[ti * 64 + tl];
      col0         = in.col[ti * 64 + tl];
    }
    const double pd0  = in.pd[ti];
    int donate        = 1 << 20;
    const unsigned iter0 = iter;
    {
      bool bchg = false;
      FPHIP_REFRESH_BOUND((t & 63u) == 0u, bchg);
    }

    int k     = Lt;
    double S  = col0;
    if constexpr (CHAIN)
      S = in.col[ti * 64 + here_lane(lane)];
    double nd = pd0;
    // the chain of first children below a root of distance exactly 0 goes through the general path (slow
    // levels) until the first step away from it: every level is "special" while zc holds
    bool zc = __builtin_amdgcn_ballot_w64(pd0 != 0.0) == 0ull;
    if constexpr (CVP)
      zc = false;  // (!is_svp, :80: no zero chain — the root expands as a zig-zag like every other node)
    // CHAIN: the sibling masks (see the header): the task root's level holds no sibling, an empty P ends the task
    unsigned long long P = 0ull, B = 0ull;
#if FPHIP_W4_PAIR
    // Q  level l is a pair level (its expansion had exactly two children).  With P: the pending sibling is READY — its
    //    column sits in the level's stack slot, its distance in lane l of pds, its coefficient in lane l of x0s; B is
    //    clear while the walk is below the first child (coefficient roundto(centre), as for any level outside B).  With
    //    B: the walk is below the second child, whose coefficient is lane l of x0s (cs and st of the lane are stale).
    //    Every place that sets P or B of a level defines its Q; a Q bit with neither is never read.
    unsigned long long Q = 0ull;
#endif
    // else: the climb that reaches the root's level ends the task: a slow marker in its lane (lane 0 when Lt = 64 —
    // level 0 keeps no sibling state: its nodes are the leaf loop's)
    if constexpr (!CHAIN)
      st = (lane == (Lt & 63)) ? ST_MARK : st;

    // The coefficients of the current path (lane = level), levels >= Lt from the task.  Without CHAIN every level
    // keeps its sibling state: x_0 + z(i) of it.  (A lambda of its own ahead of the others, as the second generation
    // always had it: folded into path_x it changes the order in which the compiler promotes the captured level
    // registers, and with that the register copies of the second generation's kernels — tests/perf/walk_isa_diff.py.)
    auto xs_now = [&]() -> double
    {
      const int idx = (lane == 0) ? 0 : (ST_IS_SLOW(st) ? ST_IW(st) : ST_I(st));
      return x0s + (double)zig_of(idx, !(cs >= x0s));
    };
    auto path_x = [&](int klo) -> double
    {
      if constexpr (!CHAIN)
        return (lane < Lt) ? xs_now() : xpre;  // (klo is not needed)
      else
      {  // levels [klo, Lt) replayed from the task's root column (a B level: x_0 + z(i) of its sibling state; any
         // other: roundto(centre)), lanes below klo zero.  The operation sequence of the walk's descents and steps,
         // so every centre is the walk's.
        const int tl = here_lane(lane);
        double Sr    = in.col[ti * 64 + tl];
        double xr    = (lane >= Lt) ? in.x[ti * 64 + tl] : 0.0;
        for (int l = Lt - 1; l >= klo; --l)
        {
          const double c = rl_f64(Sr, l);
          double x;
#if FPHIP_W4_PAIR
          if ((B >> l) & (Q >> l) & 1ull)
            x = rl_f64(x0s, l);  // (the second child of a pair level: stored as it was formed)
          else
#endif
          if ((B >> l) & 1ull)
          {
            const int s_    = rl_i32(st, l);
            const double x0 = rl_f64(x0s, l);
            x = x0 + (double)zig_of(ST_IS_SLOW(s_) ? ST_IW(s_) : ST_I(s_), !(rl_f64(cs, l) >= x0));
          }
          else
          {
            x = rint(c);
            const double al = x - c;
            if (fabs(al) == 0.5 && ((al < 0.0) == (c > 0.0)))
              x = x - (al + al);
          }
          xr = (lane == l) ? x : xr;
          const double ml = ld_row(mu_b, (unsigned)l * MUROW8, lane8);
          Sr = Sr - (DUAL ? x - c : x) * ml;
        }
        if (lane == 0)
          atomicAdd(&g->replays, 1u);
        FPHIP_JOIN();
        return xr;
      }
    };

#if !FPHIP_LIST  // (list mode: no record leaves the device during the walk — see the leaf pass)
    auto report = [&](double dist, double xleaf, bool &bchg)
    {
      unsigned long long idx = 0;
      if (lane == 0)
        idx = atomicAdd(&g->sol_head, 1ull);
      idx = rfl_u64(idx);
      for (unsigned spin = 0; idx >= load_sys_u64(&h->consumed) + FPHIP_RING_CAP; ++spin)
      {
        __builtin_amdgcn_s_sleep(64);
        if (spin > (1u << 24))
        {
          if (lane == 0)
            atomicOr(&g->error_flags, FPHIP_ERR_RING_TIMEOUT);
          break;
        }
      }
      SolRec *r  = &h->ring[idx % FPHIP_RING_CAP];
      const double xf = (CHAIN && lane == 0) ? xleaf : path_x(1);  // (without CHAIN the leaf is lane 0 of x0s)
      const int rl = here_lane(lane);
      r->x[rl]   = (lane < d) ? xf : 0.0;
      {
        const int xstr = d > 64 ? 64 * ((d - 1) >> 6) : 64;
#pragma unroll
        for (int qq = 1; qq < 4; ++qq)
          r->x[64 * qq + rl] = (64 * qq + lane < d) ? xhi_root[(size_t)rid * xstr + 64 * (qq - 1) + rl] : 0.0;
      }
      if (lane == 0)
      {
        const int z = here_lane(0);
        r->dist     = dist;
        r->kind     = z;
        r->offset   = z;
      }
      __threadfence_system();
      if (lane == 0)
        __hip_atomic_store(&r->seq, idx + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      for (unsigned spin = 0; load_sys_u64(&h->consumed) <= idx; ++spin)
      {
        __builtin_amdgcn_s_sleep(32);
        if (spin > (1u << 24))
        {
          if (lane == 0)
            atomicOr(&g->error_flags, FPHIP_ERR_RING_TIMEOUT);
          break;
        }
      }
      FPHIP_REFRESH_BOUND(true, bchg);
    };
#endif

    // The bound went down: the pending siblings of the hot levels (CHAIN: hot B levels) in [klo, Lt) — inside the
    // count n of their expansion, not visited yet — are tested again, from the last one downwards (the distances are
    // non-decreasing along the zig-zag); n shrinks past those that fail now: the reference would meet them under the
    // new bound and turn back (:93).  Lane = level: every lane handles the state of its own level.  CHAIN: a level
    // left without a sibling loses its P bit.  (Slow levels test their siblings one by one anyway.)
    auto reprune = [&](int klo)
    {
      int s_           = st;
#if FPHIP_W4_PAIR  // (a pair level keeps no (c, x_0, st): its pending sibling is tested below)
      const bool act   = lane >= klo && lane < Lt && (((B & ~Q) >> lane) & 1ull) != 0ull && !ST_IS_SLOW(s_);
#else
      const bool act   = lane >= klo && lane < Lt && (!CHAIN || ((B >> lane) & 1ull) != 0ull) && !ST_IS_SLOW(s_);
#endif
      const double r_l = g->rdiag[lane];
      const double b_l = g->pruning[lane] * maxdist;
      const int cur    = ST_I(s_);
      const bool down  = !(cs >= x0s);
      int n            = ST_N(s_);
      for (;;)
      {
        const int j      = n - 1;
        const double xj  = x0s + (double)zig_of(j, down);
        const double aj  = xj - cs;
        const double ndj = pds + aj * aj * r_l;
        const bool fail  = act && j > cur && !(ndj <= b_l);
        if (__builtin_amdgcn_ballot_w64(fail) == 0ull)
          break;
        if (fail)
          n -= 1;
      }
      s_ = (s_ & ~(0x7f << 8)) | (n << 8);
      st = act ? s_ : st;
      if constexpr (CHAIN)
        P &= ~__builtin_amdgcn_ballot_w64(act && cur + 1 >= n);
#if FPHIP_W4_PAIR
      {  // the ready sibling of a pair level: its distance is lane l of pds, formed at the descent
        const bool pend = lane >= klo && lane < Lt && (((P & Q) >> lane) & 1ull) != 0ull;
        const unsigned long long gone = __builtin_amdgcn_ballot_w64(pend && !(pds <= b_l));
        P &= ~gone;
        Q &= ~gone;
      }
#endif
      FPHIP_JOIN();
    };

    enum : int { EV_EMIT = 1, EV_DONE = 3, EV_REFRESH = 6, EV_SPECIAL = 7, EV_FAIL = 8, EV_SLOWSTEP = 10 };
    unsigned elo  = (unsigned)donate;
    unsigned erng = 0x7fffffffu;
    bool buffer_full = false;
    bool resume_step = false;
    double par = 0.0, mk = 0.0;
    double xk = 0.0, a = 0.0;
    int kc = 0;
    double mk1 = 0.0, c1 = 0.0, x1 = 0.0, a1 = 0.0;
#define FPHIP_PUSH(in_lds, kk, lds8)                                            \
  if (__builtin_expect(in_lds, 1))                                              \
    *(double *)(stk_top - (lds8)) = S;                                          \
  else                                                                          \
  {                                                                             \
    int kt = (kk);                                                              \
    asm volatile("" : "+s"(kt));                                                \
    const unsigned gk8 = ((unsigned)(kt * (kt - 1)) << 2) + lane8;              \
    *(double *)((char *)gst + ((lane < kt) ? gk8 : (unsigned)triL << 3)) = S;   \
  }
    // (par, mk) = (S_{k+1}, row k of mu) of level k: what a step needs to build S_k
#define FPHIP_LOAD_PAR_MK()                                                     \
  do                                                                            \
  {                                                                             \
    const unsigned k8_  = (unsigned)k << 3;                                     \
    const unsigned cl8_ = min(lane8, k8_ - 8u);                                 \
    if (k + 1 < Ts)                                                             \
      par = *(const double *)(stk_top - tri8(k + 2));                           \
    else                                                                        \
      par = ld_off(gst, tri8(k + 1) + cl8_);                                    \
    if constexpr (MU_LDS)                                                       \
      mk = ld_off(mu_s, tri8(k) + cl8_);                                        \
    else                                                                        \
      mk = ld_row(mu_b, (unsigned)k * MUROW8, lane8);                           \
  } while (0)
    for (;;)
    {
      int ev;
      bool at_step = resume_step;
      resume_step  = false;
      // special levels as ONE unsigned compare of the child level: kc - 1 >= spec_t  <=>  kc = 0 (level 1: leaves
      // below) or kc + 1 >= elo (emission levels); spec_t = 0 on the zero chain (every level)
      unsigned spec_t = zc ? 0u : (elo >= 2u ? elo - 2u : 0u);
      spec_t          = (unsigned)__builtin_amdgcn_readfirstlane((int)spec_t);
      int ka = lane_addr(k);  // 4 * level in a VGPR: the address operand of a level's bpermutes, carried
      // ---- the hot cycle: EXPAND chain -> (a node without children) -> STEP loop -> (a sibling is left) ->
      // EXPAND chain ...  Uniform branches only.
      for (;;)
      {
        if (!at_step)
        {
          // ================= EXPAND chain: all children of the node at level k, descend into the first ====
          // (state: a counted node at level k with column S = S_k, distance nd; ka = 4 k)
          kc = k - 1;
#if FPHIP_W5_AHEAD
          // The loop rotated: what a level's test needs from memory and from the crossbar — the centre's broadcast, the
          // (r, pruning) pair, the mu row — is asked for where the level is entered, at the end of the descent above it
          // (FPHIP_NEXT_LEVEL) and here for the first one, not at the top of the level's own iteration.  A descent forms
          // the child's column first and asks at once, so that its bookkeeping (the count, the distance's broadcast,
          // the masks) runs while the answers travel.  Same instructions, same operands: another order.
          v4i q1;
          int kb = ka;  // (the address operand of the broadcasts: 4 * the level asked for)
#define FPHIP_NEXT_LEVEL()                                           \
  do                                                                 \
  {                                                                  \
    asm volatile("" : "+s"(kc));                                     \
    kb -= 4;                                                         \
    asm("" : "+v"(kb)); /* (one address register, not two) */        \
    c1 = bp_f64(S, kb);                                              \
    q1 = rp_issue2(rptab, (unsigned)kc * MUROW8);                    \
    if constexpr (MU_LDS)                                            \
      mk1 = ld_off(mu_s, tri8(kc) + min(lane8, ((unsigned)kc << 3) - 8u)); \
    else                                                             \
      mk1 = ld_row(mu_b, (unsigned)kc * MUROW8, lane8);              \
  } while (0)
          FPHIP_NEXT_LEVEL();
#else
#define FPHIP_NEXT_LEVEL() \
  do                       \
  {                        \
  } while (0)
#endif
          for (;;)
          {
#if !FPHIP_W5_AHEAD
            asm volatile("" : "+s"(kc));
            const unsigned kc8 = (unsigned)kc << 3;
            v4i q1             = rp_issue2(rptab, (unsigned)kc * MUROW8);
            if constexpr (MU_LDS)
              mk1 = ld_off(mu_s, tri8(kc) + min(lane8, kc8 - 8u));
            else
              mk1 = ld_row(mu_b, (unsigned)kc * MUROW8, lane8);
            ka -= 4;
            c1 = bp_f64(S, ka);  // center[kk-1]
#endif
            // x_0 = rint(c) here, not roundto(c): on a tie (a1 = +-0.5 exactly) the two nearest integers give the same
            // multiset of |a1 + z_j| over the 61 candidates — {0.5, 0.5, 1.5, 1.5, ... 29.5, 29.5, 30.5} — so the
            // ballot's popcount and the distance of z = 0 are those of roundto's x_0 (tests/test_walk_tie_model.py),
            // and z = +-1 shares z = 0's distance: a tie has 0 or >= 2 children, never a chain link.  The tie is
            // corrected where x_0 is stored: in the descent with siblings below.  (The special exits redo the
            // expansion by hand with their own roundto.)
            x1 = rint(c1);
            a1 = x1 - c1;
            // candidates: x_0 + (0, +1, -1, +2, -2, ... +30, -30) — a set symmetric about x_0, so the survivors are
            // the first n of the reference's zig-zag WHICHEVER way its first step goes (:71 / :114: the step that
            // picks a child asks again); the distance by the reference's sequence (:28-29 / :91-92).  x_j - c without
            // x_j: a1 = x_0 - c is exact, x_0 + z an exact integer while |x_0| + 31 <= 2^53, so a1 + z is ONE rounding
            // of the real number x_j - c, as (x_0 + z) - c is: the same double (tests/test_walk_bcast_model.py).
            const double aj  = a1 + zz;
            rp_wait(q1);
            const double bnd = rp_p(q1) * maxdist_v;  // partdistbounds[kk-1], enumerate.cpp:218-228
            const double ndj = nd + aj * aj * rp_r(q1);
            const unsigned long long m = __builtin_amdgcn_ballot_w64(ndj <= bnd);
            if (m == 0ull)
            {  // no surviving child: next sibling at level k
              ev = EV_FAIL;
              FPHIP_EXIT();
              break;
            }
            if ((unsigned)(kc - 1) >= spec_t)
            {  // an emission level, level 1 or the zero chain: the general path
              ev = EV_SPECIAL;
              FPHIP_EXIT();
              break;
            }
            // z = 0 sits in four lanes.  The four run the same operations on the same operands, and the distance is
            // non-decreasing in |a_j| (a square, a product by r > 0 and a sum, each rounded monotonically) with |a1|
            // the smallest: whenever any candidate passes, z = 0 passes in all four of its lanes — m != 0 means
            // popcount(m) = 3 + the number of surviving children.  All 64 set: +-30 survive, +-31 may as well.
            int c = __builtin_popcountll(m);
            asm("" : "+s"(c));
            if (c == 64)
            {  // 61+ children: the general path
              ev = EV_SPECIAL;
              FPHIP_EXIT();
              break;
            }
            // ---- descend into child 0 (++nodes[kk-1])
            const unsigned long long me = lane_bit(kc);
            if (CHAIN && c == 4)
            {  // a link of a chain: level kc has no sibling to come back to — nothing of it is stored
              B &= ~me;
#if FPHIP_W5_AHEAD
              // the column first, and the next centre's broadcast at once: the count, the distance and the next
              // header's loads run while the crossbar works
              S = S - (DUAL ? a1 : x1) * mk1;
              --kc;
              FPHIP_NEXT_LEVEL();
              cnt32 = add_bit(me, cnt32);
              nd    = row_bcast0_f64(ndj);
#else
              cnt32 = add_bit(me, cnt32);
              nd    = row_bcast0_f64(ndj);  // the child's distance: ndj of z = 0, lane 0 of every row
              S     = S - (DUAL ? a1 : x1) * mk1;
              --kc;
#endif
              continue;
            }
#if FPHIP_W5_PAIR
            // (the tie test once, for the pair and for the correction below)
            unsigned long long tie = __builtin_amdgcn_ballot_w64(fabs(a1) == 0.5);
            asm("" : "+s"(tie));
            if (c == 8)
            {
              if (tie != 0ull)
              {  // a tie pair: both neighbours share a distance, the direction is roundto's — the fourth generation's
                 // computation, below
                FPHIP_EXIT();
              }
              else
              {  // exactly two children (z = 0 and one neighbour, four lanes each) and no tie: the sibling is the
                 // test's own candidate z = +1 (bit 1 of the ballot: c > x_0, the direction STEP takes) or z = -1
                 // (bit 2).  Its distance is ndj of that lane — (a1 + z) and (x_0 + z) - c are the same double, the rest
                 // is STEP's own sequence (tests/test_walk5_model_cpu.py) —, its coefficient x_0 + z.  Stored as the
                 // fourth generation stores it.
                double x2, nd2;
                if ((m & 2ull) != 0ull)
                {
                  x2  = x1 + 1.0;
                  nd2 = row_bcast_f64<1>(ndj);
                }
                else
                {
                  x2  = x1 - 1.0;
                  nd2 = row_bcast_f64<2>(ndj);
                }
                const double S1 = S - (DUAL ? a1 : x1) * mk1;
                S               = S - (DUAL ? x2 - c1 : x2) * mk1;
                FPHIP_PUSH(kc < Ts - 1, kc + 1, tri8(kc + 2));
                P |= me;
                Q |= me;
                B &= ~me;
                x0s   = sel_f64(me, x2, x0s);
                pds   = sel_f64(me, nd2, pds);
                cnt32 = add_bit(me, cnt32);
                S     = S1;
                --kc;
                FPHIP_NEXT_LEVEL();
                nd = row_bcast0_f64(ndj);
                continue;
              }
            }
            if (tie != 0ull)
#else
            if (__builtin_amdgcn_ballot_w64(fabs(a1) == 0.5) != 0ull)
#endif
            {  // roundto(): ties away from zero
              asm volatile("");
              const bool fix = (a1 < 0.0) == (c1 > 0.0);
              x1             = fix ? x1 - (a1 + a1) : x1;
              // -a1 where fix (the operand of the dual column update), as a flip of the sign bit in place
              a1 = __hiloint2double(__double2hiint(a1) ^ (fix ? (int)0x80000000 : 0), __double2loint(a1));
            }
#if FPHIP_W4_PAIR
            if (c == (FPHIP_W5_PAIR ? 8 : 5))
            {  // exactly two children: the sibling is formed HERE, where its operands are in registers, by the
               // operations, operands and order of STEP (see the header of enum_walk4.hip) — its column goes into the
               // slot of the push, its distance and coefficient into lane kc of pds and x0s; nothing else is kept
              const double sd  = __hiloint2double((c1 >= x1) ? 0x3ff00000 : (int)0xbff00000, 0);
              const double x2  = x1 + sd;
              const double a2  = x2 - c1;
              const double nd2 = nd + a2 * a2 * rp_r(q1);
              const double S1  = S - (DUAL ? a1 : x1) * mk1;
              S                = S - (DUAL ? a2 : x2) * mk1;
              FPHIP_PUSH(kc < Ts - 1, kc + 1, tri8(kc + 2));
              P |= me;
              Q |= me;
              B &= ~me;
              x0s = sel_f64(me, x2, x0s);
              pds = sel_f64(me, nd2, pds);
              cnt32 = add_bit(me, cnt32);
              nd    = row_bcast0_f64(ndj);
              S  = S1;
              --kc;
              FPHIP_NEXT_LEVEL();
              continue;
            }
            Q &= ~me;
#endif
            // (CHAIN: siblings follow) S_k is needed again when x[kc] steps to a sibling
            FPHIP_PUSH(kc < Ts - 1, kc + 1, tri8(kc + 2));
            if constexpr (CHAIN)
            {
              P |= me;
              B |= me;
            }
            cs    = sel_f64(me, c1, cs);
            x0s   = sel_f64(me, x1, x0s);
            pds   = sel_f64(me, nd, pds);
#if FPHIP_W5_PAIR
            st    = wl_i32(__builtin_popcountll(m & FPHIP_ZONCE) << 8, kc, st);
#else
            st    = wl_i32((c - 3) << 8, kc, st);
#endif
            cnt32 = add_bit(me, cnt32);
            nd    = row_bcast0_f64(ndj);  // the first child's distance, as in the chain descent
            S     = S - (DUAL ? a1 : x1) * mk1;
            --kc;
            FPHIP_NEXT_LEVEL();
          }
#undef FPHIP_NEXT_LEVEL
          k = kc + 1;
#if FPHIP_W5_AHEAD
          ka = lane_addr(k);  // (the loop has its own address register)
#else
          ka += 4;
#endif
          if (ev != EV_FAIL)
            break;  // EV_SPECIAL
          // no surviving child: the next sibling — CHAIN: at the lowest level that has one; else at level k (at the
          // task root: its marker ends the task)
        }
        at_step = false;
        int tk;
        if constexpr (CHAIN)
        {
          // ================= STEP: the next sibling, at the lowest level of P (every level below is exhausted) ====
          if (__builtin_expect(P == 0ull, 0))
          {  // nothing left above the task's root
            ev = EV_DONE;
            break;
          }
          k  = __builtin_ctzll(P);
          ka = lane_addr(k);
#if FPHIP_W4_PAIR
          if ((Q >> k) & 1ull)
          {  // ================= pair STEP: the sibling is ready — pop its column, fetch its distance ====
            if (__builtin_expect(--left < 0, 0))
            {
              ev = EV_REFRESH;
              break;
            }
            const unsigned long long me = lane_bit(k);
            P &= ~me;
            B |= me;  // (with Q: the level's coefficient is lane k of x0s)
            if (__builtin_expect(k < Tsm1, 1))
              S = *(const double *)(stk_top - tri8(k + 2));
            else
            {
              int kt = k;
              asm volatile("" : "+s"(kt));
              S = ld_off(gst, tri8(kt + 1) + min(lane8, ((unsigned)kt << 3) - 8u));
            }
            nd = bp_f64(pds, ka);
            cnt32 = add_bit(me, cnt32);  // ++nodes[kk]
            continue;
          }
#endif
          tk = rl_i32(st, k) + 1;
        }
        else
        {
          // ================= STEP loop: the next child at level k, climbing while levels are exhausted ========
          for (;;)
          {
            tk = rl_i32(st, k) + 1;
            if (__builtin_expect((tk & 0x7f) < ((tk >> 8) & 0x7f), 1))
              break;
            ++k;
            ka += 4;
          }
        }
        if (__builtin_expect((tk & 0x7f) >= 64, 0))
        {  // a slow level (without CHAIN: or the task root's marker)
          ev = EV_SLOWSTEP;
          break;
        }
        if (__builtin_expect(--left < 0, 0))
        {  // every RF steps
          ev = EV_REFRESH;
          break;
        }
        if constexpr (CHAIN)
          if ((tk & 0x7f) + 1 >= ((tk >> 8) & 0x7f))
            P &= ~lane_bit(k);  // the last sibling of level k
        {
          // child tk.i of level k: x = x_0 + z(i), its distance (:91-92), the column of its node (:104-110)
          v2u qk = r_issue(rptab, (unsigned)k * MUROW8);
          if (__builtin_expect(k < Tsm1, 1))
            par = *(const double *)(stk_top - tri8(k + 2));
          else
          {
            int kt = k;
            asm volatile("" : "+s"(kt));
            par = ld_off(gst, tri8(kt + 1) + min(lane8, ((unsigned)kt << 3) - 8u));
          }
          if constexpr (MU_LDS)
            mk = ld_off(mu_s, tri8(k) + min(lane8, ((unsigned)k << 3) - 8u));
          else
            mk = ld_row(mu_b, (unsigned)k * MUROW8, lane8);
          int zi;  // z(i) of the zig-zag with the first step up: +-ceil(i / 2) on the scalar unit
          {
            const int ii = tk & 0x7f;
            const int hh = (ii + 1) >> 1;
            zi           = (ii & 1) ? hh : -hh;
            asm("" : "+s"(zi));
          }
          const double zd  = (double)zi;
          const double x0  = bp_f64(x0s, ka);
          const double ck  = bp_f64(cs, ka);
          const double pk  = bp_f64(pds, ka);
          st               = wl_i32(tk, k, st);
          cnt32            = add_bit(lane_bit(k), cnt32);  // ++nodes[kk]
          const double sgd = __hiloint2double((ck >= x0) ? 0x3ff00000 : (int)0xbff00000, 0);
          xk               = __builtin_fma(zd, sgd, x0);
          a                = xk - ck;
          rp_wait(qk);
          nd = pk + a * a * rp_r2(qk);
          S  = par - (DUAL ? a : xk) * mk;
        }
      }
      // ---- events
      FPHIP_OPAQUE(ev);
      if (ev == EV_SPECIAL)
      {
        if ((unsigned)(k - elo) <= erng)
          ev = EV_EMIT;
#if FPHIP_LIST
        else if (k == 1)
        {
          // The children of a level-1 node under a radius that never moves: the leaves of a node are independent, so
          // they are tested 64 at a time.  Sibling j of the reference's order (:80-92) sits in lane j of a pass: the
          // zig-zag around roundto(c), or — the half tree: parent distance exactly 0, no target — the j-th step
          // upwards.  x, al and ndc are formed as the serial loop of the other modes forms them (x by exact integer
          // adds there, one exact add here), so a record's distance is that loop's bit for bit.  The distances do not
          // decrease along the sequence: the survivors are a prefix of the lanes, read off one ballot.
          const double c0 = rl_f64(S, 0);
          double x0 = rint(c0);
          {
            const double al0 = x0 - c0;
            if (fabs(al0) == 0.5 && ((al0 < 0.0) == (c0 > 0.0)))
              x0 = x0 - (al0 + al0);
          }
          const bool up = __builtin_amdgcn_ballot_w64(c0 >= x0) != 0ull;
          bool zig      = __builtin_amdgcn_ballot_w64(nd != 0.0) != 0ull;
          if constexpr (CVP)
            zig = true;
          const double r0 = g->rdiag[0], p0 = g->pruning[0];
          // the coefficients of levels >= 1: once per level-1 node that has a record (CHAIN: one path replay), not
          // once per record
          double xrow   = 0.0;
          bool have_row = false;
          for (int jb = 0;; jb += 64)
          {
            const int j      = jb + lane;
            const int zj     = zig ? zig_of(j, !up) : j;
            const double x   = x0 + (double)zj;
            const double al  = x - c0;
            const double ndc = nd + al * al * r0;
            const unsigned long long ok = __builtin_amdgcn_ballot_w64(ndc <= p0 * maxdist);
            const int n = ok == ~0ull ? 64 : __builtin_ctzll(~ok);  // (the serial loop ends at the first failure)
            cnt += (lane == 0) ? (unsigned long long)n : 0ull;      // nodes[0] grows by n
            // (:44 / :99: newdist > 0.0 || !is_svp — the zero leaf of the half tree is a node and not a record)
            unsigned long long rm = __builtin_amdgcn_ballot_w64(lane < n && (CVP || ndc > 0.0));
            if (rm != 0ull)
            {
              if (!have_row)
              {
                xrow     = path_x(1);
                have_row = true;
              }
              unsigned long long base = 0;
              if (lane == 0)
                base = atomicAdd(lst.count, (unsigned long long)__builtin_popcountll(rm));  // ONE ticket per pass
              base = rfl_u64(base);
              const unsigned long long slot = base + (unsigned long long)__builtin_popcountll(rm & ((1ull << lane) - 1ull));
              if (((rm >> lane) & 1ull) != 0ull && slot < lst.cap)
                lst.dist[slot] = ndc;
              FPHIP_JOIN();
              double *pad = lst.x + lst.cap * (unsigned long long)lst.d;
              for (unsigned long long i = base; rm != 0ull && i < lst.cap; ++i, rm &= rm - 1ull)
              {  // the row of one record, lane = level (the lanes beyond the row land in the padding)
                const double xl = rl_f64(x, __builtin_ctzll(rm));
                const int rl    = here_lane(lane);
                double *dst     = (lane < lst.d) ? lst.x + i * (unsigned long long)lst.d + rl : pad + rl;
                *dst            = (lane == 0) ? xl : xrow;
              }
            }
            if (n < 64)
              break;
          }
          resume_step = true;
          continue;
        }
#else
        else if (k == 1)
        {
          // the children of a level-1 node are leaves (:97-101): one by one, a reported candidate may lower
          // the bound its next sibling is tested against
          bool bchg       = false;
          const double c0 = rl_f64(S, 0);
          double x = rint(c0), al = x - c0;
          if (fabs(al) == 0.5 && ((al < 0.0) == (c0 > 0.0)))
          {
            x  = x - (al + al);
            al = -al;
          }
          int dx         = (c0 >= x) ? 1 : -1;
          bool zig       = __builtin_amdgcn_ballot_w64(nd != 0.0) != 0ull;
          if constexpr (CVP)
            zig = true;
          const double r0 = g->rdiag[0], p0 = g->pruning[0];
          for (;;)
          {
            const double ndc = nd + al * al * r0;
            if (__builtin_amdgcn_ballot_w64(ndc <= p0 * maxdist) == 0ull)
              break;
            cnt += (lane == 0) ? 1ull : 0ull;
            if (CVP || __builtin_amdgcn_ballot_w64(ndc > 0.0) != 0ull)  // (:44 / :99: newdist > 0.0 || !is_svp)
            {
              if constexpr (!CHAIN)
              {  // (the leaf's coefficient reaches the record through lane 0 of the level registers)
                x0s = (lane == 0) ? x : x0s;
                cs  = (lane == 0) ? x : cs;
              }
              report(ndc, x, bchg);
              FPHIP_JOIN();
            }
            if (zig)
            {
              x += (double)dx;
              dx = (dx > 0 ? -1 : 1) - dx;
            }
            else
              x += 1.0;
            al = x - c0;
          }
          if (bchg)
            reprune(1);
          resume_step = true;
          continue;
        }
#endif
        else
        {
          // the expansion by hand of a slow level: the zero chain, 61+ surviving children, or a level the mask holds
          // for no reason any more.  Only the first child is established here; its siblings are the slow step's.
          const bool nz = __builtin_amdgcn_ballot_w64(nd != 0.0) != 0ull;
          if (zc && nz)
            zc = false;  // (the special levels are recomputed from elo / zc at the top of the event loop)
          kc              = k - 1;
          const double rk = g->rdiag[kc], pk = g->pruning[kc];
          if constexpr (MU_LDS)
            mk1 = ld_off(mu_s, tri8(kc) + min(lane8, ((unsigned)kc << 3) - 8u));
          else
            mk1 = ld_row(mu_b, (unsigned)kc * MUROW8, lane8);
          c1 = rl_f64(S, kc);
          x1 = rint(c1);
          a1 = x1 - c1;
          if (fabs(a1) == 0.5 && ((a1 < 0.0) == (c1 > 0.0)))
          {
            x1 = x1 - (a1 + a1);
            a1 = -a1;
          }
          const double nd1 = nd + a1 * a1 * rk;
          if (__builtin_amdgcn_ballot_w64(nd1 <= pk * maxdist) == 0ull)
          {  // (the bound moved between the hot test and this one: the child is gone)
            resume_step = true;
            continue;
          }
          FPHIP_PUSH(k < Ts, k, tri8(k + 1));
          if constexpr (CHAIN)
          {
            P |= lane_bit(kc);
            B |= lane_bit(kc);
          }
#if FPHIP_W4_PAIR
          Q &= ~lane_bit(kc);
#endif
          cs  = (lane == kc) ? c1 : cs;
          x0s = (lane == kc) ? x1 : x0s;
          pds = (lane == kc) ? nd : pds;
          st  = (lane == kc) ? ST_MARK : st;  // (iw = 0)
          cnt += (lane == kc) ? 1ull : 0ull;  // ++nodes[kk-1]: the first child
          nd  = nd1;
          S   = S - (DUAL ? a1 : x1) * mk1;
          k   = kc;
          FPHIP_JOIN();
          continue;  // -> EXPAND at the child
        }
      }
      if (CHAIN && ev == EV_DONE)
        break;
      if (ev == EV_SLOWSTEP)
      {
        if (!CHAIN && k >= Lt)
          break;  // the root's marker: task done
        // the next child of a slow level, one test per child as the reference has it (:80-94): only the odd
        // indices of the zig-zag (x only grows) where the parent's distance is exactly 0
        const int stk_  = rl_i32(st, k);
        const int cur   = ST_IW(stk_);
        const double x0 = rl_f64(x0s, k), ck = rl_f64(cs, k), pk = rl_f64(pds, k);
        const double rk = g->rdiag[k], pr = g->pruning[k];
        bool grow       = __builtin_amdgcn_ballot_w64(pk != 0.0) == 0ull;
        if constexpr (CVP)
          grow = false;
        const bool down = __builtin_amdgcn_ballot_w64(ck >= x0) == 0ull;
        const int nxt   = grow ? (cur == 0 ? 1 : cur + 2) : cur + 1;
        xk              = x0 + (double)zig_of(nxt, down);
        a               = xk - ck;
        const double ndn = pk + a * a * rk;
        const bool ok    = nxt < 32760 && __builtin_amdgcn_ballot_w64(ndn <= pr * maxdist) != 0ull;
        if (!ok)
        {  // exhausted: a level above steps
          if constexpr (CHAIN)
            P &= ~lane_bit(k);
          else
          {
            st = (lane == k) ? 0 : st;
            ++k;
          }
          resume_step = true;
          FPHIP_JOIN();
          continue;
        }
        st = (lane == k) ? (ST_MARK | (nxt << 17)) : st;
        cnt += (lane == k) ? 1ull : 0ull;  // ++nodes[kk]
        FPHIP_LOAD_PAR_MK();
        nd = ndn;
        S  = par - (DUAL ? a : xk) * mk;
        FPHIP_JOIN();
        continue;  // -> EXPAND at level k
      }
      if (ev == EV_EMIT)
      {
        unsigned oi = 0;
        if (lane == 0)
          oi = atomicAdd(out.count, 1u);
        oi = (unsigned)__builtin_amdgcn_readfirstlane((int)oi);
        if (oi < out.cap)
        {
          const int el                              = here_lane(lane);
          out.col[(unsigned long long)oi * 64 + el] = S;
          const double xf                           = path_x(k);
          out.x[(unsigned long long)oi * 64 + el]   = xf;
          if (lane == 0)
          {
            out.pd[oi]    = nd;
            out.level[oi] = k;
            out.root[oi]  = rid;
          }
          FPHIP_JOIN();
        }
        else
        {
          if (lane == 0)
            atomicOr(&g->error_flags, FPHIP_FLAG_TASK_OVERFLOW);
          FPHIP_JOIN();
          buffer_full = true;
          donate      = 1 << 20;
          elo         = 1u << 20;
          erng        = 0u;
          continue;
        }
      }
      else if (ev == EV_REFRESH)
      {
        cnt += cnt32;
        cnt32 = 0u;
        iter += 64u;  // (in the units of enum_phase_kernel's budgets: RF steps are about 64 of its failed steps)
        left = RF - 1;
        bool bchg = false;
        FPHIP_REFRESH_BOUND((iter & 16383u) == 0u, bchg);  // (the pinned host word every 256 refreshes)
        if (bchg)
          reprune(k);
        const unsigned titer = iter - iter0;
        // (a task may shed work from its first refresh on — RF steps, each step closing a chain of at most 64
        //  nodes: about the 256 failed steps enum_phase_kernel waits for)
        if (budget != 0u && titer >= 64u && !buffer_full)
        {
          const unsigned dr = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(
              &g->drain[launch_idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          if (dr != 0u || titer >= budget)
          {
            donate = min(donate, k + 1);
            elo    = (unsigned)donate;
          }
        }
        FPHIP_JOIN();
      }
      resume_step = true;
    }
#undef FPHIP_PUSH
#undef FPHIP_LOAD_PAR_MK
    cnt += cnt32;
    cnt32 = 0u;
  }
#undef FPHIP_REFRESH_BOUND

  if (count_nodes && cnt != 0)
    atomicAdd(&g->nodes[lane], cnt);
  if (lane == 0)
    atomicAdd(&g->iters, (unsigned long long)iter);
}

#if FPHIP_WALK4
#define FPHIP_INST4(M, D)                                                                            \
  template __global__ void FPHIP_WALK_KERNEL<M, D>(DevShared *, HostCtl *, TaskBuf, TaskBuf, int, int, \
                                                  unsigned, unsigned, const unsigned *, int, int,       \
                                                  unsigned, const double *, double *, int, unsigned *,   \
                                                  const unsigned *, unsigned, unsigned long long);
FPHIP_INST4(true, false)
FPHIP_INST4(false, false)
FPHIP_INST4(true, true)
FPHIP_INST4(false, true)
#undef FPHIP_INST4
#else
#define FPHIP_INST(M, D, C)                                                                             \
  template __global__ void FPHIP_WALK_KERNEL<M, D, C>(DevShared *, HostCtl *, TaskBuf, TaskBuf, int, int, \
                                                  unsigned, unsigned, const unsigned *, int, int,       \
                                                  unsigned, const double *, double *, int, unsigned *,   \
                                                  const unsigned *, unsigned, unsigned long long FPHIP_LIST_TYPE);
FPHIP_INST(true, false, false)
FPHIP_INST(false, false, false)
#if !FPHIP_CVP && !FPHIP_LIST  // (no dual instantiation with a target: the reference refuses the pair,
                               //  enumerate.cpp:73; a list call has no dual form)
FPHIP_INST(true, true, false)
FPHIP_INST(false, true, false)
#endif
FPHIP_INST(true, false, true)
FPHIP_INST(false, false, true)
#if !FPHIP_CVP && !FPHIP_LIST
FPHIP_INST(true, true, true)
FPHIP_INST(false, true, true)
#endif
#undef FPHIP_INST
#endif

}  // namespace fphip
