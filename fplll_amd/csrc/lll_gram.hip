// lll_gram.hip — batched LLL reduction of integer quadratic forms for gfx950:
// LLLReduction<Z_NR<long>, FP_NR<double>>::lll over MatGSOGram<Z_NR<long>, FP_NR<double>>(g, u, u_inv_t, GSO_INT_GRAM),
// one wavefront per form, bit-exact decisions; and the batched update_gso() of such forms.
//
// Reference behaviour reproduced:
//   LLLReduction::lll            fplll/lll.cpp:44-164   (kappa loop, Lovasz test, insertion index, zero rows, set_r,
//                                                        iteration limit, symmetrize_g at the end; no early
//                                                        reduction with enable_int_gram, lll.cpp:31-35)
//   LLLReduction::babai          fplll/lll.cpp:166-224
//   MatGSOGram                   fplll/gso_gram.cpp:25-400 (row_add / row_sub / row_addmul_si on g and u, move_row,
//                                                        discover_row), fplll/gso_gram.h:153-262 (get_gram =
//                                                        f.set_z(g(i, j)), b_row_is_zero = g(i, i) == 0,
//                                                        get_max_exp_of_b = g.get_max_exp() / 2)
//   update_gso_row, row_op_end   fplll/gso_interface.cpp:131-164, :32-53
//   rotate_gram_left / _right    fplll/nr/matrix.cpp:65-93
//
// Design.  The state of a form is g itself: int64 [d][ldd], both triangles stored and kept equal, addressed
// [slot_i][slot_j] through the lane-resident slot table of lll_kernel.hip (SlotMap) — rows never move, so a row move
// costs nothing on g (the reference's rotate_gram_left / _right is O(d^2) element moves on the lower triangle).
// gf is its double mirror, entry by entry ((double) of an int64 rounds to nearest, as Z_NR<long>::get_d does): the
// Gram cache of update_row_cached (lll_wave.h) is then always complete and its dot-product passes are never entered;
// the column recurrence, babai's mu sweep and the control flow are the shared code on the block streams.
//
// The row operation i <- i + sum_j x_j j of one babai pass (the reference applies the x_j one by one, j descending;
// all of it is arithmetic modulo 2^64, where the order of the additions is free):
//     g'(i, k) = g(i, k) + sum_j x_j g(j, k)                                   (k != i)
//     g'(i, i) = g(i, i) + sum_j x_j (g(i, j) + g'(i, j))
// (the second line is 2 sum_j x_j g(i, j) + sum_j sum_l x_j x_l g(j, l), what the reference's
// g(i, i) += 2 x g(i, j) + x^2 g(j, j) steps add up to).  Lane k owns column k + 64 q of row slot_i; the rows
// slot_j are streamed through the LDS ring like the rows of b in the basis kernel (AxpyPh), the new row is stored
// coalesced and its mirror column as one scattered vector store per chunk, and gf gets the converted values at once.
//
// One thing is NOT a property of the vectors: with zero rows the reference's MatGSOGram::move_row rotates mu, r, u
// and the valid-column counts over [old, new] but g only over [old, min(new, n_known_rows - 1)] (and not at all when
// old >= n_known_rows - 1, gso_gram.cpp:334-345).  The kernel follows it — parity is with the reference as it is —
// by moving g's entries for once (gram_move_to_end: O(d^2), zero rows only); n_known_rows is tracked for this.

#include "gram_device.h"
#include "lll_wave.h"
#include "kernels.h"

namespace fphip
{

template <int NQ> __device__ __forceinline__ long long gram_lane_get(const long long (&v)[NQ], int idx)
{
  long long r = 0;
  dispatch_chunk<NQ>(idx, [&](auto q, int ii) { r = g_rl_i64(v[decltype(q)::value], ii); });
  return r;
}

// gf = (double) g for the whole form; slots = positions; nothing known of mu / r
template <int NQ>
__device__ __forceinline__ void gram_init_state(Lattice<NQ> &T, LllCtx &C, SlotMap<NQ> &M, const long long *G)
{
  const int lane = T.lane, d = T.d, ldd = T.ldd;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    M.sl[q] = lane + 64 * q;
  for (int i = 0; i < d; ++i)
  {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
      const int c = lane + 64 * q;
      if (c < d)
        C.gf[(size_t)i * ldd + c] = (double)G[(size_t)i * ldd + c];
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (lane + 64 * q < d)
      C.vc[lane + 64 * q] = 0;
  __threadfence_block();
}

// row kappa <- row kappa + sum_j x_j row j on g (and gf), x_j = lxv of lane j, nz = the rows with x_j != 0
template <int NQ>
__device__ __forceinline__ void gram_row_op(Lattice<NQ> &T, LllCtx &C, const SlotMap<NQ> &M, LStream<NQ> &S,
                                            long long *G, int kappa, const unsigned long long (&nz)[NQ],
                                            const long long (&lxv)[NQ])
{
  const int lane = T.lane, d = T.d, ldd = T.ldd;
  const int si = M.phys(kappa);
  long long bv[NQ], g0[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
  {
    const int c = lane + 64 * q;
    bv[q]       = (c < d) ? G[(size_t)si * ldd + c] : 0;
    g0[q]       = bv[q];
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
  {
    settle(bv[q]);
    settle(g0[q]);
  }
  int rows = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    rows += __builtin_popcountll(nz[q]);
  {
    AxpyPh<NQ, false> ph{(const char *)G, (long)ldd * 8, ls_make_win(d * 8), S.lane16, lane, M, bv, lxv, {}, {}};
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      ph.ic.m[q] = ph.cc.m[q] = nz[q];
    ls_run<NQ>(S, ph, rows);
  }
  // the diagonal from the values before and after: g(i, i) + sum_j x_j (g(i, j) + g'(i, j))
  long long t[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    t[q] = (long long)((unsigned long long)g0[q] + (unsigned long long)bv[q]);
  unsigned long long diag = (unsigned long long)gram_lane_get<NQ>(g0, si);
  RowCursor<NQ> cur;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    cur.m[q] = nz[q];
  for (int k = 0; k < rows; ++k)
  {
    const int j        = cur.next();
    const int sj       = M.phys(j);
    const long long x  = gram_lane_get<NQ>(lxv, j);
    const long long tj = gram_lane_get<NQ>(t, sj);
    diag += (unsigned long long)x * (unsigned long long)tj;
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q)
  {
    const int c = lane + 64 * q;
    if (c < d)
    {
      const long long v = (c == si) ? (long long)diag : bv[q];
      const double f    = (double)v;
      G[(size_t)si * ldd + c]    = v;
      G[(size_t)c * ldd + si]    = v;
      C.gf[(size_t)si * ldd + c] = f;
      C.gf[(size_t)c * ldd + si] = f;
    }
  }
}

// row_op_end(kappa, kappa + 1) with enable_int_gram (gso_interface.cpp:32-53): the row's own GSO row, and the
// columns >= kappa of every later row
template <int NQ>
__device__ __forceinline__ void gram_after_rowop(Lattice<NQ> &T, LllCtx &C, const SlotMap<NQ> &M, int kappa)
{
  const int lane = T.lane, d = T.d;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
  {
    const int p = lane + 64 * q;
    if (p == kappa)
      C.vc[M.sl[q]] = 0;
    else if (p > kappa && p < d)
    {
      const int s = M.sl[q];
      if (C.vc[s] > kappa)
        C.vc[s] = kappa;
    }
  }
}

// LLLReduction::babai(kappa, kappa, 0), lll.cpp:166-224, on a form: row_expo is all zero (babai_expo[j] = 0).
// 1 ok, 0 GSO failure, -1 babai failure, -2 multiplier beyond 63 bits.
template <int NQ, class Upd>
__device__ __forceinline__ int gram_babai(Lattice<NQ> &T, LllCtx &C, const SlotMap<NQ> &M, LStream<NQ> &S,
                                          long long *G, int kappa, double eta, Upd upd)
{
  const int lane = T.lane, d = T.d, ldd = T.ldd;
  const int pk = M.phys(kappa);
  long long max_expo = LLONG_MAX;
  for (int iter = 0;; ++iter)
  {
    if (!upd(kappa, kappa - 1))
      return 0;
    int e[NQ];
    bool need = false;
    int mexp  = INT_MIN;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
      const int j = lane + 64 * q;
      e[q]        = 0;
      if (j < kappa)
      {
        need |= fabs(T.murow[q]) > eta;
        mexp = max(mexp, (int)max(fexponent(T.murow[q]), (long long)INT_MIN + 2));
      }
    }
    if (!__any(need))
      break;
    if (iter >= 2)
    {  // lll.cpp:187-195
      const long long new_max = (long long)wave_max_i32(mexp);
      if (new_max > max_expo - 5)
        return -1;
      max_expo = new_max;
    }
    double bm[NQ], xs[NQ];
    unsigned long long nz[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
      bm[q] = T.murow[q];
      xs[q] = 0.0;
      nz[q] = 0;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
      settle(e[q]);
      settle(bm[q]);
    }
    // ---- lll.cpp:202-214: lane k owns babai_mu[k]; rows j = kappa-1 .. 0, descending
    {
      constexpr int U = LStream<NQ>::U;
      const int jtop  = (kappa - 1) | (U - 1);
      SweepPh<NQ> ph{(const char *)T.mu, (long)ldd * 8, jtop, kappa, 0, 0, S.lane16, lane, M, bm, xs, e, nz, {}};
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        ph.srmask[q] = ~0ull;
      ls_run<NQ>(S, ph, jtop + 1);
    }
    // ---- the multipliers: row_addmul_we(kappa, j, -X, 0) -> get_si_exp_we, nr_FP_d.inl:46-53
    long long lxv[NQ];
    bool too_big = false;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
      lxv[q] = 0;
      if (xs[q] != 0.0)
      {
        if (fexponent(-xs[q]) - 63 > 0)
          too_big = true;
        lxv[q] = (long long)(-xs[q]);
      }
    }
    if (__any(too_big))
      return -2;  // nothing has been stored yet: the form is unchanged
    gram_row_op<NQ>(T, C, M, S, G, kappa, nz, lxv);
    if (T.u != nullptr)
    {  // enable_transform (gso_gram.cpp:53-58,82-87,109-114): the same operation on the rows of u
      long long uv[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q)
      {
        const int c = lane + 64 * q;
        uv[q]       = (c < d) ? T.u[(size_t)pk * ldd + c] : 0;
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        settle(uv[q]);
      int rows = 0;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        rows += __builtin_popcountll(nz[q]);
      AxpyPh<NQ, false> ph{(const char *)T.u, (long)ldd * 8, ls_make_win(d * 8), S.lane16, lane, M, uv, lxv, {}, {}};
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        ph.ic.m[q] = ph.cc.m[q] = nz[q];
      ls_run<NQ>(S, ph, rows);
#pragma unroll
      for (int q = 0; q < NQ; ++q)
      {
        const int c = lane + 64 * q;
        if (c < d)
          T.u[(size_t)pk * ldd + c] = uv[q];
      }
    }
    gram_after_rowop<NQ>(T, C, M, kappa);
    // later reads of g / gf / u in this wave must see these stores
    __threadfence_block();
  }
  return 1;
}

// MatGSOGram::move_row(old_r, new_r) with new_r >= old_r (a zero row goes to the end), gso_gram.cpp:316-357: mu, r, u
// and the valid-column counts rotate over [old_r, new_r] — the slot table — but g only over
// [old_r, min(new_r, n_known_rows - 1)], and only when old_r < n_known_rows - 1.  Where the two differ, g's entries
// (and gf's) are moved so that position p of the slot table finds what the reference's g holds at p; tmp is the
// form's output buffer.
template <int NQ>
__device__ __forceinline__ void gram_move_to_end(Lattice<NQ> &T, LllCtx &C, SlotMap<NQ> &M, long long *G,
                                                 long long *tmp, int old_r, int new_r, int &nkr)
{
  const int lane = T.lane, d = T.d, ldd = T.ldd;
  if (new_r > old_r)
  {
    SlotMap<NQ> MG = M;  // where the reference's g has its rows
    if (old_r < nkr - 1)
      rotate_left<NQ>(MG, old_r, min(new_r, nkr - 1), lane);
    rotate_left<NQ>(M, old_r, new_r, lane);
    clamp_valid<NQ>(T, C, M, old_r);
    if (new_r >= nkr && old_r < nkr)
      --nkr;
    bool differ = false;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      differ |= (lane + 64 * q < d) && (MG.sl[q] != M.sl[q]);
    if (__any(differ))
    {
      __threadfence_block();
      for (int p = 0; p < d; ++p)
      {
        const int sp = MG.phys(p);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
        {
          const int c = lane + 64 * q;
          if (c < d)
            tmp[(size_t)p * ldd + c] = G[(size_t)sp * ldd + MG.sl[q]];
        }
      }
      __threadfence_block();
      for (int p = 0; p < d; ++p)
      {
        const int sp = M.phys(p);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
        {
          const int c = lane + 64 * q;
          if (c < d)
          {
            const long long v                  = tmp[(size_t)p * ldd + c];
            G[(size_t)sp * ldd + M.sl[q]]      = v;
            C.gf[(size_t)sp * ldd + M.sl[q]]   = (double)v;
          }
        }
      }
    }
  }
  __threadfence_block();
}

// LLLReduction::lll(0, 0, d, 0), lll.cpp:44-164, on a form.  status as lll_run (lll_wave.h).
template <int NQ>
__device__ __forceinline__ int gram_lll_run(Lattice<NQ> &T, LllCtx &C, SlotMap<NQ> &M, LStream<NQ> &ring,
                                            long long *G, long long *tmp, double delta, double eta, double logdelta,
                                            bool siegel, int &final_kappa, int &nswaps, int &zeros, long long &iter)
{
  // siegel (LLL_SIEGEL, lll.cpp:38-40,122,134): `delta` is then the caller's swap_threshold = delta - eta^2 and the two
  // tests compare with lovasz_tests[kappa] instead of [kappa - 1]; logdelta stays log(delta)
  const int lane = T.lane, d = T.d, ldd = T.ldd;
  const int kmin = 0, kend = d, dd = d;
  // ---- iteration limit, lll.cpp:79-80: get_max_exp_of_b() = g.get_max_exp() / 2 (gso_gram.h:169-182)
  int mexp = 0;
  for (int i = 0; i < d; ++i)
  {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
      const int c = lane + 64 * q;
      if (c < d)
        mexp = max(mexp, zexponent(G[(size_t)i * ldd + c]));
    }
  }
  mexp = wave_max_i32(mexp) / 2;
  const long long max_iter =
      (long long)((double)dd - (double)(2 * dd * (dd + 1)) * ((double)(mexp + 3) / logdelta));

  int nkr  = 0;  // n_known_rows
  auto upd = [&](int k, int last)
  {
    if (k >= nkr)
    {  // discover_row(), gso_gram.cpp:25-39
      if (lane == 0)
        C.vc[M.phys(k)] = 0;
      ++nkr;
      __threadfence_block();
    }
    return update_row_cached(T, C, M, ring, k, last);
  };

  int status  = 1;
  final_kappa = 0;
  zeros       = 0;
  nswaps      = 0;
  iter        = 0;
  bool ok     = true;
  // zero rows go to the end, lll.cpp:66-69 (b_row_is_zero(0): g(0, 0) == 0)
  for (; zeros < dd; ++zeros)
  {
    const int s0 = M.phys(0);
    if (uni(G[(size_t)s0 * ldd + s0] != 0 ? 1 : 0))
      break;
    gram_move_to_end<NQ>(T, C, M, G, tmp, kmin, kend - 1 - zeros, nkr);
  }
  if (zeros < dd)
  {
    if (!upd(0, 0))
    {
      status      = 0;
      ok          = false;
      final_kappa = 0;
    }
    __threadfence_block();
  }
  int kappa = 1;
  for (; ok && iter < max_iter && kappa < kend - zeros; ++iter)
  {
    // ---- lazy size reduction, lll.cpp:103-108
    const int rc = gram_babai<NQ>(T, C, M, ring, G, kappa, eta, upd);
    if (rc != 1)
    {
      status      = rc;
      final_kappa = kappa;
      ok          = false;
      break;
    }
    const int sk = M.phys(kappa);
    // ---- Lovasz prefix values, lll.cpp:110-116: lt[0] = g(kappa,kappa),
    //      lt[i] = lt[i-1] - mu(kappa,i-1) r(kappa,i-1); lane i keeps lt[i] for i < kappa
    const double lt0 = C.gf[(size_t)sk * ldd + sk];
    double prod[NQ], ltv[NQ], f[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
      const int t = lane + 64 * q;
      prod[q]     = T.murow[q] * T.rrow[q];
      ltv[q]      = 0.0;
      f[q]        = 0.0;
      if (t < kappa)
        f[q] = T.rdg[M.sl[q]] * delta;  // delta * r(t,t), lll.cpp:116,129
    }
    double g = lt0;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
      const int hi = min(kappa - 64 * q, 64);
      for (int kk = 0; kk < hi; ++kk)
      {
        ltv[q] = (lane == kk) ? g : ltv[q];
        g      = g - g_rl_f64(prod[q], kk);
      }
    }
    // g = lt[kappa]
    double ltc[NQ];  // lane t: the value row t's threshold is compared with: lt[t], or lt[t + 1] with Siegel
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      ltc[q] = ltv[q];
    if (siegel)
    {
#pragma unroll
      for (int q = 0; q < NQ; ++q)
      {
        double dn = __shfl_down(ltv[q], 1);
        if (q + 1 < NQ)
        {
          const double carry = g_rl_f64(ltv[q + 1 < NQ ? q + 1 : q], 0);
          dn                 = (lane == 63) ? carry : dn;
        }
        ltc[q] = (lane + 64 * q == kappa - 1) ? g : dn;
      }
    }
    bool swp = false;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      swp |= (lane + 64 * q == kappa - 1) && (f[q] > ltc[q]);
    double ltk = g;
    if (__any(swp))
    {
      ++nswaps;
      const int old_k = kappa;
      // insertion index: largest kappa' in (kmin, old_k) with delta r(kappa'-1) < lt[kappa'-1]
      int knew = kmin;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
      {
        const int t      = lane + 64 * q;
        const bool cand  = t >= kmin && t <= old_k - 2 && f[q] < ltc[q];
        const uint64_t m = __ballot(cand);
        if (m)
          knew = max(knew, 64 * q + (63 - __clzll((long long)m)) + 1);
      }
      knew = uni(knew);
      ltk  = lane_get<NQ>(ltv, knew);
      if (ltk > 0.0)
      {
        // move_row(old_k, knew), gso_gram.cpp:286-314: rotate_gram_right over the whole range — the slot table
        rotate_right<NQ>(M, knew, old_k, lane);
        clamp_valid<NQ>(T, C, M, knew);
        kappa = knew;
      }
      else
      {  // linearly dependent row: to the end, lll.cpp:144-150
        ++zeros;
        gram_move_to_end<NQ>(T, C, M, G, tmp, old_k, kend - zeros, nkr);
        kappa = old_k;
        continue;
      }
    }
    // ---- set_r(kappa, kappa, lt[kappa]), lll.cpp:153
    {
      const int s = M.phys(kappa);
      if (lane == 0)
      {
        T.r[(size_t)s * ldd + kappa] = ltk;
        T.rdg[s]                     = ltk;
        if (C.vc[s] == kappa)
          C.vc[s] = kappa + 1;
      }
    }
    ++kappa;
    __threadfence_block();
  }
  if (ok)
    status = (kappa < kend - zeros) ? -3 : 1;
  return status;
}

template <int NQ> __device__ __forceinline__ Lattice<NQ> gram_lattice(const GramBatch &P, int L, int lane)
{
  Lattice<NQ> T;
  const int d = P.d, ldd = P.ldd;
  T.d           = d;
  T.n           = d;
  T.ldd         = ldd;
  T.ldn         = ldd;
  T.row_expo_on = 0;
  T.lane        = lane;
  T.b           = nullptr;  // no basis: the Gram cache is complete, nothing ever asks for a row of b
  T.bfT         = nullptr;
  T.mu          = P.mu + (size_t)L * d * ldd;
  T.muT         = P.muT + (size_t)L * d * ldd;
  T.r           = P.r + (size_t)L * d * ldd;
  T.rdg         = P.rdg + (size_t)L * d;
  T.rexp        = nullptr;
  T.bfT32       = nullptr;
  T.b32         = nullptr;
  T.narrow_flag = nullptr;
  T.np          = 0;
  T.f32ok       = 0;
  T.wide_ring   = 0;
  T.u           = P.u ? P.u + (size_t)L * d * ldd : nullptr;
  return T;
}

// info[4] per form: final_kappa, n_swaps, zeros, loop iterations (low 31 bits)
template <int NQ>
__global__ void __launch_bounds__(256) lll_gram_kernel(GramBatch P, double delta, double eta, double logdelta, int siegel)
{
  const int lane = threadIdx.x & 63;
  const int wpb  = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  ReduceRing<NQ> ring;
  ring.init(wave, lane);
  const int d = P.d, ldd = P.ldd;
  for (int L = blockIdx.x * wpb + wave; L < P.batch; L += gridDim.x * wpb)
  {
    Lattice<NQ> T = gram_lattice<NQ>(P, L, lane);
    LllCtx C{P.gf + (size_t)L * d * ldd, P.vc + (size_t)L * d};
    long long *G  = P.g + (size_t)L * d * ldd;
    long long *Go = P.g2 + (size_t)L * d * ldd;
    SlotMap<NQ> M;
    gram_init_state<NQ>(T, C, M, G);
    int final_kappa, nswaps, zeros;
    long long iter;
    const int status =
        gram_lll_run<NQ>(T, C, M, ring, G, Go, delta, eta, logdelta, siegel != 0, final_kappa, nswaps, zeros, iter);
    __threadfence_block();
    // symmetrize_g (lll.cpp:157-158) has nothing to do: both triangles were kept.  g in position order:
    for (int p = 0; p < d; ++p)
    {
      const int sp = M.phys(p);
#pragma unroll
      for (int q = 0; q < NQ; ++q)
      {
        const int c = lane + 64 * q;
        if (c < d)
          Go[(size_t)p * ldd + c] = G[(size_t)sp * ldd + M.sl[q]];
      }
    }
    if (T.u != nullptr)
      u_write_ordered<NQ>(T, M, P.u2 + (size_t)L * d * ldd);
    if (lane == 0)
    {
      P.status[L]       = status;
      P.info[4 * L + 0] = final_kappa;
      P.info[4 * L + 1] = nswaps;
      P.info[4 * L + 2] = zeros;
      P.info[4 * L + 3] = (int)(iter & 0x7fffffff);
    }
    __threadfence_block();
  }
}

// MatGSOInterface::update_gso() (gso_interface.h:767-775) of every form: update_gso_row(i) for i = 0 .. d-1 on a fresh
// object; mu / r in the identity layout.  status 1, or 0 where a mu is not finite (the reference stops at that row)
template <int NQ> __global__ void __launch_bounds__(256) gram_update_kernel(GramBatch P)
{
  const int lane = threadIdx.x & 63;
  const int wpb  = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  ReduceRing<NQ> ring;
  ring.init(wave, lane);
  const int d = P.d, ldd = P.ldd;
  for (int L = blockIdx.x * wpb + wave; L < P.batch; L += gridDim.x * wpb)
  {
    Lattice<NQ> T = gram_lattice<NQ>(P, L, lane);
    LllCtx C{P.gf + (size_t)L * d * ldd, P.vc + (size_t)L * d};
    SlotMap<NQ> M;
    gram_init_state<NQ>(T, C, M, P.g + (size_t)L * d * ldd);
    bool ok = true;
    for (int i = 0; i < d; ++i)
    {
      ok &= update_row_cached(T, C, M, ring, i, i);
      __threadfence_block();
    }
    if (lane == 0)
      P.status[L] = ok ? 1 : 0;
  }
}

template __global__ void lll_gram_kernel<1>(GramBatch, double, double, double, int);
template __global__ void lll_gram_kernel<2>(GramBatch, double, double, double, int);
template __global__ void lll_gram_kernel<3>(GramBatch, double, double, double, int);
template __global__ void lll_gram_kernel<4>(GramBatch, double, double, double, int);
template __global__ void gram_update_kernel<1>(GramBatch);
template __global__ void gram_update_kernel<2>(GramBatch);
template __global__ void gram_update_kernel<3>(GramBatch);
template __global__ void gram_update_kernel<4>(GramBatch);

}  // namespace fphip
