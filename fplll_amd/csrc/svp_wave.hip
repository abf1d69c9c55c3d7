// svp_wave.hip — the shortest-vector solver for a BATCH of small and medium lattices (at most 64 rows): one
// wavefront per lattice, the whole batch in one launch.  shortest_vector(b, sol_coord, SVPM_FAST) of the reference
// (svpcvp.cpp:84-241) on the state fphip_gso_update leaves (b, mu, r, row exponents), with the decision on EXACT
// integers: tests/svp_model.py is the model, operation by operation.
//
// Per lattice:
//   1. the exact int64 squared norm of every row, lanes = columns; a norm beyond 63 bits: status -2, outputs zero;
//   2. last_useful_index (svpcvp.cpp:32-43) on the true r_ii (row exponents applied): rows >= d_eff keep 0;
//   3. get_basis_min (svpcvp.cpp:47-59): the initial answer is the shortest of the rows < d_eff, e_i0, norm N0;
//   4. the depth-first walk of bkz_kernel.hip (CHILD chain / STEP loop, half tree, round() ties away from zero,
//      separate multiplies and adds, normalisation by 2^normexp as enumerate.cpp:88-141) under the level bounds
//      pruning[k] * maxdist; column stack and mu triangle in LDS;
//   5. the evaluator: a leaf with 0 < nd <= bound is a candidate; the wave forms v = sum x_i b_i and |v|^2 in int64
//      (lanes = columns, overflow detected); it replaces the best only if its exact norm is strictly smaller, and the
//      radius becomes (double)(N_best - 1) (1 + 2^-30): squared norms are integers, only norm <= N_best - 1 improves.
//      The 2^-30 is the heuristic margin of the closest-vector and list solvers, not a proved bound.
// The walk is sequential in the reference's order: the answer is the first vector of minimal exact norm in
// depth-first order, or e_i0 when nothing shorter exists.
//
// Branches in the walk are wave-uniform (k, the distances and the bounds are read through readlane); level registers
// are read across lanes with g_rl_f64 / readlane, never through lane-masked branches.
#include "gso_wave.h"
#include "kernels.h"

namespace fphip
{

__device__ __forceinline__ int stri(int k) { return (k * (k - 1)) >> 1; }

// sum over the wave of non-negative addends; ovf collects a sum beyond 63 bits (every partial sum of the butterfly
// is a sub-sum of the total, so one of them overflows exactly when the total does)
__device__ __forceinline__ long long wave_sum_nonneg(long long v, bool &ovf)
{
  for (int off = 32; off > 0; off >>= 1)
  {
    const long long o = (long long)__shfl_xor(v, off);
    long long s;
    ovf |= __builtin_add_overflow(v, o, &s);
    v = s;
  }
  return v;
}

// |row|^2 of the values a wave holds as lanes = columns; false: beyond 63 bits
template <int NQ> __device__ __forceinline__ bool exact_norm(const long long (&v)[NQ], long long &out)
{
  bool ovf      = false;
  long long acc = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
  {
    long long p, s;
    ovf |= __builtin_mul_overflow(v[q], v[q], &p);
    ovf |= __builtin_add_overflow(acc, p, &s);
    acc = s;
  }
  acc = ovf ? 0 : acc;  // (a wrapped value may be negative: keep the butterfly's addends non-negative)
  out = g_rl_i64(wave_sum_nonneg(acc, ovf), 0);  // (every lane holds the total: a scalar from here on)
  return !__any(ovf);
}

template <int NQ> __global__ void __launch_bounds__(256) svp_wave_kernel(GsoBatch P, SvpWave A)
{
  extern __shared__ __attribute__((aligned(16))) char svp_smem[];
  const int lane = threadIdx.x & 63;
  const int wpb  = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int d = P.d, n = P.n, ldd = P.ldd, ldn = P.ldn;
  // per wave: the triangular column stack of the walk, then the scaled mu triangle
  double *stk    = (double *)svp_smem + (size_t)wave * (A.stack_doubles + A.mu_doubles);
  double *mu_blk = stk + A.stack_doubles;
  for (int W = blockIdx.x * wpb + wave; W < A.count; W += gridDim.x * wpb)
  {
    if (A.take && A.take[W] == 0)
      continue;
    const size_t L     = (size_t)(A.first + W);
    const long long *b = P.b + L * d * ldn;
    const double *mu   = P.mu + L * d * ldd;
    const double *rdg  = P.rdg + L * d;
    const long long *rexp = P.rexp + L * d;
    long long *o_sol = A.sol_coord + (size_t)W * d;
    long long *o_vec = A.vec + (size_t)W * n;

    int status               = P.status[L] == 1 ? 1 : 0;
    long long nbest          = 0;
    unsigned long long nodes = 0;
    double best_x            = 0.0;  // lane i: coefficient of the best vector
    long long bv[NQ];                // the best vector, lanes = columns
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      bv[q] = 0;

    // ---- 1. exact row norms: lane i keeps |b_i|^2 ----------------------------------------------
    long long rn = 0;
    if (status == 1)
    {
      for (int i = 0; i < d; ++i)
      {
        long long row[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
        {
          const int c = lane + 64 * q;
          row[q]      = (c < n) ? b[(size_t)i * ldn + c] : 0;
        }
        long long nr;
        if (!exact_norm<NQ>(row, nr))
        {
          status = -2;
          break;
        }
        rn = (lane == i) ? nr : rn;
      }
    }
    if (status == 1)
    {
      // ---- 2. last_useful_index on the true r_ii ------------------------------------------------
      const bool in      = lane < d;
      const double rr    = in ? rdg[lane] : 0.0;
      const long long ei = (in && P.row_expo) ? rexp[lane] : 0;
      const long long e0 = g_rl_i64(ei, 0);
      const double r00x2 = g_rl_f64(rr, 0) * 2.0;
      const long long de = 2 * (ei - e0);
      const double ri    = ldexp(rr, (int)max(min(de, 4000ll), -4000ll));
      const uint64_t um  = __ballot(in && lane > 0 && ri <= r00x2);
      const int d_eff    = um ? 64 - __clzll((long long)um) : 1;
      // ---- 3. get_basis_min: the shortest row below d_eff, the lowest index on ties --------------
      int i0 = 0;
      nbest  = g_rl_i64(rn, 0);
      for (int i = 1; i < d_eff; ++i)
      {
        const long long ni = g_rl_i64(rn, i);
        if (ni < nbest)
        {
          nbest = ni;
          i0    = i;
        }
      }
      best_x = (lane == i0) ? 1.0 : 0.0;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
      {
        const int c = lane + 64 * q;
        bv[q]       = (c < n) ? b[(size_t)i0 * ldn + c] : 0;
      }
      const double radius0 = (double)(nbest - 1) * (1.0 + 0x1p-30);
      if (d_eff >= 2 && radius0 > 0.0)
      {
        // ---- 4. normalisation, enumerate.cpp:88-141 ---------------------------------------------
        const int bs     = d_eff;
        const bool inb   = lane < bs;
        const int e2     = inb ? (int)(2 * ei) : 0;
        int ne           = inb ? (int)min((long long)e2 + fexponent(rr), (long long)INT_MAX) : INT_MIN;
        ne               = max(wave_max_i32(ne), -1);  // normexp starts at -1, enumerate.cpp:88
        const double rd  = inb ? ldexp(rr, e2 - ne) : 0.0;  // lane i: rdiag[i]
        const double prn = (inb && A.pruning) ? A.pruning[lane] : 1.0;
        double maxdist   = ldexp(radius0, -ne);
        double pb        = prn * maxdist;  // lane k: the bound of level k
        // mu rows with the row exponents applied (get_mu, gso_interface.h:694-702), packed like the column stack
        for (int k = 1; k < bs; ++k)
        {
          const long long ek = g_rl_i64(ei, k);
          if (lane < k)
          {
            const double m = mu[(size_t)k * ldd + lane];
            mu_blk[stri(k) + lane] = ldexp(m, (int)(ek - ei));
          }
        }
        __threadfence_block();
        // ---- the walk: enumerate_recursive, depth-first ----------------------------------------
        double xs = 0.0, cs = 0.0, pds = 0.0;
        int dxs = 0, ddxs = 0;
        unsigned long long cnt = 0;
        int k     = bs;
        double S  = 0.0;
        double nd = 0.0;
        bool done = false;
        // 5. the evaluator: the leaf in xs is within the bound with nd > 0
        auto candidate = [&]()
        {
          long long v[NQ];
#pragma unroll
          for (int q = 0; q < NQ; ++q)
            v[q] = 0;
          bool ovf = false;
          for (int i = 0; i < bs; ++i)
          {
            const double xi = g_rl_f64(xs, i);
            if (xi == 0.0)
              continue;
            if (!(fabs(xi) < 9223372036854775808.0))
            {
              ovf = true;
              break;
            }
            const long long lx = (long long)xi;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
            {
              const int c        = lane + 64 * q;
              const long long bi = (c < n) ? b[(size_t)i * ldn + c] : 0;
              long long p, s;
              ovf |= __builtin_mul_overflow(lx, bi, &p);
              ovf |= __builtin_add_overflow(v[q], p, &s);
              v[q] = s;
            }
          }
          long long nv = 0;
          if (__any(ovf) || !exact_norm<NQ>(v, nv))
          {  // a candidate beyond 63 bits: the lattice is given up
            status = -2;
            done   = true;
            return;
          }
          if (nv > 0 && nv < nbest)
          {
            nbest  = nv;
            best_x = xs;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
              bv[q] = v[q];
            maxdist = ldexp((double)(nbest - 1) * (1.0 + 0x1p-30), -ne);
            pb      = prn * maxdist;
            if (nbest == 1)
              done = true;  // nothing non-zero is shorter
          }
        };
        while (!done)
        {
          // CHILD chain: descend while the first child survives
          for (;;)
          {
            k               = __builtin_amdgcn_readfirstlane(k);
            const int kc    = k - 1;
            const double c1 = g_rl_f64(S, kc);
            const double x1 = round(c1);  // roundto(), enumerate_base.h:33-34
            const double a1 = x1 - c1;
            const double n1 = nd + a1 * a1 * g_rl_f64(rd, kc);
            if (!(n1 <= g_rl_f64(pb, kc)))
            {
              done = k >= bs;
              break;
            }
            if (lane < k)
              stk[stri(k) + lane] = S;
            {
              const int s1  = (c1 >= x1) ? 1 : -1;
              const bool me = lane == kc;
              cs            = me ? c1 : cs;
              xs            = me ? x1 : xs;
              pds           = me ? nd : pds;
              dxs           = me ? s1 : dxs;
              ddxs          = me ? s1 : ddxs;
              cnt += me ? 1ull : 0ull;
            }
            k  = kc;
            nd = n1;
            if (k == 0)
            {
              if (nd > 0.0)
                candidate();
              break;
            }
            const double mk = mu_blk[stri(k) + min(lane, k - 1)];
            S               = S - x1 * mk;
          }
          if (done)
            break;
          // STEP loop: next sibling at level k, climbing while they fail
          for (;;)
          {
            k                = __builtin_amdgcn_readfirstlane(k);
            const double par = stk[stri(k + 1) + min(lane, k)];  // S_{k+1}
            const double mk  = mu_blk[stri(k) + max(min(lane, k - 1), 0)];
            double xk        = g_rl_f64(xs, k);
            const double ck  = g_rl_f64(cs, k);
            const double pdk = g_rl_f64(pds, k);
            int dxk = __builtin_amdgcn_readlane(dxs, k), ddxk = __builtin_amdgcn_readlane(ddxs, k);
            if (pdk != 0.0)
            {
              xk += (double)dxk;
              ddxk = -ddxk;
              dxk  = ddxk - dxk;
            }
            else
            {
              xk += 1.0;
            }
            const bool me  = lane == k;
            xs             = me ? xk : xs;
            dxs            = me ? dxk : dxs;
            ddxs           = me ? ddxk : ddxs;
            const double a = xk - ck;
            nd             = pdk + a * a * g_rl_f64(rd, k);
            if (!(nd <= g_rl_f64(pb, k)))
            {
              ++k;
              if (k >= bs)
              {
                done = true;
                break;
              }
              continue;
            }
            cnt += me ? 1ull : 0ull;
            if (k == 0)
            {
              if (nd > 0.0)
              {
                candidate();
                if (done)
                  break;
              }
              continue;
            }
            S = par - xk * mk;
            break;
          }
        }
        // node total by the fplll rule (the initial descent is compensated, enumerate_base.cpp:181)
        unsigned long long tot = cnt;
        for (int off = 32; off > 0; off >>= 1)
          tot += (unsigned long long)__shfl_xor((long long)tot, off);
        nodes = (unsigned long long)g_rl_i64((long long)tot, 0) - (unsigned long long)(bs - 1);
      }
    }
    // ---- 6. outputs -----------------------------------------------------------------------------
    const bool ok = status == 1;
    if (lane < d)
      o_sol[lane] = ok ? (long long)best_x : 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
      const int c = lane + 64 * q;
      if (c < n)
        o_vec[c] = ok ? bv[q] : 0;
    }
    if (lane == 0)
    {
      A.norm[W]   = ok ? nbest : 0;
      A.nodes[W]  = ok ? nodes : 0;
      A.status[W] = status;
    }
    __threadfence_block();
  }
}

template __global__ void svp_wave_kernel<1>(GsoBatch, SvpWave);
template __global__ void svp_wave_kernel<2>(GsoBatch, SvpWave);
template __global__ void svp_wave_kernel<3>(GsoBatch, SvpWave);
template __global__ void svp_wave_kernel<4>(GsoBatch, SvpWave);

}  // namespace fphip
