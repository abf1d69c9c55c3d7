// cvp_wave.hip — the closest-vector solver for a BATCH of targets against ONE lattice of at most 64 rows: one
// wavefront per target, the whole batch in one launch (a grid-stride loop over the targets).  The closest-vector twin
// of svp_wave.hip; tests/cvp_wave_model.py is the model, operation by operation.
//
// Inputs: what the preparation (cvp_prepare.hip) leaves on the device — coef, target_coord, descent, status —, the
// integer targets, and the TRUE mu and r_ii of cvp_unscale_kernel (the row exponents applied), exactly what the ENUM
// route hands fphip_enum_run.  Per target with status 1, d >= 2, a finite descent > 0 and finite r_ii > 0:
//   1. the reduced target t_red = target - sum coef_i b_i in exact int64, lanes = columns (rows in ascending order,
//      a zero coefficient skipped); a product or a difference beyond 63 bits: status -2.  It is the vector whose
//      Gram-Schmidt coordinates are target_coord.
//   2. the depth-first walk of svp_wave.hip (CHILD chain / STEP loop, round() ties away from zero, separate
//      multiplies and adds, !(nd <= bound) as the cut) with these differences: the root's centre row is
//      target_coord; siblings ALWAYS zig-zag (enumerate_base.cpp:80, !is_svp); every leaf within the bound is a
//      candidate, distance 0 included; no normalisation and no pruning — every level's bound is the radius.
//   3. the evaluator, on exact integers: N = |t_red - sum x_i b_i|^2 in int64 (overflow: status -2).  The first
//      candidate wins, later ones only with a strictly smaller N.  After a win at walk distance nd the radius is
//      min(radius, nd + nd 2^-30); N = 0 ends the walk.  The initial radius is descent + descent 2^-30, as in the
//      ENUM route.  The 2^-30 is the heuristic margin of the solvers, not a proved bound.
//   4. nodes: the plain count of accepted (level, coefficient) pairs, leaves included.  max_nodes > 0 is a budget,
//      tested at the top of every pass of the STEP loop: once the count has reached it the walk stops, status 2, the
//      best point so far in the outputs.
// A target that is not walked (and a walk that ends without a candidate: found = 0) is left to the host, which fills
// in the rounding descent as the ENUM route does.
//
// LDS: the mu triangle is the same for every wave of the workgroup (one lattice): ONE copy per workgroup, d (d - 1) / 2
// doubles, loaded once with one barrier before the target loop and none in the walk; every wave has its own column
// stack of d (d + 1) / 2 + 2 doubles behind it.
//
// Branches in the walk are wave-uniform (k, the distances and the radius are scalars or read through readlane); level
// registers are read across lanes with g_rl_f64 / readlane, never through lane-masked branches.
#include "gso_wave.h"
#include "kernels.h"

namespace fphip
{

__device__ __forceinline__ int ctri(int k) { return (k * (k - 1)) >> 1; }

// sum over the wave of non-negative addends; ovf collects a sum beyond 63 bits (every partial sum of the butterfly
// is a sub-sum of the total, so one of them overflows exactly when the total does)
__device__ __forceinline__ long long cvp_wave_sum_nonneg(long long v, bool &ovf)
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

// |v|^2 of the values a wave holds as lanes = columns; false: beyond 63 bits
template <int NQ> __device__ __forceinline__ bool cvp_exact_norm(const long long (&v)[NQ], long long &out)
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
  out = g_rl_i64(cvp_wave_sum_nonneg(acc, ovf), 0);  // (every lane holds the total: a scalar from here on)
  return !__any(ovf);
}

// v -= x * row of b (lanes = columns), exact or ovf
template <int NQ>
__device__ __forceinline__ void cvp_sub_row(long long (&v)[NQ], long long x, const long long *row, int n, int lane,
                                            bool &ovf)
{
#pragma unroll
  for (int q = 0; q < NQ; ++q)
  {
    const int c        = lane + 64 * q;
    const long long bi = (c < n) ? row[c] : 0;
    long long p, s;
    ovf |= __builtin_mul_overflow(x, bi, &p);
    ovf |= __builtin_sub_overflow(v[q], p, &s);
    v[q] = s;
  }
}

template <int NQ> __global__ void __launch_bounds__(256) cvp_wave_kernel(GsoBatch P, CvpWave A)
{
  extern __shared__ __attribute__((aligned(16))) char cvp_smem[];
  const int lane = threadIdx.x & 63;
  const int wpb  = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int d = P.d, n = P.n, ldn = P.ldn;
  // per workgroup: the mu triangle; per wave: the triangular column stack of the walk
  double *mu_blk     = (double *)cvp_smem;
  double *stk        = mu_blk + A.mu_doubles + (size_t)wave * A.stack_doubles;
  const long long *b = P.b + (size_t)A.lattice * d * ldn;
  for (int k = 1 + wave; k < d; k += wpb)
    if (lane < k)
      mu_blk[ctri(k) + lane] = A.mu[(size_t)k * d + lane];
  const double rd  = lane < d ? A.rd[lane] : 1.0;  // lane i: r_ii
  const bool rd_ok = __all(rd > 0.0 && rd < __builtin_inf());
  __syncthreads();
  for (int W = blockIdx.x * wpb + wave; W < A.T; W += gridDim.x * wpb)
  {
    int status               = A.pstatus[W];
    const double desc        = A.descent[W];
    long long nbest          = 0;
    unsigned long long nodes = 0;
    double best_x = 0.0, best_nd = 0.0;  // lane i: coefficient of the best point; its walk distance
    int found = 0;
    if (status == 1 && d >= 2 && desc > 0.0 && desc < __builtin_inf() && rd_ok)
    {
      // ---- 1. the reduced target, lanes = columns ------------------------------------------------
      long long tr[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q)
      {
        const int c = lane + 64 * q;
        tr[q]       = (c < n) ? A.targets[(size_t)W * n + c] : 0;
      }
      bool tovf = false;
      for (int i = 0; i < d; ++i)
      {
        const long long ci = A.coef[(size_t)W * d + i];
        if (ci == 0)
          continue;
        cvp_sub_row<NQ>(tr, ci, b + (size_t)i * ldn, n, lane, tovf);
      }
      if (__any(tovf))
        status = -2;
      else
      {
        // ---- 2. the walk: enumerate_recursive with a target, depth-first -----------------------
        double radius = desc + desc * 0x1p-30;
        double xs = 0.0, cs = 0.0, pds = 0.0;
        int dxs = 0, ddxs = 0;
        int k     = d;
        double S  = lane < d ? A.tcoord[(size_t)W * d + lane] : 0.0;
        double nd = 0.0;
        bool done = false;
        // 3. the evaluator: the leaf in xs is within the bound
        auto candidate = [&]()
        {
          long long v[NQ];
#pragma unroll
          for (int q = 0; q < NQ; ++q)
            v[q] = tr[q];
          bool ovf = false;
          for (int i = 0; i < d; ++i)
          {
            const double xi = g_rl_f64(xs, i);
            if (xi == 0.0)
              continue;
            if (!(fabs(xi) < 9223372036854775808.0))
            {
              ovf = true;
              break;
            }
            cvp_sub_row<NQ>(v, (long long)xi, b + (size_t)i * ldn, n, lane, ovf);
          }
          long long nv = 0;
          if (__any(ovf) || !cvp_exact_norm<NQ>(v, nv))
          {  // a candidate beyond 63 bits: the target is given up
            status = -2;
            done   = true;
            return;
          }
          if (!found || nv < nbest)
          {
            found           = 1;
            nbest           = nv;
            best_x          = xs;
            best_nd         = nd;
            const double r2 = nd + nd * 0x1p-30;
            radius          = r2 < radius ? r2 : radius;
            if (nbest == 0)
              done = true;  // nothing is closer
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
            if (!(n1 <= radius))
            {
              done = k >= d;
              break;
            }
            if (lane < k)
              stk[ctri(k) + lane] = S;
            {
              const int s1  = (c1 >= x1) ? 1 : -1;
              const bool me = lane == kc;
              cs            = me ? c1 : cs;
              xs            = me ? x1 : xs;
              pds           = me ? nd : pds;
              dxs           = me ? s1 : dxs;
              ddxs          = me ? s1 : ddxs;
            }
            ++nodes;
            k  = kc;
            nd = n1;
            if (k == 0)
            {
              candidate();
              break;
            }
            const double mk = mu_blk[ctri(k) + min(lane, k - 1)];
            S               = S - x1 * mk;
          }
          if (done)
            break;
          // STEP loop: next sibling at level k (zig-zag), climbing while they fail
          for (;;)
          {
            if (A.max_nodes != 0ull && nodes >= A.max_nodes)
            {  // 4. the budget
              status = 2;
              done   = true;
              break;
            }
            k                = __builtin_amdgcn_readfirstlane(k);
            const double par = stk[ctri(k + 1) + min(lane, k)];  // S_{k+1}
            const double mk  = mu_blk[ctri(k) + max(min(lane, k - 1), 0)];
            double xk        = g_rl_f64(xs, k);
            const double ck  = g_rl_f64(cs, k);
            const double pdk = g_rl_f64(pds, k);
            int dxk = __builtin_amdgcn_readlane(dxs, k), ddxk = __builtin_amdgcn_readlane(ddxs, k);
            xk += (double)dxk;
            ddxk           = -ddxk;
            dxk            = ddxk - dxk;
            const bool me  = lane == k;
            xs             = me ? xk : xs;
            dxs            = me ? dxk : dxs;
            ddxs           = me ? ddxk : ddxs;
            const double a = xk - ck;
            nd             = pdk + a * a * g_rl_f64(rd, k);
            if (!(nd <= radius))
            {
              ++k;
              if (k >= d)
              {
                done = true;
                break;
              }
              continue;
            }
            ++nodes;
            if (k == 0)
            {
              candidate();
              if (done)
                break;
              continue;
            }
            S = par - xk * mk;
            break;
          }
        }
      }
    }
    // ---- outputs --------------------------------------------------------------------------------
    const bool ok = (status == 1 || status == 2) && found;
    if (lane < d)
      A.x[(size_t)W * d + lane] = ok ? (long long)best_x : 0;
    if (lane == 0)
    {
      A.dist[W]   = ok ? best_nd : 0.0;
      A.norm[W]   = ok ? nbest : 0;
      A.nodes[W]  = status == -2 ? 0ull : nodes;
      A.found[W]  = ok ? 1 : 0;
      A.status[W] = status;
    }
    __threadfence_block();
  }
}

template __global__ void cvp_wave_kernel<1>(GsoBatch, CvpWave);
template __global__ void cvp_wave_kernel<2>(GsoBatch, CvpWave);
template __global__ void cvp_wave_kernel<3>(GsoBatch, CvpWave);
template __global__ void cvp_wave_kernel<4>(GsoBatch, CvpWave);

}  // namespace fphip
