// cvp_prepare.hip — what closest_vector (svpcvp.cpp:532-659) does to a target before it enumerates, for a BATCH of
// targets against one lattice; and MatGSOInterface::babai (gso_interface.cpp:292-311) for a batch of vectors.
//
// One target per lane, as hh_rows.hip places one lattice per lane: the loops over rows and columns are the same for
// every lane, so the basis, mu and r are read wave-uniformly (the compiler's scalar loads), and a lane's own vectors
// live in a column of a workspace in global memory — element i of lane t at [i][t], consecutive lanes consecutive
// addresses.  No LDS, no cross-lane traffic: the targets are independent.
//
// Per target (cvp_prepare_kernel), plain double, every operation a separate IEEE multiply / add / divide in the
// order the reference's loops state (-ffp-contract=off; the reference runs them in MPFR at max(53, min_prec + 10)
// bits, so parity with it is asked of the solver's integer result, not of these doubles):
//   pass:   v[j] = (double) t[j]                                                 svpcvp.cpp:576-579
//           c[i] = sum_j v[j] bf(i,j), then c[i] -= mu(i,j) c[j] for j < i; c[i] /= r(i,i)    get_gscoords, :494-515
//           x = c; for i = d-1 .. 0: x[i] = round(x[i]); x[j] -= mu(i,j) x[i] for j < i      babai, :524-529
//           every x[i] in [-1, 1]: done.  Otherwise coef += x, t -= sum_i x[i] b_i (exact int64) and again  :582-594
//   result: coef, target_coord = c of the last pass (:597 recomputes exactly that), and the squared distance of the
//           rounding descent from target_coord in prepare_enumeration's operand order (enumerate.cpp:167-215:
//           newcenter -= x[j] * mu(j,k), j ascending; alpha = x[k] - newcenter; dist += alpha * alpha * r(k,k)).
// round() is mpfr_round's rule: ties away from zero.  mu and r are the TRUE values: cvp_unscale_kernel applies the row
// exponents of the device GSO first (get_mu_exp / get_r_exp: mu 2^(e_i - e_j), r 2^(2 e_i)) and floats the basis.
// status: 1 ok; -2 a rounded coordinate, a coefficient or an entry of the running target left the 63-bit range (the
// caller falls back); -1 the loop limit (the reference only warns, at 0x100 passes) — a lane never spins.
// One more way out of the loop than the reference has: a pass whose x is exactly minus the x of the pass before would
// bring back the target of two passes ago — the loop would alternate between two targets for ever, which is what a
// target exactly halfway between two lattice points does to it (a tie rounds away from zero: 1/2 -> 1, then -1/2 -> -1;
// the reference never returns from such a target).  Both targets are as near the origin as the loop brings them, so
// the lane ends there, status 1, with the coefficients and the coordinates of this pass.
//
// cvp_babai_kernel is the nearest-plane loop alone on rows [start, start + dimension) with FP_NR<double>::rnd's rule
// (rint: ties to even), one pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gso_device.h"
#include "kernels.h"

namespace fphip
{
// mu / r without the row exponents, the basis as doubles: what the reference's solver holds (its MatGSO has no
// GSO_ROW_EXPO, svpcvp.cpp:552).  ldexp is exact short of overflow / underflow.
__global__ void __launch_bounds__(256) cvp_unscale_kernel(GsoBatch P, int lattice, double *bfd, double *mu, double *rd)
{
  const int d = P.d, n = P.n;
  const size_t L        = (size_t)lattice;
  const double *mus     = P.mu + L * d * P.ldd;
  const double *rs      = P.r + L * d * P.ldd;
  const long long *bs   = P.b + L * d * P.ldn;
  const long long *rexp = P.rexp + L * d;
  const int stride      = gridDim.x * blockDim.x;
  const int tid         = blockIdx.x * blockDim.x + threadIdx.x;
  for (int e = tid; e < d * d; e += stride)
  {
    const int i = e / d, j = e % d;
    double v = 0.0;
    if (j < i)
    {
      const long long de = P.row_expo ? rexp[i] - rexp[j] : 0;
      v                  = ldexp(mus[(size_t)i * P.ldd + j], (int)de);
    }
    mu[e] = v;
  }
  for (int e = tid; e < d * n; e += stride)
    bfd[e] = (double)bs[(size_t)(e / n) * P.ldn + (e % n)];
  for (int i = tid; i < d; i += stride)
    rd[i] = ldexp(rs[(size_t)i * P.ldd + i], P.row_expo ? (int)(2 * rexp[i]) : 0);
}

__device__ __forceinline__ bool fits63(double x) { return fabs(x) < 9223372036854775808.0; }  // (false for a NaN)

__global__ void __launch_bounds__(64) cvp_prepare_kernel(CvpPrep P)
{
  const int t      = blockIdx.x * 64 + threadIdx.x;
  const bool mine  = t < P.T;
  const int d = P.d, n = P.n;
  const size_t ldt = (size_t)P.ldt;
  double *wv       = P.wv + t;
  double *wc       = P.wc + t;
  double *wx       = P.wx + t;
  long long *wt    = P.wt + t;
  long long *wk    = P.wk + t;
  double *wp       = P.wp + t;
  int st           = 0;  // 0: still reducing
  if (mine)
  {
    for (int j = 0; j < n; ++j)
      wt[j * ldt] = P.targets[(size_t)t * n + j];
    for (int i = 0; i < d; ++i)
      wk[i * ldt] = 0;
  }
  else
    st = 1;  // (a lane past the batch: nothing to do, and it keeps the loop below uniform)
  // every lane of the wave runs the same passes; a lane that is done sits them out
  for (int pass = 0; __ballot(st == 0) != 0ull; ++pass)
  {
    if (st != 0)
      continue;
    if (pass >= P.max_passes)
    {
      st = -1;
      continue;
    }
    for (int j = 0; j < n; ++j)
      wv[j * ldt] = (double)wt[j * ldt];
    // get_gscoords
    for (int i = 0; i < d; ++i)
    {
      double acc = 0.0;
      for (int j = 0; j < n; ++j)
        acc = acc + wv[j * ldt] * P.bfd[(size_t)i * n + j];
      for (int j = 0; j < i; ++j)
        acc = acc - P.mu[(size_t)i * d + j] * wc[j * ldt];
      wc[i * ldt] = acc;
    }
    for (int i = 0; i < d; ++i)
    {
      const double c = wc[i * ldt] / P.rd[i];
      wc[i * ldt]    = c;
      wx[i * ldt]    = c;
    }
    // babai
    bool small = true, undo = pass > 0;  // undo: x == -(the x of the pass before)
    for (int i = d - 1; i >= 0; --i)
    {
      const double xi = round(wx[i * ldt]);
      wx[i * ldt]     = xi;
      small           = small && (xi >= -1.0 && xi <= 1.0);
      undo            = undo && xi == -wp[i * ldt];
      wp[i * ldt]     = xi;
      for (int j = 0; j < i; ++j)
        wx[j * ldt] = wx[j * ldt] - P.mu[(size_t)i * d + j] * xi;
    }
    if (small || undo)
    {
      st = 1;
      continue;
    }
    // coef += x, target -= sum x_i b_i: exact, or the lane gives up
    bool ok = true;
    for (int i = 0; i < d && ok; ++i)
    {
      const double xi = wx[i * ldt];
      if (!fits63(xi))
      {
        ok = false;
        break;
      }
      const long long ci = (long long)xi;
      long long s;
      if (__builtin_add_overflow(wk[i * ldt], ci, &s))
      {
        ok = false;
        break;
      }
      wk[i * ldt] = s;
      if (ci == 0)
        continue;
      for (int j = 0; j < n; ++j)
      {
        long long p, q;
        if (__builtin_mul_overflow(ci, P.b[(size_t)i * P.ldn + j], &p) || __builtin_sub_overflow(wt[j * ldt], p, &q))
        {
          ok = false;
          break;
        }
        wt[j * ldt] = q;
      }
    }
    if (!ok)
      st = -2;
  }
  if (!mine)
    return;
  P.status[t] = st;
  if (st != 1)
  {
    for (int i = 0; i < d; ++i)
    {
      P.coef[(size_t)t * d + i]   = 0;
      P.tcoord[(size_t)t * d + i] = 0.0;
    }
    P.descent[t] = 0.0;
    return;
  }
  // the rounding descent from target_coord (prepare_enumeration's operand order)
  double dist = 0.0;
  for (int k = d - 1; k >= 0; --k)
  {
    double newcenter = wc[k * ldt];
    for (int j = k + 1; j < d; ++j)
      newcenter = newcenter - wx[j * ldt] * P.mu[(size_t)j * d + k];
    const double xk    = round(newcenter);
    wx[k * ldt]        = xk;
    const double alpha = xk - newcenter;
    dist               = dist + alpha * alpha * P.rd[k];
  }
  P.descent[t] = dist;
  for (int i = 0; i < d; ++i)
  {
    P.coef[(size_t)t * d + i]   = wk[i * ldt];
    P.tcoord[(size_t)t * d + i] = wc[i * ldt];
  }
}

// MatGSOInterface::babai(w, v, start, dimension): x = v; for i = dimension-1 .. 0: x[i] = rint(x[i]),
// x[j] -= mu(start + i, start + j) x[i] for j < i; w = x as integers.  v, w [T][dimension]; wx [dimension][ldt].
__global__ void __launch_bounds__(64)
cvp_babai_kernel(int T, int ldt_, int d, int start, int dimension, const double *mu, const double *v, long long *w,
                 int *status, double *wxa)
{
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= T)
    return;
  const size_t ldt = (size_t)ldt_;
  double *wx       = wxa + t;
  for (int i = 0; i < dimension; ++i)
    wx[i * ldt] = v[(size_t)t * dimension + i];
  for (int i = dimension - 1; i >= 0; --i)
  {
    const double xi = rint(wx[i * ldt]);
    wx[i * ldt]     = xi;
    for (int j = 0; j < i; ++j)
      wx[j * ldt] = wx[j * ldt] - mu[(size_t)(start + i) * d + (start + j)] * xi;
  }
  int st = 1;
  for (int i = 0; i < dimension; ++i)
    if (!fits63(wx[i * ldt]))
      st = -2;
  for (int i = 0; i < dimension; ++i)
    w[(size_t)t * dimension + i] = st == 1 ? (long long)wx[i * ldt] : 0;
  status[t] = st;
}
}  // namespace fphip
