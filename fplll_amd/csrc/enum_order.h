// enum_order.h — the reference's depth-first ORDER, recomputed from coefficients (reference-order mode,
// fphip_enum_opts::ordered; DESIGN.md "reference-order mode").
//
// The reference visits the children of a node in zig-zag order around the rounded centre
// (enumerate_base.cpp:70-71, 80-85) and, below an all-zero prefix, upwards only (:86-89).  The position of a
// child in that sequence is its RANK; the ranks of a coefficient vector from the top level down, compared
// lexicographically, are its place in the reference's walk.  One source for the host (keys of the reported
// candidates, the replay, the frontier between two windows) and the device (task_order_kernel, enum_order.hip):
// the per-level primitives below are all the arithmetic there is, with the reference's operation order and no
// contraction (the library is compiled with -ffp-contract=off).
#ifndef FPHIP_ENUM_ORDER_H
#define FPHIP_ENUM_ORDER_H

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define FPHIP_HD __host__ __device__
#else
#define FPHIP_HD
#endif

namespace fphip
{

// roundto (enumerate_base.h: round(), ties away from zero), the walk kernels' expression
FPHIP_HD inline double order_round(double c)
{
  double x        = rint(c);
  const double al = x - c;
  if (fabs(al) == 0.5 && ((al < 0.0) == (c > 0.0)))
    x = x - (al + al);
  return x;
}

// one term of the centre, from the top: c = c - x[j] * mu(j,k), j = d-1 ... k+1 (enumerate_base.cpp:63-64)
FPHIP_HD inline double order_centre_step(double c, double xj, double mu_jk) { return c - xj * mu_jk; }

// what level k adds to the partial distance: alpha * alpha * r_kk (enumerate_base.cpp:28-29)
FPHIP_HD inline double order_term(double xk, double c, double r_kk)
{
  const double a = xk - c;
  return a * a * r_kk;
}

// Rank of coefficient xk among the children of its parent, whose centre at this level is c.  zero_chain: the
// partial distance above the level is exactly 0.0 — the reference only counts upwards there (:86-89).
// A coefficient the reference never reaches (behind the start of the zero chain) gets the largest rank.
#define FPHIP_ORDER_RANK_MAX 0xffffffffu
FPHIP_HD inline unsigned order_rank(double xk, double c, bool zero_chain)
{
  const double x0 = order_round(c);
  double rk;
  if (zero_chain)
    rk = xk - x0;
  else
  {
    const double t = (c >= x0) ? (xk - x0) : (x0 - xk);
    rk             = t > 0.0 ? t + t - 1.0 : -(t + t);
  }
  if (!(rk >= 0.0) || rk >= 4294967295.0)
    return FPHIP_ORDER_RANK_MAX;
  return (unsigned)rk;
}

// Ranks and partial distances of the coefficients x[lo..d) (levels below lo: rank 0, nd untouched):
// mut[k * d + j] = mu(j,k) for j > k (the layout fphip_enum_run receives); rank[k], nd[k] = the partial
// distance INCLUDING level k (the reference's newdist at level k; nd[0] is the vector's squared norm).
inline void order_vector(int d, const double *mut, const double *rdiag, const double *x, int lo, unsigned *rank,
                         double *nd)
{
  double pd = 0.0;
  for (int k = 0; k < lo; ++k)
    rank[k] = 0u;
  for (int k = d - 1; k >= lo; --k)
  {
    double c = 0.0;
    for (int j = d - 1; j > k; --j)
      c = order_centre_step(c, x[j], mut[(size_t)k * d + j]);
    rank[k] = order_rank(x[k], c, pd == 0.0);
    pd      = pd + order_term(x[k], c, rdiag[k]);
    if (nd)
      nd[k] = pd;
  }
}

// lexicographic from the top level: a before b in the reference's walk
inline bool order_before(int d, const unsigned *a, const unsigned *b)
{
  for (int k = d - 1; k >= 0; --k)
    if (a[k] != b[k])
      return a[k] < b[k];
  return false;
}

}  // namespace fphip
#endif
