// svp_host.h — private to the host translation units: what the N-shortest-vectors entry points of a basis
// (gso_host.hip, fphip_shortest_vectors) and of a quadratic form (gram_host.hip, fphip_gram_shortest_vectors) share on
// the ENUM and AUTO routes — the AUTO limit's default, the device blocks of one call, the rows under enumeration, the
// BEST_N table behind fphip_enum_run's callback, the walk of a single row, and the order of the answers.  The exact candidate is the caller's: a type Cand with the members
// `int d` (the rows under enumeration) and `bool overflow`, and a function
//   bool svp_exact_candidate(Cand *, const double *sol, long long *norm)     false: beyond 63 bits
// next to it (found by argument-dependent lookup).
#ifndef FPHIP_SVP_HOST_H
#define FPHIP_SVP_HOST_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "dev_mem.h"

namespace fphip
{
// The default of FPHIP_SVP_WAVE_MAX_NODES: the Gaussian-heuristic node estimate (radius min(r_00, GH^2)) up to which
// the AUTO route gives a lattice to the wave-per-lattice kernel.  Measured (profiles/svp_solver.md, LLL-reduced q-ary
// lattices, batch 1024): at d = 32 (estimate 5.8e4) WAVE takes 0.179 ms per lattice against ENUM's 0.625 ms, at d = 40
// (estimate 5.0e6) 31.9 ms against 1.43 ms; the two times are equal at an estimate of 2.08e5 (log-log interpolation).
// 0 would mean no limit.  ONE value for fphip_shortest_vector, fphip_shortest_vectors and
// fphip_gram_shortest_vectors: measured on bases, not retuned for K > 1 (profiles/svp_best.md) nor for forms
// (profiles/svp_gram.md).
constexpr double SVP_WAVE_MAX_NODES_DEFAULT = 2.0e5;

// device blocks of one call, back to the cache when it returns
struct CvpBufs
{
  hipStream_t s;
  std::vector<void *> ptrs;
  explicit CvpBufs(hipStream_t s_) : s(s_) {}
  ~CvpBufs()
  {
    for (void *p : ptrs)
      fphip_dev_free(p, s);
  }
  template <class T> hipError_t get(T **p, size_t count)
  {
    void *q            = nullptr;
    const hipError_t e = fphip_dev_alloc(&q, (count ? count : 1) * sizeof(T), s);
    if (e == hipSuccess)
      ptrs.push_back(q);
    *p = (T *)q;
    return e;
  }
};

// last_useful_index (svpcvp.cpp:32-43) on the true r_ii
inline int svp_last_useful_index(int d, const double *rd)
{
  int i;
  for (i = d - 1; i > 0; --i)
    if (rd[i] <= 2.0 * rd[0])
      break;
  return i + 1;
}

// the rows under enumeration: last_useful_index without a caller's bound; with one the threshold max(2 r_00, radius)
inline int svp_best_rows(int d, const double *rd, bool has_bound, double radius0)
{
  if (!has_bound)
    return svp_last_useful_index(d, rd);
  const double thr = std::max(2.0 * rd[0], radius0);
  int i;
  for (i = d - 1; i > 0; --i)
    if (rd[i] <= thr)
      break;
  return i + 1;
}

// the ENUM route's BEST_N evaluator: at most K records sorted by exact norm, ties in arrival order; the accept rule
// and the radius are those of svp_best.hip
template <class Cand> struct SvpTable
{
  Cand cand;  // the exact candidate (d = the rows under enumeration)
  int K;
  long long B0;
  std::vector<long long> norms;           // sorted
  std::vector<std::vector<long long>> x;  // [found][d_eff]
  double radius0() const { return (double)B0 * (1.0 + 0x1p-30); }
  // the radius after a candidate: unchanged until the table is full, then (worst - 1) (1 + 2^-30); 0 = stop
  double bound() const
  {
    if ((int)norms.size() < K)
      return radius0();
    return (double)(norms.back() - 1) * (1.0 + 0x1p-30);
  }
  void offer(long long nv, const double *sol)
  {
    const bool full = (int)norms.size() == K;
    if (!(nv > 0 && nv <= B0 && (!full || nv < norms.back())))
      return;
    const size_t p = (size_t)(std::upper_bound(norms.begin(), norms.end(), nv) - norms.begin());
    norms.insert(norms.begin() + p, nv);
    std::vector<long long> xi((size_t)cand.d);
    for (int i = 0; i < cand.d; ++i)
      xi[i] = (long long)sol[i];
    x.insert(x.begin() + p, xi);
    if ((int)norms.size() > K)
      norms.pop_back(), x.pop_back();
  }
  // the kept records by (norm, the coefficient order of fphip_list_vectors: from level d - 1 down): the arrival order
  // is the parallel walk's
  std::vector<size_t> order() const
  {
    std::vector<size_t> ord(norms.size());
    for (size_t i = 0; i < ord.size(); ++i)
      ord[i] = i;
    const size_t de = (size_t)cand.d;
    std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {
      if (norms[a] != norms[b])
        return norms[a] < norms[b];
      for (size_t k = de; k-- > 0;)
        if (x[a][k] != x[b][k])
          return x[a][k] < x[b][k];
      return a < b;
    });
    return ord;
  }
};

template <class Cand> double svp_table_cb(void *user, double dist, const double *sol)
{
  (void)dist;  // (the decision is the integers')
  SvpTable<Cand> *T = (SvpTable<Cand> *)user;
  long long nv      = 0;
  if (!svp_exact_candidate(&T->cand, sol, &nv))
  {
    T->cand.overflow = true;
    return 0.0;  // stop
  }
  T->offer(nv, sol);
  return T->bound();  // (0 once the table is full with worst = 1: nothing non-zero is shorter)
}

// d_eff == 1: the multiples of row 0, as the walk steps through them: x = 1, 2, ... while the leaf is within the
// level bound.  Returns the node count.
template <class Cand> unsigned long long svp_table_line(SvpTable<Cand> *T, double r00, double p0)
{
  double radius            = T->radius0();
  unsigned long long nodes = 1;  // (the leaf x = 0)
  for (double x = 1.0;; x += 1.0)
  {
    if (!(x * x * r00 <= p0 * radius))
      break;
    ++nodes;
    radius = svp_table_cb<Cand>(T, 0.0, &x);
    if (radius == 0.0)
      break;
  }
  return nodes;
}
}  // namespace fphip

#endif
