// cvp_ref_driver.cpp — records what fplll's own enumerator does with a target (closest-vector enumeration) into the
// fixtures tests/golden/cvp_*.json.  Test infrastructure: it uses fplll's public API only (MatGSO, Enumeration,
// FastEvaluator), build() does not compile it and no test needs the binary.
//
// Build (from the repository root, against the reference built into oracle/_ref by `make -C oracle ref`):
//   g++ -std=c++11 -O2 -w -Ioracle/_ref/include -Ioracle/_ref/include/fplll -I$REF -I$REF/fplll -I$CONDA/include \
//       tests/native/cvp_ref_driver.cpp -o oracle/_ref/cvp_ref_driver -Loracle/_ref -lfplll \
//       $CONDA/lib/libmpfr.so $CONDA/lib/libgmp.so -pthread -Wl,-rpath,'$ORIGIN'
//   (REF = fplll's source tree, CONDA = the prefix of gmp / mpfr: the variables of oracle/Makefile)
// Fixtures: tests/golden/make_cvp_fixtures.sh.
//
//   cvp_ref_driver d seed slope radius pruning target
//     d, seed, slope   a general-position block like conftest.synthetic_block's: mu uniform in [-1/2, 1/2], log r_ii
//                      falling by 2 slope per row with a seeded factor in [0.9, 1.1] — realised as a lower-triangular
//                      INTEGER basis (diagonal 2^24 sqrt(r_ii), row i column j = mu(i,j) times the diagonal of row j,
//                      rounded), because the reference enumerates on a MatGSO; the fixture holds the mu / r that GSO
//                      handed the enumerator, not the ones drawn
//     radius           gh:<f>     f times the squared Gaussian-heuristic radius of the block
//                      babai:<f>  f times the squared distance of the rounding descent from the target
//     pruning          none | stair:<low>  (multiples of 1/8 from 1 at level 0 down to `low` at level d - 1)
//     target           real            seeded coordinates in [-4, 4]
//                      lattice         the lattice point 3 b_{d-1}: t_i = fl(3 mu(d-1,i)), t_{d-1} = 3 — every centre
//                                      of the descent is an integer EXACTLY (one product, one difference)
//                      near:<eps>      that point plus seeded offsets in [-eps, eps]
//                      bump:<m>:<v>    near:1e-4 with coordinate m moved by v on top
// Output (stdout): one JSON object, doubles as C99 hex strings — mut, rdiag, target, pruning and maxdist as
// EnumerationDyn::enumerate forms them (enumerate.cpp:85-141); per-level nodes and every eval_sol call of a run whose
// radius never shrinks; the final (dist, x) of a BEST_N(1) run from the same radius.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include <fplll.h>

using namespace fplll;
typedef Z_NR<mpz_t> ZT;
typedef FP_NR<double> FT;

struct Logged
{
  double dist;
  std::vector<double> x;
};

// FastEvaluator that keeps every call: the distance is the enumerator's own (normalised) one
struct LogEvaluator : public FastEvaluator<FT>
{
  std::vector<Logged> log;
  LogEvaluator(size_t n) : FastEvaluator<FT>(n, EVALSTRATEGY_BEST_N_SOLUTIONS, false) {}
  virtual void eval_sol(const std::vector<FT> &c, const enumf &dist, enumf &max_dist)
  {
    Logged l;
    l.dist = dist;
    for (size_t i = 0; i < c.size(); ++i)
      l.x.push_back(c[i].get_d());
    log.push_back(l);
    FastEvaluator<FT>::eval_sol(c, dist, max_dist);
  }
};

static void hexlist(const char *name, const std::vector<double> &v, const char *tail)
{
  printf("\"%s\":[", name);
  for (size_t i = 0; i < v.size(); ++i)
    printf("%s\"%a\"", i ? "," : "", v[i]);
  printf("]%s\n", tail);
}

static void intlist(const std::vector<double> &v)
{
  printf("[");
  for (size_t i = 0; i < v.size(); ++i)
    printf("%s%.0f", i ? "," : "", v[i]);
  printf("]");
}

int main(int argc, char **argv)
{
  if (argc != 7)
  {
    fprintf(stderr, "usage: %s d seed slope gh:<f>|babai:<f> none|stair:<low> real|lattice|near:<eps>|bump:<m>:<v>\n", argv[0]);
    return 2;
  }
  const int d        = atoi(argv[1]);
  const int seed     = atoi(argv[2]);
  const double slope = atof(argv[3]);
  const std::string rspec = argv[4], pspec = argv[5], tspec = argv[6];
  std::mt19937_64 rng((unsigned long long)seed * 7919u + 17u);
  std::uniform_real_distribution<double> half(-0.5, 0.5), fac(0.9, 1.1), box(-4.0, 4.0), unit(-1.0, 1.0);

  // the integer basis
  ZZ_mat<mpz_t> A(d, d), U, UT;
  std::vector<double> diag(d);
  for (int i = 0; i < d; ++i)
  {
    diag[i] = std::floor(std::ldexp(std::sqrt(std::exp(-2.0 * slope * i) * fac(rng)), 24) + 0.5);
    for (int j = 0; j < i; ++j)
      A[i][j] = (long)std::floor(half(rng) * diag[j] + 0.5);
    A[i][i] = (long)diag[i];
  }
  MatGSO<ZT, FT> M(A, U, UT, 0);
  M.update_gso();

  // what EnumerationDyn::enumerate(0, d, ...) makes of it (enumerate.cpp:91-141, primal)
  FT fr, fmu;
  long rexpo, normexp = -1;
  for (int i = 0; i < d; ++i)
  {
    fr      = M.get_r_exp(i, i, rexpo);
    normexp = std::max(normexp, rexpo + fr.exponent());
  }
  std::vector<double> rdiag(d), mut((size_t)d * d, 0.0);
  for (int i = 0; i < d; ++i)
  {
    fr = M.get_r_exp(i, i, rexpo);
    fr.mul_2si(fr, rexpo - normexp);
    rdiag[i] = fr.get_d();
    for (int j = i + 1; j < d; ++j)
    {
      M.get_mu(fmu, j, i);
      mut[(size_t)i * d + j] = fmu.get_d();
    }
  }

  // the target
  std::vector<double> target(d, 0.0);
  if (tspec == "real")
    for (int i = 0; i < d; ++i)
      target[i] = box(rng);
  else
  {
    for (int i = 0; i + 1 < d; ++i)
      target[i] = 3.0 * mut[(size_t)i * d + (d - 1)];
    target[d - 1] = 3.0;
    double eps = 0.0;
    if (tspec.compare(0, 5, "near:") == 0)
      eps = atof(tspec.c_str() + 5);
    else if (tspec.compare(0, 5, "bump:") == 0)
      eps = 1e-4;
    else if (tspec != "lattice")
    {
      fprintf(stderr, "unknown target %s\n", tspec.c_str());
      return 2;
    }
    if (eps > 0.0)
      for (int i = 0; i < d; ++i)
        target[i] += eps * unit(rng);
    if (tspec.compare(0, 5, "bump:") == 0)
    {
      int m    = 0;
      double v = 0.0;
      sscanf(tspec.c_str() + 5, "%d:%lf", &m, &v);
      target[m] += v;
    }
  }

  // the radius (normalised like rdiag)
  double maxdist = 0.0;
  if (rspec.compare(0, 3, "gh:") == 0)
  {
    double slog = 0.0;
    for (int i = 0; i < d; ++i)
      slog += std::log(rdiag[i]);
    maxdist = atof(rspec.c_str() + 3) * std::exp((2.0 / d) * std::lgamma(d / 2.0 + 1.0) - std::log(M_PI) + slog / d);
  }
  else if (rspec.compare(0, 6, "babai:") == 0)
  {
    std::vector<double> x(d, 0.0);
    double dist = 0.0;
    for (int k = d - 1; k >= 0; --k)
    {
      double c = target[k];
      for (int j = k + 1; j < d; ++j)
        c -= x[j] * mut[(size_t)k * d + j];
      x[k] = std::round(c);
      dist += (x[k] - c) * (x[k] - c) * rdiag[k];
    }
    maxdist = atof(rspec.c_str() + 6) * dist;
  }
  else
  {
    fprintf(stderr, "unknown radius %s\n", rspec.c_str());
    return 2;
  }

  std::vector<double> pruning;
  if (pspec.compare(0, 6, "stair:") == 0)
  {
    const int lo8 = (int)std::floor(atof(pspec.c_str() + 6) * 8.0 + 0.5);
    for (int k = 0; k < d; ++k)
      pruning.push_back((8 - ((8 - lo8) * k) / std::max(1, d - 1)) / 8.0);
  }
  else if (pspec != "none")
  {
    fprintf(stderr, "unknown pruning %s\n", pspec.c_str());
    return 2;
  }

  std::vector<FT> tc(d);
  for (int i = 0; i < d; ++i)
    tc[i] = target[i];

  // run 1: a radius that never shrinks (BEST_N with room for everything)
  LogEvaluator ev1(1000000000);
  {
    Enumeration<ZT, FT> E(M, ev1);
    FT fmax = std::ldexp(maxdist, (int)normexp);
    E.enumerate(0, d, fmax, 0, tc, std::vector<enumxt>(), pruning);
    printf("{\"desc\":\"cvp d=%d seed=%d slope=%s radius=%s pruning=%s target=%s\",\n\"d\":%d,\n", d, seed, argv[3],
           rspec.c_str(), pspec.c_str(), tspec.c_str(), d);
    printf("\"maxdist\":\"%a\",\n", maxdist);
    hexlist("mut", mut, ",");
    hexlist("rdiag", rdiag, ",");
    hexlist("target", target, ",");
    if (pruning.empty())
      pruning.assign(d, 1.0);
    hexlist("pruning", pruning, ",");
    printf("\"nodes\":[");
    for (int k = 0; k < d; ++k)
      printf("%s%llu", k ? "," : "", (unsigned long long)E.get_nodes(k));
    printf(",0],\n\"sol_log\":[");
    for (size_t s = 0; s < ev1.log.size(); ++s)
    {
      printf("%s\n{\"dist\":\"%a\",\"x\":", s ? "," : "", ev1.log[s].dist);
      intlist(ev1.log[s].x);
      printf("}");
    }
    printf("],\n");
  }
  // run 2: BEST_N(1), the radius shrinks with every candidate
  {
    LogEvaluator ev2(1);
    Enumeration<ZT, FT> E(M, ev2);
    FT fmax = std::ldexp(maxdist, (int)normexp);
    std::vector<double> pr = pspec == "none" ? std::vector<double>() : pruning;
    E.enumerate(0, d, fmax, 0, tc, std::vector<enumxt>(), pr);
    printf("\"best_calls\":%zu,\n\"best\":", ev2.log.size());
    if (ev2.log.empty())
      printf("null\n}\n");
    else
    {
      printf("{\"dist\":\"%a\",\"x\":", ev2.log.back().dist);
      intlist(ev2.log.back().x);
      printf("}\n}\n");
    }
  }
  return 0;
}
