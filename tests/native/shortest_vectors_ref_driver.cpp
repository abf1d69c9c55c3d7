// shortest_vectors_ref_driver.cpp — records the N-best enumeration of fplll itself into the fixtures
// tests/golden/svpbest_*.json: what shortest_vectors(gso, sol_coord, sol_dist, max_sols) runs — Enumeration under a
// FastEvaluator with EVALSTRATEGY_BEST_N_SOLUTIONS — at a given radius on a given basis.  Test infrastructure: it uses
// fplll's public API only (ZZ_mat, MatGSO, FastEvaluator, Enumeration), build() does not compile it and no test needs
// the binary.
//
// Build (from the repository root, against the reference built into oracle/_ref by `make -C oracle ref`):
//   g++ -std=c++11 -O2 -w -Ioracle/_ref/include -Ioracle/_ref/include/fplll -I$REF -I$REF/fplll -I$CONDA/include \
//       tests/native/shortest_vectors_ref_driver.cpp -o oracle/_ref/shortest_vectors_ref_driver -Loracle/_ref -lfplll \
//       $CONDA/lib/libmpfr.so $CONDA/lib/libgmp.so -pthread -Wl,-rpath,'$ORIGIN'
//   (REF = fplll's source tree, CONDA = the prefix of gmp / mpfr: the variables of oracle/Makefile)
// Fixtures: tests/golden/make_svp_best_fixtures.sh.
//
//   shortest_vectors_ref_driver PATH NAME bound_sq max_sols
//     the basis of PATH (fplll's matrix text, [[a b ...] [...]], d x n with d <= n) as it stands, all rows; the
//     enumeration starts at the radius bound_sq (1 + 2^-30) (a vector of norm exactly bound_sq is inside whatever the
//     rounding of its distance) and the evaluator keeps the max_sols best.  NAME goes into the output as "source".
// Output (stdout): one JSON object — source, bound_sq, max_sols, the basis, found, and the kept coefficient vectors with
// the exact squared norms of sol_coord b, sorted by that norm (the evaluator's own order is by its floating-point
// distance; ties keep its order).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include <fplll.h>

using namespace fplll;

static void zprint(const Z_NR<mpz_t> &v)
{
  char *s = mpz_get_str(nullptr, 10, v.get_data());
  printf("%s", s);
  free(s);
}

static void zlist(const std::vector<Z_NR<mpz_t>> &v)
{
  printf("[");
  for (size_t i = 0; i < v.size(); ++i)
  {
    printf("%s", i ? "," : "");
    zprint(v[i]);
  }
  printf("]");
}

int main(int argc, char **argv)
{
  if (argc != 5)
  {
    fprintf(stderr, "usage: %s PATH NAME bound_sq max_sols\n", argv[0]);
    return 2;
  }
  ZZ_mat<mpz_t> A;
  std::ifstream in(argv[1]);
  if (!in || !(in >> A) || A.get_rows() < 1 || A.get_rows() > A.get_cols())
  {
    fprintf(stderr, "%s: no d x n matrix with d <= n\n", argv[1]);
    return 2;
  }
  const int d = A.get_rows(), n = A.get_cols();
  const long bound = atol(argv[3]);
  const int K      = atoi(argv[4]);
  if (bound < 1 || K < 1)
  {
    fprintf(stderr, "bound_sq and max_sols are positive\n");
    return 2;
  }
  ZZ_mat<mpz_t> B = A, U, UT;
  MatGSO<Z_NR<mpz_t>, FP_NR<double>> gso(B, U, UT, GSO_DEFAULT);
  gso.update_gso();
  FastEvaluator<FP_NR<double>> evaluator((size_t)K, EVALSTRATEGY_BEST_N_SOLUTIONS, false);
  Enumeration<Z_NR<mpz_t>, FP_NR<double>> enumobj(gso, evaluator);
  FP_NR<double> max_dist = (double)bound * (1.0 + 1.0 / 1073741824.0);  // 1 + 2^-30
  enumobj.enumerate(0, d, max_dist, 0);

  struct Rec
  {
    Z_NR<mpz_t> norm;
    std::vector<Z_NR<mpz_t>> x;
  };
  std::vector<Rec> recs;
  for (auto it = evaluator.begin(); it != evaluator.end(); ++it)
  {
    Rec r;
    r.x.resize(d);
    for (int i = 0; i < d; ++i)
      r.x[i].set_f(it->second[i]);
    Z_NR<mpz_t> acc, tmp;
    r.norm = 0;
    for (int j = 0; j < n; ++j)
    {
      acc = 0;
      for (int i = 0; i < d; ++i)
      {
        tmp.mul(r.x[i], A[i][j]);
        acc.add(acc, tmp);
      }
      tmp.mul(acc, acc);
      r.norm.add(r.norm, tmp);
    }
    recs.push_back(r);
  }
  std::reverse(recs.begin(), recs.end());  // (the evaluator iterates from its worst to its best)
  std::stable_sort(recs.begin(), recs.end(), [](const Rec &a, const Rec &b) { return a.norm < b.norm; });

  printf("{\"desc\":\"Enumeration under FastEvaluator(BEST_N) on a given %d x %d basis\",\n\"source\":\"%s\",\n"
         "\"bound_sq\":%ld,\n\"max_sols\":%d,\n\"d\":%d,\n\"n\":%d,\n\"basis\":[", d, n, argv[2], bound, K, d, n);
  for (int i = 0; i < d; ++i)
  {
    std::vector<Z_NR<mpz_t>> row(n);
    for (int j = 0; j < n; ++j)
      row[j] = A[i][j];
    printf("%s\n", i ? "," : "");
    zlist(row);
  }
  printf("],\n\"found\":%d,\n\"norm\":[", (int)recs.size());
  for (size_t k = 0; k < recs.size(); ++k)
  {
    printf("%s", k ? "," : "");
    zprint(recs[k].norm);
  }
  printf("],\n\"sol_coord\":[");
  for (size_t k = 0; k < recs.size(); ++k)
  {
    printf("%s\n", k ? "," : "");
    zlist(recs[k].x);
  }
  printf("]}\n");
  return 0;
}
