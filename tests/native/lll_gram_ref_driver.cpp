// lll_gram_ref_driver.cpp — records LLLReduction<Z_NR<long>, FP_NR<double>> over MatGSOGram<Z_NR<long>, FP_NR<double>>
// (g, u, u_inv_t, GSO_INT_GRAM) of fplll itself into the fixtures tests/golden/lllgram_*.json.  Test infrastructure:
// it uses fplll's public API only (ZZ_mat, MatGSOGram, LLLReduction), build() does not compile it and no test needs
// the binary.
//
// Build (from the repository root, against the reference built into oracle/_ref by `make -C oracle ref`):
//   g++ -std=c++11 -O2 -w -Ioracle/_ref/include -Ioracle/_ref/include/fplll -I$REF -I$REF/fplll -I$CONDA/include \
//       tests/native/lll_gram_ref_driver.cpp -o oracle/_ref/lll_gram_ref_driver -Loracle/_ref -lfplll \
//       $CONDA/lib/libmpfr.so $CONDA/lib/libgmp.so -pthread -Wl,-rpath,'$ORIGIN'
//   (REF = fplll's source tree, CONDA = the prefix of gmp / mpfr: the variables of oracle/Makefile)
// Fixtures: tests/golden/make_lll_gram_fixtures.sh.
//
//   lll_gram_ref_driver name delta eta flags intrel d bits seed [reps]
//                                            the form of ZZ_mat::gen_intrel(bits) on d x (d + 1) under
//                                            RandGen::init_with_seed(seed)
//   lll_gram_ref_driver name delta eta flags A    a basis in fplll's matrix format on stdin; the form is A A^T
//   lll_gram_ref_driver name delta eta flags G    the form itself on stdin (no basis behind it)
// reps (intrel only): the reduction is repeated on fresh copies and the fastest run is reported as ref_ms.
// Output (stdout): one JSON object — G_in, A where there is one, the parameters, and of the run G_out (after
// lll()'s symmetrize_g), u, status, final_kappa, n_swaps, zeros, then mu (j < i) and r (j <= i) of an update_gso()
// of the result as hexadecimal doubles, row by row (the gso_rows rows whose update_gso_row succeeded), and the time of lll() on this machine's one core.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include <fplll.h>

using namespace fplll;

static void print_zmat(const char *key, const ZZ_mat<long> &M)
{
  printf("\"%s\":[", key);
  for (int i = 0; i < M.get_rows(); ++i)
  {
    printf("%s\n[", i ? "," : "");
    for (int j = 0; j < M.get_cols(); ++j)
      printf("%s%ld", j ? "," : "", M[i][j].get_si());
    printf("]");
  }
  printf("]");
}

int main(int argc, char **argv)
{
  if (argc < 6)
  {
    fprintf(stderr, "usage: %s name delta eta flags (intrel d bits seed [reps] | A | G)\n", argv[0]);
    return 2;
  }
  const std::string name = argv[1];
  const double delta = atof(argv[2]), eta = atof(argv[3]);
  const int flags = atoi(argv[4]);
  const std::string kind = argv[5];
  ZZ_mat<mpz_t> A;
  ZZ_mat<mpz_t> Gz;
  bool have_a = true;
  int reps    = 1;
  if (kind == "intrel")
  {
    if (argc < 9)
      return 2;
    const int d = atoi(argv[6]), bits = atoi(argv[7]);
    RandGen::init_with_seed((unsigned long)atol(argv[8]));
    if (argc > 9)
      reps = atoi(argv[9]);
    A.resize(d, d + 1);
    A.gen_intrel(bits);
  }
  else if (kind == "A")
    std::cin >> A;
  else if (kind == "G")
  {
    std::cin >> Gz;
    have_a = false;
  }
  else
    return 2;
  if (have_a)
  {
    const int r = A.get_rows(), c = A.get_cols();
    Gz.resize(r, r);
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < r; ++j)
        A[i].dot_product(Gz(i, j), A[j], c);
  }
  const int d = Gz.get_rows();
  if (d <= 0 || Gz.get_cols() != d)
  {
    fprintf(stderr, "no square form\n");
    return 1;
  }
  ZZ_mat<long> Gin(d, d);
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j)
    {
      if (!mpz_fits_slong_p(Gz[i][j].get_data()))
      {
        fprintf(stderr, "entry (%d, %d) does not fit a long\n", i, j);
        return 1;
      }
      Gin[i][j] = mpz_get_si(Gz[i][j].get_data());
    }

  ZZ_mat<long> G, U, UT;
  int status = 0, final_kappa = 0, n_swaps = 0, zeros = 0;
  double best_ms = -1.0;
  for (int rep = 0; rep < reps; ++rep)
  {
    G = Gin;
    U.gen_identity(d);
    UT.resize(0, 0);
    MatGSOGram<Z_NR<long>, FP_NR<double>> M(G, U, UT, GSO_INT_GRAM);
    LLLReduction<Z_NR<long>, FP_NR<double>> L(M, delta, eta, flags);
    const auto t0 = std::chrono::steady_clock::now();
    L.lll();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (best_ms < 0 || ms < best_ms)
      best_ms = ms;
    status      = L.status;
    final_kappa = L.final_kappa;
    n_swaps     = L.n_swaps;
    zeros       = L.zeros;
  }
  // mu and r of a fresh update_gso() of the result (a new object: nothing of the run's caches)
  ZZ_mat<long> G2 = G, U2, UT2;
  MatGSOGram<Z_NR<long>, FP_NR<double>> M2(G2, U2, UT2, GSO_INT_GRAM);
  int gso_rows = 0;  // rows whose update_gso_row() succeeded (update_gso() stops at the first that fails)
  while (gso_rows < d && M2.update_gso_row(gso_rows))
    ++gso_rows;
  const Matrix<FP_NR<double>> &mu = M2.get_mu_matrix();
  const Matrix<FP_NR<double>> &r  = M2.get_r_matrix();

  printf("{\"name\":\"%s\",\n\"d\":%d,\n\"delta\":\"%a\",\n\"eta\":\"%a\",\n\"flags\":%d,\n", name.c_str(), d, delta, eta, flags);
  print_zmat("G_in", Gin);
  printf(",\n");
  if (have_a)
  {
    const int c = A.get_cols();
    ZZ_mat<long> Al(d, c);
    for (int i = 0; i < d; ++i)
      for (int j = 0; j < c; ++j)
        Al[i][j] = mpz_get_si(A[i][j].get_data());
    print_zmat("A", Al);
    printf(",\n");
  }
  printf("\"status\":%d,\n\"final_kappa\":%d,\n\"n_swaps\":%d,\n\"zeros\":%d,\n\"gso_rows\":%d,\n\"ref_ms\":%.3f,\n", status,
         final_kappa, n_swaps, zeros, gso_rows, best_ms);
  print_zmat("G_out", G);
  printf(",\n");
  print_zmat("u", U);
  printf(",\n\"mu\":[");
  for (int i = 0; i < gso_rows; ++i)
  {
    printf("%s\n[", i ? "," : "");
    for (int j = 0; j < i; ++j)
      printf("%s\"%a\"", j ? "," : "", mu[i][j].get_d());
    printf("]");
  }
  printf("],\n\"r\":[");
  for (int i = 0; i < gso_rows; ++i)
  {
    printf("%s\n[", i ? "," : "");
    for (int j = 0; j <= i; ++j)
      printf("%s\"%a\"", j ? "," : "", r[i][j].get_d());
    printf("]");
  }
  printf("]}\n");
  return 0;
}
