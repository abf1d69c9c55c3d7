// shortest_vector_ref_driver.cpp — records lll_reduction + shortest_vector of fplll itself into the fixtures
// tests/golden/svpsolve_*.json.  Test infrastructure: it uses fplll's public API only (ZZ_mat, lll_reduction,
// shortest_vector), build() does not compile it and no test needs the binary.
//
// Build (from the repository root, against the reference built into oracle/_ref by `make -C oracle ref`):
//   g++ -std=c++11 -O2 -w -Ioracle/_ref/include -Ioracle/_ref/include/fplll -I$REF -I$REF/fplll -I$CONDA/include \
//       tests/native/shortest_vector_ref_driver.cpp -o oracle/_ref/shortest_vector_ref_driver -Loracle/_ref -lfplll \
//       $CONDA/lib/libmpfr.so $CONDA/lib/libgmp.so -pthread -Wl,-rpath,'$ORIGIN'
//   (REF = fplll's source tree, CONDA = the prefix of gmp / mpfr: the variables of oracle/Makefile)
// Fixtures: tests/golden/make_svp_solver_fixtures.sh.
//
//   shortest_vector_ref_driver d seed qbits
//     a q-ary basis (ZZ_mat::gen_qary_prime(d / 2, qbits) under RandGen::init_with_seed(seed)), LLL-reduced by
//     lll_reduction(LLL_DEF_DELTA, LLL_DEF_ETA, LM_WRAPPER), then shortest_vector with SVPM_FAST and with SVPM_PROVED.
//   shortest_vector_ref_driver --file PATH
//     the basis of PATH (fplll's matrix text, [[a b ...] [...]], d x n with d <= n) as it stands — no reduction: the
//     families of tests/solver_families.py are reduced in exact arithmetic — then the same two calls.  Exit status 0
//     whether or not the two norms agree (the test compares them).
// Output (stdout): one JSON object — the reduced basis and per method the sol_coord shortest_vector returned, the
// squared norm of sol_coord b (exact), the status and the time of the call on this machine's one core (milliseconds).
// Exit status 3: the two methods' norms differ (the fixture script replaces such a seed).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  const bool from_file = argc == 3 && !strcmp(argv[1], "--file");
  if (argc != 4 && !from_file)
  {
    fprintf(stderr, "usage: %s d seed qbits | %s --file PATH\n", argv[0], argv[0]);
    return 2;
  }
  int d = 0, n = 0, seed = 0, qbits = 0, status = RED_SUCCESS;
  ZZ_mat<mpz_t> A;
  if (from_file)
  {
    std::ifstream in(argv[2]);
    if (!in || !(in >> A) || A.get_rows() < 1 || A.get_rows() > A.get_cols())
    {
      fprintf(stderr, "%s: no d x n matrix with d <= n\n", argv[2]);
      return 2;
    }
    d = A.get_rows(), n = A.get_cols();
  }
  else
  {
    d = n = atoi(argv[1]), seed = atoi(argv[2]), qbits = atoi(argv[3]);
    RandGen::init_with_seed((unsigned long)seed);
    A.resize(d, d);
    A.gen_qary_prime(d / 2, qbits);
    status = lll_reduction(A, LLL_DEF_DELTA, LLL_DEF_ETA, LM_WRAPPER, FT_DEFAULT, 0, LLL_DEFAULT);
  }
  if (status != RED_SUCCESS)
  {
    fprintf(stderr, "lll_reduction: %s\n", get_red_status_str(status));
    return 1;
  }
  if (from_file)
    printf("{\"desc\":\"shortest_vector of a given %d x %d basis\",\n\"d\":%d,\n\"n\":%d,\n\"basis\":[", d, n, d, n);
  else
    printf("{\"desc\":\"shortest_vector d=%d seed=%d qbits=%d\",\n\"d\":%d,\n\"n\":%d,\n\"basis\":[", d, seed, qbits, d, d);
  for (int i = 0; i < d; ++i)
  {
    std::vector<Z_NR<mpz_t>> row(n);
    for (int j = 0; j < n; ++j)
      row[j] = A[i][j];
    printf("%s\n", i ? "," : "");
    zlist(row);
  }
  printf("]");
  Z_NR<mpz_t> norms[2];
  const SVPMethod methods[2] = {SVPM_FAST, SVPM_PROVED};
  const char *names[2]       = {"fast", "proved"};
  for (int m = 0; m < 2; ++m)
  {
    ZZ_mat<mpz_t> B = A;  // (shortest_vector takes the basis by reference)
    std::vector<Z_NR<mpz_t>> sol;
    const auto t0 = std::chrono::steady_clock::now();
    status        = shortest_vector(B, sol, methods[m], SVP_DEFAULT);
    const double ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    Z_NR<mpz_t> acc, tmp;
    norms[m] = 0;
    for (int j = 0; j < n; ++j)
    {
      acc = 0;
      for (int i = 0; i < d && i < (int)sol.size(); ++i)
      {
        tmp.mul(sol[i], A[i][j]);
        acc.add(acc, tmp);
      }
      tmp.mul(acc, acc);
      norms[m].add(norms[m], tmp);
    }
    printf(",\n\"%s\":{\"status\":%d,\"ref_ms\":%.3f,\"norm\":", names[m], status, ms);
    zprint(norms[m]);
    printf(",\n\"sol_coord\":");
    zlist(sol);
    printf("}");
  }
  printf("}\n");
  return from_file || norms[0] == norms[1] ? 0 : 3;
}
