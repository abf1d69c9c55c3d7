// closest_vector_ref_driver.cpp — records lll_reduction + closest_vector of fplll itself into the fixtures
// tests/golden/cvpsolve_*.json.  Test infrastructure: it uses fplll's public API only (ZZ_mat, lll_reduction,
// closest_vector), build() does not compile it and no test needs the binary.
//
// Build (from the repository root, against the reference built into oracle/_ref by `make -C oracle ref`):
//   g++ -std=c++11 -O2 -w -Ioracle/_ref/include -Ioracle/_ref/include/fplll -I$REF -I$REF/fplll -I$CONDA/include \
//       tests/native/closest_vector_ref_driver.cpp -o oracle/_ref/closest_vector_ref_driver -Loracle/_ref -lfplll \
//       $CONDA/lib/libmpfr.so $CONDA/lib/libgmp.so -pthread -Wl,-rpath,'$ORIGIN'
//   (REF = fplll's source tree, CONDA = the prefix of gmp / mpfr: the variables of oracle/Makefile)
// Fixtures: tests/golden/make_cvp_solver_fixtures.sh.
//
//   closest_vector_ref_driver d seed qbits target...
//     d, seed, qbits   a q-ary basis (ZZ_mat::gen_qary_prime(d / 2, qbits) under RandGen::init_with_seed(seed)),
//                      LLL-reduced by lll_reduction(LLL_DEF_DELTA, LLL_DEF_ETA, LM_WRAPPER)
//     target           rand          seeded entries in [0, 2^qbits)
//                      near:<s>      a lattice point with seeded coefficients in [-8, 8] plus offsets in [-s, s]
//                      lattice       such a lattice point itself
//                      far:<s>       a lattice point with coefficients around 2^34 (entries around 2^40) plus offsets
//                                    in [-s, s]: the Babai loop of closest_vector runs more than once
// Output (stdout): one JSON object — the reduced basis, and per target its integers, the sol_coord closest_vector
// returned (CVPM_FAST), its status and the time of the call on this machine's one core (milliseconds).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include <fplll.h>

using namespace fplll;

static void zlist(const std::vector<Z_NR<mpz_t>> &v)
{
  printf("[");
  for (size_t i = 0; i < v.size(); ++i)
  {
    char *s = mpz_get_str(nullptr, 10, v[i].get_data());
    printf("%s%s", i ? "," : "", s);
    free(s);
  }
  printf("]");
}

int main(int argc, char **argv)
{
  if (argc < 5)
  {
    fprintf(stderr, "usage: %s d seed qbits rand|near:<s>|lattice|far:<s> ...\n", argv[0]);
    return 2;
  }
  const int d = atoi(argv[1]), seed = atoi(argv[2]), qbits = atoi(argv[3]);
  RandGen::init_with_seed((unsigned long)seed);
  ZZ_mat<mpz_t> A(d, d);
  A.gen_qary_prime(d / 2, qbits);
  int status = lll_reduction(A, LLL_DEF_DELTA, LLL_DEF_ETA, LM_WRAPPER, FT_DEFAULT, 0, LLL_DEFAULT);
  if (status != RED_SUCCESS)
  {
    fprintf(stderr, "lll_reduction: %s\n", get_red_status_str(status));
    return 1;
  }
  printf("{\"desc\":\"closest_vector d=%d seed=%d qbits=%d\",\n\"d\":%d,\n\"n\":%d,\n\"basis\":[", d, seed, qbits, d, d);
  for (int i = 0; i < d; ++i)
  {
    std::vector<Z_NR<mpz_t>> row(d);
    for (int j = 0; j < d; ++j)
      row[j] = A[i][j];
    printf("%s\n", i ? "," : "");
    zlist(row);
  }
  printf("],\n\"targets\":[");
  for (int a = 4; a < argc; ++a)
  {
    const std::string spec = argv[a];
    std::mt19937_64 rng((unsigned long long)seed * 104729u + (unsigned long long)a * 7919u + 3u);
    std::vector<Z_NR<mpz_t>> t(d);
    for (int j = 0; j < d; ++j)
      t[j] = 0;
    if (spec == "rand")
    {
      std::uniform_int_distribution<long> u(0, (1L << qbits) - 1);
      for (int j = 0; j < d; ++j)
        t[j] = u(rng);
    }
    else
    {
      const bool far = spec.compare(0, 4, "far:") == 0;
      long s         = 0;
      if (far)
        s = atol(spec.c_str() + 4);
      else if (spec.compare(0, 5, "near:") == 0)
        s = atol(spec.c_str() + 5);
      else if (spec != "lattice")
      {
        fprintf(stderr, "unknown target %s\n", spec.c_str());
        return 2;
      }
      std::uniform_int_distribution<long> c(far ? -(1L << 34) : -8, far ? (1L << 34) : 8), off(-s, s);
      Z_NR<mpz_t> ci, tmp;
      for (int i = 0; i < d; ++i)
      {
        ci = c(rng);
        for (int j = 0; j < d; ++j)
        {
          tmp.mul(ci, A[i][j]);
          t[j].add(t[j], tmp);
        }
      }
      for (int j = 0; j < d && s > 0; ++j)
      {
        tmp = off(rng);
        t[j].add(t[j], tmp);
      }
    }
    std::vector<Z_NR<mpz_t>> sol;
    const auto t0 = std::chrono::steady_clock::now();
    status        = closest_vector(A, t, sol, CVPM_FAST);
    const double ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("%s\n{\"kind\":\"%s\",\"status\":%d,\"ref_ms\":%.3f,\n\"target\":", a > 4 ? "," : "", spec.c_str(), status, ms);
    zlist(t);
    printf(",\n\"sol_coord\":");
    zlist(sol);
    printf("}");
  }
  printf("]}\n");
  return 0;
}
