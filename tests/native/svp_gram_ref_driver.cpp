// svp_gram_ref_driver.cpp — records what fplll itself answers for the shortest vectors of a quadratic form into the
// fixtures tests/golden/svpgram_*.json: LLLReduction over MatGSOGram<Z_NR<mpz_t>, FP_NR<mpfr_t>>, symmetrize_g(),
// shortest_vector(Mgram, sol_coord, SVPM_FAST) and shortest_vectors(Mgram, sol_coord, sol_dist, max_sols, SVPM_FAST,
// SVP_DEFAULT) — the sequence of the reference's own test of forms.  Test infrastructure: it uses fplll's public API
// only, build() does not compile it and no test needs the binary.
//
// Build (from the repository root, against the reference built into oracle/_ref by `make -C oracle ref`):
//   g++ -std=c++11 -O2 -w -Ioracle/_ref/include -Ioracle/_ref/include/fplll -I$REF -I$REF/fplll -I$CONDA/include \
//       tests/native/svp_gram_ref_driver.cpp -o oracle/_ref/svp_gram_ref_driver -Loracle/_ref -lfplll \
//       $CONDA/lib/libmpfr.so $CONDA/lib/libgmp.so -pthread -Wl,-rpath,'$ORIGIN'
//   (REF = fplll's source tree, CONDA = the prefix of gmp / mpfr: the variables of oracle/Makefile)
// Fixtures: tests/golden/make_svp_gram_fixtures.sh.
//
//   svp_gram_ref_driver PATH NAME max_sols
//     the form of PATH (fplll's matrix text, [[a b ...] [...]], d x d, symmetric).  NAME goes into the output as
//     "source".
// Output (stdout): one JSON object — source, max_sols, d, G_in, the reduced form G (what the solvers ran on), the
// coefficients and the exact value x G x^T of shortest_vector's answer, and found / sol_coord / norm / sol_dist of
// shortest_vectors, sorted by the exact norm (ties keep the evaluator's order, best first).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include <fplll.h>

using namespace fplll;

typedef Z_NR<mpz_t> Z;

static void zprint(const Z &v)
{
  char *s = mpz_get_str(nullptr, 10, v.get_data());
  printf("%s", s);
  free(s);
}

static void zlist(const std::vector<Z> &v)
{
  printf("[");
  for (size_t i = 0; i < v.size(); ++i)
  {
    printf("%s", i ? "," : "");
    zprint(v[i]);
  }
  printf("]");
}

static void zmat(const ZZ_mat<mpz_t> &M)
{
  printf("[");
  for (int i = 0; i < M.get_rows(); ++i)
  {
    std::vector<Z> row(M.get_cols());
    for (int j = 0; j < M.get_cols(); ++j)
      row[j] = M[i][j];
    printf("%s\n", i ? "," : "");
    zlist(row);
  }
  printf("]");
}

// x G x^T in integers
static Z form_value(const ZZ_mat<mpz_t> &G, const std::vector<Z> &x)
{
  Z acc, row, tmp;
  acc = 0;
  for (int j = 0; j < G.get_cols(); ++j)
  {
    row = 0;
    for (int i = 0; i < G.get_rows(); ++i)
    {
      tmp.mul(x[i], G[i][j]);
      row.add(row, tmp);
    }
    tmp.mul(row, x[j]);
    acc.add(acc, tmp);
  }
  return acc;
}

int main(int argc, char **argv)
{
  if (argc != 4)
  {
    fprintf(stderr, "usage: %s PATH NAME max_sols\n", argv[0]);
    return 2;
  }
  ZZ_mat<mpz_t> G;
  std::ifstream in(argv[1]);
  if (!in || !(in >> G) || G.get_rows() < 1 || G.get_rows() != G.get_cols())
  {
    fprintf(stderr, "%s: no d x d matrix\n", argv[1]);
    return 2;
  }
  const int d = G.get_rows();
  const int K = atoi(argv[3]);
  if (K < 1)
  {
    fprintf(stderr, "max_sols is positive\n");
    return 2;
  }
  const ZZ_mat<mpz_t> G_in = G;
  FP_NR<mpfr_t>::set_prec(128);
  ZZ_mat<mpz_t> empty_mat;
  MatGSOGram<Z, FP_NR<mpfr_t>> Mgram(G, empty_mat, empty_mat, GSO_INT_GRAM);
  Mgram.update_gso();
  LLLReduction<Z, FP_NR<mpfr_t>> lll(Mgram, LLL_DEF_DELTA, LLL_DEF_ETA, LLL_DEFAULT);
  if (!lll.lll())
  {
    fprintf(stderr, "lll: %s\n", get_red_status_str(lll.status));
    return 1;
  }
  Mgram.symmetrize_g();

  std::vector<Z> sv;
  int status = shortest_vector(Mgram, sv, SVPM_FAST, SVP_DEFAULT);
  if (status != RED_SUCCESS)
  {
    fprintf(stderr, "shortest_vector: %s\n", get_red_status_str(status));
    return 1;
  }
  std::vector<std::vector<Z>> sols;
  std::vector<enumf> dist;
  status = shortest_vectors(Mgram, sols, dist, K, SVPM_FAST, SVP_DEFAULT);
  if (status != RED_SUCCESS)
  {
    fprintf(stderr, "shortest_vectors: %s\n", get_red_status_str(status));
    return 1;
  }
  struct Rec
  {
    Z norm;
    std::vector<Z> x;
    double dist;
  };
  std::vector<Rec> recs;
  for (size_t k = 0; k < sols.size(); ++k)
  {
    std::vector<Z> x = sols[k];
    x.resize(d);  // (the rows above last_useful_index are not in the answer)
    recs.push_back(Rec{form_value(G, x), x, (double)dist[k]});
  }
  std::stable_sort(recs.begin(), recs.end(), [](const Rec &a, const Rec &b) { return a.norm < b.norm; });
  sv.resize(d);

  printf("{\"desc\":\"LLL over MatGSOGram, symmetrize_g, shortest_vector and shortest_vectors(max_sols) of a %d x %d "
         "form, SVPM_FAST\",\n\"source\":\"%s\",\n\"max_sols\":%d,\n\"d\":%d,\n\"G_in\":", d, d, argv[2], K, d);
  zmat(G_in);
  printf(",\n\"G\":");
  zmat(G);
  printf(",\n\"sv_coord\":");
  zlist(sv);
  printf(",\n\"sv_norm\":");
  zprint(form_value(G, sv));
  printf(",\n\"found\":%d,\n\"norm\":[", (int)recs.size());
  for (size_t k = 0; k < recs.size(); ++k)
  {
    printf("%s", k ? "," : "");
    zprint(recs[k].norm);
  }
  printf("],\n\"sol_dist\":[");
  for (size_t k = 0; k < recs.size(); ++k)
    printf("%s%.17g", k ? "," : "", recs[k].dist);
  printf("],\n\"sol_coord\":[");
  for (size_t k = 0; k < recs.size(); ++k)
  {
    printf("%s\n", k ? "," : "");
    zlist(recs[k].x);
  }
  printf("]}\n");
  return 0;
}
