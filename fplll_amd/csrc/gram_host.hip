// gram_host.hip — C ABI (include/fplll_hip.h, fphip_gram_*) for batches of integer quadratic forms on the device:
// MatGSOGram<Z_NR<long>, FP_NR<double>>(g, u, u_inv_t, GSO_INT_GRAM) with update_gso(),
// LLLReduction<Z_NR<long>, FP_NR<double>>::lll() and shortest_vectors(MatGSOGram, ...).  The kernels are in
// lll_gram.hip and svp_gram.hip.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "../../include/fplll_hip.h"
#include "dev_mem.h"
#include "host_common.h"
#include "kernels.h"
#include "svp_host.h"
#include "trace.h"

using namespace fphip;

struct fphip_gram
{
  fphip_ctx *ctx;
  GramBatch P;
  hipEvent_t ev[2];
  float last_ms;
  int waves_per_block;
};

#define QCHK(call) CHK(h->ctx, call)

static const size_t kPad = 4096;  // the LDS-DMA ring reads whole 16-byte lanes past the end of a row

static int gram_allocate(fphip_gram *h)
{
  const size_t B = (size_t)h->P.batch, d = (size_t)h->P.d;
  h->P.ldd       = (int)std::min<size_t>((d + 15) / 16 * 16, 256);
  const size_t ldd = (size_t)h->P.ldd;
  hipStream_t s    = fphip_ctx_stream(h->ctx);
  QCHK(fphip_dev_alloc((void **)&h->P.g, B * d * ldd * 8 + kPad, s));
  QCHK(fphip_dev_alloc((void **)&h->P.g2, B * d * ldd * 8 + kPad, s));
  QCHK(fphip_dev_alloc((void **)&h->P.gf, B * d * ldd * 8 + kPad, s));
  QCHK(fphip_dev_alloc((void **)&h->P.mu, B * d * ldd * 8 + kPad, s));
  QCHK(fphip_dev_alloc((void **)&h->P.muT, B * d * ldd * 8 + kPad, s));
  QCHK(fphip_dev_alloc((void **)&h->P.r, B * d * ldd * 8 + kPad, s));
  QCHK(fphip_dev_alloc((void **)&h->P.rdg, B * d * 8, s));
  QCHK(fphip_dev_alloc((void **)&h->P.vc, B * d * sizeof(int), s));
  QCHK(fphip_dev_alloc((void **)&h->P.status, B * sizeof(int), s));
  QCHK(fphip_dev_alloc((void **)&h->P.info, B * 4 * sizeof(int), s));
  QCHK(hipMemsetAsync(h->P.g, 0, B * d * ldd * 8 + kPad, s));
  QCHK(hipMemsetAsync(h->P.g2, 0, B * d * ldd * 8 + kPad, s));
  QCHK(hipMemsetAsync(h->P.gf, 0, B * d * ldd * 8 + kPad, s));
  QCHK(hipMemsetAsync(h->P.mu, 0, B * d * ldd * 8 + kPad, s));
  QCHK(hipMemsetAsync(h->P.muT, 0, B * d * ldd * 8 + kPad, s));
  QCHK(hipMemsetAsync(h->P.r, 0, B * d * ldd * 8 + kPad, s));
  QCHK(hipMemsetAsync(h->P.rdg, 0, B * d * 8, s));
  QCHK(hipMemsetAsync(h->P.status, 0, B * sizeof(int), s));
  QCHK(hipMemsetAsync(h->P.info, 0, B * 4 * sizeof(int), s));
  QCHK(hipStreamSynchronize(s));
  QCHK(hipEventCreate(&h->ev[0]));
  QCHK(hipEventCreate(&h->ev[1]));
  h->waves_per_block = 4;
  return FPHIP_OK;
}

extern "C" int fphip_gram_create(fphip_ctx *ctx, int batch, int d, fphip_gram **out)
{
  if (!ctx || !out)
    return FPHIP_ERROR;
  *out = nullptr;
  if (batch <= 0 || d <= 0)
  {
    snprintf(fphip_ctx_errbuf(ctx), 512, "fphip_gram_create: bad shape");
    return FPHIP_ERROR;
  }
  if (d > 256)
    return FPHIP_UNSUPPORTED;  // the caller keeps the form on fplll's MatGSOGram
  if (!fphip_ctx_stream(ctx))
  {
    snprintf(fphip_ctx_errbuf(ctx), 512, "fphip_gram_create: context has no device");
    return FPHIP_ERROR;
  }
  fphip_gram *h = new fphip_gram();
  h->ctx        = ctx;
  h->P.batch    = batch;
  h->P.d        = d;
  const int rc  = gram_allocate(h);
  if (rc != FPHIP_OK)
  {
    fphip_gram_destroy(h);
    return rc;
  }
  *out = h;
  return FPHIP_OK;
}

extern "C" void fphip_gram_destroy(fphip_gram *h)
{
  if (!h)
    return;
  hipStream_t s = fphip_ctx_stream(h->ctx);
  hipStreamSynchronize(s);
  void *blocks[] = {h->P.g, h->P.g2, h->P.gf, h->P.mu, h->P.muT, h->P.r, h->P.rdg, h->P.vc, h->P.status, h->P.info,
                    h->P.u, h->P.u2};
  for (void *p : blocks)
    if (p)
      fphip_dev_free(p, s);
  if (h->ev[0])
    hipEventDestroy(h->ev[0]);
  if (h->ev[1])
    hipEventDestroy(h->ev[1]);
  delete h;
}

// a form is symmetric: MatGSOGram reads the lower triangle only (sym_g, gso_interface.h:664-672) and lll() ends with
// symmetrize_g(); the device keeps both triangles and has to be given both
static int check_symmetric(fphip_gram *h, const int64_t *g, int count, const char *what)
{
  const size_t d = (size_t)h->P.d;
  for (int L = 0; L < count; ++L)
    for (size_t i = 0; i < d; ++i)
      for (size_t j = 0; j < i; ++j)
        if (g[((size_t)L * d + i) * d + j] != g[((size_t)L * d + j) * d + i])
        {
          snprintf(fphip_ctx_errbuf(h->ctx), 512, "%s: form %d is not symmetric (g(%zu, %zu) != g(%zu, %zu))", what, L, i,
                   j, j, i);
          return FPHIP_ERROR;
        }
  return FPHIP_OK;
}

extern "C" int fphip_gram_set(fphip_gram *h, const int64_t *g)
{
  if (!h || !g)
    return FPHIP_ERROR;
  if (int rc = check_symmetric(h, g, h->P.batch, "fphip_gram_set"))
    return rc;
  const size_t d = (size_t)h->P.d, ldd = (size_t)h->P.ldd;
  QCHK(hipMemcpy2D(h->P.g, ldd * 8, g, d * 8, d * 8, d * (size_t)h->P.batch, hipMemcpyHostToDevice));
  // (the kernels run on a non-blocking stream: the upload has to be complete on the device when this returns)
  QCHK(hipStreamSynchronize(nullptr));
  return FPHIP_OK;
}

// one form [d][d] into every entry of the batch (benchmarks)
extern "C" int fphip_gram_broadcast(fphip_gram *h, const int64_t *g)
{
  if (!h || !g)
    return FPHIP_ERROR;
  if (int rc = check_symmetric(h, g, 1, "fphip_gram_broadcast"))
    return rc;
  const size_t d = (size_t)h->P.d, ldd = (size_t)h->P.ldd, per = d * ldd;
  QCHK(hipMemcpy2D(h->P.g, ldd * 8, g, d * 8, d * 8, d, hipMemcpyHostToDevice));
  QCHK(hipStreamSynchronize(nullptr));
  hipStream_t s = fphip_ctx_stream(h->ctx);
  size_t have   = 1;
  while (have < (size_t)h->P.batch)
  {
    const size_t m = std::min(have, (size_t)h->P.batch - have);
    QCHK(hipMemcpyAsync(h->P.g + have * per, h->P.g, m * per * 8, hipMemcpyDeviceToDevice, s));
    have += m;
  }
  QCHK(hipStreamSynchronize(s));
  return FPHIP_OK;
}

static int get_plane(fphip_gram *h, const void *src, void *dst)
{
  const size_t d = (size_t)h->P.d, ldd = (size_t)h->P.ldd;
  QCHK(hipMemcpy2D(dst, d * 8, src, ldd * 8, d * 8, d * (size_t)h->P.batch, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

extern "C" int fphip_gram_get(fphip_gram *h, int64_t *g_out)
{
  if (!h || !g_out)
    return FPHIP_ERROR;
  return get_plane(h, h->P.g, g_out);
}
extern "C" int fphip_gram_get_mu(fphip_gram *h, double *mu)
{
  if (!h || !mu)
    return FPHIP_ERROR;
  return get_plane(h, h->P.mu, mu);
}
extern "C" int fphip_gram_get_r(fphip_gram *h, double *r)
{
  if (!h || !r)
    return FPHIP_ERROR;
  return get_plane(h, h->P.r, r);
}

static int set_identity_u(fphip_gram *h)
{
  const size_t B = (size_t)h->P.batch, d = (size_t)h->P.d, ldd = (size_t)h->P.ldd;
  std::vector<long long> id(d * ldd, 0);
  for (size_t i = 0; i < d; ++i)
    id[i * ldd + i] = 1;
  QCHK(hipMemcpy(h->P.u, id.data(), d * ldd * 8, hipMemcpyHostToDevice));
  QCHK(hipStreamSynchronize(nullptr));
  hipStream_t s = fphip_ctx_stream(h->ctx);
  for (size_t have = 1; have < B;)
  {  // the first form's identity doubled across the batch, on the device
    const size_t m = std::min(have, B - have);
    QCHK(hipMemcpyAsync(h->P.u + have * d * ldd, h->P.u, m * d * ldd * 8, hipMemcpyDeviceToDevice, s));
    have += m;
  }
  QCHK(hipStreamSynchronize(s));
  return FPHIP_OK;
}

// MatGSOGram(g, u, ...) with a non-empty u: enable_transform, u starts as the identity (and again with every call)
extern "C" int fphip_gram_enable_transform(fphip_gram *h)
{
  if (!h)
    return FPHIP_ERROR;
  const size_t B = (size_t)h->P.batch, d = (size_t)h->P.d, ldd = (size_t)h->P.ldd;
  hipStream_t s  = fphip_ctx_stream(h->ctx);
  if (!h->P.u)
  {
    QCHK(fphip_dev_alloc((void **)&h->P.u, B * d * ldd * 8 + kPad, s));
    QCHK(fphip_dev_alloc((void **)&h->P.u2, B * d * ldd * 8 + kPad, s));
    QCHK(hipMemsetAsync(h->P.u, 0, B * d * ldd * 8 + kPad, s));
    QCHK(hipMemsetAsync(h->P.u2, 0, B * d * ldd * 8 + kPad, s));
    QCHK(hipStreamSynchronize(s));
  }
  return set_identity_u(h);
}

extern "C" int fphip_gram_get_transform(fphip_gram *h, int64_t *u)
{
  if (!h || !u)
    return FPHIP_ERROR;
  if (!h->P.u)
  {
    snprintf(fphip_ctx_errbuf(h->ctx), 512, "fphip_gram_get_transform: no transformation is tracked (fphip_gram_enable_transform)");
    return FPHIP_ERROR;
  }
  return get_plane(h, h->P.u, u);
}

// which: 0 = gram_update_kernel, 1 = lll_gram_kernel
static int gram_launch(fphip_gram *h, int which, double delta, double eta, double logdelta, int siegel)
{
  const int nq   = (h->P.d + 63) / 64;
  const int wpb  = h->waves_per_block;
  int grid       = (h->P.batch + wpb - 1) / wpb;
  const size_t lds = (size_t)wpb * fphip_reduce_ring_bytes(nq);
  int bpc          = (int)((160 * 1024) / lds);
  if (bpc * wpb > 32)
    bpc = 32 / wpb;
  const int cap = fphip_ctx_num_cus(h->ctx) * (bpc > 0 ? bpc : 1);
  if (grid > cap)
    grid = cap;
  hipStream_t s = fphip_ctx_stream(h->ctx);
  QCHK(hipEventRecord(h->ev[0], s));
  dispatch_nq(nq, [&](auto NQ) {
    if (which == 1)
      hipLaunchKernelGGL(lll_gram_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, h->P, delta, eta, logdelta, siegel);
    else
      hipLaunchKernelGGL(gram_update_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, h->P);
  });
  QCHK(hipGetLastError());
  QCHK(hipEventRecord(h->ev[1], s));
  QCHK(hipStreamSynchronize(s));
  QCHK(hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]));
  return FPHIP_OK;
}

// MatGSOInterface::update_gso() of every form; mu (j < i) and r (j <= i) are readable afterwards, every other entry 0.
// status (nullable) [batch]: 1, or 0 where a mu is not finite (update_gso_row returns false)
extern "C" int fphip_gram_update(fphip_gram *h, int *status)
{
  FPHIP_RANGE("fphip_gram_update");
  if (!h)
    return FPHIP_ERROR;
  const size_t B = (size_t)h->P.batch, d = (size_t)h->P.d, ldd = (size_t)h->P.ldd;
  hipStream_t s  = fphip_ctx_stream(h->ctx);
  QCHK(hipMemsetAsync(h->P.mu, 0, B * d * ldd * 8, s));
  QCHK(hipMemsetAsync(h->P.r, 0, B * d * ldd * 8, s));
  const int rc = gram_launch(h, 0, 0.0, 0.0, 0.0, 0);
  if (rc != FPHIP_OK)
    return rc;
  if (status)
    QCHK(hipMemcpy(status, h->P.status, sizeof(int) * B, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

// LLLReduction<Z_NR<long>, FP_NR<double>>(m, delta, eta, flags).lll() on a fresh MatGSOGram of every form, then
// update_gso() of the results.  flags: fplll's LLLFlags — LLL_VERBOSE (1) is ignored, LLL_EARLY_RED (2) is accepted
// and ignored as the reference does with enable_int_gram (lll.cpp:31-35), LLL_SIEGEL (4) runs on the device.
extern "C" int fphip_gram_lll(fphip_gram *h, double delta, double eta, int flags, int *status, int *info)
{
  FPHIP_RANGE("fphip_gram_lll");
  if (!h)
    return FPHIP_ERROR;
  if (flags & ~7)
  {
    snprintf(fphip_ctx_errbuf(h->ctx), 512, "fphip_gram_lll: unknown flags 0x%x", flags);
    return FPHIP_ERROR;
  }
  const int siegel = (flags & 4) ? 1 : 0;
  const size_t B   = (size_t)h->P.batch;
  if (h->P.u)
    if (int rcu = set_identity_u(h))
      return rcu;
  // (swap_threshold = siegel ? delta - eta * eta : delta, lll.cpp:40; the iteration limit keeps log(delta))
  int rc = gram_launch(h, 1, siegel ? delta - eta * eta : delta, eta, std::log(delta), siegel);
  if (rc != FPHIP_OK)
    return rc;
  const float lll_ms = h->last_ms;
  std::swap(h->P.g, h->P.g2);  // the kernel wrote the form in position order into g2
  if (h->P.u)
    std::swap(h->P.u, h->P.u2);
  std::vector<int> st(B);
  QCHK(hipMemcpy(st.data(), h->P.status, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (info)
    QCHK(hipMemcpy(info, h->P.info, sizeof(int) * 4 * B, hipMemcpyDeviceToHost));
  rc         = fphip_gram_update(h, nullptr);
  h->last_ms = lll_ms;
  if (status)
    memcpy(status, st.data(), sizeof(int) * B);
  return rc;
}

extern "C" double fphip_gram_last_kernel_ms(const fphip_gram *h) { return h ? (double)h->last_ms : 0.0; }

// ---- the N shortest vectors of a form (svp_gram.hip; the ENUM route: fphip_enum_run under the host table) -----------
namespace
{
typedef __int128 i128;
// the ENUM route's exact candidate: x G x^T by the steps of svp_gram.hip
struct GramCand
{
  int d;               // rows under enumeration (d_eff)
  int ld;              // the host copy's row stride (the form's d)
  const long long *g;  // [d][ld] host copy of the form
  bool overflow;
};
// false: the norm is beyond 63 bits (or a coefficient is 2^57 and more); *norm = 0 for a negative value (an
// indefinite form the doubles did not catch): the table does not accept it
bool svp_exact_candidate(GramCand *C, const double *sol, long long *norm)
{
  const int d = C->d;
  for (int i = 0; i < d; ++i)
    if (!(std::fabs(sol[i]) < 144115188075855872.0))  // 2^57: below it no step leaves the 128 bits
      return false;
  i128 H = 0, L = 0;
  for (int j = 0; j < d; ++j)
  {
    const long long xj = (long long)sol[j];
    if (xj == 0)
      continue;
    i128 y = 0;
    for (int i = 0; i < d; ++i)
      y += (i128)(long long)sol[i] * (i128)C->g[(size_t)i * C->ld + j];
    const long long yh          = (long long)(y >> 64);
    const unsigned long long yl = (unsigned long long)y;
    H += (i128)xj * (i128)yh;
    L += (i128)xj * (i128)(unsigned __int128)yl;
  }
  const i128 T = H + (L >> 64);  // x G x^T = T 2^64 + (the low word of L)
  const long long lo = (long long)(unsigned long long)L;
  if (T < 0)
  {
    *norm = 0;
    return true;
  }
  if (T != 0 || lo < 0)
    return false;
  *norm = lo;
  return true;
}
}  // namespace

// the wave-per-form kernel over the range; outputs of the forms with take_h[w] == 0 are left alone
static int svp_gram_wave_run(fphip_gram *h, int first, int count, int K, const int64_t *bound_sq, const double *pruning,
                             const int *take_h, int *found, int64_t *sol_coord, int64_t *norm, uint64_t *nodes,
                             int *status)
{
  const size_t d = h->P.d, kk = (size_t)K;
  int wpb        = 4;
  SvpGramWave A;
  memset(&A, 0, sizeof A);
  A.first = first, A.count = count, A.max_sols = K;
  A.stack_doubles = (int)(d * (d + 1) / 2 + 2);
  A.mu_doubles    = (int)std::max<size_t>(d * (d - 1) / 2, 2);
  const size_t per_wave = (size_t)(A.stack_doubles + A.mu_doubles) * sizeof(double);
  const size_t lds      = per_wave * wpb;  // d <= 64: at most 131136 bytes
  int bpc = (int)((160 * 1024) / lds);
  if (bpc * wpb > 32)
    bpc = 32 / wpb;
  int grid = (count + wpb - 1) / wpb;
  int cap  = fphip_ctx_num_cus(h->ctx) * std::max(bpc, 1);
  if (const char *e = getenv("FPHIP_SVP_WAVE_GRID"))  // (tests: a small grid makes a small batch go round the grid-stride loop)
    cap = std::max(1, atoi(e));
  grid = std::min(grid, cap);
  hipStream_t s = fphip_ctx_stream(h->ctx);
  CvpBufs B(s);
  double *pr_d = nullptr;
  int *take_d  = nullptr;
  long long *bound_d = nullptr;
  QCHK(B.get(&A.rec, (size_t)count * kk * d));
  QCHK(B.get(&A.sol_coord, (size_t)count * kk * d));
  QCHK(B.get(&A.norm, (size_t)count * kk));
  QCHK(B.get(&A.found, (size_t)count));
  QCHK(B.get(&A.nodes, (size_t)count));
  QCHK(B.get(&A.status, (size_t)count));
  if (pruning)
  {
    QCHK(B.get(&pr_d, d));
    QCHK(hipMemcpy(pr_d, pruning, d * sizeof(double), hipMemcpyHostToDevice));
  }
  if (take_h)
  {
    QCHK(B.get(&take_d, (size_t)count));
    QCHK(hipMemcpy(take_d, take_h, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
  }
  if (bound_sq)
  {
    QCHK(B.get(&bound_d, (size_t)count));
    QCHK(hipMemcpy(bound_d, bound_sq, (size_t)count * sizeof(long long), hipMemcpyHostToDevice));
  }
  QCHK(hipStreamSynchronize(nullptr));  // (see fphip_gram_set)
  A.pruning = pr_d;
  A.take    = take_d;
  A.bound   = bound_d;
  if (lds > 64 * 1024)
    QCHK(allow_lds(svp_gram_kernel, lds));
  QCHK(hipEventRecord(h->ev[0], s));
  hipLaunchKernelGGL(svp_gram_kernel, dim3(grid), dim3(wpb * 64), lds, s, h->P, A);
  QCHK(hipGetLastError());
  QCHK(hipEventRecord(h->ev[1], s));
  QCHK(hipStreamSynchronize(s));
  QCHK(hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]));
  if (!take_h)
  {  // the whole range: straight into the caller's arrays
    QCHK(hipMemcpy(sol_coord, A.sol_coord, (size_t)count * kk * d * sizeof(long long), hipMemcpyDeviceToHost));
    QCHK(hipMemcpy(norm, A.norm, (size_t)count * kk * sizeof(long long), hipMemcpyDeviceToHost));
    QCHK(hipMemcpy(found, A.found, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    QCHK(hipMemcpy(nodes, A.nodes, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    QCHK(hipMemcpy(status, A.status, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    return FPHIP_OK;
  }
  for (int w = 0; w < count; ++w)
  {
    if (!take_h[w])
      continue;
    QCHK(hipMemcpy(sol_coord + (size_t)w * kk * d, A.sol_coord + (size_t)w * kk * d, kk * d * sizeof(long long), hipMemcpyDeviceToHost));
    QCHK(hipMemcpy(norm + (size_t)w * kk, A.norm + (size_t)w * kk, kk * sizeof(long long), hipMemcpyDeviceToHost));
    QCHK(hipMemcpy(found + w, A.found + w, sizeof(int), hipMemcpyDeviceToHost));
    QCHK(hipMemcpy(nodes + w, A.nodes + w, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    QCHK(hipMemcpy(status + w, A.status + w, sizeof(int), hipMemcpyDeviceToHost));
  }
  return FPHIP_OK;
}

// one form by the enumerator under the host table: gh [d][d], mu [d][d], rd [d] host copies; outputs [K][d], [K]
static int svp_gram_enum_one(fphip_gram *h, fphip_ctx *ectx, int form, int K, long long bound, const double *pruning,
                             const long long *gh, const double *mu, const double *rd, int *found, int64_t *sol,
                             int64_t *norm, uint64_t *nodes, int *status)
{
  const int d = h->P.d;
  const size_t dd = (size_t)d, kk = (size_t)K;
  memset(sol, 0, kk * dd * sizeof(int64_t));
  memset(norm, 0, kk * sizeof(int64_t));
  *found = 0, *nodes = 0, *status = 1;
  for (size_t i = 0; i < dd; ++i)
    if (gh[i * dd + i] <= 0)
    {
      *status = 0;
      return FPHIP_OK;
    }
  long long B0 = bound;
  int d_eff;
  if (bound > 0)
    d_eff = svp_best_rows(d, rd, true, (double)bound * (1.0 + 0x1p-30));
  else
  {
    d_eff = svp_best_rows(d, rd, false, 0.0);
    B0    = gh[0];
    for (int i = 1; i < d_eff; ++i)
      B0 = std::min(B0, gh[(size_t)i * dd + i]);
  }
  for (int i = 0; i < d_eff; ++i)
    if (!(rd[i] > 0.0 && std::isfinite(rd[i])))
    {
      *status = 0;  // not positive definite on the rows walked, as far as the doubles see
      return FPHIP_OK;
    }
  SvpTable<GramCand> T{GramCand{d_eff, d, gh, false}, K, B0, {}, {}};
  if (T.radius0() > 0.0)
  {
    if (d_eff == 1)
      *nodes = svp_table_line(&T, rd[0], pruning ? pruning[0] : 1.0);  // the multiples of the first variable
    else
    {
      const size_t de = (size_t)d_eff;
      std::vector<double> mut(de * de, 0.0);
      for (size_t i = 0; i < de; ++i)
        for (size_t j = i + 1; j < de; ++j)
          mut[i * de + j] = mu[j * dd + i];  // the layout a plugin receives: mut[i][j] = mu(j,i), j > i
      fphip_enum_opts o;
      memset(&o, 0, sizeof o);
      o.shard_count       = 1;
      o.exchange_chunks   = 1;
      o.min_nodes_decline = 0;  // never declined for being small
      std::vector<uint64_t> nd(FPHIP_ENUM_MAX_DIM + 1, 0);
      const int rc = fphip_enum_run(ectx, d_eff, T.radius0(), mut.data(), rd, pruning, &o, svp_table_cb<GramCand>, nullptr,
                                    &T, nd.data(), nullptr);
      if (rc != FPHIP_OK)
      {
        if (ectx != h->ctx)
          snprintf(fphip_ctx_errbuf(h->ctx), 512, "fphip_gram_shortest_vectors: enumeration of form %d: %s", form,
                   fphip_last_error(ectx));
        return rc;
      }
      for (int k = 0; k <= d_eff; ++k)
        *nodes += nd[k];
    }
  }
  if (T.cand.overflow)
  {
    *status = -2;
    *nodes  = 0;
    return FPHIP_OK;
  }
  // ties in the coefficient order of fphip_list_vectors (from level d - 1 down): the arrival order is the parallel walk's
  const std::vector<size_t> ord = T.order();
  for (size_t o = 0; o < ord.size(); ++o)
  {
    const std::vector<long long> &xi = T.x[ord[o]];
    for (int i = 0; i < d_eff; ++i)
      sol[o * dd + i] = xi[i];
    norm[o] = T.norms[ord[o]];
  }
  *found = (int)ord.size();
  return FPHIP_OK;
}

extern "C" int fphip_gram_shortest_vectors(fphip_gram *h, fphip_ctx *ectx, int first_form, int count, int max_sols,
                                           const int64_t *bound_sq, int method, int flags, const double *pruning,
                                           int route, int *found, int64_t *sol_coord, int64_t *norm, uint64_t *nodes,
                                           int *status)
{
  FPHIP_RANGE("fphip_gram_shortest_vectors");
  if (!h)
    return FPHIP_ERROR;
  if (!found || !sol_coord || !norm || !nodes || !status)
    return fail_msg(h->ctx, "fphip_gram_shortest_vectors: found, sol_coord, norm, nodes and status are all required");
  if (!ectx)
    ectx = h->ctx;
  if (first_form < 0 || count <= 0 || first_form > h->P.batch - count)
    return fail_msg(h->ctx, "fphip_gram_shortest_vectors: forms [first_form, first_form + count) outside the batch");
  char *err = fphip_ctx_errbuf(h->ctx);
  if (max_sols < 1 || max_sols > 64)
  {
    snprintf(err, 512, "fphip_gram_shortest_vectors: max_sols = %d is outside 1 .. 64", max_sols);
    return FPHIP_ERROR;
  }
  bool any_bound = false;
  if (bound_sq)
    for (int w = 0; w < count; ++w)
    {
      if (bound_sq[w] < 0)
        return fail_msg(h->ctx, "fphip_gram_shortest_vectors: a negative bound_sq (0 = the default bound)");
      any_bound = any_bound || bound_sq[w] > 0;
    }
  if (method != FPHIP_SVPM_FAST)
  {
    snprintf(err, 512, "fphip_gram_shortest_vectors: method %d (SVPM_PROVED and its exact evaluator, or an unknown one) is "
             "not offered: SVPM_FAST only", method);
    return FPHIP_UNSUPPORTED;
  }
  if (flags != 0)
  {
    snprintf(err, 512, "fphip_gram_shortest_vectors: flags 0x%x (SVP_DUAL, SVP_OVERRIDE_BND, or unknown ones) are not "
             "offered: 0 only", flags);
    return FPHIP_UNSUPPORTED;
  }
  const int d = h->P.d, K = max_sols;
  if (route != FPHIP_SVP_ROUTE_AUTO && route != FPHIP_SVP_ROUTE_WAVE && route != FPHIP_SVP_ROUTE_ENUM)
    return fail_msg(h->ctx, "fphip_gram_shortest_vectors: unknown route");
  if (route == FPHIP_SVP_ROUTE_WAVE && d > 64)
  {
    snprintf(err, 512, "fphip_gram_shortest_vectors: the WAVE route takes at most 64 rows (d = %d): use the ENUM route", d);
    return FPHIP_UNSUPPORTED;
  }
  if (d > FPHIP_ENUM_MAX_DIM)
  {  // (not reachable today: fphip_gram_create declines d > 256 = FPHIP_ENUM_MAX_DIM; kept so that the two limits stay
     //  independent — fphip_shortest_vectors has the same line)
    snprintf(err, 512, "fphip_gram_shortest_vectors: more than %d rows", FPHIP_ENUM_MAX_DIM);
    return FPHIP_UNSUPPORTED;
  }
  if (pruning)
    for (int i = 0; i < d; ++i)
      if (!(pruning[i] > 0.0) || !std::isfinite(pruning[i]))
        return fail_msg(h->ctx, "fphip_gram_shortest_vectors: a pruning coefficient that is not a positive finite number");
  std::vector<int> gst(h->P.batch, 0);
  if (int rc = fphip_gram_update(h, gst.data()))
    return rc;
  h->last_ms = 0.0f;
  const size_t dd = (size_t)d, ldd = (size_t)h->P.ldd, kk = (size_t)K;
  // the route of every form of the range: 1 = WAVE
  std::vector<int> take((size_t)count, route == FPHIP_SVP_ROUTE_ENUM || d > 64 ? 0 : 1);
  const bool auto_est = route == FPHIP_SVP_ROUTE_AUTO && d <= 64;
  // host copies for the estimate and the enumerator: r_ii of the range; the form and mu of one form at a time
  std::vector<double> rs;
  if (auto_est || route != FPHIP_SVP_ROUTE_WAVE)
  {
    rs.resize((size_t)count * dd);
    QCHK(hipMemcpy(rs.data(), h->P.rdg + (size_t)first_form * dd, rs.size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  std::vector<long long> gh(dd * dd), diag;
  std::vector<double> muh(dd * dd);
  if (auto_est)
  {
    const char *e    = getenv("FPHIP_SVP_WAVE_MAX_NODES");
    const double lim = e ? atof(e) : SVP_WAVE_MAX_NODES_DEFAULT;
    if (lim > 0.0)
    {
      const bool as_one = K == 1 && !any_bound;  // the decision of fphip_shortest_vector
      for (int w = 0; w < count; ++w)
      {
        if (gst[first_form + w] != 1)
          continue;  // (the kernel reports it)
        const double *rd   = &rs[(size_t)w * dd];
        const long long bw = bound_sq ? bound_sq[w] : 0;
        const int d_eff    = svp_best_rows(d, rd, bw > 0, (double)bw * (1.0 + 0x1p-30));
        bool pos = true;
        for (int i = 0; i < d_eff; ++i)
          pos = pos && rd[i] > 0.0 && std::isfinite(rd[i]);
        if (!pos)
          continue;
        double radius;
        if (as_one)
        {
          double logdet = 0.0;
          for (int i = 0; i < d_eff; ++i)
            logdet += std::log(rd[i]);
          const double gh2 = std::exp((2.0 / d_eff) * (std::lgamma(0.5 * d_eff + 1.0) - 0.5 * d_eff * std::log(M_PI) + 0.5 * logdet));
          radius = std::min(rd[0], gh2);
        }
        else if (bw > 0)
          radius = (double)bw;
        else
        {  // B0: the smallest diagonal entry below d_eff, as a double (an estimate's radius)
          if (diag.empty())
          {  // the diagonals of the whole range, once: one copy of the forms, not one per form
            diag.resize((size_t)count * dd);
            std::vector<long long> all((size_t)count * dd * ldd);
            QCHK(hipMemcpy(all.data(), h->P.g + (size_t)first_form * dd * ldd, all.size() * 8, hipMemcpyDeviceToHost));
            for (size_t f = 0; f < (size_t)count; ++f)
              for (size_t i = 0; i < dd; ++i)
                diag[f * dd + i] = all[f * dd * ldd + i * (ldd + 1)];
          }
          radius = std::numeric_limits<double>::infinity();
          for (int i = 0; i < d_eff; ++i)
            radius = std::min(radius, (double)diag[(size_t)w * dd + i]);
        }
        // the radius never falls below the K-th norm: B0 is the safe side of the estimate
        if (fphip_enum_gh_nodes(d_eff, rd, pruning, radius) > lim)
          take[w] = 0;
      }
    }
  }
  const bool any_wave = std::find(take.begin(), take.end(), 1) != take.end();
  const bool all_wave = std::find(take.begin(), take.end(), 0) == take.end();
  if (any_wave)
    if (int rc = svp_gram_wave_run(h, first_form, count, K, bound_sq, pruning, all_wave ? nullptr : take.data(), found,
                                   sol_coord, norm, nodes, status))
      return rc;
  const float wave_ms = h->last_ms;
  for (int w = 0; w < count; ++w)
  {
    if (take[w])
      continue;
    if (gst[first_form + w] != 1)
    {
      memset(sol_coord + (size_t)w * kk * dd, 0, kk * dd * sizeof(int64_t));
      memset(norm + (size_t)w * kk, 0, kk * sizeof(int64_t));
      found[w] = 0, nodes[w] = 0, status[w] = 0;
      continue;
    }
    const size_t L = (size_t)(first_form + w);
    QCHK(hipMemcpy2D(gh.data(), dd * 8, h->P.g + L * dd * ldd, ldd * 8, dd * 8, dd, hipMemcpyDeviceToHost));
    QCHK(hipMemcpy2D(muh.data(), dd * 8, h->P.mu + L * dd * ldd, ldd * 8, dd * 8, dd, hipMemcpyDeviceToHost));
    if (int rc = svp_gram_enum_one(h, ectx, first_form + w, K, bound_sq ? bound_sq[w] : 0, pruning, gh.data(), muh.data(),
                                   &rs[(size_t)w * dd], found + w, sol_coord + (size_t)w * kk * dd, norm + (size_t)w * kk,
                                   nodes + w, status + w))
      return rc;
  }
  h->last_ms = wave_ms;
  return FPHIP_OK;
}
