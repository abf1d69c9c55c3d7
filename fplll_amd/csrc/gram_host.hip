// gram_host.hip — C ABI (include/fplll_hip.h, fphip_gram_*) for batches of integer quadratic forms on the device:
// MatGSOGram<Z_NR<long>, FP_NR<double>>(g, u, u_inv_t, GSO_INT_GRAM) with update_gso() and
// LLLReduction<Z_NR<long>, FP_NR<double>>::lll().  The kernels are in lll_gram.hip.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/fplll_hip.h"
#include "dev_mem.h"
#include "host_common.h"
#include "kernels.h"
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
