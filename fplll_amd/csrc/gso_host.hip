// gso_host.hip — C ABI (include/fplll_hip.h) for the batched device-resident GSO:
// MatGSO<Z_NR<long>, FP_NR<double>> look-alike entry points at SWEEP granularity
// (update_gso / size_reduction over a row range), because a per-row device call would be
// launch-bound (SURVEY.md §7 "Granularity").

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <limits>
#include <cstring>
#include <utility>
#include <algorithm>
#include <vector>
#include <string>
#include <chrono>
#include <fstream>
#include <sstream>
#include <iomanip>

#include "../../include/fplll_hip.h"
#include "../../include/fplll_hip_debug.h"
#include "gso_device.h"
#include "gso_sweep2.h"
#include "dev_mem.h"
#include "trace.h"
#include "ftx.h"
#include "pruner_engine.h"
namespace fphip_pruner
{
// pruner_search.hip: prune<FP_NR<double>> of one block under PRUNER_METRIC_PROBABILITY_OF_SHORTEST on the
// given volume engine (nullptr: the host loop)
__attribute__((visibility("hidden"))) int prune_block(VolumeEngine *eng, int n, const double *gso_r, double radius,
                                                      double preproc, double target, int flags,
                                                      double *coefficients, double *expectation);
}  // namespace fphip_pruner

#include "host_common.h"
#include "kernels.h"
#include "svp_host.h"
using namespace fphip;

struct fphip_gso
{
  fphip_ctx *ctx;
  GsoBatch P;
  hipEvent_t ev[2];
  float last_ms;
  int waves_per_block;
  int blocks_per_cu;
  bool dirty;  // the integer basis was uploaded after the last (re)float of the rows
  // planes of mu for gso_sweep2_kernel (low / high words; row-major and transposed), [batch][2][d][ldd]
  double *muA;  // anchored transpose of mu for gso_sweep2_kernel's recurrence, [batch][d][ldd] (gso_sweep2.hip)
  short *m16;   // 2-byte mirrors: [batch][n*ldd + d*ldn] (bT16 then b16 of each lattice)
  int *flag16;  // [batch][d]
  int sweep_version;  // 2 (default) or 1 (FPHIP_GSO_SWEEP=1: the first-generation kernel)
  fphip_ctx *ectx;    // hand-off mode of the strategy-BKZ kernel: the enumeration context (same device)
  std::vector<fphip_ctx *> ectx_more;  // … and the further ones of a BATCH of tours (one per hand-off worker)
  double *xbuf;       // lll_x.hip workspace: bf rows [B][d][ldn], then the low planes of mu, r, gf [B][d][ldd] each
  int xbuf_planes = 0;  // ... 3 of them, or 9 once a quad-double run has asked for components 2 and 3
  // opt-in (fphip_debug_gso_lll_ex_keep) for fphip_debug_gso_lll_ex_plane: the leading planes of mu and r as the
  // kernel of the last run left them (the getters' mu / r are recomputed in double from the new basis), [B][d][ldd]
  // each, then the slot of every position, [B][d] ints; x_prec = the precision of that run (0: nothing kept)
  double *xkeep = nullptr;
  int x_keep = 0, x_prec = 0;
  // in-loop pruning of the strategy-BKZ service (FPHIP_BKZ_PRUNE_IN_LOOP; fphip_gso_bkz_inloop_pruning)
  double il_preproc = 1e6, il_target = 0.5;
  int il_min_block = 24, il_flags = 0x4 /* PRUNER_GRADIENT */, il_device = 1;
  unsigned long long il_calls = 0, il_device_jobs = 0, il_host_jobs = 0, il_launches = 0;
  // BKZ_MAX_TIME / BKZ_DUMP_GSO of the device BKZ drivers (fphip_gso_bkz_limits): seconds, file name
  double bkz_max_time = 0.0;
  std::string bkz_dump_path = "gso.json";  // (BKZParam::dump_gso_filename's default, bkz_param.h:120)
  // resident LLL session (fphip_gso_session_lll): the rows live in the kernel's slots while it is active
  bool session_active  = false;
  bool u_in_slots      = false;  // a session left the rows of u in the kernel's slots (restore_position_order)
  bool b_in_slots      = false;  // ... and those of b
  long long *sess_in_d = nullptr;  // device: positions then rows of the caller's row operations
  long long *sess_in_h = nullptr;  // pinned staging of the same
  char *sess_out_h     = nullptr;  // pinned: the state in position order after the last session call
  // FPHIP_BKZ_TRANSFORM: the BKZ call in progress carries u (the _u kernels run, u / u2 are swapped with b / b2);
  // the insertion counters of that call on the device (allocated by the first such call) and as read back
  bool bkz_u                       = false;
  unsigned long long *bkz_stats_d  = nullptr;
  unsigned long long bkz_stats[5]  = {0, 0, 0, 0, 0};
};

#define GCHK(call) CHK(g->ctx, call)

// (internal hook of fphip_destroy, enum_host.hip: not exported)
extern "C" __attribute__((visibility("hidden"))) void fphip_gso_release_all(fphip_ctx *ctx) { (void)ctx; }

static int gso_allocate(fphip_gso *g);

extern "C" int fphip_gso_create(fphip_ctx *ctx, int batch, int d, int n, int row_expo,
                                fphip_gso **out)
{
  if (!ctx || !out)
    return FPHIP_ERROR;
  *out = nullptr;
  if (batch <= 0 || d <= 0 || n <= 0)
  {
    snprintf(fphip_ctx_errbuf(ctx), 512, "fphip_gso_create: bad shape");
    return FPHIP_ERROR;
  }
  if (d > 256 || n > 256)
    return FPHIP_UNSUPPORTED;  // caller keeps the lattice on the CPU path (fplll's MatGSO)
  if (!fphip_ctx_stream(ctx))
  {
    snprintf(fphip_ctx_errbuf(ctx), 512, "fphip_gso_create: context has no device");
    return FPHIP_ERROR;
  }
  fphip_gso *g = new fphip_gso();  // (value-initialised: every plain member zero, the defaults of the class applied)
  g->il_preproc = 1e6, g->il_target = 0.5, g->il_min_block = 24, g->il_flags = 0x4, g->il_device = 1;
  g->ctx        = ctx;
  g->P.batch    = batch;
  g->P.d        = d;
  g->P.n        = n;
  g->P.row_expo = row_expo ? 1 : 0;
  const int rc  = gso_allocate(g);
  if (rc != FPHIP_OK)
  {
    fphip_gso_destroy(g);  // frees whatever was allocated before the failure
    return rc;
  }
  *out = g;
  return FPHIP_OK;
}

static int gso_allocate(fphip_gso *g)
{
  fphip_ctx *ctx = g->ctx;
  const int batch = g->P.batch, d = g->P.d, n = g->P.n;
  // leading dimensions padded to 16 elements: every row starts on a 128-byte line, so the DMA
  // windows that begin at column 0 waste no partial line (FPHIP_GSO_LD_ALIGN=2 keeps them dense)
  const char *la_s = getenv("FPHIP_GSO_LD_ALIGN");
  const int la     = la_s ? atoi(la_s) : 16;
  g->P.ldd         = (d + la - 1) / la * la;
  g->P.ldn         = (n + la - 1) / la * la;
  if (g->P.ldd > 256)
    g->P.ldd = 256;
  if (g->P.ldn > 256)
    g->P.ldn = 256;
  const size_t B   = (size_t)batch;
  const size_t ldd = g->P.ldd, ldn = g->P.ldn;
  const size_t pad = 4096;  // the DMA ring reads whole 16-byte lanes past the end of a row
  GCHK(fphip_dev_alloc((void **)&g->P.b, B * d * ldn * sizeof(long long) + pad, fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->P.bfT, B * n * ldd * sizeof(double) + pad, fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->P.mu, B * d * ldd * sizeof(double) + pad, fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->P.muT, B * d * ldd * sizeof(double) + pad, fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->P.r, B * d * ldd * sizeof(double) + pad, fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->P.rdg, B * d * sizeof(double), fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->P.rexp, B * d * sizeof(long long), fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->P.status, B * sizeof(int), fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->P.bfT32, B * n * ldd * sizeof(float) + pad, fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->P.b32, B * d * ldn * sizeof(int) + pad, fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->P.narrow, B * d * sizeof(int), fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->muA, B * d * ldd * sizeof(double) + pad, fphip_ctx_stream(g->ctx)));
  hipStream_t s0 = fphip_ctx_stream(ctx);
  GCHK(hipMemsetAsync(g->muA, 0, B * d * ldd * sizeof(double) + pad, s0));
  GCHK(fphip_dev_alloc((void **)&g->m16, B * ((size_t)n * ldd + (size_t)d * ldn) * sizeof(short) + pad, fphip_ctx_stream(g->ctx)));
  GCHK(fphip_dev_alloc((void **)&g->flag16, B * d * sizeof(int), fphip_ctx_stream(g->ctx)));
  GCHK(hipMemsetAsync(g->m16, 0, B * ((size_t)n * ldd + (size_t)d * ldn) * sizeof(short) + pad, s0));
  GCHK(hipMemsetAsync(g->flag16, 0, B * d * sizeof(int), s0));
  {
    const char *sv   = getenv("FPHIP_GSO_SWEEP");
    g->sweep_version = (sv && atoi(sv) == 1) ? 1 : 2;
  }
  GCHK(hipMemsetAsync(g->P.bfT32, 0, B * n * ldd * sizeof(float) + pad, s0));
  GCHK(hipMemsetAsync(g->P.b32, 0, B * d * ldn * sizeof(int) + pad, s0));
  GCHK(hipMemsetAsync(g->P.narrow, 0, B * d * sizeof(int), s0));
  {
    const char *nv = getenv("FPHIP_GSO_NARROW");  // 0 keeps every pass on the 8-byte rows (A/B runs)
    // FPHIP_GSO_NARROW: 0 = 8-byte arrays only, 1 = 4-byte mirrors, 2 (default) = 2-byte mirrors too
    g->P.use_narrow = nv ? atoi(nv) : 3;  // 3 = 2-byte mirrors + the integer AXPY fused into the Gram pass (gso_sweep2.hip)
    {
      const char *wr = getenv("FPHIP_GSO_WIDE_RING");
      g->P.wide_ring = wr ? atoi(wr) : 1;
    }
  }
  GCHK(hipMemsetAsync(g->P.b, 0, B * d * ldn * sizeof(long long) + pad, s0));
  GCHK(hipMemsetAsync(g->P.bfT, 0, B * n * ldd * sizeof(double) + pad, s0));
  GCHK(hipMemsetAsync(g->P.mu, 0, B * d * ldd * sizeof(double) + pad, s0));
  GCHK(hipMemsetAsync(g->P.muT, 0, B * d * ldd * sizeof(double) + pad, s0));
  GCHK(hipMemsetAsync(g->P.r, 0, B * d * ldd * sizeof(double) + pad, s0));
  GCHK(hipStreamSynchronize(s0));  // uploads use blocking copies on the null stream
  GCHK(hipEventCreate(&g->ev[0]));
  GCHK(hipEventCreate(&g->ev[1]));
  const char *w      = getenv("FPHIP_GSO_WAVES_PER_BLOCK");
  g->waves_per_block = w ? atoi(w) : 4;
  const char *bp     = getenv("FPHIP_GSO_BLOCKS_PER_CU");
  g->blocks_per_cu   = bp ? atoi(bp) : 0;  // 0 = as many as the LDS ring allows
  return FPHIP_OK;
}

extern "C" void fphip_gso_destroy(fphip_gso *g)
{
  if (!g)
    return;
  if (g->ectx)
    fphip_destroy(g->ectx);
  for (auto *c : g->ectx_more)
    fphip_destroy(c);
  if (g->xbuf)
    fphip_dev_free(g->xbuf, fphip_ctx_stream(g->ctx));
  if (g->xkeep)
    fphip_dev_free(g->xkeep, fphip_ctx_stream(g->ctx));
  hipStreamSynchronize(fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.b, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.bfT, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.mu, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.muT, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.r, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.rdg, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.rexp, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.status, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.bfT32, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.b32, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.narrow, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->muA, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->m16, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->flag16, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.sess_slots, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.sess_state, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->P.sess_out, fphip_ctx_stream(g->ctx));
  fphip_dev_free(g->sess_in_d, fphip_ctx_stream(g->ctx));
  if (g->sess_in_h)
    fphip_pinned_put(g->sess_in_h);
  if (g->sess_out_h)
    fphip_pinned_put(g->sess_out_h);
  if (g->P.gf)
    fphip_dev_free(g->P.gf, fphip_ctx_stream(g->ctx));
  if (g->P.vc)
    fphip_dev_free(g->P.vc, fphip_ctx_stream(g->ctx));
  if (g->P.b2)
    fphip_dev_free(g->P.b2, fphip_ctx_stream(g->ctx));
  if (g->P.u)
    fphip_dev_free(g->P.u, fphip_ctx_stream(g->ctx));
  if (g->P.u2)
    fphip_dev_free(g->P.u2, fphip_ctx_stream(g->ctx));
  if (g->bkz_stats_d)
    fphip_dev_free(g->bkz_stats_d, fphip_ctx_stream(g->ctx));
  if (g->P.lll_info)
    fphip_dev_free(g->P.lll_info, fphip_ctx_stream(g->ctx));
  if (g->P.enum_mu)
    fphip_dev_free(g->P.enum_mu, fphip_ctx_stream(g->ctx));
  if (g->P.bkz_active)
    fphip_dev_free(g->P.bkz_active, fphip_ctx_stream(g->ctx));
  if (g->P.bkz_rows)
    fphip_dev_free(g->P.bkz_rows, fphip_ctx_stream(g->ctx));
  if (g->ev[0])
    hipEventDestroy(g->ev[0]);
  if (g->ev[1])
    hipEventDestroy(g->ev[1]);
  delete g;
}

struct LllArgs
{
  int kstart;
  double delta, logdelta;
};

// A session leaves the rows of b (and of u) in the kernel's slots; its last call also wrote them in position order
// behind the caller's view of the state: that copy becomes b / u when the session ends — by fphip_gso_set_basis
// (which may re-upload only part of the batch: the other lattices get their rows back in position order) or by a
// call that ended with a status other than 1 (the stateless entry points are no longer blocked after it and must
// find b and u consistent).
static int restore_position_order(fphip_gso *g)
{
  if (!g->P.sess_out)
    return FPHIP_OK;
  const size_t B = (size_t)g->P.batch, d = g->P.d, ldd = g->P.ldd, ldn = g->P.ldn;
  if (g->b_in_slots)
  {
    for (size_t L = 0; L < B; ++L)
      GCHK(hipMemcpy(g->P.b + L * d * ldn, g->P.sess_out + L * fphip_session_out_stride(d, ldd, ldn),
                     d * ldn * sizeof(long long), hipMemcpyDeviceToDevice));
    g->b_in_slots = false;
    g->dirty      = true;
  }
  if (g->u_in_slots && g->P.u)
  {
    for (size_t L = 0; L < B; ++L)
      GCHK(hipMemcpy(g->P.u + L * d * ldd,
                     g->P.sess_out + L * fphip_session_out_stride(d, ldd, ldn) + fphip_session_out_bytes(d, ldd, ldn),
                     d * ldd * sizeof(long long), hipMemcpyDeviceToDevice));
  }
  g->u_in_slots = false;
  return FPHIP_OK;
}

static int session_guard(fphip_gso *g, const char *what)
{
  if (!g->session_active)
    return FPHIP_OK;
  snprintf(fphip_ctx_errbuf(g->ctx), 512, "%s: a resident LLL session is active (the rows live in the kernel's slots); "
           "fphip_gso_set_basis ends it", what);
  return FPHIP_ERROR;
}

// With a transformation matrix on the device only the entry points that keep it in step with b may change b
static int transform_guard(fphip_gso *g, const char *what)
{
  if (!g->P.u)
    return FPHIP_OK;
  snprintf(fphip_ctx_errbuf(g->ctx), 512, "%s: the transformation matrix u is tracked (fphip_gso_enable_transform) and "
           "this entry point does not update it; fphip_gso_lll / _lll_flags / _lll_ex / _lll_ladder do", what);
  return FPHIP_UNSUPPORTED;
}

// FPHIP_BKZ_TRANSFORM of the two BKZ entry points.  begin: the flag needs a tracked u; the insertion counters
// (fphip_gso_bkz_insert_stats) start at zero on the device — the array exists only once the flag has been used.
// end: the counters of the call's launches come back, and the object forgets the mode.
static int bkz_transform_begin(fphip_gso *g, bool want, const char *what)
{
  g->bkz_u = false;
  memset(g->bkz_stats, 0, sizeof g->bkz_stats);
  if (!want)
    return FPHIP_OK;
  if (!g->P.u)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "%s: FPHIP_BKZ_TRANSFORM needs a transformation matrix on the device: "
             "call fphip_gso_enable_transform first", what);
    return FPHIP_ERROR;
  }
  if (!g->bkz_stats_d)
    GCHK(fphip_dev_alloc((void **)&g->bkz_stats_d, sizeof g->bkz_stats, fphip_ctx_stream(g->ctx)));
  GCHK(hipMemsetAsync(g->bkz_stats_d, 0, sizeof g->bkz_stats, fphip_ctx_stream(g->ctx)));
  g->bkz_u = true;
  return FPHIP_OK;
}
static void bkz_transform_end(fphip_gso *g)
{
  if (g->bkz_u && g->bkz_stats_d)
    if (hipMemcpy(g->bkz_stats, g->bkz_stats_d, sizeof g->bkz_stats, hipMemcpyDeviceToHost) != hipSuccess)
      memset(g->bkz_stats, 0, sizeof g->bkz_stats);
  g->bkz_u = false;
}
struct BkzTransformScope
{
  fphip_gso *g;
  ~BkzTransformScope() { bkz_transform_end(g); }
};

extern "C" int fphip_gso_bkz_insert_stats(const fphip_gso *g, unsigned long long counts[5])
{
  if (!g || !counts)
    return FPHIP_ERROR;
  memcpy(counts, g->bkz_stats, sizeof g->bkz_stats);
  return FPHIP_OK;
}

static int launch(fphip_gso *g, int kmin, int kend, double eta, int mode, const LllArgs *la = nullptr)
{
  if (mode == 1)
    if (int rct = transform_guard(g, "size_reduce"))
      return rct;
  if (g->P.sess_mode != 2)
    if (int rcg = session_guard(g, "gso"))
      return rcg;
  if (mode == 2)
    g->dirty = false;
  else if (g->dirty)
  {  // a sweep on a freshly uploaded basis: float the rows first (MatGSO::update_bf for every row)
    const int rc0 = launch(g, 0, g->P.d, 0.0, 2);
    if (rc0 != FPHIP_OK)
      return rc0;
  }
  const int need = (g->P.d > g->P.n ? g->P.d : g->P.n);
  const int nq   = (need + 63) / 64;
  const int wpb  = g->waves_per_block;
  int grid       = (g->P.batch + wpb - 1) / wpb;
  hipStream_t s = fphip_ctx_stream(g->ctx);
  if (!la && g->sweep_version == 2)
  {  // gso_sweep2_kernel: its own ring geometry (gso_sweep2.h)
    const int ring   = dispatch_nq(nq, [](auto NQ) { return s2::Cfg<NQ>::RING; });
    const int wps    = dispatch_nq(nq, [](auto NQ) { return s2::Cfg<NQ>::WAVES_PER_SIMD; });
    const size_t lds2 = (size_t)wpb * ring;
    // NQ = 3: three blocks of four waves per CU, not the four that fit — measured 100.8-101.9 ms against
    // 104.5-105.1 ms at batch 8192 (three alternating repetitions on one box, profiles/r04_gso_roof_ab.log):
    // the kernel is bound by the memory system, a quarter fewer lattices in flight thrash it less
    int bpc2          = g->blocks_per_cu > 0 ? g->blocks_per_cu : std::min((int)((160 * 1024) / lds2), nq == 3 ? 3 : 4);
    if (bpc2 * wpb > 4 * wps)
      bpc2 = 4 * wps / wpb;
    if (bpc2 < 1)
      bpc2 = 1;
    const int cap2 = fphip_ctx_num_cus(g->ctx) * bpc2;
    if (grid > cap2)
      grid = cap2;
    GCHK(hipEventRecord(g->ev[0], s));
    dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL(s2::gso_sweep2_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds2, s, g->P, g->muA, g->m16, g->flag16, kmin, kend, eta, mode); });
    GCHK(hipGetLastError());
    GCHK(hipEventRecord(g->ev[1], s));
    GCHK(hipStreamSynchronize(s));
    GCHK(hipEventElapsedTime(&g->last_ms, g->ev[0], g->ev[1]));
    return FPHIP_OK;
  }
  // per-wave LDS-DMA ring: FPHIP_GSO_RING slots of IPS KiB (IPS = ceil(NQ/2))
  const size_t lds = la ? (size_t)wpb * fphip_reduce_ring_bytes(nq)
                        : (size_t)wpb * FPHIP_GSO_RING * (size_t)((nq + 1) / 2) * 1024;
  int bpc          = g->blocks_per_cu > 0 ? g->blocks_per_cu : (lds ? (int)((160 * 1024) / lds) : 32);  // (no LDS: the register streams)
  if (bpc * wpb > 32)
    bpc = 32 / wpb;
  const int cap = fphip_ctx_num_cus(g->ctx) * (bpc > 0 ? bpc : 1);
  if (grid > cap)
    grid = cap;
  if (lds > 64 * 1024)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "gso: LDS ring of %zu bytes exceeds the 64 KiB the DMA base can address", lds);
    return FPHIP_ERROR;
  }
  GCHK(hipEventRecord(g->ev[0], s));
  if (la)
    dispatch_nq(nq, [&](auto NQ) {
      // (the LLL_EARLY_RED instantiations live in lll_kernel_early.hip)
      if (g->P.lll_early || g->P.u)
        hipLaunchKernelGGL((lll_kernel<NQ, true>), dim3(grid), dim3(wpb * 64), lds, s, g->P, kmin, la->kstart, kend,
                           la->delta, eta, la->logdelta);
      else
        hipLaunchKernelGGL((lll_kernel<NQ, false>), dim3(grid), dim3(wpb * 64), lds, s, g->P, kmin, la->kstart, kend,
                           la->delta, eta, la->logdelta);
    });
  else
    dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL(gso_sweep_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, g->P, kmin, kend, eta, mode); });
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(g->ev[1], s));
  if (g->P.sess_mode != 0)
    return FPHIP_OK;  // (a session call: its copies are queued behind the kernel, one wait for all of it)
  GCHK(hipStreamSynchronize(s));
  GCHK(hipEventElapsedTime(&g->last_ms, g->ev[0], g->ev[1]));
  return FPHIP_OK;
}

static int fetch_status(fphip_gso *g, int *status)
{
  if (status)
    GCHK(hipMemcpy(status, g->P.status, sizeof(int) * g->P.batch, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

extern "C" int fphip_gso_set_basis(fphip_gso *g, int first, int count, const int64_t *b)
{
  if (!g || !b || first < 0 || count <= 0 || first + count > g->P.batch)
    return FPHIP_ERROR;
  const size_t rows = (size_t)g->P.d * count;
  // a session ends here for every lattice of the batch: those outside [first, first + count) get their rows back
  // in position order (and so do the rows of u) before the new ones are written
  g->session_active = false;
  if (int rc = restore_position_order(g))
    return rc;
  GCHK(hipMemcpy2D(g->P.b + (size_t)first * g->P.d * g->P.ldn, (size_t)g->P.ldn * 8, b,
                   (size_t)g->P.n * 8, (size_t)g->P.n * 8, rows, hipMemcpyHostToDevice));
  // The kernels run on a NON-BLOCKING stream, which nothing orders against the null stream: the upload has to be
  // complete on the device, not merely handed to the DMA engine from its staging buffer, when this returns.  (The
  // API text allows a pageable upload to return at that point; one of 1536 lattices of a stress test once came back
  // reduced from an all-zero input.)
  GCHK(hipStreamSynchronize(nullptr));
  g->dirty          = true;
  return FPHIP_OK;
}

// replicate lattice `src` into every slot of the batch (device-side copies; used by benchmarks)
extern "C" int fphip_gso_broadcast_basis(fphip_gso *g, int src)
{
  if (!g || src < 0 || src >= g->P.batch)
    return FPHIP_ERROR;
  const size_t per = (size_t)g->P.d * g->P.ldn * sizeof(long long);
  for (int L = 0; L < g->P.batch; ++L)
    if (L != src)
      GCHK(hipMemcpyAsync(g->P.b + (size_t)L * g->P.d * g->P.ldn,
                          g->P.b + (size_t)src * g->P.d * g->P.ldn, per, hipMemcpyDeviceToDevice,
                          fphip_ctx_stream(g->ctx)));
  GCHK(hipStreamSynchronize(fphip_ctx_stream(g->ctx)));
  g->dirty = true;
  return FPHIP_OK;
}

// lattices count, count+1, … become copies of lattices 0 … count-1, cyclically (device-side
// copies: a batch of `count` distinct inputs replicated to the full batch; used by benchmarks)
extern "C" int fphip_gso_tile_basis(fphip_gso *g, int count)
{
  if (!g || count <= 0 || count > g->P.batch)
    return FPHIP_ERROR;
  const size_t per = (size_t)g->P.d * g->P.ldn;
  int have         = count;  // always a multiple of count: the cyclic pattern survives the doubling
  while (have < g->P.batch)
  {
    const int m = have < g->P.batch - have ? have : g->P.batch - have;
    GCHK(hipMemcpyAsync(g->P.b + (size_t)have * per, g->P.b, (size_t)m * per * sizeof(long long),
                        hipMemcpyDeviceToDevice, fphip_ctx_stream(g->ctx)));
    have += m;
  }
  GCHK(hipStreamSynchronize(fphip_ctx_stream(g->ctx)));
  g->dirty = true;
  return FPHIP_OK;
}

extern "C" int fphip_gso_get_basis(fphip_gso *g, int first, int count, int64_t *b)
{
  if (!g || !b || first < 0 || count <= 0 || first + count > g->P.batch)
    return FPHIP_ERROR;
  if (int rcg = session_guard(g, "fphip_gso_get_basis"))  // (fphip_gso_session_read has the basis in position order)
    return rcg;
  const size_t rows = (size_t)g->P.d * count;
  GCHK(hipMemcpy2D(b, (size_t)g->P.n * 8, g->P.b + (size_t)first * g->P.d * g->P.ldn,
                   (size_t)g->P.ldn * 8, (size_t)g->P.n * 8, rows, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

// MatGSO(b, u, ...) with a non-empty u: enable_transform (gso_interface.h:96-110).  u ([batch][d][d], or NULL for
// the identity) goes to the device; the LLL entry points then apply every row operation to its rows as well and
// rotate them with b's (gso.cpp:84-158, 289-366).
extern "C" int fphip_gso_enable_transform(fphip_gso *g, const int64_t *u)
{
  if (!g)
    return FPHIP_ERROR;
  if (int rcg = session_guard(g, "fphip_gso_enable_transform"))
    return rcg;
  const size_t B = (size_t)g->P.batch, d = g->P.d, ldd = g->P.ldd;
  hipStream_t s = fphip_ctx_stream(g->ctx);
  const size_t bytes = B * d * ldd * sizeof(long long);
  if (!g->P.u)
    GCHK(fphip_dev_alloc((void **)&g->P.u, bytes + 4096, s));
  if (!g->P.u2)
    GCHK(fphip_dev_alloc((void **)&g->P.u2, bytes + 4096, s));
  GCHK(hipMemsetAsync(g->P.u, 0, bytes + 4096, s));
  GCHK(hipMemsetAsync(g->P.u2, 0, bytes + 4096, s));
  GCHK(hipStreamSynchronize(s));
  if (u)
    GCHK(hipMemcpy2D(g->P.u, ldd * 8, u, d * 8, d * 8, B * d, hipMemcpyHostToDevice));
  else
  {
    std::vector<long long> id(d * ldd, 0);
    for (size_t i = 0; i < d; ++i)
      id[i * ldd + i] = 1;
    for (size_t L = 0; L < B; ++L)
      GCHK(hipMemcpy(g->P.u + L * d * ldd, id.data(), d * ldd * sizeof(long long), hipMemcpyHostToDevice));
  }
  GCHK(hipStreamSynchronize(nullptr));  // (see fphip_gso_set_basis)
  g->u_in_slots = false;
  return FPHIP_OK;
}

extern "C" int fphip_gso_get_transform(fphip_gso *g, int first, int count, int64_t *u)
{
  if (!g || !u || first < 0 || count <= 0 || first + count > g->P.batch)
    return FPHIP_ERROR;
  if (!g->P.u)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_gso_get_transform: no transformation matrix (fphip_gso_enable_transform)");
    return FPHIP_ERROR;
  }
  if (int rcg = session_guard(g, "fphip_gso_get_transform"))
    return rcg;
  const size_t d = g->P.d, ldd = g->P.ldd;
  GCHK(hipMemcpy2D(u, d * 8, g->P.u + (size_t)first * d * ldd, ldd * 8, d * 8, d * (size_t)count, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

// (re)float every row from the integer basis: MatGSO::update_bf for all rows, gso.cpp:24-48
extern "C" int fphip_gso_refresh(fphip_gso *g)
{
  FPHIP_RANGE("fphip_gso_refresh");
  if (!g)
    return FPHIP_ERROR;
  return launch(g, 0, g->P.d, 0.0, 2);
}

// MatGSOInterface::update_gso(), gso_interface.h:767-775, for every lattice of the batch
extern "C" int fphip_gso_update(fphip_gso *g, int *status)
{
  FPHIP_RANGE("fphip_gso_update");
  if (!g)
    return FPHIP_ERROR;
  int rc = launch(g, 0, g->P.d, 0.0, 0);
  if (rc != FPHIP_OK)
    return rc;
  return fetch_status(g, status);
}

// LLLReduction::size_reduction(kappa_min, kappa_end), lll.h:107-122, for every lattice
extern "C" int fphip_gso_size_reduce(fphip_gso *g, int kappa_min, int kappa_end, double eta,
                                     int *status)
{
  FPHIP_RANGE("fphip_gso_size_reduce");
  if (!g)
    return FPHIP_ERROR;
  if (kappa_end < 0)
    kappa_end = g->P.d;
  if (kappa_min < 0 || kappa_min > kappa_end || kappa_end > g->P.d)
    return FPHIP_ERROR;
  int rc = launch(g, kappa_min, kappa_end, eta, 1);
  if (rc != FPHIP_OK)
    return rc;
  return fetch_status(g, status);
}

static int ensure_lll_buffers(fphip_gso *g);

// LLLReduction<Z_NR<long>, FP_NR<double>>(m, delta, eta, LLL_DEFAULT).lll(kappa_min, kappa_start,
// kappa_end, 0) on a fresh MatGSO(b, GSO_ROW_EXPO) of every lattice (lll.cpp:44-164,
// wrapper.cpp lll_reduction_zf with LM_FAST), then update_gso() so that mu / r are readable in
// place.  info (nullable): 4 ints per lattice — final_kappa, n_swaps, zeros, loop iterations.
extern "C" int fphip_gso_lll(fphip_gso *g, int kappa_min, int kappa_start, int kappa_end,
                             double delta, double eta, int *status, int *info)
{
  return fphip_gso_lll_flags(g, kappa_min, kappa_start, kappa_end, delta, eta, 0, status, info);
}

// fplll's LLLFlags (defs.h:222-227): LLL_VERBOSE (1) is ignored, LLL_EARLY_RED (2) and LLL_SIEGEL (4) run on the
// device (early reduction on the block streams only: FPHIP_UNSUPPORTED in a -DFPHIP_LLL_STREAM=0 build)
static int lll_flags_check(fphip_gso *g, int flags, int *siegel, int *early)
{
  if (flags & ~7)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "lll: unknown flags 0x%x", flags);
    return FPHIP_ERROR;
  }
#if !FPHIP_LLL_STREAM
  if (flags & 2)
    return FPHIP_UNSUPPORTED;
#endif
  *early  = (flags & 2) ? 1 : 0;
  *siegel = (flags & 4) ? 1 : 0;
  return FPHIP_OK;
}

extern "C" int fphip_gso_lll_flags(fphip_gso *g, int kappa_min, int kappa_start, int kappa_end,
                                   double delta, double eta, int flags, int *status, int *info)
{
  FPHIP_RANGE("fphip_gso_lll");
  if (!g)
    return FPHIP_ERROR;
  int siegel = 0, early = 0;
  if (int rcf = lll_flags_check(g, flags, &siegel, &early))
    return rcf;
  if (kappa_end < 0)
    kappa_end = g->P.d;
  if (kappa_min < 0 || kappa_min > kappa_start || kappa_start >= kappa_end || kappa_end > g->P.d)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_gso_lll: need 0 <= kappa_min <= kappa_start < kappa_end <= d");
    return FPHIP_ERROR;
  }
  const size_t B = (size_t)g->P.batch;
  {
    const int rc0 = ensure_lll_buffers(g);
    if (rc0 != FPHIP_OK)
      return rc0;
  }
  int rc = launch(g, 0, g->P.d, 0.0, 2);  // bf / row_expo of every row from b
  if (rc != FPHIP_OK)
    return rc;
  // (swap_threshold = siegel ? delta - eta * eta : delta, lll.cpp:40; the iteration limit keeps log(delta))
  LllArgs la{kappa_start, siegel ? delta - eta * eta : delta, std::log(delta)};
  g->P.lll_siegel = siegel;
  g->P.lll_early  = early;
  rc              = launch(g, kappa_min, kappa_end, eta, 3, &la);
  g->P.lll_siegel = 0;
  g->P.lll_early  = 0;
  if (rc != FPHIP_OK)
    return rc;
  const float lll_ms = g->last_ms;
  std::swap(g->P.b, g->P.b2);  // the kernel wrote the rows in position order into b2
  if (g->P.u)
    std::swap(g->P.u, g->P.u2);  // ... and those of u into u2
  std::vector<int> st(B);
  GCHK(hipMemcpy(st.data(), g->P.status, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (info)
    GCHK(hipMemcpy(info, g->P.lll_info, sizeof(int) * 4 * B, hipMemcpyDeviceToHost));
  // identity-layout GSO of the reduced bases (same values: every entry is a function of b)
  rc = launch(g, 0, g->P.d, 0.0, 2);
  if (rc == FPHIP_OK)
    rc = launch(g, 0, g->P.d, 0.0, 0);
  g->last_ms = lll_ms;
  if (status)
    memcpy(status, st.data(), sizeof(int) * B);
  return rc;
}

// ---- resident LLL session --------------------------------------------------------------------------------
// What MatGSOHip (csrc/dropin/) keeps between the reference's lll() calls: the reference's MatGSO is an OBJECT —
// its rows, Gram cache, mu / r and gso_valid_cols persist from one lll() to the next (gso_interface.h:675-732 the
// accessors, gso_interface.cpp:26-53 the validity tracking), and BKZ's 16 000 lll() calls of a config-2 run each
// touch a few rows.  The stateless fphip_gso_lll rebuilds all of it per call (upload, re-float, every Gram row,
// update_gso, download: 6.2 ms); here the kernel's own state stays on the device: the rows in their slots, slot
// table, symmetric Gram cache, mu / r by slot, valid-column counts, verified prefix.
static int ensure_session_buffers(fphip_gso *g)
{
  const size_t B = (size_t)g->P.batch, d = g->P.d, ldd = g->P.ldd, ldn = g->P.ldn;
  hipStream_t s = fphip_ctx_stream(g->ctx);
  const size_t outb = fphip_session_out_stride(d, ldd, ldn);
  if (!g->P.sess_slots)
    GCHK(fphip_dev_alloc((void **)&g->P.sess_slots, B * 256 * sizeof(int), s));
  if (!g->P.sess_state)
    GCHK(fphip_dev_alloc((void **)&g->P.sess_state, B * 4 * sizeof(int), s));
  if (!g->P.sess_out)
    GCHK(fphip_dev_alloc((void **)&g->P.sess_out, B * outb + 4096, s));
  if (!g->sess_in_d)
    GCHK(fphip_dev_alloc((void **)&g->sess_in_d, (d + d * ldn + d * ldd) * sizeof(long long) + 4096, s));
  if (!g->sess_in_h)
    g->sess_in_h = (long long *)fphip_pinned_get((d + d * ldn + d * ldd) * sizeof(long long));
  if (!g->sess_out_h)
    g->sess_out_h = (char *)fphip_pinned_get(B * outb);
  if (!g->sess_in_h || !g->sess_out_h)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_gso_session_lll: no pinned staging memory");
    return FPHIP_ERROR;
  }
  return FPHIP_OK;
}

extern "C" int fphip_gso_session_lll(fphip_gso *g, int resume, int kappa_min, int kappa_start, int kappa_end,
                                     double delta, double eta, int flags, int n_dirty, const int *dirty_pos,
                                     const int64_t *dirty_rows, int *status, int *info)
{
  FPHIP_RANGE("fphip_gso_session_lll");
  if (!g)
    return FPHIP_ERROR;
  int siegel = 0, early = 0;
  if (int rcf = lll_flags_check(g, flags, &siegel, &early))
    return rcf;
  if (kappa_end < 0)
    kappa_end = g->P.d;
  if (kappa_min < 0 || kappa_min > kappa_start || kappa_start >= kappa_end || kappa_end > g->P.d)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_gso_session_lll: need 0 <= kappa_min <= kappa_start < kappa_end <= d");
    return FPHIP_ERROR;
  }
  const size_t B = (size_t)g->P.batch, d = g->P.d, ldn = g->P.ldn, n = g->P.n, ldd = g->P.ldd;
  const size_t rec = n + (g->P.u ? d : 0);  // a dirty row: its n integers, then its d integers of u when u is tracked
  if (resume && !g->session_active)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_gso_session_lll: no session to resume (start one with resume = 0)");
    return FPHIP_ERROR;
  }
  if (n_dirty < 0 || n_dirty > (int)d || (n_dirty > 0 && (!resume || B != 1 || !dirty_pos || !dirty_rows)))
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_gso_session_lll: row operations need a running session of a batch of one");
    return FPHIP_ERROR;
  }
  int rc = ensure_lll_buffers(g);
  if (rc == FPHIP_OK)
    rc = ensure_session_buffers(g);
  if (rc != FPHIP_OK)
    return rc;
  hipStream_t s = fphip_ctx_stream(g->ctx);
  if (!resume)
  {
    g->session_active = false;
    rc = restore_position_order(g);  // (a new session on the rows an earlier one left in its slots)
    if (rc != FPHIP_OK)
      return rc;
    rc = launch(g, 0, g->P.d, 0.0, 2);  // bf / row_expo / narrow flags of every row from b
    if (rc != FPHIP_OK)
      return rc;
  }
  else if (n_dirty > 0)
  {
    for (int t = 0; t < n_dirty; ++t)
    {
      if (dirty_pos[t] < 0 || dirty_pos[t] >= (int)d)
        return FPHIP_ERROR;
      g->sess_in_h[t] = dirty_pos[t];
      long long *row = g->sess_in_h + n_dirty + (size_t)t * ldn;
      memcpy(row, dirty_rows + (size_t)t * rec, n * sizeof(long long));
      for (size_t c = n; c < ldn; ++c)
        row[c] = 0;
      if (g->P.u)
      {
        long long *urow = g->sess_in_h + n_dirty + (size_t)n_dirty * ldn + (size_t)t * ldd;
        memcpy(urow, dirty_rows + (size_t)t * rec + n, d * sizeof(long long));
        for (size_t c = d; c < ldd; ++c)
          urow[c] = 0;
      }
    }
    GCHK(hipMemcpyAsync(g->sess_in_d, g->sess_in_h,
                        ((size_t)n_dirty + (size_t)n_dirty * ldn + (g->P.u ? (size_t)n_dirty * ldd : 0)) * sizeof(long long),
                        hipMemcpyHostToDevice, s));
  }
  g->P.sess_mode   = resume ? 2 : 1;
  g->P.sess_ndirty = n_dirty;
  g->P.sess_in     = g->sess_in_d;
  LllArgs la{kappa_start, siegel ? delta - eta * eta : delta, std::log(delta)};
  g->P.lll_siegel  = siegel;
  g->P.lll_early   = early;
  rc               = launch(g, kappa_min, kappa_end, eta, 3, &la);
  g->P.lll_siegel  = 0;
  g->P.lll_early   = 0;
  g->P.sess_mode   = 0;
  g->P.sess_ndirty = 0;
  g->session_active = false;
  if (rc != FPHIP_OK)
    return rc;
  std::vector<int> st(B);
  const size_t outb = fphip_session_out_stride(d, g->P.ldd, ldn);
  GCHK(hipMemcpyAsync(g->sess_out_h, g->P.sess_out, B * outb, hipMemcpyDeviceToHost, s));
  GCHK(hipMemcpyAsync(st.data(), g->P.status, sizeof(int) * B, hipMemcpyDeviceToHost, s));
  if (info)
    GCHK(hipMemcpyAsync(info, g->P.lll_info, sizeof(int) * 4 * B, hipMemcpyDeviceToHost, s));
  GCHK(hipStreamSynchronize(s));
  GCHK(hipEventElapsedTime(&g->last_ms, g->ev[0], g->ev[1]));
  // a failed reduction leaves a state the reference would not continue from either; -2 (a multiplier beyond
  // 63 bits) has changed rows the caller's host copy does not have: either way the next call starts over
  bool all_ok = true;
  for (size_t L = 0; L < B; ++L)
    all_ok &= (st[L] == 1);
  g->session_active = all_ok;
  g->u_in_slots     = g->P.u != nullptr;
  g->b_in_slots     = true;
  if (!all_ok)
    if (int rc2 = restore_position_order(g))
      return rc2;
  if (status)
    memcpy(status, st.data(), sizeof(int) * B);
  return FPHIP_OK;
}

extern "C" int fphip_gso_session_read_transform(fphip_gso *g, int lattice, int64_t *u)
{
  if (!g || !u || lattice < 0 || lattice >= g->P.batch || !g->sess_out_h || !g->P.u)
    return FPHIP_ERROR;
  const size_t d = g->P.d, ldd = g->P.ldd, ldn = g->P.ldn;
  const long long *ou = (const long long *)(g->sess_out_h + (size_t)lattice * fphip_session_out_stride(d, ldd, ldn) +
                                            fphip_session_out_bytes(d, ldd, ldn));
  for (size_t i = 0; i < d; ++i)
    memcpy(u + i * d, ou + i * ldd, d * sizeof(long long));
  return FPHIP_OK;
}

extern "C" int fphip_gso_session_read(fphip_gso *g, int lattice, int64_t *b, double *mu, double *r,
                                      int *valid_cols, int64_t *row_expo)
{
  if (!g || lattice < 0 || lattice >= g->P.batch || !g->sess_out_h)
    return FPHIP_ERROR;
  const size_t d = g->P.d, ldd = g->P.ldd, ldn = g->P.ldn, n = g->P.n;
  const char *out      = g->sess_out_h + (size_t)lattice * fphip_session_out_stride(d, ldd, ldn);
  const long long *ob  = (const long long *)out;
  const double *omu    = (const double *)(out + d * ldn * 8);
  const double *orr    = omu + d * ldd;
  const long long *oex = (const long long *)(orr + d * ldd);
  const int *ovc       = (const int *)(oex + d);
  for (size_t i = 0; i < d; ++i)
  {
    if (b)
      memcpy(b + i * n, ob + i * ldn, n * sizeof(long long));
    if (mu)
      memcpy(mu + i * d, omu + i * ldd, d * sizeof(double));
    if (r)
      memcpy(r + i * d, orr + i * ldd, d * sizeof(double));
    if (row_expo)
      row_expo[i] = oex[i];
    if (valid_cols)
      valid_cols[i] = ovc[i];
  }
  return FPHIP_OK;
}

// LLLReduction::lll in a selectable floating-point type (lll_x.hip): precision 106 = double-double on
// the device (the stand-in for FP_NR<dd_real>: Wrapper::lll's fast_lll<dd_real>, wrapper.cpp:322-330),
// 53 = plain double with the same (per-lane) summation order.  Same statuses / info as fphip_gso_lll.
// With a transformation matrix on the device (fphip_gso_enable_transform) the launch is lll_x_u_kernel (lll_x_u.hip):
// u takes every row operation b takes and leaves in position order through u2, like b through b2.
//
// Quad-double with more than one column per lane has never been launched in any form (and the wide quad-double
// instantiations of the sibling HLLL kernel faulted with the cause still open): with a tracked u
// that territory is not extended — lll_x_u_kernel<NQ >= 2, QD> does not exist.
static bool lll_x_u_covers_quad_double(const fphip_gso *g)
{
  return !g->P.u || (g->P.d <= 64 && g->P.n <= 64);
}

static int gso_lll_ex(fphip_gso *g, int kappa_min, int kappa_start, int kappa_end, double delta, double eta,
                      int precision, const int *d_only_failed, int *status, int *info)
{
  if (!g || (precision != 53 && precision != 106 && precision != 212))
    return FPHIP_ERROR;
  if (kappa_end < 0)
    kappa_end = g->P.d;
  if (kappa_min < 0 || kappa_min > kappa_start || kappa_start >= kappa_end || kappa_end > g->P.d || g->P.d > 256)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_gso_lll_ex: need 0 <= kappa_min <= kappa_start < kappa_end <= d <= 256");
    return FPHIP_ERROR;
  }
  if (precision == 212 && !lll_x_u_covers_quad_double(g))
  {  // before anything is allocated or launched: b and u stay as they are
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_gso_lll_ex: the transformation matrix u is tracked and quad-double "
             "(precision 212) carries it for max(d, n) <= 64 only (d = %d, n = %d): the wider quad-double kernels have "
             "never been launched; precision 106 carries u at every width", g->P.d, g->P.n);
    return FPHIP_UNSUPPORTED;
  }
  int rc = ensure_lll_buffers(g);
  if (rc != FPHIP_OK)
    return rc;
  const size_t B = (size_t)g->P.batch, d = g->P.d, ldd = g->P.ldd, ldn = g->P.ldn;
  hipStream_t s = fphip_ctx_stream(g->ctx);
  if (g->P.u && !g->P.u2)
  {  // (fphip_gso_enable_transform allocates the pair; an object that lost the second buffer gets it back)
    GCHK(fphip_dev_alloc((void **)&g->P.u2, B * d * ldd * sizeof(long long) + 4096, s));
    GCHK(hipMemsetAsync(g->P.u2, 0, B * d * ldd * sizeof(long long) + 4096, s));
  }
  const size_t n_bf = B * d * ldn, n_pl = B * d * ldd;
  // (bf, then the low planes of mu / r / gf, then — quad-double — two more planes of each)
  const int planes = precision == 212 ? 9 : 3;
  if (g->xbuf && g->xbuf_planes < planes)
  {
    fphip_dev_free(g->xbuf, s);
    g->xbuf = nullptr;
  }
  if (!g->xbuf)
  {
    GCHK(fphip_dev_alloc((void **)&g->xbuf, (n_bf + planes * n_pl) * sizeof(double) + 4096, s));
    g->xbuf_planes = planes;
  }
  g->x_prec = 0;
  if (g->x_keep)
  {  // the slot table starts as the identity: a lattice the kernel skips (only_failed) keeps its rows where they are
    if (!g->xkeep)
      GCHK(fphip_dev_alloc((void **)&g->xkeep, (2 * n_pl + B * d) * sizeof(double), s));
    std::vector<int> ident(B * d);
    for (size_t i = 0; i < B * d; ++i)
      ident[i] = (int)(i % d);
    GCHK(hipMemcpy(g->xkeep + 2 * n_pl, ident.data(), B * d * sizeof(int), hipMemcpyHostToDevice));
  }
  GCHK(hipMemsetAsync(g->xbuf, 0, (n_bf + planes * n_pl) * sizeof(double), s));
  const bool wide = precision >= 106;
  LllX A;
  A.batch    = g->P.batch;
  A.d        = g->P.d;
  A.n        = g->P.n;
  A.ldn      = g->P.ldn;
  A.ldd      = g->P.ldd;
  A.row_expo = g->P.row_expo;
  A.b        = g->P.b;
  A.b2       = g->P.b2;
  A.bf       = g->xbuf;
  A.mu_hi    = g->P.mu;
  A.mu_lo    = wide ? g->xbuf + n_bf : nullptr;
  A.r_hi     = g->P.r;
  A.r_lo     = wide ? g->xbuf + n_bf + n_pl : nullptr;
  A.gf_hi    = g->P.gf;
  A.gf_lo    = wide ? g->xbuf + n_bf + 2 * n_pl : nullptr;
  A.mu_x     = precision == 212 ? g->xbuf + n_bf + 3 * n_pl : nullptr;
  A.r_x      = precision == 212 ? g->xbuf + n_bf + 5 * n_pl : nullptr;
  A.gf_x     = precision == 212 ? g->xbuf + n_bf + 7 * n_pl : nullptr;
  A.rexp     = g->P.rexp;
  A.status   = g->P.status;
  A.info     = g->P.lll_info;
  A.only_failed = d_only_failed;
  A.kmin     = kappa_min;
  A.kstart   = kappa_start;
  A.kend     = kappa_end;
  A.delta    = delta;
  A.eta      = eta;
  A.slot_out = g->x_keep ? (int *)(g->xkeep + 2 * n_pl) : nullptr;
  if (d_only_failed)  // the lattices that are skipped keep their rows: b2 := b first
    GCHK(hipMemcpyAsync(g->P.b2, g->P.b, B * d * ldn * sizeof(long long), hipMemcpyDeviceToDevice, s));
  if (d_only_failed && g->P.u)  // ... and their rows of u: u2 := u
    GCHK(hipMemcpyAsync(g->P.u2, g->P.u, B * d * ldd * sizeof(long long), hipMemcpyDeviceToDevice, s));
  const int need = (g->P.d > g->P.n ? g->P.d : g->P.n);
  const int nq   = (need + 63) / 64;
  int grid       = g->P.batch;
  if (grid > fphip_ctx_num_cus(g->ctx) * 8)
    grid = fphip_ctx_num_cus(g->ctx) * 8;
  GCHK(hipEventRecord(g->ev[0], s));
  if (g->P.u)
  {
    long long *u = g->P.u, *u2 = g->P.u2;
    const int ldu = g->P.ldd;
    dispatch_precision(precision, [&](auto ft) {
      using FT = typename decltype(ft)::type;
      if constexpr (std::is_same<FT, QD>::value)  // (nq == 1: lll_x_u_covers_quad_double above)
        hipLaunchKernelGGL((lll_x_u_kernel<1, QD>), dim3(grid), dim3(64), 0, s, A, u, u2, ldu);
      else
        dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL((lll_x_u_kernel<NQ, FT>), dim3(grid), dim3(64), 0, s, A, u, u2, ldu); });
    });
  }
  else
    dispatch_precision(precision, [&](auto ft) {
      using FT = typename decltype(ft)::type;
      dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL((lll_x_kernel<NQ, FT>), dim3(grid), dim3(64), 0, s, A); });
    });
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(g->ev[1], s));
  GCHK(hipStreamSynchronize(s));
  float ms = 0;
  GCHK(hipEventElapsedTime(&ms, g->ev[0], g->ev[1]));
  std::swap(g->P.b, g->P.b2);  // the kernel wrote the rows in position order into b2
  if (g->P.u)
    std::swap(g->P.u, g->P.u2);  // ... and those of u into u2 (every launch, whatever its statuses)
  if (g->x_keep)
  {
    GCHK(hipMemcpyAsync(g->xkeep, g->P.mu, n_pl * sizeof(double), hipMemcpyDeviceToDevice, s));
    GCHK(hipMemcpyAsync(g->xkeep + n_pl, g->P.r, n_pl * sizeof(double), hipMemcpyDeviceToDevice, s));
    g->x_prec = precision;
  }
  if (status)
    GCHK(hipMemcpy(status, g->P.status, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (info)
    GCHK(hipMemcpy(info, g->P.lll_info, sizeof(int) * 4 * B, hipMemcpyDeviceToHost));
  // identity-layout double GSO of the new bases for the getters (its values are functions of b; on a
  // lattice that needs more than 53 bits they are as good as doubles get)
  rc = launch(g, 0, g->P.d, 0.0, 2);
  if (rc == FPHIP_OK)
    rc = launch(g, 0, g->P.d, 0.0, 0);
  g->last_ms = ms;
  return rc;
}

// mu (which = 0) or r (which = 1) of the last fphip_gso_lll_ex run as lll_x.hip left them, one component plane
// (0 .. 3) at a time: out[d][d] row-major, rows in POSITION order (the kernel keys them by slot), columns are
// positions; mu(i,j) for j < i and r(i,j) for j <= i are meaningful, stored like fphip_gso_get_mu / _get_r (row
// exponents: fphip_gso_get_row_expo).  A plane the run's type does not have reads as zeros.  Needs
// fphip_debug_gso_lll_ex_keep(g, 1) BEFORE the run (FPHIP_ERROR otherwise): the production path keeps nothing.
extern "C" int fphip_debug_gso_lll_ex_keep(fphip_gso *g, int on)
{
  if (!g)
    return FPHIP_ERROR;
  g->x_keep = on != 0;
  g->x_prec = 0;
  return FPHIP_OK;
}

extern "C" int fphip_debug_gso_lll_ex_plane(fphip_gso *g, int lattice, int which, int plane, double *out)
{
  if (!g || !out || !g->xbuf || !g->xkeep || g->x_prec == 0 || lattice < 0 || lattice >= g->P.batch || which < 0 || which > 1 ||
      plane < 0 || plane > 3)
    return FPHIP_ERROR;
  const size_t B = (size_t)g->P.batch, d = g->P.d, ldd = g->P.ldd, ldn = g->P.ldn;
  const size_t n_bf = B * d * ldn, n_pl = B * d * ldd;
  const int have = g->x_prec == 212 ? 4 : (g->x_prec == 106 ? 2 : 1);
  if (plane >= have)
  {
    memset(out, 0, d * d * sizeof(double));
    return FPHIP_OK;
  }
  // the layout of gso_lll_ex: bf, the low planes of mu / r / gf, two more planes of each (quad-double)
  const double *tail = g->xkeep;
  const double *src  = plane == 0 ? tail + which * n_pl
                       : plane == 1 ? g->xbuf + n_bf + which * n_pl
                                    : g->xbuf + n_bf + (3 + 2 * which + (plane - 2)) * n_pl;
  std::vector<double> rows(d * d);
  std::vector<int> slot(d);
  GCHK(hipMemcpy2D(rows.data(), d * 8, src + (size_t)lattice * d * ldd, ldd * 8, d * 8, d, hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(slot.data(), (const int *)(tail + 2 * n_pl) + (size_t)lattice * d, d * sizeof(int),
                 hipMemcpyDeviceToHost));
  for (size_t p = 0; p < d; ++p)
  {
    if (slot[p] < 0 || (size_t)slot[p] >= d)
      return FPHIP_ERROR;
    memcpy(out + p * d, rows.data() + (size_t)slot[p] * d, d * sizeof(double));
  }
  return FPHIP_OK;
}

extern "C" int fphip_gso_lll_ex(fphip_gso *g, int kappa_min, int kappa_start, int kappa_end, double delta,
                                double eta, int precision, int *status, int *info)
{
  FPHIP_RANGE("fphip_gso_lll_ex");
  if (g && g->P.u)  // (a tracked u used to be refused here; a session keeps its rows in the kernel's slots)
    if (int rcg = session_guard(g, "fphip_gso_lll_ex"))
      return rcg;
  return gso_lll_ex(g, kappa_min, kappa_start, kappa_end, delta, eta, precision, nullptr, status, info);
}

// The LLL-side precision ladder of the reference's wrapper (Wrapper::lll, wrapper.cpp:281-359:
// fast_lll<double>, then the wider types, each on the basis the failed attempt left) with both
// stages on the device: the exact-order double kernel (lll_kernel.hip) for the whole batch, then
// double-double (lll_x.hip) for the lattices that stopped with RED_GSO_FAILURE (0), RED_BABAI_FAILURE
// (-1) or RED_LLL_FAILURE (-3), then quad-double for those it gives up on (round 6).  stage[batch] (nullable): 53,
// 106 or 212.  A lattice that fails at 212 bits keeps its status: the caller's MPFR stage (fplll's CPU path) is next.
extern "C" int fphip_gso_lll_ladder(fphip_gso *g, int kappa_min, int kappa_start, int kappa_end, double delta,
                                    double eta, int *status, int *info, int *stage)
{
  FPHIP_RANGE("fphip_gso_lll_ladder");
  if (!g)
    return FPHIP_ERROR;
  const size_t B = (size_t)g->P.batch;
  std::vector<int> st(B, 0), inf(4 * B, 0), stg(B, 53);
  int rc = fphip_gso_lll(g, kappa_min, kappa_start, kappa_end, delta, eta, st.data(), inf.data());
  if (rc != FPHIP_OK)
    return rc;
  float ms = g->last_ms;
  bool any = false;
  std::vector<int> mask(B);
  if (getenv("FPHIP_LLL_LADDER_TEST") && atoi(getenv("FPHIP_LLL_LADDER_TEST")) >= 1)
    for (size_t L = 1; L < B; L += 2)  // (tests only: the odd lattices as if the double stage had failed)
      if (st[L] == 1)
        st[L] = -1;
  for (size_t L = 0; L < B; ++L)
  {
    const bool failed = (st[L] == 0 || st[L] == -1 || st[L] == -3);
    mask[L]           = failed ? 0 : 1;
    any |= failed;
  }
  if (any)
  {
    std::vector<int> st2(B, 0), inf2(4 * B, 0);
    int *d_mask = nullptr;
    GCHK(fphip_dev_alloc((void **)&d_mask, B * sizeof(int), fphip_ctx_stream(g->ctx)));
    hipError_t e = hipMemcpy(d_mask, mask.data(), B * sizeof(int), hipMemcpyHostToDevice);
    // (the wider stage restarts the loop from the top of the range, like a fresh fast_lll<dd_real>)
    rc = (e == hipSuccess) ? gso_lll_ex(g, kappa_min, kappa_min, kappa_end, delta, eta, 106, d_mask, st2.data(), inf2.data())
                           : FPHIP_ERROR;
    fphip_dev_free(d_mask, fphip_ctx_stream(g->ctx));
    if (rc != FPHIP_OK)
      return rc;
    ms += g->last_ms;
    for (size_t L = 0; L < B; ++L)
      if (!mask[L])
      {
        st[L]  = st2[L];
        stg[L] = 106;
        for (int t = 0; t < 4; ++t)
          inf[4 * L + t] = (t == 0 || t == 2) ? inf2[4 * L + t] : inf[4 * L + t] + inf2[4 * L + t];
      }
    // third stage (Wrapper::lll goes on to fast_lll<qd_real>, wrapper.cpp:331-339): quad-double for the lattices
    // double-double gave up on (FPHIP_LLL_LADDER_TEST=2, tests only: every fourth lattice as if it had)
    // With a tracked u and more than 64 rows or columns there is no third stage (lll_x_u_covers_quad_double): the
    // lattices double-double gave up on keep their status and stage 106.
    const bool qd = lll_x_u_covers_quad_double(g);
    if (qd && getenv("FPHIP_LLL_LADDER_TEST") && atoi(getenv("FPHIP_LLL_LADDER_TEST")) == 2)
      for (size_t L = 3; L < B; L += 4)
        if (!mask[L] && st[L] == 1)
          st[L] = -1;
    std::vector<int> mask3(B);
    bool any3 = false;
    for (size_t L = 0; L < B; ++L)
    {
      const bool failed = qd && !mask[L] && (st[L] == 0 || st[L] == -1 || st[L] == -3);
      mask3[L]          = failed ? 0 : 1;
      any3 |= failed;
    }
    if (any3)
    {
      std::vector<int> st3(B, 0), inf3(4 * B, 0);
      int *d_mask3 = nullptr;
      GCHK(fphip_dev_alloc((void **)&d_mask3, B * sizeof(int), fphip_ctx_stream(g->ctx)));
      hipError_t e3 = hipMemcpy(d_mask3, mask3.data(), B * sizeof(int), hipMemcpyHostToDevice);
      rc = (e3 == hipSuccess) ? gso_lll_ex(g, kappa_min, kappa_min, kappa_end, delta, eta, 212, d_mask3, st3.data(), inf3.data())
                              : FPHIP_ERROR;
      fphip_dev_free(d_mask3, fphip_ctx_stream(g->ctx));
      if (rc != FPHIP_OK)
        return rc;
      ms += g->last_ms;
      for (size_t L = 0; L < B; ++L)
        if (!mask3[L])
        {
          st[L]  = st3[L];
          stg[L] = 212;
          for (int t = 0; t < 4; ++t)
            inf[4 * L + t] = (t == 0 || t == 2) ? inf3[4 * L + t] : inf[4 * L + t] + inf3[4 * L + t];
        }
    }
  }
  g->last_ms = ms;
  if (status)
    memcpy(status, st.data(), B * sizeof(int));
  if (info)
    memcpy(info, inf.data(), 4 * B * sizeof(int));
  if (stage)
    memcpy(stage, stg.data(), B * sizeof(int));
  return FPHIP_OK;
}

static int ensure_lll_buffers(fphip_gso *g)
{
  const size_t B = (size_t)g->P.batch, d = g->P.d, ldd = g->P.ldd, ldn = g->P.ldn;
  // (each buffer on its own: a failed allocation must not leave a half-initialised set behind)
  if (!g->P.gf)
    GCHK(fphip_dev_alloc((void **)&g->P.gf, B * d * ldd * sizeof(double) + 4096, fphip_ctx_stream(g->ctx)));
  if (!g->P.vc)
    GCHK(fphip_dev_alloc((void **)&g->P.vc, B * d * sizeof(int), fphip_ctx_stream(g->ctx)));
  if (!g->P.lll_info)
    GCHK(fphip_dev_alloc((void **)&g->P.lll_info, B * 4 * sizeof(int), fphip_ctx_stream(g->ctx)));
  if (!g->P.b2)
  {
    GCHK(fphip_dev_alloc((void **)&g->P.b2, B * d * ldn * sizeof(long long) + 4096, fphip_ctx_stream(g->ctx)));
    // (stream-ordered: no device-wide synchronisation — other contexts may have kernels running)
    GCHK(hipMemsetAsync(g->P.b2, 0, B * d * ldn * sizeof(long long) + 4096, fphip_ctx_stream(g->ctx)));
  }
  return FPHIP_OK;
}

// BKZReduction<Z_NR<long>, FP_NR<double>>(m, lll_obj, BKZParam(block_size, {}, delta, flags,
// max_loops)).bkz() (bkz.cpp:522-668) on every lattice: primal BKZ with empty strategies (no
// pruning, no preprocessing — what bkz_reduction(b, beta, BKZ_DEFAULT, FT_DOUBLE) runs without a
// strategies file, BASELINE config 2).  flags: FPHIP_BKZ_MAX_LOOPS (0x4) with max_loops and / or
// FPHIP_BKZ_AUTO_ABORT (0x20), fplll's values.  Without AUTO_ABORT the whole reduction is one
// launch; with it the tours are launched one by one and BKZAutoAbort::test_abort (scale 1.0, 5
// tours, bkz.cpp:800-809) runs on the host between them — the slope needs the host's log(), the
// reference's — on the r_ii of every lattice that is still active.  The input is expected
// LLL-reduced, as bkz_reduction guarantees (bkz.cpp:870-885): call fphip_gso_lll first.
// status[batch]: 1 RED_SUCCESS, 8 RED_BKZ_LOOPS_LIMIT, <= 0 the failing LLL status.
// info (nullable) [batch][4]: tours, enumeration nodes (low, high 32 bits; fplll rule), enumeration calls.
static int bkz_launch(fphip_gso *g, int block_size, double delta, double eta, int use_loops,
                      int max_loops, float *ms, int *st_out, int *info_out)
{
  if (int rcg = session_guard(g, "bkz"))
    return rcg;
  if (!g->bkz_u)
    if (int rct = transform_guard(g, "bkz"))
      return rct;
  const int need = (g->P.d > g->P.n ? g->P.d : g->P.n);
  const int nq   = (need + 63) / 64;
  const int wpb  = g->waves_per_block;
  const int bs   = block_size < 2 ? 2 : (block_size < g->P.d ? block_size : g->P.d);
  const int stack_doubles = (bs * (bs + 1)) / 2 + 2;
  const size_t ring_bytes = (size_t)wpb * fphip_reduce_ring_bytes(nq);
  const size_t lds        = ring_bytes + (size_t)wpb * stack_doubles * sizeof(double);
  if (ring_bytes > 64 * 1024 || lds > 160 * 1024)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "bkz: %zu bytes of LDS per workgroup do not fit", lds);
    return FPHIP_ERROR;
  }
  int bpc = lds ? (int)((160 * 1024) / lds) : 32;
  if (bpc * wpb > 32)
    bpc = 32 / wpb;
  int grid      = (g->P.batch + wpb - 1) / wpb;
  const int cap = fphip_ctx_num_cus(g->ctx) * (bpc > 0 ? bpc : 1);
  if (grid > cap)
    grid = cap;
  hipStream_t s     = fphip_ctx_stream(g->ctx);
  const double logd = std::log(delta);
  if (lds > 64 * 1024 && g->bkz_u)
    GCHK(dispatch_nq(nq, [&](auto NQ) { return allow_lds(bkz_kernel_u<NQ>, lds); }));
  else if (lds > 64 * 1024)
    GCHK(dispatch_nq(nq, [&](auto NQ) { return allow_lds(bkz_kernel<NQ>, lds); }));
  GCHK(hipEventRecord(g->ev[0], s));
  if (g->bkz_u)
    dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL(bkz_kernel_u<NQ>, dim3(grid), dim3(wpb * 64), lds, s, g->P, block_size, delta, eta, logd, use_loops, max_loops, stack_doubles, g->bkz_stats_d); });
  else
    dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL(bkz_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, g->P, block_size, delta, eta, logd, use_loops, max_loops, stack_doubles); });
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(g->ev[1], s));
  GCHK(hipStreamSynchronize(s));
  GCHK(hipEventElapsedTime(ms, g->ev[0], g->ev[1]));
  // (the sweep launches below reuse P.status)
  GCHK(hipMemcpy(st_out, g->P.status, sizeof(int) * g->P.batch, hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(info_out, g->P.lll_info, sizeof(int) * 4 * g->P.batch, hipMemcpyDeviceToHost));
  std::swap(g->P.b, g->P.b2);  // the kernel wrote the rows in position order into b2
  if (g->bkz_u)
    std::swap(g->P.u, g->P.u2);  // ... and those of u into u2 (every launch, whatever its statuses)
  // identity-layout GSO of the current bases (same values: every entry is a function of b)
  int rc = launch(g, 0, g->P.d, 0.0, 2);
  if (rc == FPHIP_OK)
    rc = launch(g, 0, g->P.d, 0.0, 0);
  return rc;
}

// info accumulation across one-tour launches: tours, 64-bit node count (two 32-bit halves), calls
static void accumulate_info(int *inf, const int *one, size_t L)
{
  inf[4 * L + 0] += one[4 * L + 0];
  const unsigned long long a = ((unsigned long long)(unsigned)inf[4 * L + 2] << 32) | (unsigned)inf[4 * L + 1];
  const unsigned long long b = ((unsigned long long)(unsigned)one[4 * L + 2] << 32) | (unsigned)one[4 * L + 1];
  const unsigned long long t = a + b;
  inf[4 * L + 1] = (int)(unsigned)(t & 0xffffffffull);
  inf[4 * L + 2] = (int)(unsigned)(t >> 32);
  inf[4 * L + 3] += one[4 * L + 3];
}

// BKZ_AUTO_ABORT for both device BKZ drivers: one tour per launch, BKZAutoAbort::test_abort(1.0, 5)
// (bkz.cpp:800-809) on the host in between — the slope of log r_ii (MatGSOInterface::
// get_current_slope, gso_interface.cpp:198-218) needs the host's log(), the one the reference calls.
// run_tour(loop, &ms, s1, one) launches exactly one tour for the lattices with active[L] != 0 and
// leaves the identity-layout GSO (r_ii, row exponents) of the new bases on the device.
// slope_test: BKZ_AUTO_ABORT (the slope test between the tours).  slide: BKZ_SLD_RED — a launch is one
// slide_tour, and the tour's own progress test runs here: get_slide_potential (gso_interface.cpp:230-258:
// sum over the blocks of (p - i) log det, the host's log) of the new basis against the previous one,
// bkz.cpp:512-518 — "clean" (no progress) ends the loop with RED_SUCCESS like any clean tour.
// BKZ_MAX_TIME (bkz.cpp:563,588-592) and BKZ_DUMP_GSO (:373-377, 456-460, 508-512, 536-539, 667-670; dump_gso
// :729-790) of the tour loop below.  Time is the wall clock of the call (the reference reads the process's CPU time,
// cputime(): the same thing for its single thread).  The dump is the reference's hand-written JSON, one file per
// lattice (lattice 0: the name itself, lattice L > 0: name.L): "Input", one entry per tour, "Output".
struct TourHooks
{
  bool use_time = false, dump = false;
  double max_time = 0.0;
  const char *step = "End of BKZ loop";
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

static std::string dump_name(const fphip_gso *g, size_t L)
{
  return L == 0 ? g->bkz_dump_path : g->bkz_dump_path + "." + std::to_string(L);
}

// BKZReduction::dump_gso (bkz.cpp:729-790): norms = log(r_ii) + expo log 2 of the rows below num_rows, 8 digits
static int dump_gso_entry(const fphip_gso *g, size_t L, bool append, const char *step, int loop, double time,
                          const double *rdg, const long long *rex, int num_rows)
{
  std::ofstream dump;
  if (append)
    dump.open(dump_name(g, L).c_str(), std::ios_base::app);
  else
  {
    dump.open(dump_name(g, L).c_str());
    dump << "[" << std::endl;
  }
  if (!dump)
    return FPHIP_ERROR;
  dump << std::string(8, ' ') << "{" << std::endl;
  dump << std::string(16, ' ') << "\"step\": \"" << step << "\"," << std::endl;
  dump << std::string(16, ' ') << "\"loop\": " << loop << "," << std::endl;
  dump << std::string(16, ' ') << "\"time\": " << time << "," << std::endl;
  std::stringstream ss;
  for (int i = 0; i < num_rows; ++i)
  {
    const double log_f = std::log(rdg[i]);
    const long expo    = (long)(2 * rex[i]);  // get_r_exp(i, i, expo), gso_interface.h:711-716
    ss << std::setprecision(8) << log_f + expo * std::log(2.0) << ", ";
  }
  const std::string str = ss.str();
  dump << std::string(16, ' ') << "\"norms\": [" << str.substr(0, str.size() >= 2 ? str.size() - 2 : 0) << "]"
       << std::endl;
  dump << std::string(8, ' ') << "}";
  if (std::string(step) == "Output")
    dump << std::endl << "]";
  else
    dump << "," << std::endl;
  return dump ? FPHIP_OK : FPHIP_ERROR;
}

// the "Output" entry (bkz.cpp:667-670): the GSO norms of the bases as the call leaves them
static int dump_gso_output(fphip_gso *g, const TourHooks &hooks, const std::vector<int> &st, const std::vector<int> &rows)
{
  const size_t B = (size_t)g->P.batch, d = (size_t)g->P.d;
  int rc = launch(g, 0, g->P.d, 0.0, 0);
  if (rc != FPHIP_OK)
    return rc;
  std::vector<double> rdg(B * d);
  std::vector<long long> rex(B * d);
  GCHK(hipMemcpy(rdg.data(), g->P.rdg, sizeof(double) * B * d, hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(rex.data(), g->P.rexp, sizeof(long long) * B * d, hipMemcpyDeviceToHost));
  for (size_t L = 0; L < B; ++L)
    if (st[L] == 1 || st[L] == 7 || st[L] == 8)  // (a failing tour throws past the dump, bkz.cpp:611-614)
      if (dump_gso_entry(g, L, true, "Output", -1, hooks.seconds(), &rdg[L * d], &rex[L * d], rows[L]) != FPHIP_OK)
        return fail_msg(g->ctx, "BKZ_DUMP_GSO: cannot write the dump file");
  return FPHIP_OK;
}

template <class RunTour>
static int auto_abort_loop(fphip_gso *g, int block_size, bool use_loops, int max_loops, std::vector<int> &active,
                           std::vector<int> &st, std::vector<int> &inf, std::vector<int> &rows, float &total_ms,
                           RunTour run_tour, bool slope_test = true, bool slide = false,
                           const TourHooks &hooks = TourHooks())
{
  const size_t B = (size_t)g->P.batch, d = (size_t)g->P.d;
  std::vector<char> ran(B, 0);  // the lattice took part in the tour before this iteration
  int rc = launch(g, 0, g->P.d, 0.0, 0);  // r_ii of the input bases
  if (rc != FPHIP_OK)
    return rc;
  std::vector<double> rdg(B * d), old_slope(B, std::numeric_limits<double>::max());
  std::vector<long long> rex(B * d);
  std::vector<int> no_dec(B, -1), one(4 * B), s1(B);
  std::vector<double> sld_potential(B, 0.0);
  bool rows_known = false;
  for (int loop = 0;; ++loop)
  {
    size_t n_active = 0;
    GCHK(hipMemcpy(rdg.data(), g->P.rdg, sizeof(double) * B * d, hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(rex.data(), g->P.rexp, sizeof(long long) * B * d, hipMemcpyDeviceToHost));
    if (!rows_known)
    {  // trailing zero rows (bkz.cpp:35-37) have r_ii == 0 exactly
      for (size_t L = 0; L < B; ++L)
      {
        int nr = (int)d;
        while (nr > 0 && rdg[L * d + nr - 1] == 0.0)
          --nr;
        rows[L] = nr;
      }
      rows_known = true;
    }
    for (size_t L = 0; L < B; ++L)
    {
      if (hooks.dump && (loop == 0 ? active[L] != 0 : ran[L] != 0))
      {  // "Input" (bkz.cpp:536-539) / the entry at the end of tour loop - 1 (:373-377)
        if (dump_gso_entry(g, L, loop != 0, loop == 0 ? "Input" : hooks.step, loop == 0 ? -1 : loop - 1,
                           loop == 0 ? 0.0 : hooks.seconds(), &rdg[L * d], &rex[L * d], rows[L]) != FPHIP_OK)
          return fail_msg(g->ctx, "BKZ_DUMP_GSO: cannot write the dump file");
      }
      ran[L] = 0;
      if (!active[L])
        continue;
      if (block_size < 2)
      {
        active[L] = 0;
        continue;
      }
      if (slide)
      {
        const int n = rows[L];
        double potential = 0.0;
        int p            = n / block_size;
        if (n % block_size == 0)
          --p;
        for (int i = 0; i < p; ++i)
        {
          double log_det = 0.0;  // get_log_det(i bs, (i + 1) bs)
          for (int k = i * block_size; k < std::min(n, (i + 1) * block_size); ++k)
            log_det += std::log(std::ldexp(rdg[L * d + k], (int)(2 * rex[L * d + k])));
          potential += (p - i) * log_det;
        }
        if (loop == 0)
          sld_potential[L] = potential;  // bkz.cpp:567-571
        else if (potential >= sld_potential[L] || block_size >= n)
        {  // slide_tour returned clean (or one tour was all there is): the loop ends, RED_SUCCESS
          st[L]     = 1;
          active[L] = 0;
          continue;
        }
        else
          sld_potential[L] = potential;
      }
      if (use_loops && loop >= max_loops)
      {
        st[L]     = 8;
        active[L] = 0;
        continue;
      }
      if (hooks.use_time && hooks.seconds() >= hooks.max_time)
      {  // RED_BKZ_TIME_LIMIT, bkz.cpp:588-592
        st[L]     = 7;
        active[L] = 0;
        continue;
      }
      const int n = rows[L];
      if (slope_test)
      {
      double v1 = 0, v2 = (double)(n + 1) * n * (n - 1) / 12.0, weight = (1.0 - n) / 2.0;
      for (int i = 0; i < n; ++i)
      {
        const double logf = std::log(rdg[L * d + i]);
        const long expo   = (long)(2 * rex[L * d + i]);
        v1 += weight * (logf + expo * std::log(2.0));
        weight++;
      }
      const double new_slope = -(v1 / v2);
      if (no_dec[L] == -1 || new_slope < 1.0 * old_slope[L])
        no_dec[L] = 0;
      else
        no_dec[L]++;
      old_slope[L] = std::min(old_slope[L], new_slope);
      if (no_dec[L] >= 5)
      {
        active[L] = 0;  // abort: status stays RED_SUCCESS
        continue;
      }
      }
      ++n_active;
    }
    if (n_active == 0)
      break;
    GCHK(hipMemcpy(g->P.bkz_active, active.data(), sizeof(int) * B, hipMemcpyHostToDevice));
    for (size_t L = 0; L < B; ++L)
      ran[L] = active[L] ? 1 : 0;
    float ms = 0;
    rc       = run_tour(loop, &ms, s1.data(), one.data());
    if (rc != FPHIP_OK)
      return rc;
    total_ms += ms;
    for (size_t L = 0; L < B; ++L)
    {
      if (!active[L])
        continue;
      accumulate_info(inf.data(), one.data(), L);
      if (s1[L] == 8)
        continue;        // tour done, not clean: next loop
      st[L]     = s1[L];  // 1: clean (or block_size >= num_rows); <= 0: failure
      active[L] = 0;
    }
  }
  return FPHIP_OK;
}

// BKZParam::max_time (seconds) and BKZParam::dump_gso_filename (bkz_param.h:151,167) of the device BKZ drivers
extern "C" int fphip_gso_bkz_limits(fphip_gso *g, double max_time, const char *dump_gso_filename)
{
  if (!g)
    return FPHIP_ERROR;
  g->bkz_max_time = max_time;
  if (dump_gso_filename)
    g->bkz_dump_path = dump_gso_filename;
  return FPHIP_OK;
}

extern "C" int fphip_gso_bkz(fphip_gso *g, int block_size, double delta, double eta, int flags,
                             int max_loops, int *status, int *info)
{
  FPHIP_RANGE("fphip_gso_bkz");
  if (!g)
    return FPHIP_ERROR;
  if (block_size > 64 || (flags & ~(0x4 | 0x8 | 0x20 | 0x40 | 0x4000)))
    return FPHIP_UNSUPPORTED;  // blocks beyond one wavefront / other BKZ variants: fplll's CPU code
  // FPHIP_BKZ_TRANSFORM (0x4000): bkz_kernel_u keeps u in step with b (without it a tracked u is refused, bkz_launch)
  int rc = bkz_transform_begin(g, (flags & 0x4000) != 0, "bkz");
  if (rc != FPHIP_OK)
    return rc;
  BkzTransformScope u_scope{g};
  flags &= ~0x4000;
  rc = ensure_lll_buffers(g);
  if (rc != FPHIP_OK)
    return rc;
  const size_t B = (size_t)g->P.batch, d = g->P.d;
  if (!g->P.enum_mu)
    GCHK(fphip_dev_alloc((void **)&g->P.enum_mu, B * (64 * 63 / 2) * sizeof(double), fphip_ctx_stream(g->ctx)));
  if (!g->P.bkz_active)
    GCHK(fphip_dev_alloc((void **)&g->P.bkz_active, B * sizeof(int), fphip_ctx_stream(g->ctx)));
  if (!g->P.bkz_rows)
    GCHK(fphip_dev_alloc((void **)&g->P.bkz_rows, B * sizeof(int), fphip_ctx_stream(g->ctx)));
  std::vector<int> active(B, 1), st(B, 1), inf(4 * B, 0), one(4 * B), rows(B, (int)d);
  GCHK(hipMemcpy(g->P.bkz_active, active.data(), sizeof(int) * B, hipMemcpyHostToDevice));
  rc = launch(g, 0, g->P.d, 0.0, 2);  // bf / row_expo of every row from b
  if (rc != FPHIP_OK)
    return rc;
  const bool use_loops = (flags & 0x4) != 0, auto_abort = (flags & 0x20) != 0;
  // BKZ_MAX_TIME (0x8) / BKZ_DUMP_GSO (0x40), fplll's values: one tour per launch, the clock and the dump in between
  TourHooks hooks;
  hooks.use_time = (flags & 0x8) != 0;
  hooks.dump     = (flags & 0x40) != 0;
  hooks.max_time = g->bkz_max_time;
  float total_ms = 0, ms = 0;
  if (!auto_abort && !hooks.use_time && !hooks.dump)
  {
    rc = bkz_launch(g, block_size, delta, eta, use_loops ? 1 : 0, max_loops, &ms, st.data(), inf.data());
    if (rc != FPHIP_OK)
      return rc;
    total_ms = ms;
  }
  else
  {
    rc = auto_abort_loop(g, block_size, use_loops, max_loops, active, st, inf, rows, total_ms,
                         [&](int, float *tms, int *s1, int *one)
                         { return bkz_launch(g, block_size, delta, eta, 1, 1, tms, s1, one); },
                         auto_abort, false, hooks);
    if (rc == FPHIP_OK && hooks.dump)
      rc = dump_gso_output(g, hooks, st, rows);
    if (rc != FPHIP_OK)
      return rc;
  }
  g->last_ms = total_ms;
  if (status)
    memcpy(status, st.data(), sizeof(int) * B);
  if (info)
    memcpy(info, inf.data(), sizeof(int) * 4 * B);
  return FPHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// BKZ with strategies: BKZReduction::bkz() with a BKZParam(block_size, strategies, delta, flags,
// max_loops, ..., gh_factor) — recursive preprocessing tours, pruning sets chosen by the radius /
// Gaussian-heuristic ratio, the GH radius bound, the success-probability loop with
// rerandomize_block (bkz.cpp:43-124, 274-441, 522-668).  The wave of each lattice runs the whole
// reduction (bkzs_kernel.hip); this thread serves its mailbox requests while the kernel is in
// flight: the radius / pruning decision (host libm: log, exp, lgamma, pow — the reference's own
// roundings) and the rerandomisation plan (drawn from the caller's generator, rnd(user, lattice,
// n) = gmp_urandomm_ui(state of that lattice, n)).
#include <atomic>
#include <functional>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
static inline void *pinned_get(size_t bytes) { return fphip_pinned_get(bytes); }
static inline void pinned_put(void *p) { fphip_pinned_put(p); }

// ---------------------------------------------------------------------------------------------
namespace
{
// adjust_radius_to_gh_bound, gso_interface.cpp:260-276
void adjust_radius_to_gh_bound(double &max_dist, long max_dist_expo, int block_size, double root_det,
                               double gh_factor)
{
  double t = (double)block_size / 2.0 + 1;
  t        = lgamma(t);
  t        = pow(M_E, t * 2.0 / (double)block_size);
  t        = t / M_PI;
  double f = t;
  f        = f * root_det;
  f        = std::ldexp(f, (int)-max_dist_expo);
  f        = f * gh_factor;
  if (f < max_dist)
    max_dist = f;
}

struct BkzsHost
{
  const fphip_strategies *S;
  double gh_factor;
  fphip_rand_fn rnd;
  void *rnd_user;
  double handoff_nodes;  // > 0: blocks above that many estimated nodes go to the multi-wave enumerator
  // in-loop pruning: blocks of the top-level tour of at least il_min_block rows get coefficients from
  // prune() on their own r-profile instead of a set of the strategies table
  int inloop           = 0;
  double il_preproc    = 0, il_target = 0;
  int il_min_block     = 0, il_flags = 0;
  std::atomic<int> *il_errors = nullptr;  // prune() calls that failed for another reason than the profile
};
// the blocks in-loop pruning applies to: primal blocks of the top-level tour (not of a preprocessing
// tour: 0x10000, not dual: 0x20000)
static inline bool inloop_block(const BkzsHost &H, const BkzMail *m)
{
  return H.inloop && m->type == 1 && !(m->flags & 0x30000) && m->bs >= H.il_min_block && m->bs >= 4;
}

// Gaussian-heuristic size of the pruned tree of a block (what enum_host.hip's estimate_levels
// computes, in logarithms: the r_ii carry their row exponents here): sum over the levels k of
// 1/2 V_{bs-k}(R_k) / prod_{i>=k} sqrt(r_ii), R_k^2 = pruning_k * radius.  Scheduling only.
double estimate_block_nodes(int bs, const double *logr, double log_radius, const double *prune)
{
  double sumlog = 0.0, tot = 0.0;
  for (int k = bs - 1; k >= 0; --k)
  {
    sumlog += 0.5 * logr[k];
    const int n       = bs - k;
    const double logV = 0.5 * n * std::log(M_PI) - std::lgamma(0.5 * n + 1.0);
    const double pr   = prune ? prune[k] : 1.0;
    tot += std::exp(std::min(std::log(0.5) + logV + 0.5 * n * (std::log(pr > 0 ? pr : 1e-300) + log_radius) - sumlog, 80.0));
  }
  return tot;
}

// type 1: radius (bkz.cpp:309-323) and pruning set (get_pruning :82-98, Strategy::get_pruning
// bkz_param.cpp:64-80) of the block whose r_ii the wave has written
void serve_radius(const BkzsHost &H, BkzMail *m, fphip_pruner::VolumeEngine *engine = nullptr)
{
  const int bs      = m->bs;
  const bool dual   = (m->flags & 0x20000) != 0;  // a dual block of self-dual BKZ (bkzs_kernel.hip, DUALS)
  long expo         = m->e2[0];
  const double r0   = m->r[0];
  double max_dist   = r0;
  if (dual)
  {  // radius from the LAST row: max_dist.pow_si(max_dist, -1); max_dist_expo *= -1, bkz.cpp:311-316
    max_dist = ::pow(m->r[bs - 1], static_cast<double>(-1));
    expo     = -(long)m->e2[bs - 1];
  }
  max_dist = max_dist * m->delta;  // max_dist *= delta
  const long expo0 = m->e2[0];     // get_pruning always looks at r(kappa, kappa), bkz.cpp:89-97
  // MatGSOInterface::get_root_det / get_log_det, gso_interface.cpp:220-242
  double log_det = 0.0;
  for (int i = 0; i < bs; ++i)
  {
    const double h = std::ldexp(m->r[i], m->e2[i]);  // get_r(h, i, i)
    log_det += std::log(h);
  }
  double root_det = log_det / (double)bs;
  root_det        = std::exp(root_det);
  if ((m->flags & 0x80) && bs > 30)
    adjust_radius_to_gh_bound(max_dist, expo, bs, root_det,
                              (m->flags & 0x10000) ? 1.1 /* BKZ_DEF_GH_FACTOR of a preprocessing BKZParam */ : H.gh_factor);
  int best           = -1;
  double expectation = 1.0;
  if (H.S)
  {
    double gh_max_dist = r0;
    adjust_radius_to_gh_bound(gh_max_dist, expo0, bs, root_det, 1.0);
    const double radius    = r0 * pow(2, expo0);
    const double gh        = gh_max_dist * pow(2, expo0);
    const double gh_factor = radius / gh;
    double closest         = pow(2, 80);
    best                   = H.S->prune_off[bs];
    for (int p = H.S->prune_off[bs]; p < H.S->prune_off[bs + 1]; ++p)
      if (fabs(H.S->prune_gh[p] - gh_factor) < closest)
      {
        closest = fabs(H.S->prune_gh[p] - gh_factor);
        best    = p;
      }
    expectation = H.S->prune_exp[best];
  }
  const double *inloop_pr = nullptr;
  if (inloop_block(H, m))
  {
    // Pruning chosen where the reference chooses it (bkz.cpp:325, after the preprocessing and the radius)
    // — but computed for THIS block: prune<FP_NR<double>>(radius, preproc_cost, r_ii of the block, target,
    // PROBABILITY_OF_SHORTEST, flags) (pruner.h:187-193) on the profile the wave has just sent; the
    // strategies' set stays in force if the pruner fails (a degenerate profile)
    double rr[64], co[64], ex = 1.0;
    for (int i = 0; i < bs; ++i)
      rr[i] = std::ldexp(m->r[i], m->e2[i]);
    const double radius = max_dist * pow(2, expo);
    int prc = FPHIP_UNSUPPORTED;
    if (std::isfinite(radius) && radius > 0)
    {
      prc = fphip_pruner::prune_block(engine, bs, rr, radius, H.il_preproc, H.il_target, H.il_flags, co, &ex);
      // a device engine that failed (its message is in error()) is not a degenerate profile: the call reports it
      if (prc != FPHIP_OK && engine && engine->error()[0] && H.il_errors)
        H.il_errors->fetch_add(1);
    }
    if (prc == FPHIP_OK)
    {
      for (int i = 0; i < bs; ++i)
        m->prn[i] = co[i];
      best        = -2;  // "the coefficients are in the mailbox"
      expectation = ex;
      inloop_pr   = m->prn;
    }
  }
  m->max_dist    = max_dist;
  m->expectation = expectation;
  m->prune       = best;
  m->handoff     = 0;
  if (H.handoff_nodes > 0 && bs >= 24)
  {
    // the tree the wave is about to walk: primal block r_ii 2^e2_i, radius max_dist 2^expo; a dual
    // block is the index-reversed inverse (enumerate.cpp:107-123)
    double logr[64];
    for (int i = 0; i < bs; ++i)
    {
      const double lr = std::log(m->r[i]) + m->e2[i] * M_LN2;
      if (dual)
        logr[bs - 1 - i] = -lr;
      else
        logr[i] = lr;
    }
    const double *pr = inloop_pr;
    if (H.S && best >= 0 && H.S->coeff_off[best + 1] - H.S->coeff_off[best] == bs)
      pr = H.S->coeff + H.S->coeff_off[best];
    // expected number of nodes of this enumeration: the pruner's cost function (pruner_host.hip:
    // Pruner::single_enum_cost, volumes of the cylinder intersections — what the reference's pruner
    // optimises); the plain Gaussian-heuristic sum (2-5x high on pruned trees) only if it fails
    double est = -1.0;
    {
      double rr[64], ones[64], cost = 0.0;
      for (int i = 0; i < bs; ++i)
      {
        rr[i]   = std::exp(logr[i]);
        ones[i] = 1.0;
      }
      const double radius = std::exp(std::log(max_dist) + expo * M_LN2);
      if (std::isfinite(radius) && fphip_pruner_enum_cost(bs, rr, radius, pr ? pr : ones, 0, &cost, nullptr, nullptr) == FPHIP_OK &&
          std::isfinite(cost))
        est = cost;
    }
    if (est < 0.0)
      est = 0.25 * estimate_block_nodes(bs, logr, std::log(max_dist) + expo * M_LN2, pr);
    m->handoff = est >= H.handoff_nodes ? 1 : 0;
  }
}

// type 3: the enumeration of a large block on the multi-wave enumerator (enum_host.hip) with
// FastEvaluator(1) semantics (evaluator.h:122-156, max_sols = 1: every delivered solution replaces
// the last one and becomes the radius).  Runs on the hand-off worker thread.
struct HandoffSol
{
  double sol[64];
  int have;
  int dim;
};
double handoff_cb(void *user, double dist, const double *sol)
{
  HandoffSol *h = static_cast<HandoffSol *>(user);
  for (int i = 0; i < h->dim; ++i)
    h->sol[i] = sol[i];
  h->have = 1;
  return dist;
}
int serve_enumeration(fphip_ctx *ectx, BkzMail *m, const double *mu_tri)
{
  const int bs = m->bs;
  std::vector<double> mut((size_t)bs * bs, 0.0);
  for (int k = 1; k < bs; ++k)
    for (int l = 0; l < k; ++l)
      mut[(size_t)l * bs + k] = mu_tri[(k * (k - 1)) / 2 + l];  // mut[i*dim + j] = mu(j, i), j > i
  HandoffSol hs;
  hs.have = 0;
  hs.dim  = bs;
  fphip_enum_opts o;
  memset(&o, 0, sizeof o);
  o.dual = m->dual3;
  std::vector<uint64_t> nodes(bs + 1, 0);
  fphip_enum_stats stt;
  memset(&stt, 0, sizeof stt);
  const int rc = fphip_enum_run(ectx, bs, m->maxdist3, mut.data(), m->rd, m->prn, &o, handoff_cb, nullptr, &hs,
                                nodes.data(), &stt);
  if (rc != FPHIP_OK)
    return rc;
  m->have_sol = hs.have;
  for (int i = 0; i < 64; ++i)
    m->sol[i] = (i < bs && hs.have) ? hs.sol[i] : 0.0;
  m->nodes3 = stt.total_nodes;
  return FPHIP_OK;
}

// type 2: the random choices of rerandomize_block(min_row, max_row, density), bkz.cpp:43-80 — they
// do not depend on the basis, so the whole call is drawn at once, in the reference's order
int serve_plan(const BkzsHost &H, int lattice, BkzMail *m)
{
  const int min_row = m->lo, max_row = m->hi, density = m->density;
  int np = 0, n_moves = 0, n_ops = 0;
  // (a range of exactly two rows makes the reference spin for ever — gmp_urandomm_ui(state, 1) is
  // always 0, so `while (b == a)` never ends, bkz.cpp:53-58; the block is left as it is instead)
  if (max_row - min_row > 2 && H.rnd)
  {
    const size_t niter = 4 * (size_t)(max_row - min_row);
    for (size_t i = 0; i < niter && np < FPHIP_BKZS_PLAN_MAX; ++i)
    {
      const size_t a = H.rnd(H.rnd_user, lattice, (unsigned long)(max_row - min_row - 1)) + min_row;
      size_t b       = a;
      // (the reference's loop is unbounded, bkz.cpp:56-57; a generator that keeps returning the
      // same value — e.g. the 0 a failed Python callback yields through ctypes — must not hang the
      // service thread with a kernel waiting on it: give up after 4096 equal draws)
      for (int tries = 0; b == a; ++tries)
      {
        if (tries >= 4096)
          return -1;
        b = H.rnd(H.rnd_user, lattice, (unsigned long)(max_row - min_row - 1)) + min_row;
      }
      m->plan[np++] = (unsigned)b | ((unsigned)a << 8);
      ++n_moves;
    }
    for (long a = min_row; a < max_row - 2; ++a)
      for (long i = 0; i < density && np < FPHIP_BKZS_PLAN_MAX; i++)
      {
        const size_t b = H.rnd(H.rnd_user, lattice, (unsigned long)(max_row - (a + 1) - 1)) + a + 1;
        const unsigned add = H.rnd(H.rnd_user, lattice, 2) ? 1u : 0u;
        m->plan[np++] = (unsigned)a | ((unsigned)b << 8) | (add << 16);
        ++n_ops;
      }
  }
  m->n_moves = n_moves;
  m->n_ops   = n_ops;
  return np;
}
}  // namespace

// The two host-side decisions on their own (no device involved): what the mailbox service answers
// for a block with the given r_ii / exponents, and the plan it draws for a rerandomisation.  Used by
// the CPU test-suite to check this arithmetic against the oracle (tests/test_bkzs_host_cpu.py).
extern "C" int fphip_debug_bkz_radius(const fphip_strategies *S, double gh_factor, int bs, int flags,
                                      double delta, const double *r, const int *e2, double *max_dist,
                                      int *prune, double *expectation)
{
  if (bs < 1 || bs > 64 || !r || !e2)
    return FPHIP_ERROR;
  BkzMail m;
  memset(&m, 0, sizeof m);
  m.type  = 1;
  m.bs    = bs;
  m.flags = flags;
  m.delta = delta;
  for (int i = 0; i < bs; ++i)
  {
    m.r[i]  = r[i];
    m.e2[i] = e2[i];
  }
  BkzsHost H{S, gh_factor, nullptr, nullptr};
  serve_radius(H, &m);
  if (max_dist)
    *max_dist = m.max_dist;
  if (prune)
    *prune = m.prune;
  if (expectation)
    *expectation = m.expectation;
  return FPHIP_OK;
}

extern "C" int fphip_debug_bkz_plan(fphip_rand_fn rnd, void *rnd_user, int lattice, int lo, int hi,
                                    int density, unsigned *plan, int *n_moves, int *n_ops)
{
  if (!rnd || !plan || hi - lo > 63)
    return FPHIP_ERROR;
  BkzMail m;
  memset(&m, 0, sizeof m);
  m.type    = 2;
  m.lo      = lo;
  m.hi      = hi;
  m.density = density;
  BkzsHost H{nullptr, 1.1, rnd, rnd_user};
  const int np = serve_plan(H, lattice, &m);
  memcpy(plan, m.plan, sizeof(unsigned) * (size_t)np);
  if (n_moves)
    *n_moves = m.n_moves;
  if (n_ops)
    *n_ops = m.n_ops;
  return FPHIP_OK;
}

// One pass of slide reduction on a subset of its (disjoint) blocks: the unit of the block-parallel mode
// (slide_tour's p primal blocks and p - 1 dual blocks, bkz.cpp:475-480, 495-499).
extern "C" int fphip_gso_slide_pass(fphip_gso *g, int block_size, double delta, double eta, int flags,
                                    double gh_factor, const fphip_strategies *S, fphip_rand_fn rnd, void *rnd_user,
                                    int pass, unsigned long long block_mask, int *status, int *info)
{
  if (!g || pass < 1 || pass > 3 || block_size < 2)
    return FPHIP_ERROR;
  if (int rct = transform_guard(g, "slide_pass"))
    return rct;
  // without BKZ_BOUNDED_LLL every svp_reduction starts with an LLL from row 0: the blocks of a pass are
  // not independent then (bkz.cpp:107-108)
  if (!(flags & 0x10))
    return FPHIP_UNSUPPORTED;
  // the block mask has 64 bits (advisor, round 4: a wider pass would silently reduce nothing)
  if ((g->P.d + block_size - 1) / block_size > 64)
    return FPHIP_UNSUPPORTED;
  g->P.sld_pass = pass;
  g->P.sld_mask = block_mask;
  const int rc  = fphip_gso_bkz_strategies(g, block_size, delta, eta, (flags & (0x10 | 0x80 | 0x2000)) | 0x4 | 0x200, 1,
                                           gh_factor, S, rnd, rnd_user, status, info);
  g->P.sld_pass = 0;
  g->P.sld_mask = 0;
  return rc;
}

// The block-parallel slide TOUR over several batch-of-one objects (one per context / device), host threads in
// this process: what fplll_amd.distributed.slide_reduction_blocks does with LocalGather, behind the C ABI so
// that a C++ caller (an fplll process that holds several devices) needs no Python.  Same calls in the same
// order per participant, hence the same result: block i of a pass is reduced by gs[i % count] from the
// pass-start basis, the merged basis replaces every copy, the bounded LLL / the potential test / the closing
// hkz run on every copy alike.
extern "C" int fphip_gso_slide_reduction_blocks(fphip_gso **gs, int count, int block_size, double delta, double eta,
                                                int flags, int max_loops, double gh_factor,
                                                const fphip_strategies *S, fphip_rand_fn rnd, void *rnd_user,
                                                int *status, unsigned long long *nodes_out, int *tours_out)
{
  if (!gs || count < 1 || block_size < 2)
    return FPHIP_ERROR;
  for (int r = 0; r < count; ++r)
    if (!gs[r] || gs[r]->P.batch != 1 || gs[r]->P.d != gs[0]->P.d || gs[r]->P.n != gs[0]->P.n)
      return FPHIP_ERROR;
  if (!(flags & 0x10))
    return FPHIP_UNSUPPORTED;  // the blocks of a pass are independent only with BKZ_BOUNDED_LLL
  // A caller generator cannot be shared by the participants: the host threads would race on its state, and
  // every copy / rank would consume a different number of draws, so that the closing hkz's rerandomisations
  // (and with them the result) would depend on the number of devices (advisor, round 4).  The block-parallel
  // tour is defined for the deterministic case — no rerandomisation: rnd == NULL.
  if (rnd)
    return FPHIP_UNSUPPORTED;
  const int d = gs[0]->P.d, n = gs[0]->P.n;
  const int p = (d + block_size - 1) / block_size;
  if (p > 64)
    return FPHIP_UNSUPPORTED;  // 64-bit block masks
  // the GSO entry points launch on the calling thread's current device: gs[0]'s while this thread uses it
  int caller_dev0 = 0;
  (void)hipGetDevice(&caller_dev0);
  (void)hipSetDevice(fphip_ctx_device(gs[0]->ctx));
  struct RestoreDev
  {
    int dev;
    ~RestoreDev() { (void)hipSetDevice(dev); }
  } restore_dev{caller_dev0};
  struct Blk
  {
    int lo, hi;
  };
  std::vector<Blk> primal, dual;
  for (int i = 0; i < p; ++i)
    primal.push_back(Blk{i * block_size, std::min(d, (i + 1) * block_size)});
  for (int i = 0; i + 1 < p; ++i)
    dual.push_back(Blk{i * block_size + 1, (i + 1) * block_size + 1});
  const size_t rowsz = (size_t)n;
  std::vector<int64_t> start((size_t)d * n), merged((size_t)d * n);
  std::atomic<int> failed{0};
  unsigned long long total_nodes = 0;
  // every participant on a thread of its own: f(r) for r = 0 .. count-1
  int caller_dev = 0;
  (void)hipGetDevice(&caller_dev);
  auto on_all = [&](const std::function<void(int)> &f)
  {
    // (the GSO entry points launch on their context's stream with the calling thread's current device:
    //  every thread selects its object's device first)
    auto on_dev = [&](int r)
    {
      (void)hipSetDevice(fphip_ctx_device(gs[r]->ctx));
      f(r);
    };
    std::vector<std::thread> ts;
    for (int r = 1; r < count; ++r)
      ts.emplace_back(on_dev, r);
    on_dev(0);
    for (auto &t : ts)
      t.join();
    (void)hipSetDevice(caller_dev);
  };
  auto set_all = [&](const std::vector<int64_t> &b)
  {
    on_all([&](int r)
           {
             if (fphip_gso_set_basis(gs[r], 0, 1, b.data()) != FPHIP_OK || fphip_gso_refresh(gs[r]) != FPHIP_OK)
               failed = 1;
           });
  };
  auto run_pass = [&](int pass, const std::vector<Blk> &layout, bool &clean) -> unsigned long long
  {
    if (fphip_gso_get_basis(gs[0], 0, 1, start.data()) != FPHIP_OK)
      failed = 1;
    merged = start;
    std::atomic<int> all_clean{1};
    std::atomic<unsigned long long> nd{0};
    on_all([&](int r)
           {
             std::vector<int64_t> mine((size_t)d * n);
             for (int i = r; i < (int)layout.size(); i += count)
             {
               int st = 0, info[4] = {0, 0, 0, 0};
               if (fphip_gso_set_basis(gs[r], 0, 1, start.data()) != FPHIP_OK || fphip_gso_refresh(gs[r]) != FPHIP_OK ||
                   fphip_gso_slide_pass(gs[r], block_size, delta, eta, flags & (0x10 | 0x80 | 0x2000), gh_factor, S, rnd,
                                        rnd_user, pass, 1ull << i, &st, info) != FPHIP_OK ||
                   st <= 0 || fphip_gso_get_basis(gs[r], 0, 1, mine.data()) != FPHIP_OK)
               {
                 failed = 1;
                 return;
               }
               // (the blocks of a pass are disjoint row ranges: no two threads write the same rows)
               memcpy(&merged[(size_t)layout[i].lo * rowsz], &mine[(size_t)layout[i].lo * rowsz],
                      sizeof(int64_t) * rowsz * (size_t)(layout[i].hi - layout[i].lo));
               if (pass == 1 && !info[0])
                 all_clean = 0;
               nd += ((unsigned long long)(unsigned)info[2] << 32) | (unsigned)info[1];
             }
           });
    set_all(merged);
    clean = all_clean.load() != 0;
    return nd.load();
  };
  auto potential = [&]() -> double
  {
    int st = 0;
    std::vector<double> rm((size_t)d * d), diag(d);
    std::vector<int64_t> re(d);
    if (fphip_gso_update(gs[0], &st) != FPHIP_OK || st != 1 || fphip_gso_get_r(gs[0], 0, rm.data()) != FPHIP_OK ||
        fphip_gso_get_row_expo(gs[0], 0, re.data()) != FPHIP_OK)
    {
      failed = 1;
      return 0.0;
    }
    for (int i = 0; i < d; ++i)
      diag[i] = rm[(size_t)i * d + i];
    return fphip_gso_util_slide_potential(diag.data(), re.data(), d, 0, d, block_size);
  };
  int st_out = 1, tours = 0;
  double old = potential();
  while (!failed)
  {
    if (max_loops > 0 && tours >= max_loops)
    {
      st_out = 8;  // RED_BKZ_LOOPS_LIMIT
      break;
    }
    for (;;)
    {  // primal passes until one leaves every block, and the bounded LLL, unchanged (bkz.cpp:472-494)
      bool clean = true;
      total_nodes += run_pass(1, primal, clean);
      if (failed)
        break;
      std::atomic<int> lll_bad{0}, swaps{0};
      on_all([&](int r)
             {
               int st = 0, info[4] = {0, 0, 0, 0};
               if (fphip_gso_lll(gs[r], 0, 0, d, delta, eta, &st, info) != FPHIP_OK)
                 failed = 1;
               else if (st != 1)
                 lll_bad = st == 0 ? -100 : st;
               if (r == 0)
                 swaps = info[1];
             });
      if (failed)
        break;
      if (lll_bad.load())
      {
        st_out = lll_bad.load() == -100 ? 0 : lll_bad.load();
        failed = 2;  // (a reduction status, not a device error)
        break;
      }
      if (swaps.load() > 0)
        clean = false;
      if (clean)
        break;
    }
    if (failed)
      break;
    if (!dual.empty())
    {
      bool unused = true;
      total_nodes += run_pass(2, dual, unused);
      if (failed)
        break;
    }
    ++tours;
    const double now = potential();
    if (failed || now >= old || block_size >= d)
      break;
    old = now;
  }
  if (failed == 1)
  {
    snprintf(fphip_ctx_errbuf(gs[0]->ctx), 512, "fphip_gso_slide_reduction_blocks: a pass failed: %s",
             fphip_last_error(gs[0]->ctx));
    return FPHIP_ERROR;
  }
  if (failed == 0)
  {  // the closing hkz of every block (bkz.cpp:643-660) on every copy alike; counted once
    std::atomic<int> bad{0};
    std::atomic<unsigned long long> nd{0};
    on_all([&](int r)
           {
             int st = 0, info[4] = {0, 0, 0, 0};
             if (fphip_gso_slide_pass(gs[r], block_size, delta, eta, flags & (0x10 | 0x80 | 0x2000), gh_factor, S, rnd,
                                      rnd_user, 3, 0, &st, info) != FPHIP_OK)
               bad = 1;
             else if (r == 0)
             {
               nd = ((unsigned long long)(unsigned)info[2] << 32) | (unsigned)info[1];
               if (st <= 0)
                 bad = 2 + (st == 0 ? 100 : -st);
             }
           });
    if (bad.load() == 1)
      return FPHIP_ERROR;
    total_nodes += nd.load();
    if (bad.load() >= 2)
      st_out = bad.load() - 2 == 100 ? 0 : -(bad.load() - 2);
  }
  if (status)
    *status = st_out;
  if (nodes_out)
    *nodes_out = total_nodes;
  if (tours_out)
    *tours_out = tours;
  return FPHIP_OK;
}

extern "C" int fphip_gso_bkz_inloop_pruning(fphip_gso *g, double preproc_cost, double target, int min_block_size,
                                            int pruner_flags, int on_device)
{
  if (!g || !(target > 0.0 && target < 1.0) || !(preproc_cost >= 0.0) || (pruner_flags & 0x10))
    return FPHIP_ERROR;
  g->il_preproc   = preproc_cost;
  g->il_target    = target;
  g->il_min_block = min_block_size;
  g->il_flags     = pruner_flags;
  g->il_device    = on_device ? 1 : 0;
  return FPHIP_OK;
}
extern "C" int fphip_gso_bkz_inloop_stats(const fphip_gso *g, unsigned long long *prune_calls,
                                          unsigned long long *device_jobs, unsigned long long *host_jobs,
                                          unsigned long long *launches)
{
  if (!g)
    return FPHIP_ERROR;
  if (prune_calls)
    *prune_calls = g->il_calls;
  if (device_jobs)
    *device_jobs = g->il_device_jobs;
  if (host_jobs)
    *host_jobs = g->il_host_jobs;
  if (launches)
    *launches = g->il_launches;
  return FPHIP_OK;
}

// What the kernel can run of the caller's strategies up to block size bsz: FPHIP_OK, FPHIP_UNSUPPORTED (the caller
// keeps these on fplll's CPU path) or FPHIP_ERROR with its text
static int check_strategies(fphip_ctx *ctx, const fphip_strategies *S, fphip_rand_fn rnd, int bsz)
{
  if (!rnd)
  {
    snprintf(fphip_ctx_errbuf(ctx), 512, "fphip_gso_bkz_strategies: strategies need the caller's generator");
    return FPHIP_ERROR;
  }
  if (S->max_block_size < bsz || !S->pre_off || !S->prune_off || !S->coeff_off)
  {
    snprintf(fphip_ctx_errbuf(ctx), 512, "fphip_gso_bkz_strategies: strategies do not cover block size %d", bsz);
    return FPHIP_ERROR;
  }
  // every block size needs a pruning set whose coefficient vector is empty or of that size;
  // preprocessing block sizes must be proper (2 <= p < b) and nest at most MAX_DEPTH - 1 deep
  std::vector<int> depth(bsz + 1, 0);
  for (int b = 0; b <= bsz; ++b)
  {
    if (S->prune_off[b + 1] <= S->prune_off[b])
      return FPHIP_UNSUPPORTED;
    for (int p = S->prune_off[b]; p < S->prune_off[b + 1]; ++p)
    {
      const int len = S->coeff_off[p + 1] - S->coeff_off[p];
      if (len != 0 && len != b)
        return FPHIP_UNSUPPORTED;
    }
    for (int p = S->pre_off[b]; p < S->pre_off[b + 1]; ++p)
    {
      const int pb = S->pre[p];
      if (pb < 2 || pb >= b)
        return FPHIP_UNSUPPORTED;
      // a tour of block size pb reaches every block size <= pb through hkz
      int dmax = 0;
      for (int c = 2; c <= pb; ++c)
        dmax = std::max(dmax, depth[c]);
      depth[b] = std::max(depth[b], dmax + 1);
    }
  }
  int dtop = 0;
  for (int b = 2; b <= bsz; ++b)
    dtop = std::max(dtop, depth[b]);
  if (dtop + 1 > FPHIP_BKZS_MAX_DEPTH)
    return FPHIP_UNSUPPORTED;
  return FPHIP_OK;
}

// One launch of the strategy kernel the call needs — with u or without, the self-dual / slide variant (dual) or the
// primal one — at the geometry fphip_gso_bkz_strategies worked out; the kernel is first allowed its dynamic LDS where
// that exceeds the default limit.  The caller records the events around it and reads hipGetLastError().
struct BkzsGeometry
{
  int nq, wpb, grid, stack_doubles, mu_lds_flag;
  size_t lds;
};
static hipError_t bkzs_launch(fphip_gso *g, const BkzsGeometry &geo, hipStream_t s, bool sd, bool sld,
                              const BkzStrat &DS, BkzMail *mail, int *d_abort, int block_size, int kflags,
                              double delta, double eta, double logd, int kloops, int run_mode)
{
  const int nq = geo.nq, wpb = geo.wpb, grid = geo.grid, stack_doubles = geo.stack_doubles, mu_lds_flag = geo.mu_lds_flag;
  const size_t lds = geo.lds;
  const bool big = lds > 64 * 1024;
  unsigned long long *us = g->bkz_stats_d;
  hipError_t e = hipSuccess;
  if (g->bkz_u && (sd || sld))
    dispatch_nq(nq, [&](auto NQ) {
      if (!big || (e = allow_lds(sdv::bkzd_kernel_u<NQ>, lds)) == hipSuccess)
        hipLaunchKernelGGL(sdv::bkzd_kernel_u<NQ>, dim3(grid), dim3(wpb * 64), lds, s, g->P, DS, mail, d_abort, block_size, kflags | (sd ? 0x100 : 0) | mu_lds_flag, delta, eta, logd, kloops, stack_doubles, run_mode, us);
    });
  else if (g->bkz_u)
    dispatch_nq(nq, [&](auto NQ) {
      if (!big || (e = allow_lds(bkzs_kernel_u<NQ>, lds)) == hipSuccess)
        hipLaunchKernelGGL(bkzs_kernel_u<NQ>, dim3(grid), dim3(wpb * 64), lds, s, g->P, DS, mail, d_abort, block_size, kflags | mu_lds_flag, delta, eta, logd, kloops, stack_doubles, us);
    });
  else if (sd || sld)
    dispatch_nq(nq, [&](auto NQ) {
      if (!big || (e = allow_lds(sdv::bkzd_kernel<NQ>, lds)) == hipSuccess)
        hipLaunchKernelGGL(sdv::bkzd_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, g->P, DS, mail, d_abort, block_size, kflags | (sd ? 0x100 : 0) | mu_lds_flag, delta, eta, logd, kloops, stack_doubles, run_mode);
    });
  else
    dispatch_nq(nq, [&](auto NQ) {
      if (!big || (e = allow_lds(bkzs_kernel<NQ>, lds)) == hipSuccess)
        hipLaunchKernelGGL(bkzs_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, g->P, DS, mail, d_abort, block_size, kflags | mu_lds_flag, delta, eta, logd, kloops, stack_doubles);
    });
  return e;
}

extern "C" int fphip_gso_bkz_strategies(fphip_gso *g, int block_size, double delta, double eta,
                                        int flags, int max_loops, double gh_factor,
                                        const fphip_strategies *S, fphip_rand_fn rnd, void *rnd_user,
                                        int *status, int *info)
{
  if (g)
    if (int rcg = session_guard(g, "bkz_strategies"))
      return rcg;
  if (g && !(flags & 0x4000))
    if (int rct = transform_guard(g, "bkz_strategies"))
      return rct;
  FPHIP_RANGE("fphip_gso_bkz_strategies");
  if (!g)
    return FPHIP_ERROR;
  // one wavefront enumerates a block: sizes up to 64; BKZ_MAX_LOOPS, BKZ_BOUNDED_LLL, BKZ_AUTO_ABORT,
  // BKZ_GH_BND
  // BKZ_SD_VARIANT (0x100): self-dual BKZ, bkzs_body<NQ, true>
  const bool sd  = (flags & 0x100) != 0;
  const bool sld = (flags & 0x200) != 0;  // BKZ_SLD_RED: slide reduction (slide_tour, bkz.cpp:465-520)
  if (block_size > 64 ||
      (flags & ~(0x4 | 0x8 | 0x10 | 0x20 | 0x40 | 0x80 | 0x100 | 0x200 | 0x1000 | 0x2000 | 0x4000)) || (sd && sld))
    return FPHIP_UNSUPPORTED;
  // FPHIP_BKZ_TRANSFORM (0x4000): bkzs_kernel_u / bkzd_kernel_u keep u in step with b
  if (int rcu = bkz_transform_begin(g, (flags & 0x4000) != 0, "bkz_strategies"))
    return rcu;
  BkzTransformScope u_scope{g};
  flags &= ~0x4000;
  // BKZ_MAX_TIME (0x8) / BKZ_DUMP_GSO (0x40): one tour per launch, the clock and the dump on the host in between
  TourHooks hooks;
  hooks.use_time = (flags & 0x8) != 0;
  hooks.dump     = (flags & 0x40) != 0;
  hooks.max_time = g->bkz_max_time;
  hooks.step     = sd ? "End of SD-BKZ loop" : (sld ? "End of SLD loop" : "End of BKZ loop");
  flags &= ~(0x8 | 0x40);
  // FPHIP_BKZ_PRUNE_IN_LOOP (0x2000): pruning per block from the mailbox service (serve_radius)
  const bool inloop = (flags & 0x2000) != 0;
  flags &= ~0x2000;
  // (a last block of one row — d = k bs + 1 — would be an svp_reduction of block size 1: not offered)
  if (sld && block_size >= 2 && g->P.d % block_size == 1)
    return FPHIP_UNSUPPORTED;
  // FPHIP_BKZ_HANDOFF (0x1000, or FPHIP_BKZ_HANDOFF=1 in the environment): blocks whose tree is large
  // are enumerated by the multi-wave enumerator on a second context instead of by the lattice's wave
  const bool handoff = (flags & 0x1000) != 0 || (getenv("FPHIP_BKZ_HANDOFF") && atoi(getenv("FPHIP_BKZ_HANDOFF")) != 0);
  flags &= ~0x1000;
  if (sd && !(flags & (0x4 | 0x20)) && !hooks.use_time)
    flags |= 0x20;  // "SD Variant of BKZ requires explicit termination condition", bkz.cpp:548-554
  const int bsz = block_size < g->P.d ? block_size : g->P.d;
  if (S)
    if (int rcs = check_strategies(g->ctx, S, rnd, bsz))
      return rcs;
  int rc = ensure_lll_buffers(g);
  if (rc != FPHIP_OK)
    return rc;
  const size_t B = (size_t)g->P.batch;
  if (!g->P.enum_mu)
    GCHK(fphip_dev_alloc((void **)&g->P.enum_mu, B * (64 * 63 / 2) * sizeof(double), fphip_ctx_stream(g->ctx)));
  if (!g->P.bkz_active)
    GCHK(fphip_dev_alloc((void **)&g->P.bkz_active, B * sizeof(int), fphip_ctx_stream(g->ctx)));
  if (!g->P.bkz_rows)
    GCHK(fphip_dev_alloc((void **)&g->P.bkz_rows, B * sizeof(int), fphip_ctx_stream(g->ctx)));

  // device copy of what the kernel reads of the strategies; mailboxes; abort flag
  BkzStrat DS;
  memset(&DS, 0, sizeof DS);
  int *d_pre_off = nullptr, *d_pre = nullptr, *d_coeff_off = nullptr, *d_abort = nullptr;
  double *d_coeff = nullptr;
  BkzMail *mail   = nullptr;
  std::vector<fphip_pruner::VolumeEngine *> il_engines;  // in-loop pruning: one volume engine per service worker
  auto cleanup = [&]()
  {
    for (auto *x : il_engines)  // (every error return goes through here: streams and pinned staging go with it)
      fphip_pruner::destroy_volume_engine(x);
    il_engines.clear();
    fphip_dev_free(d_pre_off, fphip_ctx_stream(g->ctx));
    fphip_dev_free(d_pre, fphip_ctx_stream(g->ctx));
    fphip_dev_free(d_coeff_off, fphip_ctx_stream(g->ctx));
    fphip_dev_free(d_coeff, fphip_ctx_stream(g->ctx));
    fphip_dev_free(d_abort, fphip_ctx_stream(g->ctx));
    if (mail)
      pinned_put(mail);
    if (g->P.enum_mu_h)
    {
      pinned_put(g->P.enum_mu_h);
      g->P.enum_mu_h = nullptr;
    }
  };
#define BCHK(call)                         \
  do                                       \
  {                                        \
    hipError_t e_ = (call);                \
    if (e_ != hipSuccess)                  \
    {                                      \
      cleanup();                           \
      return fail(g->ctx, #call, e_);     \
    }                                      \
  } while (0)
  if (S)
  {
    const int nb   = S->max_block_size + 2;
    const int npre = S->pre_off[S->max_block_size + 1];
    const int nset = S->prune_off[S->max_block_size + 1];
    const int ncoe = S->coeff_off[nset];
    BCHK(fphip_dev_alloc((void **)&d_pre_off, sizeof(int) * nb, fphip_ctx_stream(g->ctx)));
    BCHK(fphip_dev_alloc((void **)&d_pre, sizeof(int) * (npre > 0 ? npre : 1), fphip_ctx_stream(g->ctx)));
    BCHK(fphip_dev_alloc((void **)&d_coeff_off, sizeof(int) * (nset + 1), fphip_ctx_stream(g->ctx)));
    BCHK(fphip_dev_alloc((void **)&d_coeff, sizeof(double) * (ncoe > 0 ? ncoe : 1), fphip_ctx_stream(g->ctx)));
    BCHK(hipMemcpy(d_pre_off, S->pre_off, sizeof(int) * nb, hipMemcpyHostToDevice));
    if (npre > 0)
      BCHK(hipMemcpy(d_pre, S->pre, sizeof(int) * npre, hipMemcpyHostToDevice));
    BCHK(hipMemcpy(d_coeff_off, S->coeff_off, sizeof(int) * (nset + 1), hipMemcpyHostToDevice));
    if (ncoe > 0)
      BCHK(hipMemcpy(d_coeff, S->coeff, sizeof(double) * ncoe, hipMemcpyHostToDevice));
    DS.max_block_size = S->max_block_size;
    DS.pre_off        = d_pre_off;
    DS.pre            = d_pre;
    DS.coeff_off      = d_coeff_off;
    DS.coeff          = d_coeff;
  }
  BCHK(fphip_dev_alloc((void **)&d_abort, sizeof(int), fphip_ctx_stream(g->ctx)));  // (cleared before every launch)
  mail = (BkzMail *)pinned_get(B * sizeof(BkzMail));
  if (!mail)
  {
    cleanup();
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "bkz_strategies: no pinned memory for %zu mailboxes", B);
    return FPHIP_ERROR;
  }
  memset(mail, 0, B * sizeof(BkzMail));

  const int need = (g->P.d > g->P.n ? g->P.d : g->P.n);
  const int nq   = (need + 63) / 64;
  int wpb        = g->waves_per_block;
  const int bs   = block_size < 2 ? 2 : bsz;
  size_t ring_bytes = (size_t)wpb * fphip_reduce_ring_bytes(nq);
  // The scaled mu rows of the block under enumeration go to LDS (behind the column stack) when few
  // lattices share a CU — every row's L1 latency is exposed to a lone wave — and when they fit;
  // large batches keep them in global memory and spend the LDS on resident waves.
  int stack_doubles = (bs * (bs + 1)) / 2 + 2;
  int mu_lds_flag   = 0;
  {
    const int with_mu  = stack_doubles + (bs * (bs - 1)) / 2;
    const size_t lds_m = ring_bytes + (size_t)wpb * with_mu * sizeof(double) + (size_t)wpb * FPHIP_BKZS_MAX_DEPTH * 64;
    const int def      = (B <= (size_t)4 * (size_t)fphip_ctx_num_cus(g->ctx)) ? 1 : 0;
    const char *e      = getenv("FPHIP_BKZ_MU_LDS");
    if ((e ? atoi(e) : def) && lds_m <= 160 * 1024)
    {
      stack_doubles = with_mu;
      mu_lds_flag   = 0x40000000;
    }
  }
  // A big batch of lattices of at most 64 columns (primal schedule): bkzs_kernel<1> is built for two waves per SIMD
  // (256 registers), and what then bounds the resident waves is the LDS per workgroup — ring + column stack, 22.6 KB
  // per wave for blocks of 40: one workgroup of four waves per CU, but three of two.  Measured (call r5z3, BKZ-40 on
  // 64-dim lattices): 327 reductions/s with four waves per workgroup, 397-399 with two (1536 / 3072 lattices); one
  // wave per workgroup: 259.
  if (nq == 1 && !sd && !sld && !mu_lds_flag && !getenv("FPHIP_GSO_WAVES_PER_BLOCK") && wpb == 4)
  {
    const size_t per_wave = fphip_reduce_ring_bytes(nq) + (size_t)stack_doubles * sizeof(double) + FPHIP_BKZS_MAX_DEPTH * 64;
    if ((160 * 1024) / (4 * per_wave) * 4 < (160 * 1024) / (2 * per_wave) * 2)
    {
      wpb        = 2;
      ring_bytes = (size_t)wpb * fphip_reduce_ring_bytes(nq);
    }
  }
  const size_t lds = ring_bytes + (size_t)wpb * stack_doubles * sizeof(double) +
                     (size_t)wpb * FPHIP_BKZS_MAX_DEPTH * 64;  // sizeof(BkzsFrame) == 64
  if (ring_bytes > 64 * 1024 || lds > 160 * 1024)
  {
    cleanup();
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "bkz: %zu bytes of LDS per workgroup do not fit", lds);
    return FPHIP_ERROR;
  }
  int bpc = lds ? (int)((160 * 1024) / lds) : 32;
  if (bpc * wpb > 32)
    bpc = 32 / wpb;
  int grid      = (g->P.batch + wpb - 1) / wpb;
  const int cap = fphip_ctx_num_cus(g->ctx) * (bpc > 0 ? bpc : 1);
  if (grid > cap)
    grid = cap;
  hipStream_t s     = fphip_ctx_stream(g->ctx);
  const double logd = std::log(delta);
  const BkzsGeometry geo{nq, wpb, grid, stack_doubles, mu_lds_flag, lds};
  BkzsHost H{S, gh_factor, rnd, rnd_user, 0.0};
  // in-loop pruning: a pool of worker threads (one prune() is tens of milliseconds; the lattices of a batch
  // ask at about the same time), each with a volume engine of its own (stream, staging, device buffers)
  int n_workers = 1, n_handoff = 1;
  if (inloop)
  {
    H.inloop       = 1;
    H.il_preproc   = g->il_preproc;
    H.il_target    = g->il_target;
    H.il_min_block = g->il_min_block;
    H.il_flags     = g->il_flags;
    const char *we = getenv("FPHIP_BKZ_PRUNE_WORKERS");
    n_workers      = we ? atoi(we) : 8;
    n_workers      = std::max(1, std::min(n_workers, (int)std::min<size_t>(B, 64)));
    for (int w = 0; w < n_workers && g->il_device; ++w)
    {
      char why[256] = {0};
      fphip_pruner::VolumeEngine *e = fphip_pruner::create_device_volume_engine(fphip_ctx_device(g->ctx), why, sizeof why);
      if (!e)
      {
        cleanup();
        snprintf(fphip_ctx_errbuf(g->ctx), 512, "bkz_strategies: %s", why);
        return FPHIP_ERROR;
      }
      il_engines.push_back(e);
    }
  }
  std::atomic<unsigned long long> il_calls{0};
  std::atomic<int> il_errors{0};
  H.il_errors = &il_errors;
  const unsigned long long il_host_jobs0 = inloop ? (unsigned long long)fphip_pruner::host_volume_engine()->host_jobs : 0ull;
  if (handoff)
  {
    // hand-off mode: a second context on this device for the enumerations, the blocks' mu rows in
    // pinned host memory (the wave writes them, the worker thread reads them without a HIP call)
    if (!g->ectx && fphip_create_ex(fphip_ctx_device(g->ctx), 1 /* never behind the schedule kernel */, &g->ectx) != FPHIP_OK)
    {
      snprintf(fphip_ctx_errbuf(g->ctx), 512, "bkz_strategies: no enumeration context for the hand-off: %s",
               g->ectx ? fphip_last_error(g->ectx) : "?");
      if (g->ectx)
        fphip_destroy(g->ectx);
      g->ectx = nullptr;
      cleanup();
      return FPHIP_ERROR;
    }
    // the enumeration's task buffers exist before the schedule kernel runs (advisor, round 4: the first
    // fphip_enum_run of a context allocates them — here that would be the worker thread, mid-launch)
    {
      int cur_dev = 0;
      (void)hipGetDevice(&cur_dev);
      const int erc = fphip_ctx_ensure_task_buffers(g->ectx);
      (void)hipSetDevice(cur_dev);
      if (erc != FPHIP_OK)
      {
        snprintf(fphip_ctx_errbuf(g->ctx), 512, "bkz_strategies: task buffers of the hand-off context: %s",
                 fphip_last_error(g->ectx));
        cleanup();
        return FPHIP_ERROR;
      }
    }
    // a BATCH of tours shares the hand-off service: one worker thread and one enumeration context per worker (the
    // extra contexts with a small task capacity: these blocks have at most 64 rows), so that the blocks of
    // different tours are enumerated side by side instead of queueing behind one context
    {
      const char *hw = getenv("FPHIP_BKZ_HANDOFF_WORKERS");
      const int want = std::max(1, std::min(hw ? atoi(hw) : 8, (int)std::min<size_t>(B, 16)));
      n_handoff      = want;
      int cur_dev = 0;
      (void)hipGetDevice(&cur_dev);
      while ((int)g->ectx_more.size() + 1 < want)
      {
        fphip_ctx *c = nullptr;
        if (fphip_create_ex(fphip_ctx_device(g->ctx), 1, &c) != FPHIP_OK || fphip_ctx_set_task_cap(c, 1u << 18) != FPHIP_OK ||
            fphip_ctx_ensure_task_buffers(c) != FPHIP_OK)
        {
          snprintf(fphip_ctx_errbuf(g->ctx), 512, "bkz_strategies: hand-off context %zu: %s", g->ectx_more.size() + 1,
                   c ? fphip_last_error(c) : "?");
          if (c)
            fphip_destroy(c);
          (void)hipSetDevice(cur_dev);
          cleanup();
          return FPHIP_ERROR;
        }
        g->ectx_more.push_back(c);
      }
      (void)hipSetDevice(cur_dev);
    }
    g->P.enum_mu_h = (double *)pinned_get(B * (64 * 63 / 2) * sizeof(double));
    if (!g->P.enum_mu_h)
    {
      cleanup();
      snprintf(fphip_ctx_errbuf(g->ctx), 512, "bkz_strategies: no pinned memory for the hand-off");
      return FPHIP_ERROR;
    }
    const char *hn  = getenv("FPHIP_BKZ_HANDOFF_NODES");
    H.handoff_nodes = hn ? atof(hn) : 800.0;
  }
  unsigned long long handoff_calls = 0;
  int handoff_rc                   = FPHIP_OK;
  fphip_ctx *handoff_ectx          = nullptr;  // the context whose enumeration failed (its error text)
  bool rnd_failed              = false;
  unsigned long long heartbeat = 0;
  std::vector<unsigned long long> handled(B, 0);
  std::vector<int> active(B, 1);
  BCHK(hipMemcpy(g->P.bkz_active, active.data(), sizeof(int) * B, hipMemcpyHostToDevice));
  // one launch (kflags / kloops as the kernel sees them) with the mailbox service; afterwards the
  // identity-layout GSO of the new bases (same values: every entry is a function of b)
  auto run_once = [&](int kflags, int kloops, float *ms, int *st_out, int *info_out, int run_mode = 7) -> int
  {
    int rc1 = launch(g, 0, g->P.d, 0.0, 2);  // bf / row_expo of every row from b
    if (rc1 != FPHIP_OK)
      return rc1;
    GCHK(hipMemsetAsync(d_abort, 0, sizeof(int), s));  // one launch's timeout must not poison the next
    GCHK(hipEventRecord(g->ev[0], s));
    GCHK(bkzs_launch(g, geo, s, sd, sld, DS, mail, d_abort, block_size, kflags, delta, eta, logd, kloops, run_mode));
    GCHK(hipGetLastError());
    GCHK(hipEventRecord(g->ev[1], s));
    // Serve the mailboxes while the kernel runs, from a thread of its own that makes NO HIP call:
    // the kernel's liveness test watches mail[0].heartbeat, and a HIP call (even hipStreamQuery)
    // can stall for seconds behind another host thread's runtime work in the same process
    // (measured: the config-3 tour timed out next to the rest of the GPU test suite).  This thread
    // only waits for the stream.
    std::atomic<bool> stop{false};
    // hand-off mode: type-3 requests are answered by a worker thread of their own (it makes HIP calls
    // — launches on the enumeration context's stream — and may take milliseconds per request; the
    // service thread goes on sweeping, so the heartbeat never stands still)
    std::mutex hq_m;
    std::condition_variable hq_cv;
    std::deque<std::pair<size_t, unsigned long long>> hq;
    bool hq_stop = false;
    // (every hand-off enumeration runs on a context of its own worker; workers beyond the contexts — in-loop pruning
    //  may want more threads than there are hand-off contexts — share the last one under a mutex)
    std::mutex enum_m;
    std::mutex hrc_m;
    std::vector<std::thread> workers;
    const int n_threads = (handoff || inloop) ? std::max(inloop ? n_workers : 1, handoff ? n_handoff : 1) : 0;
    for (int w = 0; w < n_threads; ++w)
      workers.emplace_back([&, w]()
      {
        fphip_pruner::VolumeEngine *engine = w < (int)il_engines.size() ? il_engines[w] : nullptr;
        const int nctx      = 1 + (int)g->ectx_more.size();
        const bool own_ctx  = handoff && w < nctx - 1;  // (the last context may be shared)
        const int ci        = std::min(w, nctx - 1);    // (0 = the object's own context — also every worker's when
        fphip_ctx *my_ectx  = !handoff ? nullptr : (ci == 0 ? g->ectx : g->ectx_more[ci - 1]);  //  there is no other)
        for (;;)
        {
          std::pair<size_t, unsigned long long> job;
          {
            std::unique_lock<std::mutex> lk(hq_m);
            hq_cv.wait(lk, [&] { return hq_stop || !hq.empty(); });
            if (hq.empty())
              return;
            job = hq.front();
            hq.pop_front();
          }
          BkzMail *m   = &mail[job.first];
          if (m->type == 1)
          {  // in-loop pruning: radius, prune() on the block's profile (its batches on the engine's stream)
            serve_radius(H, m, engine);
            ++il_calls;
            __atomic_store_n(&m->rsp_seq, job.second, __ATOMIC_RELEASE);
            continue;
          }
          int rc;
          if (own_ctx)
            rc = serve_enumeration(my_ectx, m, g->P.enum_mu_h + job.first * (64 * 63 / 2));
          else
          {
            std::lock_guard<std::mutex> lk(enum_m);
            rc = serve_enumeration(my_ectx, m, g->P.enum_mu_h + job.first * (64 * 63 / 2));
          }
          {
            std::lock_guard<std::mutex> lk(hrc_m);
            if (rc != FPHIP_OK)
            {  // the wave cannot walk the block itself any more: no solution, and the call reports the error
              m->have_sol = 0;
              m->nodes3   = 0;
              handoff_rc  = rc;
              handoff_ectx = my_ectx;
            }
            ++handoff_calls;
          }
          __atomic_store_n(&m->rsp_seq, job.second, __ATOMIC_RELEASE);
        }
      });
    std::thread server([&]()
    {
      for (;;)
      {
        const bool last = stop.load(std::memory_order_acquire);  // one more sweep after the kernel ended
        for (size_t L = 0; L < B; ++L)
        {
          BkzMail *m = &mail[L];
          const unsigned long long seq = __atomic_load_n(&m->req_seq, __ATOMIC_ACQUIRE);
          if (seq == handled[L])
            continue;
          if ((m->type == 3 && handoff) || inloop_block(H, m))
          {  // to the worker; it stores rsp_seq when the enumeration (or the block's prune()) is done
            handled[L] = seq;
            {
              std::lock_guard<std::mutex> lk(hq_m);
              hq.emplace_back(L, seq);
            }
            hq_cv.notify_one();
            continue;
          }
          if (m->type == 1)
            serve_radius(H, m);
          else if (m->type == 2 && serve_plan(H, (int)L, m) < 0)
          {  // unusable generator: answer with an empty plan, report the error after the launch
            m->n_moves = m->n_ops = 0;
            rnd_failed            = true;
          }
          handled[L] = seq;
          __atomic_store_n(&m->rsp_seq, seq, __ATOMIC_RELEASE);
        }
        __atomic_store_n(&mail[0].heartbeat, ++heartbeat, __ATOMIC_RELEASE);
        if (last)
          break;
      }
    });
    const hipError_t q = hipStreamSynchronize(s);
    stop.store(true, std::memory_order_release);
    server.join();
    if (handoff || inloop)
    {
      {
        std::lock_guard<std::mutex> lk(hq_m);
        hq_stop = true;
      }
      hq_cv.notify_all();
      for (auto &t : workers)
        t.join();
    }
    if (q != hipSuccess)
      return fail(g->ctx, "bkzs_kernel", q);
    GCHK(hipEventElapsedTime(ms, g->ev[0], g->ev[1]));
    GCHK(hipMemcpy(st_out, g->P.status, sizeof(int) * B, hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(info_out, g->P.lll_info, sizeof(int) * 4 * B, hipMemcpyDeviceToHost));
    std::swap(g->P.b, g->P.b2);  // the kernel wrote the rows in position order into b2
    if (g->bkz_u)
      std::swap(g->P.u, g->P.u2);  // ... and those of u into u2 (every launch, whatever its statuses)
    rc1 = launch(g, 0, g->P.d, 0.0, 2);
    if (rc1 == FPHIP_OK)
      rc1 = launch(g, 0, g->P.d, 0.0, 0);
    return rc1;
  };

  std::vector<int> st(B, 1), inf(4 * B, 0), hook_rows(B, (int)g->P.d);
  float total_ms = 0, ms = 0;
  const bool use_loops = (flags & 0x4) != 0, auto_abort = (flags & 0x20) != 0;
  const int kbase = flags & (0x10 | 0x80);
  if (sld && g->P.sld_pass != 0)
  {
    // block-parallel mode (fphip_gso_slide_pass): ONE pass of a slide tour restricted to the blocks of
    // g->P.sld_mask (1 primal, 2 dual), or the closing hkz of every block (3) — the caller runs the tour
    rc       = run_once(kbase | 0x4 | 0x200, 1, &ms, st.data(), inf.data(), g->P.sld_pass == 3 ? 4 : 2);
    total_ms = ms;
  }
  else if (sld)
  {
    // slide reduction: one slide_tour per launch (the kernel's 0x200 frame), the potential test on the
    // host in between; then the closing hkz of every block (run_mode 4)
    rc = auto_abort_loop(g, block_size, use_loops, max_loops, active, st, inf, hook_rows, total_ms,
                         [&](int, float *tms, int *s1, int *one)
                         { return run_once(kbase | 0x4 | 0x200, 1, tms, s1, one, 2); },
                         auto_abort, true, hooks);
    std::vector<int> one(4 * B), s1(B);
    if (rc == FPHIP_OK)
    {
      for (size_t L = 0; L < B; ++L)
        active[L] = (st[L] == 1 || st[L] == 8 || st[L] == 7) ? 1 : 0;
      BCHK(hipMemcpy(g->P.bkz_active, active.data(), sizeof(int) * B, hipMemcpyHostToDevice));
      rc = run_once(kbase | 0x4 | 0x200, 1, &ms, s1.data(), one.data(), 4);
      total_ms += ms;
      for (size_t L = 0; L < B && rc == FPHIP_OK; ++L)
      {
        if (!active[L])
          continue;
        const unsigned long long a0 = ((unsigned long long)(unsigned)inf[4 * L + 2] << 32) | (unsigned)inf[4 * L + 1];
        const unsigned long long a1 = ((unsigned long long)(unsigned)one[4 * L + 2] << 32) | (unsigned)one[4 * L + 1];
        const unsigned long long t  = a0 + a1;
        inf[4 * L + 1] = (int)(unsigned)(t & 0xffffffffull);
        inf[4 * L + 2] = (int)(unsigned)(t >> 32);
        inf[4 * L + 3] += one[4 * L + 3];
        if (s1[L] <= 0)
          st[L] = s1[L];
      }
    }
  }
  else if (!auto_abort && !hooks.use_time && !hooks.dump)
  {
    rc       = run_once(kbase | (use_loops ? 0x4 : 0), max_loops, &ms, st.data(), inf.data());
    total_ms = ms;
  }
  else
  {
    // one tour per launch (self-dual BKZ: the prelude lll() goes with the first one only)
    rc = auto_abort_loop(g, block_size, use_loops, max_loops, active, st, inf, hook_rows, total_ms,
                         [&](int loop, float *tms, int *s1, int *one)
                         { return run_once(kbase | 0x4, 1, tms, s1, one, sd && loop == 0 ? 3 : 2); },
                         auto_abort, false, hooks);
    std::vector<int> one(4 * B), s1(B);
    if (sd && rc == FPHIP_OK)
    {
      // closing pass of self-dual BKZ on every lattice that ended regularly: hkz of the last window
      // (bkz.cpp:627-641), its own launch
      for (size_t L = 0; L < B; ++L)
        active[L] = (st[L] == 1 || st[L] == 8 || st[L] == 7) ? 1 : 0;
      BCHK(hipMemcpy(g->P.bkz_active, active.data(), sizeof(int) * B, hipMemcpyHostToDevice));
      rc = run_once(kbase | 0x4, 1, &ms, s1.data(), one.data(), 4);
      total_ms += ms;
      for (size_t L = 0; L < B && rc == FPHIP_OK; ++L)
      {
        if (!active[L])
          continue;
        const unsigned long long a0 = ((unsigned long long)(unsigned)inf[4 * L + 2] << 32) | (unsigned)inf[4 * L + 1];
        const unsigned long long a1 = ((unsigned long long)(unsigned)one[4 * L + 2] << 32) | (unsigned)one[4 * L + 1];
        const unsigned long long t  = a0 + a1;
        inf[4 * L + 1] = (int)(unsigned)(t & 0xffffffffull);
        inf[4 * L + 2] = (int)(unsigned)(t >> 32);
        inf[4 * L + 3] += one[4 * L + 3];
        if (s1[L] <= 0)
          st[L] = s1[L];
      }
    }
  }
#undef BCHK
  if (rc == FPHIP_OK && hooks.dump && !(sld && g->P.sld_pass != 0))
    rc = dump_gso_output(g, hooks, st, hook_rows);  // "Output", bkz.cpp:667-670 (after the closing hkz passes)
  if (inloop)
  {
    g->il_calls += il_calls.load();
    for (auto *e : il_engines)
    {
      g->il_device_jobs += e->device_jobs;
      g->il_host_jobs += e->host_jobs;
      g->il_launches += e->launches;
    }
    // without device engines the workers share the host engine: its jobs of this call
    if (il_engines.empty())
      g->il_host_jobs += fphip_pruner::host_volume_engine()->host_jobs - il_host_jobs0;
  }
  cleanup();  // (run_once's GCHKs return to this function, never past it: nothing leaks on a HIP error; the
              //  volume engines go here too)
  if (handoff && getenv("FPHIP_DEBUG"))
    fprintf(stderr, "[fphip] bkz_strategies: %llu block enumerations handed to the multi-wave enumerator\n",
            handoff_calls);
  if (handoff_rc != FPHIP_OK && rc == FPHIP_OK)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "bkz_strategies: a handed-off enumeration failed: %s",
             handoff_ectx ? fphip_last_error(handoff_ectx) : (g->ectx ? fphip_last_error(g->ectx) : "?"));
    rc = FPHIP_ERROR;
  }
  if (il_errors.load() > 0 && rc == FPHIP_OK)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "bkz_strategies: %d in-loop prune() calls lost their volume engine "
             "(the strategies' sets were used for those blocks)", il_errors.load());
    rc = FPHIP_ERROR;
  }
  if (rnd_failed && rc == FPHIP_OK)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512,
             "bkz_strategies: the caller's rnd() kept returning the same value (rerandomize_block "
             "needs two different rows); for large batches rnd should be a C function");
    rc = FPHIP_ERROR;
  }
  g->last_ms = total_ms;
  if (status)
    memcpy(status, st.data(), sizeof(int) * B);
  if (info)
    memcpy(info, inf.data(), sizeof(int) * 4 * B);
  return rc;
}

extern "C" int fphip_gso_get_mu(fphip_gso *g, int lattice, double *mu)
{
  if (!g || !mu || lattice < 0 || lattice >= g->P.batch)
    return FPHIP_ERROR;
  if (int rcg = session_guard(g, "fphip_gso_get_mu"))
    return rcg;
  GCHK(hipMemcpy2D(mu, (size_t)g->P.d * 8, g->P.mu + (size_t)lattice * g->P.d * g->P.ldd,
                   (size_t)g->P.ldd * 8, (size_t)g->P.d * 8, g->P.d, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

extern "C" int fphip_gso_get_r(fphip_gso *g, int lattice, double *r)
{
  if (!g || !r || lattice < 0 || lattice >= g->P.batch)
    return FPHIP_ERROR;
  if (int rcg = session_guard(g, "fphip_gso_get_r"))
    return rcg;
  GCHK(hipMemcpy2D(r, (size_t)g->P.d * 8, g->P.r + (size_t)lattice * g->P.d * g->P.ldd,
                   (size_t)g->P.ldd * 8, (size_t)g->P.d * 8, g->P.d, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

extern "C" int fphip_gso_get_row_expo(fphip_gso *g, int lattice, int64_t *row_expo)
{
  if (!g || !row_expo || lattice < 0 || lattice >= g->P.batch)
    return FPHIP_ERROR;
  if (int rcg = session_guard(g, "fphip_gso_get_row_expo"))
    return rcg;
  GCHK(hipMemcpy(row_expo, g->P.rexp + (size_t)lattice * g->P.d, sizeof(long long) * g->P.d,
                 hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

// ---- closest vectors: target preparation, MatGSOInterface::babai, the solver (cvp_prepare.hip) -------------------
namespace
{
// (CvpBufs — the device blocks of one call, back to the cache when it returns — is in svp_host.h: gram_host.hip
//  uses it too)
}  // namespace

static int cvp_lattice_guard(fphip_gso *g, int lattice, int T, const char *what)
{
  if (lattice < 0 || lattice >= g->P.batch || T <= 0)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "%s: bad lattice index or number of targets", what);
    return FPHIP_ERROR;
  }
  return session_guard(g, what);
}

// true mu [d][d], true r_ii [d] and the basis as doubles [d][n] of one lattice, on the device
static int cvp_unscale(fphip_gso *g, int lattice, CvpBufs &B, double **bfd, double **mu, double **rd)
{
  const size_t d = g->P.d, n = g->P.n;
  GCHK(B.get(bfd, d * n));
  GCHK(B.get(mu, d * d));
  GCHK(B.get(rd, d));
  const size_t work = std::max(d * d, d * n);
  hipLaunchKernelGGL(cvp_unscale_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, B.s, g->P, lattice, *bfd, *mu,
                     *rd);
  GCHK(hipGetLastError());
  return FPHIP_OK;
}

// the preparation over T targets, its results left on the device in blocks of B: P's outputs, the targets, the true
// mu [d][d] and r_ii [d] the kernel used
static int cvp_prepare_dev(fphip_gso *g, int lattice, int T, const int64_t *targets, CvpBufs &B, CvpPrep &P,
                           long long **tg_out, double **mu_out, double **rd_out)
{
  const size_t d = g->P.d, n = g->P.n, ldt = ((size_t)T + 63) / 64 * 64;
  hipStream_t s = B.s;
  memset(&P, 0, sizeof P);
  double *bfd = nullptr, *mu = nullptr, *rd = nullptr;
  if (int rc = cvp_unscale(g, lattice, B, &bfd, &mu, &rd))
    return rc;
  long long *tg = nullptr;
  GCHK(B.get(&tg, (size_t)T * n));
  GCHK(B.get(&P.coef, (size_t)T * d));
  GCHK(B.get(&P.tcoord, (size_t)T * d));
  GCHK(B.get(&P.descent, (size_t)T));
  GCHK(B.get(&P.status, (size_t)T));
  GCHK(B.get(&P.wv, n * ldt));
  GCHK(B.get(&P.wc, d * ldt));
  GCHK(B.get(&P.wx, d * ldt));
  GCHK(B.get(&P.wt, n * ldt));
  GCHK(B.get(&P.wk, d * ldt));
  GCHK(B.get(&P.wp, d * ldt));
  GCHK(hipMemcpy(tg, targets, (size_t)T * n * sizeof(long long), hipMemcpyHostToDevice));
  GCHK(hipStreamSynchronize(nullptr));  // (see fphip_gso_set_basis)
  P.T = T, P.ldt = (int)ldt, P.d = (int)d, P.n = (int)n, P.ldn = g->P.ldn;
  P.max_passes = 0x100;  // where the reference starts to warn (svpcvp.cpp:573)
  P.b          = g->P.b + (size_t)lattice * d * g->P.ldn;
  P.bfd = bfd, P.mu = mu, P.rd = rd, P.targets = tg;
  GCHK(hipEventRecord(g->ev[0], s));
  hipLaunchKernelGGL(cvp_prepare_kernel, dim3((unsigned)(ldt / 64)), dim3(64), 0, s, P);
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(g->ev[1], s));
  GCHK(hipStreamSynchronize(s));
  GCHK(hipEventElapsedTime(&g->last_ms, g->ev[0], g->ev[1]));
  *tg_out = tg, *mu_out = mu, *rd_out = rd;
  return FPHIP_OK;
}

// the preparation over T targets; mu_h / rd_h (nullable): the true mu [d][d] and r_ii [d] the kernel used
static int cvp_prepare_run(fphip_gso *g, int lattice, int T, const int64_t *targets, int64_t *coef, double *target_coord,
                           double *descent, int *status, double *mu_h, double *rd_h, CvpBufs *keep = nullptr,
                           CvpPrep *P_out = nullptr, long long **tg_out = nullptr, double **mu_out = nullptr,
                           double **rd_out = nullptr)
{
  const size_t d = g->P.d;
  CvpBufs own(fphip_ctx_stream(g->ctx));
  CvpBufs &B = keep ? *keep : own;  // (keep: the caller goes on with the device blocks)
  CvpPrep P;
  long long *tg = nullptr;
  double *mu = nullptr, *rd = nullptr;
  if (int rc = cvp_prepare_dev(g, lattice, T, targets, B, P, &tg, &mu, &rd))
    return rc;
  if (P_out)
    *P_out = P, *tg_out = tg, *mu_out = mu, *rd_out = rd;
  GCHK(hipMemcpy(coef, P.coef, (size_t)T * d * sizeof(long long), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(target_coord, P.tcoord, (size_t)T * d * sizeof(double), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(descent, P.descent, (size_t)T * sizeof(double), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(status, P.status, (size_t)T * sizeof(int), hipMemcpyDeviceToHost));
  if (mu_h)
    GCHK(hipMemcpy(mu_h, mu, d * d * sizeof(double), hipMemcpyDeviceToHost));
  if (rd_h)
    GCHK(hipMemcpy(rd_h, rd, d * sizeof(double), hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

extern "C" int fphip_cvp_prepare(fphip_gso *g, int lattice, int T, const int64_t *targets, int64_t *coef,
                                 double *target_coord, double *descent, int *status)
{
  FPHIP_RANGE("fphip_cvp_prepare");
  if (!g || !targets || !coef || !target_coord || !descent || !status)
    return FPHIP_ERROR;
  if (int rc = cvp_lattice_guard(g, lattice, T, "fphip_cvp_prepare"))
    return rc;
  return cvp_prepare_run(g, lattice, T, targets, coef, target_coord, descent, status, nullptr, nullptr);
}

extern "C" int fphip_gso_babai(fphip_gso *g, int lattice, int T, const double *v, int start, int dimension, int64_t *w,
                               int *status)
{
  FPHIP_RANGE("fphip_gso_babai");
  if (!g || !v || !w || !status)
    return FPHIP_ERROR;
  if (int rc = cvp_lattice_guard(g, lattice, T, "fphip_gso_babai"))
    return rc;
  const int d = g->P.d;
  if (start < 0 || start >= d)
    return fail_msg(g->ctx, "fphip_gso_babai: start outside the basis");
  if (dimension == -1)
    dimension = d - start;
  if (dimension < 1 || start + dimension > d)
    return fail_msg(g->ctx, "fphip_gso_babai: rows [start, start + dimension) outside the basis");
  const size_t ldt = ((size_t)T + 63) / 64 * 64, dm = (size_t)dimension;
  hipStream_t s = fphip_ctx_stream(g->ctx);
  CvpBufs B(s);
  double *bfd = nullptr, *mu = nullptr, *rd = nullptr;
  if (int rc = cvp_unscale(g, lattice, B, &bfd, &mu, &rd))
    return rc;
  double *vd = nullptr, *wx = nullptr;
  long long *wd = nullptr;
  int *sd       = nullptr;
  GCHK(B.get(&vd, (size_t)T * dm));
  GCHK(B.get(&wd, (size_t)T * dm));
  GCHK(B.get(&sd, (size_t)T));
  GCHK(B.get(&wx, dm * ldt));
  GCHK(hipMemcpy(vd, v, (size_t)T * dm * sizeof(double), hipMemcpyHostToDevice));
  GCHK(hipStreamSynchronize(nullptr));
  GCHK(hipEventRecord(g->ev[0], s));
  hipLaunchKernelGGL(cvp_babai_kernel, dim3((unsigned)(ldt / 64)), dim3(64), 0, s, T, (int)ldt, d, start, dimension, mu, vd,
                     wd, sd, wx);
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(g->ev[1], s));
  GCHK(hipStreamSynchronize(s));
  GCHK(hipEventElapsedTime(&g->last_ms, g->ev[0], g->ev[1]));
  GCHK(hipMemcpy(w, wd, (size_t)T * dm * sizeof(long long), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(status, sd, (size_t)T * sizeof(int), hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

namespace
{
// FastEvaluator(1), EVALSTRATEGY_BEST_N_SOLUTIONS: keep the closest candidate, the bound follows it
struct CvpBest
{
  int d;
  bool have;
  double dist;
  std::vector<double> x;
};
double cvp_best_cb(void *user, double dist, const double *sol)
{
  CvpBest *b = (CvpBest *)user;
  if (!b->have || dist < b->dist)
  {
    b->have = true;
    b->dist = dist;
    b->x.assign(sol, sol + b->d);
  }
  return b->dist;
}

// The default of FPHIP_CVP_WAVE_NODES_PER_TARGET: c, the number of nodes a lone wave of cvp_wave_kernel walks in the
// wall time of one ENUM-route call.  The AUTO route's budget per target is c min(T, resident waves of the launch), so
// that its wave stage never lasts longer than the ENUM route would have taken for the same batch.  Measured
// (tests/perf/cvp_wave_bench.py): a lone wave walks 2.91e6 nodes/s (the 1.2e6-node near:10 target of cvpsolve_q36); one
// ENUM call took 0.196 ms per target on the 24-row basis (trees of about a hundred nodes: the call's floor) and 6.15 ms
// on the 40-row basis with the bench's targets (trees of about 6e5 nodes).  c is the product with the SMALLER time,
// 2.91e6 x 0.196e-3 = 571, so that the bound holds on both; with the 40-row time it would be 17 900.  The session
// recorded in profiles/cvp_wave.md (the same code with this default) gives 526 and 21 100: within the box noise.
constexpr double CVP_WAVE_NODES_PER_TARGET_DEFAULT = 570.0;

// |target - sum sol_i b_i|^2 on the host in 128-bit integers; false: it leaves the int64 range
bool cvp_host_norm(int d, int n, const long long *b, const int64_t *target, const int64_t *sol, long long *out)
{
  __int128 nrm = 0;
  for (int j = 0; j < n; ++j)
  {
    __int128 w = (__int128)target[j];
    for (int i = 0; i < d; ++i)
    {
      __int128 p, q;  // (a product is below 2^126)
      if (sol[i] == 0)
        continue;
      p = (__int128)sol[i] * (__int128)b[(size_t)i * n + j];
      if (__builtin_sub_overflow(w, p, &q))
        return false;
      w = q;
    }
    __int128 p, q;
    if (__builtin_mul_overflow(w, w, &p) || __builtin_add_overflow(nrm, p, &q))
      return false;
    nrm = q;
  }
  if (nrm > (__int128)std::numeric_limits<long long>::max())
    return false;
  *out = (long long)nrm;
  return true;
}

// the AUTO route's second stage: the evaluator of cvp_wave.hip on the host, the candidate's exact squared distance to
// the reduced target in 128-bit integers.  Only a strictly smaller N replaces the best the wave stage left.
struct CvpExact
{
  int d, n;
  const long long *b;       // [d][n] host copy of the rows
  const int64_t *target;    // [n] the original target
  const int64_t *coef;      // [d] the preparation's coefficients
  bool have;                // nbest is known
  bool improved, overflow;
  long long nbest;
  double radius, dist;
  std::vector<double> x;
  std::vector<int64_t> sol;
};
double cvp_exact_cb(void *user, double dist, const double *sol)
{
  CvpExact *B = (CvpExact *)user;
  for (int i = 0; i < B->d; ++i)
  {
    long long xi;
    if (!(std::fabs(sol[i]) < 9223372036854775808.0) ||
        __builtin_add_overflow((long long)B->coef[i], (long long)sol[i], &xi))
    {
      B->overflow = true;
      return 0.0;  // stop
    }
    B->sol[i] = xi;
  }
  long long nv = 0;
  if (!cvp_host_norm(B->d, B->n, B->b, B->target, B->sol.data(), &nv))
  {
    B->overflow = true;
    return 0.0;
  }
  if (!B->have || nv < B->nbest)
  {
    B->have = B->improved = true;
    B->nbest = nv;
    B->dist  = dist;
    B->x.assign(sol, sol + B->d);
    const double r2 = dist + dist * 0x1p-30;
    B->radius       = r2 < B->radius ? r2 : B->radius;
    if (nv == 0)
      return 0.0;  // nothing is closer
  }
  return B->radius;
}
}  // namespace

// the launch geometry of cvp_wave_kernel for T targets: four waves per workgroup (one per SIMD of a compute unit, the
// mu triangle shared between them), as many workgroups per compute unit as the occupancy query allows
static int cvp_wave_geometry(fphip_gso *g, int T, CvpWave &A, int *wpb_out, int *grid_out, size_t *lds_out)
{
  const size_t d = g->P.d, n = g->P.n;
  const int nq = (int)((std::max(d, n) + 63) / 64), wpb = 4;
  A.stack_doubles  = (int)(d * (d + 1) / 2 + 2);
  A.mu_doubles     = (int)std::max<size_t>(d * (d - 1) / 2, 2);
  const size_t lds = ((size_t)A.mu_doubles + (size_t)A.stack_doubles * wpb) * sizeof(double);  // d = 64: 82 752 bytes
  if (lds > 64 * 1024)
    GCHK(dispatch_nq(nq, [&](auto NQ) { return allow_lds(cvp_wave_kernel<NQ>, lds); }));
  int bpc = 0;
  if (dispatch_nq(nq, [&](auto NQ) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, cvp_wave_kernel<NQ>, wpb * 64, lds);
      }) != hipSuccess || bpc < 1)
  {
    (void)hipGetLastError();
    bpc = std::max(1, std::min((int)((160 * 1024) / lds), 16 / wpb));
  }
  int grid = (T + wpb - 1) / wpb;
  int cap  = fphip_ctx_num_cus(g->ctx) * bpc;
  if (const char *e = getenv("FPHIP_CVP_WAVE_GRID"))  // (tests: a small grid makes a small batch go round the grid-stride loop)
    cap = std::max(1, atoi(e));
  *wpb_out = wpb, *grid_out = std::min(grid, cap), *lds_out = lds;
  return FPHIP_OK;
}

// the wave-per-target kernel over the prepared targets (device blocks of the preparation); x [T][d], found [T]
static int cvp_wave_run(fphip_gso *g, CvpBufs &B, CvpWave A, int wpb, int grid, size_t lds, int64_t *x, double *dist,
                        int64_t *norm, uint64_t *nodes, int *found, int *status)
{
  const size_t d = g->P.d, n = g->P.n, T = (size_t)A.T;
  const int nq   = (int)((std::max(d, n) + 63) / 64);
  hipStream_t s  = B.s;
  GCHK(B.get(&A.x, T * d));
  GCHK(B.get(&A.dist, T));
  GCHK(B.get(&A.norm, T));
  GCHK(B.get(&A.nodes, T));
  GCHK(B.get(&A.found, T));
  GCHK(B.get(&A.status, T));
  GCHK(hipEventRecord(g->ev[0], s));
  dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL(cvp_wave_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, g->P, A); });
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(g->ev[1], s));
  GCHK(hipStreamSynchronize(s));
  GCHK(hipEventElapsedTime(&g->last_ms, g->ev[0], g->ev[1]));
  GCHK(hipMemcpy(x, A.x, T * d * sizeof(long long), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(dist, A.dist, T * sizeof(double), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(norm, A.norm, T * sizeof(long long), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(nodes, A.nodes, T * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(found, A.found, T * sizeof(int), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(status, A.status, T * sizeof(int), hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

// closest_vector(b, int_target, sol_coord, CVPM_FAST) (svpcvp.cpp:532-659) for T targets against one lattice:
// update_gso, the preparation kernel over all targets, one closest-vector enumeration per target on ectx under a
// BEST_N(1) evaluator, sol_coord = coef + x.  The enumeration starts from the rounding descent's squared distance
// enlarged by a relative 2^-30, not from the reference's sum of the r_ii (:601-606): the descent's leaf is the first
// one the reference reaches and lies inside either radius, so the closest vector is the same, and the top of the
// parallel walk runs under the INITIAL radius.  Nothing inside the radius (the descent's own leaf can miss it by the
// rounding of another operand order): the answer is the descent.
//
// The routes: ENUM is the above; WAVE hands the prepared targets to cvp_wave_kernel in one launch;
// AUTO runs the wave kernel under a budget and finishes the targets that reached it by one enumeration each.
extern "C" int fphip_closest_vector_ex(fphip_gso *g, fphip_ctx *ectx, int lattice, int T, const int64_t *targets,
                                       int method, int route, uint64_t max_nodes, int64_t *sol_coord, double *dist,
                                       int64_t *norm, uint64_t *nodes_out, int *status)
{
  FPHIP_RANGE("fphip_closest_vector");
  if (!g || !targets || !sol_coord || !status)
    return FPHIP_ERROR;
  if (!ectx)
    ectx = g->ctx;
  if (int rc = cvp_lattice_guard(g, lattice, T, "fphip_closest_vector"))
    return rc;
  if (method != FPHIP_CVPM_FAST)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_closest_vector: method %d (CVPM_PROVED and its max_indices reset "
             "path, or an unknown one) is not offered: CVPM_FAST only", method);
    return FPHIP_UNSUPPORTED;
  }
  if (route != FPHIP_CVP_ROUTE_AUTO && route != FPHIP_CVP_ROUTE_WAVE && route != FPHIP_CVP_ROUTE_ENUM)
    return fail_msg(g->ctx, "fphip_closest_vector: unknown route");
  const int d = g->P.d, n = g->P.n;
  if (route == FPHIP_CVP_ROUTE_WAVE && (d > 64 || n > 256))
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_closest_vector: the WAVE route takes at most 64 rows and 256 columns "
             "(d = %d, n = %d): use the ENUM route", d, n);
    return FPHIP_UNSUPPORTED;
  }
  if (d > FPHIP_ENUM_MAX_DIM)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_closest_vector: more than %d rows", FPHIP_ENUM_MAX_DIM);
    return FPHIP_UNSUPPORTED;
  }
  const bool wave = route == FPHIP_CVP_ROUTE_WAVE || (route == FPHIP_CVP_ROUTE_AUTO && d <= 64 && n <= 256);
  const bool auto_route = route == FPHIP_CVP_ROUTE_AUTO;
  std::vector<int> gst(g->P.batch, 0);
  if (int rc = fphip_gso_update(g, gst.data()))
    return rc;
  if (gst[lattice] != 1)
    return fail_msg(g->ctx, "fphip_closest_vector: update_gso failed (non-finite mu: RED_GSO_FAILURE)");
  const size_t dd = (size_t)d, nn = (size_t)n;
  std::vector<int64_t> coef((size_t)T * dd);
  std::vector<double> tc((size_t)T * dd), desc((size_t)T), mu(dd * dd), rd(dd), mut(dd * dd, 0.0), xr(dd);
  std::vector<int> pst((size_t)T);
  CvpBufs B(fphip_ctx_stream(g->ctx));  // (the preparation's device blocks: the wave kernel reads them)
  CvpPrep Pd;
  long long *tg_d = nullptr;
  double *mu_d = nullptr, *rd_d = nullptr;
  if (int rc = cvp_prepare_run(g, lattice, T, targets, coef.data(), tc.data(), desc.data(), pst.data(), mu.data(), rd.data(),
                               &B, &Pd, &tg_d, &mu_d, &rd_d))
    return rc;
  float kernel_ms = g->last_ms;
  for (size_t i = 0; i < dd; ++i)
    for (size_t j = i + 1; j < dd; ++j)
      mut[i * dd + j] = mu[j * dd + i];  // the layout a plugin receives: mut[i][j] = mu(j,i), j > i
  // the rows on the host, for the exact distances computed here
  std::vector<long long> bh;
  if (norm || auto_route)
  {
    bh.resize(dd * nn);
    GCHK(hipMemcpy2D(bh.data(), nn * 8, g->P.b + (size_t)lattice * dd * g->P.ldn, (size_t)g->P.ldn * 8, nn * 8, dd,
                     hipMemcpyDeviceToHost));
  }
  // ---- the wave stage: every target in one launch ---------------------------------------------------------------
  std::vector<int64_t> wx, wnorm;
  std::vector<double> wdist;
  std::vector<uint64_t> wnodes;
  std::vector<int> wfound, wst;
  if (wave)
  {
    CvpWave A;
    memset(&A, 0, sizeof A);
    A.lattice = lattice, A.T = T;
    A.coef = Pd.coef, A.tcoord = Pd.tcoord, A.descent = Pd.descent, A.pstatus = Pd.status;
    A.targets = tg_d, A.mu = mu_d, A.rd = rd_d;
    int wpb = 0, grid = 0;
    size_t lds = 0;
    if (int rc = cvp_wave_geometry(g, T, A, &wpb, &grid, &lds))
      return rc;
    A.max_nodes = max_nodes;
    if (auto_route && max_nodes == 0)
    {
      const char *e  = getenv("FPHIP_CVP_WAVE_NODES_PER_TARGET");
      const double c = e ? atof(e) : CVP_WAVE_NODES_PER_TARGET_DEFAULT;
      const double v = std::floor(c * (double)std::min(T, grid * wpb));
      A.max_nodes    = v >= 1.0 ? (v < 1.8e19 ? (unsigned long long)v : ~0ull) : 1ull;
    }
    wx.resize((size_t)T * dd), wnorm.resize((size_t)T), wdist.resize((size_t)T), wnodes.resize((size_t)T);
    wfound.resize((size_t)T), wst.resize((size_t)T);
    if (int rc = cvp_wave_run(g, B, A, wpb, grid, lds, wx.data(), wdist.data(), wnorm.data(), wnodes.data(),
                              wfound.data(), wst.data()))
      return rc;
    kernel_ms = g->last_ms;
  }
  std::vector<uint64_t> nodes(FPHIP_ENUM_MAX_DIM + 1);
  // one closest-vector enumeration of target t on ectx at radius^2 maxdist
  auto enum_one = [&](int t, double maxdist, fphip_sol_cb cb, void *user, uint64_t *total) -> int
  {
    fphip_enum_opts o;
    memset(&o, 0, sizeof o);
    o.shard_count     = 1;
    o.exchange_chunks = 1;
    o.target          = tc.data() + (size_t)t * dd;
    std::fill(nodes.begin(), nodes.end(), 0);
    // (blocks above 64 rows: the enumerator's closest-vector mode takes them on request only; the solver asks)
    const int wide_was = fphip_ctx_allow_wide_target(ectx, 1);
    const int rc = fphip_enum_run(ectx, d, maxdist, mut.data(), rd.data(), nullptr, &o, cb, nullptr, user, nodes.data(),
                                  nullptr);
    fphip_ctx_allow_wide_target(ectx, wide_was);
    if (rc != FPHIP_OK && ectx != g->ctx)
      snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_closest_vector: enumeration of target %d: %s", t,
               fphip_last_error(ectx));
    for (int k = 0; k <= d; ++k)
      *total += nodes[k];
    return rc;
  };
  for (int t = 0; t < T; ++t)
  {
    int64_t *out = sol_coord + (size_t)t * dd;
    memset(out, 0, dd * sizeof(int64_t));
    if (dist)
      dist[t] = 0.0;
    if (norm)
      norm[t] = 0;
    if (nodes_out)
      nodes_out[t] = 0;
    status[t] = pst[t];
    if (pst[t] != 1)
      continue;
    const double *c = tc.data() + (size_t)t * dd;
    const int64_t *tgt = targets + (size_t)t * nn, *cf = coef.data() + (size_t)t * dd;
    bool have = false, norm_known = false;
    double bd = desc[t];
    long long nbest = 0;
    uint64_t total = 0;
    if (wave)
    {
      if (wst[t] == -2)
      {
        status[t] = -2;
        continue;
      }
      status[t] = wst[t];
      total     = wnodes[t];
      if (wfound[t])
      {
        have = norm_known = true;
        for (size_t i = 0; i < dd; ++i)
          xr[i] = (double)wx[(size_t)t * dd + i];
        bd    = wdist[t];
        nbest = wnorm[t];
      }
    }
    else
    {
      CvpBest best{d, false, 0.0, {}};
      if (d >= 2 && desc[t] > 0.0)
        if (int rc = enum_one(t, desc[t] + desc[t] * 0x1p-30, cvp_best_cb, &best, &total))
          return rc;
      if (best.have)
      {
        have = true;
        xr   = best.x;
        bd   = best.dist;
      }
    }
    if (!have)  // the descent itself (the same loop as the kernel's)
      for (int k = d - 1; k >= 0; --k)
      {
        double newcenter = c[k];
        for (int j = k + 1; j < d; ++j)
          newcenter -= xr[j] * mut[(size_t)k * dd + j];
        xr[k] = std::round(newcenter);
      }
    if (wave && auto_route && status[t] == FPHIP_CVP_NODE_LIMIT)
    {
      // the second stage: one enumeration at the radius the wave stage reached, decided on exact integers
      CvpExact ex{d, n, bh.data(), tgt, cf, norm_known, false, false, nbest, 0.0, bd, {}, std::vector<int64_t>(dd)};
      if (!norm_known)
      {  // (no candidate before the budget: the descent's point is the one to beat)
        bool fits = true;
        for (size_t i = 0; i < dd && fits; ++i)
        {
          long long xi = 0;
          fits = std::fabs(xr[i]) < 9223372036854775808.0 && !__builtin_add_overflow((long long)cf[i], (long long)xr[i], &xi);
          ex.sol[i] = xi;
        }
        ex.have = fits && cvp_host_norm(d, n, bh.data(), tgt, ex.sol.data(), &ex.nbest);
      }
      const double r0 = std::min(desc[t], bd);
      ex.radius       = r0 + r0 * 0x1p-30;
      if (!(ex.have && ex.nbest == 0))
        if (int rc = enum_one(t, ex.radius, cvp_exact_cb, &ex, &total))
          return rc;
      if (ex.overflow)
      {
        status[t] = -2;
        continue;
      }
      if (ex.improved)
      {
        xr = ex.x;
        bd = ex.dist;
      }
      norm_known = ex.have;
      nbest      = ex.nbest;
      status[t]  = 1;
    }
    for (size_t i = 0; i < dd; ++i)
    {
      long long xi = 0;
      if (!(std::fabs(xr[i]) < 9223372036854775808.0) ||
          __builtin_add_overflow((long long)cf[i], (long long)xr[i], &xi))
      {
        status[t] = -2;
        break;
      }
      out[i] = xi;
    }
    if (status[t] == -2)
    {
      memset(out, 0, dd * sizeof(int64_t));
      continue;
    }
    if (dist)
      dist[t] = bd;
    if (nodes_out)
      nodes_out[t] = total;
    if (norm)
    {
      if (!norm_known && !cvp_host_norm(d, n, bh.data(), tgt, out, &nbest))
        nbest = 0;
      norm[t] = nbest;
    }
  }
  g->last_ms = kernel_ms;
  return FPHIP_OK;
}

extern "C" int fphip_closest_vector(fphip_gso *g, fphip_ctx *ectx, int lattice, int T, const int64_t *targets, int method,
                                    int64_t *sol_coord, double *dist, int *status)
{
  return fphip_closest_vector_ex(g, ectx, lattice, T, targets, method, FPHIP_CVP_ROUTE_ENUM, 0, sol_coord, dist, nullptr,
                                 nullptr, status);
}

// ---- shortest vectors (svp_wave.hip; the ENUM route: fphip_enum_run) -----------------------------------------------
namespace
{
// (SVP_WAVE_MAX_NODES_DEFAULT, the default of FPHIP_SVP_WAVE_MAX_NODES, is in svp_host.h: the forms' solver uses it too)

typedef __int128 i128;
// the ENUM route's evaluator: the candidate's exact norm in 128-bit integers, strictly smaller wins, the bound
// follows as (N - 1) (1 + 2^-30)
struct SvpBest
{
  int d, n;              // rows under enumeration (d_eff), columns
  const long long *b;    // [d][n] host copy of the rows
  long long nbest;
  bool overflow;
  std::vector<long long> x, v;
  std::vector<i128> w;
  double bound() const { return (double)(nbest - 1) * (1.0 + 0x1p-30); }
};
// false: a product or a sum left the 127-bit range, or the result the int64 range
bool svp_exact_candidate(SvpBest *B, const double *sol, long long *norm)
{
  const int d = B->d, n = B->n;
  std::fill(B->w.begin(), B->w.end(), (i128)0);
  for (int i = 0; i < d; ++i)
  {
    if (sol[i] == 0.0)
      continue;
    if (!(std::fabs(sol[i]) < 9223372036854775808.0))
      return false;
    const i128 xi = (i128)(long long)sol[i];
    for (int j = 0; j < n; ++j)
    {
      i128 p, q;
      if (__builtin_mul_overflow(xi, (i128)B->b[(size_t)i * n + j], &p) || __builtin_add_overflow(B->w[j], p, &q))
        return false;
      B->w[j] = q;
    }
  }
  i128 nrm = 0;
  for (int j = 0; j < n; ++j)
  {
    i128 p, q;
    if (__builtin_mul_overflow(B->w[j], B->w[j], &p) || __builtin_add_overflow(nrm, p, &q))
      return false;
    nrm = q;
  }
  if (nrm > (i128)std::numeric_limits<long long>::max())
    return false;
  *norm = (long long)nrm;
  return true;
}
double svp_best_cb(void *user, double dist, const double *sol)
{
  (void)dist;  // (the decision is the integers')
  SvpBest *B = (SvpBest *)user;
  long long nv = 0;
  if (!svp_exact_candidate(B, sol, &nv))
  {
    B->overflow = true;
    return 0.0;  // stop
  }
  if (nv > 0 && nv < B->nbest)
  {
    B->nbest = nv;
    for (int i = 0; i < B->d; ++i)
      B->x[i] = (long long)sol[i];
    for (int j = 0; j < B->n; ++j)
      B->v[j] = (long long)B->w[j];
  }
  return B->bound();  // (0 once the norm is 1: nothing non-zero is shorter)
}
}  // namespace

// the wave-per-lattice kernel over the range; skip (device, nullable): lattices it leaves alone
static int svp_wave_run(fphip_gso *g, int first, int count, const double *pruning, const int *take_h, int64_t *sol_coord,
                        int64_t *vec, int64_t *norm, uint64_t *nodes, int *status)
{
  const size_t d = g->P.d, n = g->P.n;
  const int nq   = (int)((std::max(d, n) + 63) / 64);
  int wpb        = 4;
  SvpWave A;
  memset(&A, 0, sizeof A);
  A.first = first, A.count = count;
  A.stack_doubles = (int)(d * (d + 1) / 2 + 2);
  A.mu_doubles    = (int)std::max<size_t>(d * (d - 1) / 2, 2);
  const size_t per_wave = (size_t)(A.stack_doubles + A.mu_doubles) * sizeof(double);
  const size_t lds      = per_wave * wpb;  // d <= 64: at most 131136 bytes
  int bpc = (int)((160 * 1024) / lds);
  if (bpc * wpb > 32)
    bpc = 32 / wpb;
  int grid = (count + wpb - 1) / wpb;
  int cap  = fphip_ctx_num_cus(g->ctx) * std::max(bpc, 1);
  if (const char *e = getenv("FPHIP_SVP_WAVE_GRID"))  // (tests: a small grid makes a small batch go round the grid-stride loop)
    cap = std::max(1, atoi(e));
  grid = std::min(grid, cap);
  hipStream_t s = fphip_ctx_stream(g->ctx);
  CvpBufs B(s);
  double *pr_d = nullptr;
  int *take_d  = nullptr;
  GCHK(B.get(&A.sol_coord, (size_t)count * d));
  GCHK(B.get(&A.vec, (size_t)count * n));
  GCHK(B.get(&A.norm, (size_t)count));
  GCHK(B.get(&A.nodes, (size_t)count));
  GCHK(B.get(&A.status, (size_t)count));
  if (pruning)
  {
    GCHK(B.get(&pr_d, d));
    GCHK(hipMemcpy(pr_d, pruning, d * sizeof(double), hipMemcpyHostToDevice));
  }
  if (take_h)
  {
    GCHK(B.get(&take_d, (size_t)count));
    GCHK(hipMemcpy(take_d, take_h, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
  }
  GCHK(hipStreamSynchronize(nullptr));  // (see fphip_gso_set_basis)
  A.pruning = pr_d;
  A.take    = take_d;
  if (lds > 64 * 1024)
    GCHK(dispatch_nq(nq, [&](auto NQ) { return allow_lds(svp_wave_kernel<NQ>, lds); }));
  GCHK(hipEventRecord(g->ev[0], s));
  dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL(svp_wave_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, g->P, A); });
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(g->ev[1], s));
  GCHK(hipStreamSynchronize(s));
  GCHK(hipEventElapsedTime(&g->last_ms, g->ev[0], g->ev[1]));
  std::vector<long long> hs((size_t)count * d), hv((size_t)count * n), hn((size_t)count);
  std::vector<unsigned long long> hk((size_t)count);
  std::vector<int> ht((size_t)count);
  GCHK(hipMemcpy(hs.data(), A.sol_coord, hs.size() * sizeof(long long), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(hv.data(), A.vec, hv.size() * sizeof(long long), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(hn.data(), A.norm, hn.size() * sizeof(long long), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(hk.data(), A.nodes, hk.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(ht.data(), A.status, ht.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int w = 0; w < count; ++w)
  {
    if (take_h && !take_h[w])
      continue;
    memcpy(sol_coord + (size_t)w * d, &hs[(size_t)w * d], d * sizeof(int64_t));
    memcpy(vec + (size_t)w * n, &hv[(size_t)w * n], n * sizeof(int64_t));
    norm[w] = hn[w], nodes[w] = hk[w], status[w] = ht[w];
  }
  return FPHIP_OK;
}

// one lattice by the enumerator: true mu and r, row norms / last_useful_index / the initial answer on the host
static int svp_enum_one(fphip_gso *g, fphip_ctx *ectx, int lattice, const double *pruning, int64_t *sol, int64_t *vec,
                        int64_t *norm, uint64_t *nodes, int *status)
{
  const int d = g->P.d, n = g->P.n;
  const size_t dd = (size_t)d, nn = (size_t)n;
  memset(sol, 0, dd * sizeof(int64_t));
  memset(vec, 0, nn * sizeof(int64_t));
  *norm = 0, *nodes = 0, *status = 1;
  std::vector<double> mu(dd * dd), rd(dd);
  std::vector<long long> bh(dd * nn);
  {
    hipStream_t s = fphip_ctx_stream(g->ctx);
    CvpBufs B(s);
    double *bfd_d = nullptr, *mu_d = nullptr, *rd_d = nullptr;
    if (int rc = cvp_unscale(g, lattice, B, &bfd_d, &mu_d, &rd_d))
      return rc;
    GCHK(hipStreamSynchronize(s));
    GCHK(hipMemcpy(mu.data(), mu_d, dd * dd * sizeof(double), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(rd.data(), rd_d, dd * sizeof(double), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy2D(bh.data(), nn * 8, g->P.b + (size_t)lattice * dd * g->P.ldn, (size_t)g->P.ldn * 8, nn * 8, dd,
                     hipMemcpyDeviceToHost));
  }
  std::vector<long long> rn(dd);
  for (size_t i = 0; i < dd; ++i)
  {
    i128 acc = 0;
    for (size_t j = 0; j < nn && acc <= (i128)std::numeric_limits<long long>::max(); ++j)
      acc += (i128)bh[i * nn + j] * (i128)bh[i * nn + j];  // (a square is at most 2^126: one more fits the 127 bits)
    if (acc > (i128)std::numeric_limits<long long>::max())
    {
      *status = -2;
      return FPHIP_OK;
    }
    rn[i] = (long long)acc;
  }
  const int d_eff = svp_last_useful_index(d, rd.data());
  int i0 = 0;
  for (int i = 1; i < d_eff; ++i)
    if (rn[i] < rn[i0])
      i0 = i;
  SvpBest best{d_eff, n, bh.data(), rn[i0], false, std::vector<long long>(dd, 0),
               std::vector<long long>(bh.begin() + (size_t)i0 * nn, bh.begin() + (size_t)(i0 + 1) * nn),
               std::vector<i128>(nn)};
  best.x[i0] = 1;
  if (d_eff >= 2 && best.bound() > 0.0)
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
    o.min_nodes_decline = 0;  // a shortest-vector call can be declined for being small: never here
    std::vector<uint64_t> nd(FPHIP_ENUM_MAX_DIM + 1, 0);
    const int rc = fphip_enum_run(ectx, d_eff, best.bound(), mut.data(), rd.data(), pruning, &o, svp_best_cb, nullptr,
                                  &best, nd.data(), nullptr);
    if (rc != FPHIP_OK)
    {
      if (ectx != g->ctx)
        snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_shortest_vector: enumeration of lattice %d: %s", lattice,
                 fphip_last_error(ectx));
      return rc;
    }
    for (int k = 0; k <= d_eff; ++k)
      *nodes += nd[k];
  }
  if (best.overflow)
  {
    *status = -2;
    *nodes  = 0;
    return FPHIP_OK;
  }
  memcpy(sol, best.x.data(), dd * sizeof(int64_t));
  memcpy(vec, best.v.data(), nn * sizeof(int64_t));
  *norm = best.nbest;
  return FPHIP_OK;
}

extern "C" int fphip_shortest_vector(fphip_gso *g, fphip_ctx *ectx, int first_lattice, int count, int method, int flags,
                                     const double *pruning, int route, int64_t *sol_coord, int64_t *vec, int64_t *norm,
                                     uint64_t *nodes, int *status)
{
  FPHIP_RANGE("fphip_shortest_vector");
  if (!g)
    return FPHIP_ERROR;
  if (!sol_coord || !vec || !norm || !nodes || !status)
    return fail_msg(g->ctx, "fphip_shortest_vector: sol_coord, vec, norm, nodes and status are all required");
  if (!ectx)
    ectx = g->ctx;
  if (first_lattice < 0 || count <= 0 || first_lattice > g->P.batch - count)
    return fail_msg(g->ctx, "fphip_shortest_vector: lattices [first_lattice, first_lattice + count) outside the batch");
  if (int rcg = session_guard(g, "fphip_shortest_vector"))
    return rcg;
  char *err = fphip_ctx_errbuf(g->ctx);
  if (method != FPHIP_SVPM_FAST)
  {
    snprintf(err, 512, "fphip_shortest_vector: method %d (SVPM_PROVED and its exact evaluator, or an unknown one) is not "
             "offered: SVPM_FAST only", method);
    return FPHIP_UNSUPPORTED;
  }
  if (flags != 0)
  {
    snprintf(err, 512, "fphip_shortest_vector: flags 0x%x (SVP_DUAL, SVP_OVERRIDE_BND, or unknown ones) are not offered: "
             "0 only", flags);
    return FPHIP_UNSUPPORTED;
  }
  const int d = g->P.d;
  if (route != FPHIP_SVP_ROUTE_AUTO && route != FPHIP_SVP_ROUTE_WAVE && route != FPHIP_SVP_ROUTE_ENUM)
    return fail_msg(g->ctx, "fphip_shortest_vector: unknown route");
  if (route == FPHIP_SVP_ROUTE_WAVE && d > 64)
  {
    snprintf(err, 512, "fphip_shortest_vector: the WAVE route takes at most 64 rows (d = %d): use the ENUM route", d);
    return FPHIP_UNSUPPORTED;
  }
  if (d > FPHIP_ENUM_MAX_DIM)
  {
    snprintf(err, 512, "fphip_shortest_vector: more than %d rows", FPHIP_ENUM_MAX_DIM);
    return FPHIP_UNSUPPORTED;
  }
  if (pruning)
    for (int i = 0; i < d; ++i)
      if (!(pruning[i] > 0.0) || !std::isfinite(pruning[i]))
        return fail_msg(g->ctx, "fphip_shortest_vector: a pruning coefficient that is not a positive finite number");
  std::vector<int> gst(g->P.batch, 0);
  if (int rc = fphip_gso_update(g, gst.data()))
    return rc;
  g->last_ms = 0.0f;
  // the route of every lattice of the range: 1 = WAVE
  std::vector<int> take((size_t)count, route == FPHIP_SVP_ROUTE_ENUM || d > 64 ? 0 : 1);
  if (route == FPHIP_SVP_ROUTE_AUTO && d <= 64)
  {
    const char *e    = getenv("FPHIP_SVP_WAVE_MAX_NODES");
    const double lim = e ? atof(e) : SVP_WAVE_MAX_NODES_DEFAULT;
    if (lim > 0.0)
    {
      const size_t dd = (size_t)d;
      std::vector<double> rs((size_t)count * dd);
      std::vector<long long> es((size_t)count * dd);
      GCHK(hipMemcpy(rs.data(), g->P.rdg + (size_t)first_lattice * dd, rs.size() * sizeof(double), hipMemcpyDeviceToHost));
      GCHK(hipMemcpy(es.data(), g->P.rexp + (size_t)first_lattice * dd, es.size() * sizeof(long long), hipMemcpyDeviceToHost));
      std::vector<double> rd(dd);
      for (int w = 0; w < count; ++w)
      {
        if (gst[first_lattice + w] != 1)
          continue;  // (the kernel reports it)
        for (size_t i = 0; i < dd; ++i)
          rd[i] = std::ldexp(rs[(size_t)w * dd + i], g->P.row_expo ? (int)(2 * es[(size_t)w * dd + i]) : 0);
        const int d_eff = svp_last_useful_index(d, rd.data());
        bool pos = true;
        for (int i = 0; i < d_eff; ++i)
          pos = pos && rd[i] > 0.0 && std::isfinite(rd[i]);
        if (!pos)
          continue;
        // the radius of the estimate: r_00, or the squared Gaussian-heuristic length of the lattice where that is
        // smaller — the walk's radius falls to about that length early, and r_00 can be several times it
        double logdet = 0.0;
        for (int i = 0; i < d_eff; ++i)
          logdet += std::log(rd[i]);
        const double gh2 = std::exp((2.0 / d_eff) * (std::lgamma(0.5 * d_eff + 1.0) - 0.5 * d_eff * std::log(M_PI) + 0.5 * logdet));
        if (fphip_enum_gh_nodes(d_eff, rd.data(), pruning, std::min(rd[0], gh2)) > lim)
          take[w] = 0;
      }
    }
  }
  const bool any_wave = std::find(take.begin(), take.end(), 1) != take.end();
  const bool all_wave = std::find(take.begin(), take.end(), 0) == take.end();
  if (any_wave)
    if (int rc = svp_wave_run(g, first_lattice, count, pruning, all_wave ? nullptr : take.data(), sol_coord, vec, norm,
                              nodes, status))
      return rc;
  const float wave_ms = g->last_ms;
  const size_t dd = (size_t)d, nn = (size_t)g->P.n;
  for (int w = 0; w < count; ++w)
  {
    if (take[w])
      continue;
    if (gst[first_lattice + w] != 1)
    {
      memset(sol_coord + (size_t)w * dd, 0, dd * sizeof(int64_t));
      memset(vec + (size_t)w * nn, 0, nn * sizeof(int64_t));
      norm[w] = 0, nodes[w] = 0, status[w] = 0;
      continue;
    }
    if (int rc = svp_enum_one(g, ectx, first_lattice + w, pruning, sol_coord + (size_t)w * dd, vec + (size_t)w * nn,
                              norm + w, nodes + w, status + w))
      return rc;
  }
  g->last_ms = wave_ms;
  return FPHIP_OK;
}

// ---- the N shortest vectors (svp_best.hip; the ENUM route: fphip_enum_run under a host table) ------------------------
// (the table, the rows under enumeration and the walk of a single row are in svp_host.h: the quadratic forms'
//  entry point of gram_host.hip uses them as well)

// the wave-per-lattice kernel over the range; outputs of the lattices with take_h[w] == 0 are left alone
static int svp_best_wave_run(fphip_gso *g, int first, int count, int K, const int64_t *bound_sq, const double *pruning,
                             const int *take_h, int *found, int64_t *sol_coord, int64_t *vec, int64_t *norm,
                             uint64_t *nodes, int *status)
{
  const size_t d = g->P.d, n = g->P.n, kk = (size_t)K;
  const int nq   = (int)((std::max(d, n) + 63) / 64);
  int wpb        = 4;
  SvpBestWave A;
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
  int cap  = fphip_ctx_num_cus(g->ctx) * std::max(bpc, 1);
  if (const char *e = getenv("FPHIP_SVP_WAVE_GRID"))  // (tests: a small grid makes a small batch go round the grid-stride loop)
    cap = std::max(1, atoi(e));
  grid = std::min(grid, cap);
  hipStream_t s = fphip_ctx_stream(g->ctx);
  CvpBufs B(s);
  double *pr_d = nullptr;
  int *take_d  = nullptr;
  long long *bound_d = nullptr;
  GCHK(B.get(&A.rec, (size_t)count * kk * d));
  GCHK(B.get(&A.sol_coord, (size_t)count * kk * d));
  GCHK(B.get(&A.vec, (size_t)count * kk * n));
  GCHK(B.get(&A.norm, (size_t)count * kk));
  GCHK(B.get(&A.found, (size_t)count));
  GCHK(B.get(&A.nodes, (size_t)count));
  GCHK(B.get(&A.status, (size_t)count));
  if (pruning)
  {
    GCHK(B.get(&pr_d, d));
    GCHK(hipMemcpy(pr_d, pruning, d * sizeof(double), hipMemcpyHostToDevice));
  }
  if (take_h)
  {
    GCHK(B.get(&take_d, (size_t)count));
    GCHK(hipMemcpy(take_d, take_h, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
  }
  if (bound_sq)
  {
    GCHK(B.get(&bound_d, (size_t)count));
    GCHK(hipMemcpy(bound_d, bound_sq, (size_t)count * sizeof(long long), hipMemcpyHostToDevice));
  }
  GCHK(hipStreamSynchronize(nullptr));  // (see fphip_gso_set_basis)
  A.pruning = pr_d;
  A.take    = take_d;
  A.bound   = bound_d;
  if (lds > 64 * 1024)
    GCHK(dispatch_nq(nq, [&](auto NQ) { return allow_lds(svp_best_kernel<NQ>, lds); }));
  GCHK(hipEventRecord(g->ev[0], s));
  dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL(svp_best_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, g->P, A); });
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(g->ev[1], s));
  GCHK(hipStreamSynchronize(s));
  GCHK(hipEventElapsedTime(&g->last_ms, g->ev[0], g->ev[1]));
  if (!take_h)
  {  // the whole range: straight into the caller's arrays
    GCHK(hipMemcpy(sol_coord, A.sol_coord, (size_t)count * kk * d * sizeof(long long), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(vec, A.vec, (size_t)count * kk * n * sizeof(long long), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(norm, A.norm, (size_t)count * kk * sizeof(long long), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(found, A.found, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(nodes, A.nodes, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(status, A.status, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    return FPHIP_OK;
  }
  for (int w = 0; w < count; ++w)
  {
    if (!take_h[w])
      continue;
    GCHK(hipMemcpy(sol_coord + (size_t)w * kk * d, A.sol_coord + (size_t)w * kk * d, kk * d * sizeof(long long), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(vec + (size_t)w * kk * n, A.vec + (size_t)w * kk * n, kk * n * sizeof(long long), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(norm + (size_t)w * kk, A.norm + (size_t)w * kk, kk * sizeof(long long), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(found + w, A.found + w, sizeof(int), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(nodes + w, A.nodes + w, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(status + w, A.status + w, sizeof(int), hipMemcpyDeviceToHost));
  }
  return FPHIP_OK;
}

// one lattice by the enumerator under the host table; outputs [K][d], [K][n], [K]
static int svp_best_enum_one(fphip_gso *g, fphip_ctx *ectx, int lattice, int K, long long bound, const double *pruning,
                             int *found, int64_t *sol, int64_t *vec, int64_t *norm, uint64_t *nodes, int *status)
{
  const int d = g->P.d, n = g->P.n;
  const size_t dd = (size_t)d, nn = (size_t)n, kk = (size_t)K;
  memset(sol, 0, kk * dd * sizeof(int64_t));
  memset(vec, 0, kk * nn * sizeof(int64_t));
  memset(norm, 0, kk * sizeof(int64_t));
  *found = 0, *nodes = 0, *status = 1;
  std::vector<double> mu(dd * dd), rd(dd);
  std::vector<long long> bh(dd * nn);
  {
    hipStream_t s = fphip_ctx_stream(g->ctx);
    CvpBufs B(s);
    double *bfd_d = nullptr, *mu_d = nullptr, *rd_d = nullptr;
    if (int rc = cvp_unscale(g, lattice, B, &bfd_d, &mu_d, &rd_d))
      return rc;
    GCHK(hipStreamSynchronize(s));
    GCHK(hipMemcpy(mu.data(), mu_d, dd * dd * sizeof(double), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(rd.data(), rd_d, dd * sizeof(double), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy2D(bh.data(), nn * 8, g->P.b + (size_t)lattice * dd * g->P.ldn, (size_t)g->P.ldn * 8, nn * 8, dd,
                     hipMemcpyDeviceToHost));
  }
  std::vector<long long> rn(dd);
  for (size_t i = 0; i < dd; ++i)
  {
    i128 acc = 0;
    for (size_t j = 0; j < nn && acc <= (i128)std::numeric_limits<long long>::max(); ++j)
      acc += (i128)bh[i * nn + j] * (i128)bh[i * nn + j];
    if (acc > (i128)std::numeric_limits<long long>::max())
    {
      *status = -2;
      return FPHIP_OK;
    }
    rn[i] = (long long)acc;
  }
  long long B0 = bound;
  int d_eff;
  if (bound > 0)
    d_eff = svp_best_rows(d, rd.data(), true, (double)bound * (1.0 + 0x1p-30));
  else
  {
    d_eff = svp_best_rows(d, rd.data(), false, 0.0);
    B0    = *std::min_element(rn.begin(), rn.begin() + d_eff);
  }
  SvpTable<SvpBest> T{SvpBest{d_eff, n, bh.data(), 0, false, {}, {}, std::vector<i128>(nn)}, K, B0, {}, {}};
  if (T.radius0() > 0.0)
  {
    if (d_eff == 1)
      *nodes = svp_table_line(&T, rd[0], pruning ? pruning[0] : 1.0);  // the multiples of b_0
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
      const int rc = fphip_enum_run(ectx, d_eff, T.radius0(), mut.data(), rd.data(), pruning, &o, svp_table_cb<SvpBest>, nullptr, &T,
                                    nd.data(), nullptr);
      if (rc != FPHIP_OK)
      {
        if (ectx != g->ctx)
          snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_shortest_vectors: enumeration of lattice %d: %s", lattice,
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
  std::vector<double> xd((size_t)d_eff);
  for (size_t o = 0; o < ord.size(); ++o)
  {
    const std::vector<long long> &xi = T.x[ord[o]];
    for (int i = 0; i < d_eff; ++i)
      sol[o * dd + i] = xi[i], xd[i] = (double)xi[i];
    long long nv = 0;
    svp_exact_candidate(&T.cand, xd.data(), &nv);  // (it fitted when it was offered; the coefficients came as doubles)
    for (size_t j = 0; j < nn; ++j)
      vec[o * nn + j] = (long long)T.cand.w[j];
    norm[o] = T.norms[ord[o]];
  }
  *found = (int)ord.size();
  return FPHIP_OK;
}

extern "C" int fphip_shortest_vectors(fphip_gso *g, fphip_ctx *ectx, int first_lattice, int count, int max_sols,
                                      const int64_t *bound_sq, int method, int flags, const double *pruning, int route,
                                      int *found, int64_t *sol_coord, int64_t *vec, int64_t *norm, uint64_t *nodes,
                                      int *status)
{
  FPHIP_RANGE("fphip_shortest_vectors");
  if (!g)
    return FPHIP_ERROR;
  if (!found || !sol_coord || !vec || !norm || !nodes || !status)
    return fail_msg(g->ctx, "fphip_shortest_vectors: found, sol_coord, vec, norm, nodes and status are all required");
  if (!ectx)
    ectx = g->ctx;
  if (first_lattice < 0 || count <= 0 || first_lattice > g->P.batch - count)
    return fail_msg(g->ctx, "fphip_shortest_vectors: lattices [first_lattice, first_lattice + count) outside the batch");
  char *err = fphip_ctx_errbuf(g->ctx);
  if (max_sols < 1 || max_sols > 64)
  {
    snprintf(err, 512, "fphip_shortest_vectors: max_sols = %d is outside 1 .. 64: for longer lists use short_vectors "
             "(fphip_list_vectors), every vector within a radius", max_sols);
    return FPHIP_ERROR;
  }
  bool any_bound = false;
  if (bound_sq)
    for (int w = 0; w < count; ++w)
    {
      if (bound_sq[w] < 0)
        return fail_msg(g->ctx, "fphip_shortest_vectors: a negative bound_sq (0 = the default bound)");
      any_bound = any_bound || bound_sq[w] > 0;
    }
  if (int rcg = session_guard(g, "fphip_shortest_vectors"))
    return rcg;
  if (method != FPHIP_SVPM_FAST)
  {
    snprintf(err, 512, "fphip_shortest_vectors: method %d (SVPM_PROVED and its exact evaluator, or an unknown one) is not "
             "offered: SVPM_FAST only", method);
    return FPHIP_UNSUPPORTED;
  }
  if (flags != 0)
  {
    snprintf(err, 512, "fphip_shortest_vectors: flags 0x%x (SVP_DUAL, SVP_OVERRIDE_BND, or unknown ones) are not offered: "
             "0 only", flags);
    return FPHIP_UNSUPPORTED;
  }
  const int d = g->P.d, K = max_sols;
  if (route != FPHIP_SVP_ROUTE_AUTO && route != FPHIP_SVP_ROUTE_WAVE && route != FPHIP_SVP_ROUTE_ENUM)
    return fail_msg(g->ctx, "fphip_shortest_vectors: unknown route");
  if (route == FPHIP_SVP_ROUTE_WAVE && d > 64)
  {
    snprintf(err, 512, "fphip_shortest_vectors: the WAVE route takes at most 64 rows (d = %d): use the ENUM route", d);
    return FPHIP_UNSUPPORTED;
  }
  if (d > FPHIP_ENUM_MAX_DIM)
  {
    snprintf(err, 512, "fphip_shortest_vectors: more than %d rows", FPHIP_ENUM_MAX_DIM);
    return FPHIP_UNSUPPORTED;
  }
  if (pruning)
    for (int i = 0; i < d; ++i)
      if (!(pruning[i] > 0.0) || !std::isfinite(pruning[i]))
        return fail_msg(g->ctx, "fphip_shortest_vectors: a pruning coefficient that is not a positive finite number");
  std::vector<int> gst(g->P.batch, 0);
  if (int rc = fphip_gso_update(g, gst.data()))
    return rc;
  g->last_ms = 0.0f;
  const size_t dd = (size_t)d, nn = (size_t)g->P.n, kk = (size_t)K;
  // the route of every lattice of the range: 1 = WAVE
  std::vector<int> take((size_t)count, route == FPHIP_SVP_ROUTE_ENUM || d > 64 ? 0 : 1);
  if (route == FPHIP_SVP_ROUTE_AUTO && d <= 64)
  {
    const char *e    = getenv("FPHIP_SVP_WAVE_MAX_NODES");
    const double lim = e ? atof(e) : SVP_WAVE_MAX_NODES_DEFAULT;
    if (lim > 0.0)
    {
      const bool as_one = K == 1 && !any_bound;  // the decision of fphip_shortest_vector
      std::vector<double> rs((size_t)count * dd);
      std::vector<long long> es((size_t)count * dd), bh;
      GCHK(hipMemcpy(rs.data(), g->P.rdg + (size_t)first_lattice * dd, rs.size() * sizeof(double), hipMemcpyDeviceToHost));
      GCHK(hipMemcpy(es.data(), g->P.rexp + (size_t)first_lattice * dd, es.size() * sizeof(long long), hipMemcpyDeviceToHost));
      std::vector<double> rd(dd);
      for (int w = 0; w < count; ++w)
      {
        if (gst[first_lattice + w] != 1)
          continue;  // (the kernel reports it)
        for (size_t i = 0; i < dd; ++i)
          rd[i] = std::ldexp(rs[(size_t)w * dd + i], g->P.row_expo ? (int)(2 * es[(size_t)w * dd + i]) : 0);
        const long long bw = bound_sq ? bound_sq[w] : 0;
        const int d_eff    = svp_best_rows(d, rd.data(), bw > 0, (double)bw * (1.0 + 0x1p-30));
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
        {  // B0 = N0: the shortest row below d_eff, here from the rows' doubles (an estimate's radius)
          bh.resize(dd * nn);
          GCHK(hipMemcpy2D(bh.data(), nn * 8, g->P.b + (size_t)(first_lattice + w) * dd * g->P.ldn, (size_t)g->P.ldn * 8,
                           nn * 8, dd, hipMemcpyDeviceToHost));
          radius = std::numeric_limits<double>::infinity();
          for (int i = 0; i < d_eff; ++i)
          {
            double acc = 0.0;
            for (size_t j = 0; j < nn; ++j)
              acc += (double)bh[i * nn + j] * (double)bh[i * nn + j];
            radius = std::min(radius, acc);
          }
        }
        // the radius never falls below the K-th norm: B0 is the safe side of the estimate
        if (fphip_enum_gh_nodes(d_eff, rd.data(), pruning, radius) > lim)
          take[w] = 0;
      }
    }
  }
  const bool any_wave = std::find(take.begin(), take.end(), 1) != take.end();
  const bool all_wave = std::find(take.begin(), take.end(), 0) == take.end();
  if (any_wave)
    if (int rc = svp_best_wave_run(g, first_lattice, count, K, bound_sq, pruning, all_wave ? nullptr : take.data(), found,
                                   sol_coord, vec, norm, nodes, status))
      return rc;
  const float wave_ms = g->last_ms;
  for (int w = 0; w < count; ++w)
  {
    if (take[w])
      continue;
    if (gst[first_lattice + w] != 1)
    {
      memset(sol_coord + (size_t)w * kk * dd, 0, kk * dd * sizeof(int64_t));
      memset(vec + (size_t)w * kk * nn, 0, kk * nn * sizeof(int64_t));
      memset(norm + (size_t)w * kk, 0, kk * sizeof(int64_t));
      found[w] = 0, nodes[w] = 0, status[w] = 0;
      continue;
    }
    if (int rc = svp_best_enum_one(g, ectx, first_lattice + w, K, bound_sq ? bound_sq[w] : 0, pruning, found + w,
                                   sol_coord + (size_t)w * kk * dd, vec + (size_t)w * kk * nn, norm + (size_t)w * kk,
                                   nodes + w, status + w))
      return rc;
  }
  g->last_ms = wave_ms;
  return FPHIP_OK;
}

// ---- lists of short / near vectors (list_vectors.hip; the enumeration: fphip_enum_list) ----------------------------
// the vector kernel over m records of one lattice: vec [m][n], norm [m], status [m]
static int list_vectors_run(fphip_gso *g, int lattice, uint64_t m, const int64_t *coef, const int64_t *target, int64_t *vec,
                            int64_t *norm, int *status)
{
  const size_t d = g->P.d, n = g->P.n, ldt = ((size_t)m + 63) / 64 * 64;
  hipStream_t s = fphip_ctx_stream(g->ctx);
  CvpBufs B(s);
  ListVec P;
  memset(&P, 0, sizeof P);
  long long *cd = nullptr, *td = nullptr;
  GCHK(B.get(&cd, (size_t)m * d));
  GCHK(B.get(&td, n));
  GCHK(B.get(&P.vec, (size_t)m * n));
  GCHK(B.get(&P.norm, (size_t)m));
  GCHK(B.get(&P.status, (size_t)m));
  GCHK(B.get(&P.wv, n * ldt));
  GCHK(hipMemcpy(cd, coef, (size_t)m * d * sizeof(long long), hipMemcpyHostToDevice));
  if (target)
    GCHK(hipMemcpy(td, target, n * sizeof(long long), hipMemcpyHostToDevice));
  GCHK(hipStreamSynchronize(nullptr));  // (see fphip_gso_set_basis)
  P.m = (int)m, P.ldt = (int)ldt, P.d = (int)d, P.n = (int)n, P.ldn = g->P.ldn;
  P.b      = g->P.b + (size_t)lattice * d * g->P.ldn;
  P.coef   = cd;
  P.target = target ? td : nullptr;
  GCHK(hipEventRecord(g->ev[0], s));
  hipLaunchKernelGGL(list_vectors_kernel, dim3((unsigned)(ldt / 64)), dim3(64), 0, s, P);
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(g->ev[1], s));
  GCHK(hipStreamSynchronize(s));
  GCHK(hipEventElapsedTime(&g->last_ms, g->ev[0], g->ev[1]));
  GCHK(hipMemcpy(vec, P.vec, (size_t)m * n * sizeof(long long), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(norm, P.norm, (size_t)m * sizeof(long long), hipMemcpyDeviceToHost));
  GCHK(hipMemcpy(status, P.status, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

extern "C" int fphip_list_records_to_vectors(fphip_gso *g, int lattice, uint64_t m, const int64_t *coef,
                                             const int64_t *target, int64_t *vec, int64_t *norm, int *status)
{
  FPHIP_RANGE("fphip_list_records_to_vectors");
  if (!g || !coef || !vec || !norm || !status)
    return FPHIP_ERROR;
  if (int rc = cvp_lattice_guard(g, lattice, m > 0 && m < (1ull << 31) ? 1 : 0, "fphip_list_records_to_vectors"))
    return rc;
  return list_vectors_run(g, lattice, m, coef, target, vec, norm, status);
}

// Every lattice vector v of one lattice with |v - t|^2 <= bound_sq, exactly: update_gso, the true mu and r, with a
// target its Gram-Schmidt coordinates (get_gscoords, the operation sequence of cvp_prepare_kernel; no Babai
// reduction: the radius is the caller's), a list enumeration at bound_sq (1 + 2^-30), the vector kernel, and the
// filter norm <= bound_sq on the exact integers.  The 2^-30 is the margin of fphip_closest_vector: a heuristic
// allowance for the rounding of the enumeration's doubles, not a proved error bound (the reference enlarges its
// radius by get_max_error_aux there).
extern "C" int fphip_list_vectors(fphip_gso *g, fphip_ctx *ectx, int lattice, const int64_t *target, int64_t bound_sq,
                                  uint64_t cap, int64_t *coef, int64_t *vec, int64_t *norm, uint64_t *count)
{
  FPHIP_RANGE("fphip_list_vectors");
  if (!g || !count || (cap > 0 && (!coef || !vec || !norm)))
    return FPHIP_ERROR;
  if (!ectx)
    ectx = g->ctx;
  *count = 0;
  if (int rc = cvp_lattice_guard(g, lattice, 1, "fphip_list_vectors"))
    return rc;
  if (bound_sq < 0)
    return fail_msg(g->ctx, "fphip_list_vectors: a negative bound");
  const int d = g->P.d;
  const size_t dd = (size_t)d, n = (size_t)g->P.n;
  if (d > 64)
  {
    snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_list_vectors: more than 64 rows (list enumeration)");
    return FPHIP_UNSUPPORTED;
  }
  std::vector<int> gst(g->P.batch, 0);
  if (int rc = fphip_gso_update(g, gst.data()))
    return rc;
  if (gst[lattice] != 1)
    return fail_msg(g->ctx, "fphip_list_vectors: update_gso failed (non-finite mu: RED_GSO_FAILURE)");
  std::vector<double> mu(dd * dd), rd(dd), bfd(dd * n), mut(dd * dd, 0.0), tc(dd, 0.0);
  {
    hipStream_t s = fphip_ctx_stream(g->ctx);
    CvpBufs B(s);
    double *bfd_d = nullptr, *mu_d = nullptr, *rd_d = nullptr;
    if (int rc = cvp_unscale(g, lattice, B, &bfd_d, &mu_d, &rd_d))
      return rc;
    GCHK(hipStreamSynchronize(s));
    GCHK(hipMemcpy(mu.data(), mu_d, dd * dd * sizeof(double), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(rd.data(), rd_d, dd * sizeof(double), hipMemcpyDeviceToHost));
    GCHK(hipMemcpy(bfd.data(), bfd_d, dd * n * sizeof(double), hipMemcpyDeviceToHost));
  }
  for (size_t i = 0; i < dd; ++i)
    for (size_t j = i + 1; j < dd; ++j)
      mut[i * dd + j] = mu[j * dd + i];  // the layout a plugin receives: mut[i][j] = mu(j,i), j > i
  // a target far from the origin (a lattice point with large coefficients, or entries beyond 2^53, plus a small offset)
  // loses the offset when its coordinates are formed in double: the closest-vector solver's preparation (the Babai loop
  // in exact integers, cvp_prepare_kernel) moves it next to the origin first, and its coefficients are added back to
  // every record.  A target that is near the origin already comes back unchanged (shift 0, the same coordinates).
  std::vector<int64_t> shift(dd, 0);
  bool prepared = false;
  if (target)
  {
    std::vector<double> ptc(dd);
    std::vector<int64_t> pc(dd);
    double pdesc = 0.0;
    int pst      = 0;
    if (int rc = cvp_prepare_run(g, lattice, 1, target, pc.data(), ptc.data(), &pdesc, &pst, nullptr, nullptr))
      return rc;
    if (pst == 1)
      shift = pc, tc = ptc, prepared = true;
  }
  if (target && !prepared)
  {  // get_gscoords (svpcvp.cpp:494-515), the loops of cvp_prepare_kernel in its operand order
    for (size_t i = 0; i < dd; ++i)
    {
      double acc = 0.0;
      for (size_t j = 0; j < n; ++j)
        acc = acc + (double)target[j] * bfd[i * n + j];
      for (size_t j = 0; j < i; ++j)
        acc = acc - mu[i * dd + j] * tc[j];
      tc[i] = acc;
    }
    for (size_t i = 0; i < dd; ++i)
      tc[i] = tc[i] / rd[i];
  }
  const double radius = (double)bound_sq + (double)bound_sq * 0x1p-30;
  std::vector<uint64_t> nodes(dd + 1);
  std::vector<double> ld, lx;
  uint64_t icap = std::max<uint64_t>(cap, 4096), found = 0;
  for (int attempt = 0;; ++attempt)
  {  // (the count is exact whatever the capacity: a list that did not fit is enumerated once more, with room for it)
    ld.resize((size_t)icap);
    lx.resize((size_t)icap * dd);
    const int rc = fphip_enum_list(ectx, d, radius, mut.data(), rd.data(), nullptr, target ? tc.data() : nullptr, icap,
                                   ld.data(), lx.data(), &found, nodes.data(), nullptr);
    if (rc != FPHIP_OK)
    {
      if (ectx != g->ctx)
        snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_list_vectors: enumeration: %s", fphip_last_error(ectx));
      return rc;
    }
    if (found <= icap)
      break;
    if (attempt > 0)
      return fail_msg(g->ctx, "fphip_list_vectors: the list changed its length between two enumerations");
    icap = found;
  }
  if (found == 0)
    return FPHIP_OK;
  std::vector<int64_t> rc_coef((size_t)found * dd), rvec((size_t)found * n), rnorm((size_t)found);
  std::vector<int> rst((size_t)found);
  for (size_t i = 0; i < (size_t)found * dd; ++i)
  {
    if (!(std::fabs(lx[i]) < 9223372036854775808.0))
      return fail_msg(g->ctx, "fphip_list_vectors: a coefficient beyond the int64 range");
    long long ci = 0;
    if (__builtin_add_overflow((long long)lx[i], (long long)shift[i % dd], &ci))
      return fail_msg(g->ctx, "fphip_list_vectors: a coefficient beyond the int64 range");
    rc_coef[i] = ci;
  }
  if (int rc = list_vectors_run(g, lattice, found, rc_coef.data(), target, rvec.data(), rnorm.data(), rst.data()))
    return rc;
  // the filter on the exact norm, then (norm, canonical coefficient order: from level d - 1 down)
  std::vector<size_t> keep;
  for (size_t i = 0; i < (size_t)found; ++i)
  {
    if (rst[i] != 1)
    {
      snprintf(fphip_ctx_errbuf(g->ctx), 512, "fphip_list_vectors: a vector within the radius leaves the int64 range");
      return FPHIP_UNSUPPORTED;
    }
    if (rnorm[i] <= bound_sq)
      keep.push_back(i);
  }
  std::sort(keep.begin(), keep.end(), [&](size_t a, size_t b) {
    if (rnorm[a] != rnorm[b])
      return rnorm[a] < rnorm[b];
    for (size_t k = dd; k-- > 0;)
      if (rc_coef[a * dd + k] != rc_coef[b * dd + k])
        return rc_coef[a * dd + k] < rc_coef[b * dd + k];
    return a < b;
  });
  *count = keep.size();
  for (size_t o = 0; o < keep.size() && o < (size_t)cap; ++o)
  {
    memcpy(coef + o * dd, &rc_coef[keep[o] * dd], dd * sizeof(int64_t));
    memcpy(vec + o * n, &rvec[keep[o] * n], n * sizeof(int64_t));
    norm[o] = rnorm[keep[o]];
  }
  return FPHIP_OK;
}

extern "C" double fphip_gso_last_kernel_ms(const fphip_gso *g) { return g ? g->last_ms : 0.0; }

// FETCH_SIZE calibration (not part of the product ABI; used by tests/perf/calib_fetch.py only)
extern "C" int fphip_debug_stream(fphip_ctx *ctx, long long rows, int row_bytes, long long stride,
                                  double *ms_out)
{
  char *buf = nullptr;
  const size_t total = (size_t)rows * (size_t)stride + 4096;
  if (fphip_dev_alloc((void **)&buf, total, fphip_ctx_stream(ctx)) != hipSuccess)
    return FPHIP_ERROR;
  hipMemset(buf, 1, total);
  hipDeviceSynchronize();
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipStream_t s = fphip_ctx_stream(ctx);
  hipEventRecord(e0, s);
  hipLaunchKernelGGL(gso_calib_kernel, dim3(fphip_ctx_num_cus(ctx) * 2), dim3(256), 4 * 8 * 2048, s, buf,
                     (size_t)stride, row_bytes, rows);
  hipEventRecord(e1, s);
  hipStreamSynchronize(s);
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  if (ms_out)
    *ms_out = ms;
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  fphip_dev_free(buf, fphip_ctx_stream(ctx));
  return FPHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// Batched Householder R-factor: MatHouseholder<Z_NR<long>, FP_NR<double>> refresh_R_bf() +
// update_R() (fplll/householder.h:532-536, 610-614)
// ---------------------------------------------------------------------------------------------
struct fphip_hh
{
  fphip_ctx *ctx;
  HhBatch P;
  hipEvent_t ev[2];
  float last_ms;
  double *Tbuf;  // blocked (MFMA) mode only: T of every block of 16 reflectors, [batch][ceil(d/16)][256]
  // extended-precision HLLL (hlll_x.hip): low planes of R and V, per-row scalars
  double *Rlo, *Vlo, *xsc;
  long long *xprevE;
  double *xThi = nullptr, *xTlo = nullptr;  // hlll_x: T of every block of 16 reflectors (blocked application)
  double *xRx = nullptr, *xVx = nullptr;    // hlll_x in quad-double: components 2 and 3 of R and V
  int x_planes = 0;                         // component planes of R the last fphip_hh_hlll_ex run wrote (0: none yet)
  // the transformation matrix (fphip_hh_enable_transform), [batch][d][ldu]; null = not tracked.  Kept out of HhBatch:
  // that struct is a by-value argument of every Householder kernel, the u kernels take the two as extra parameters
  long long *u = nullptr;
  int ldu      = 0;
};

#define HCHK(call) CHK(h->ctx, call)

static int hh_allocate(fphip_hh *h);
extern "C" void fphip_hh_destroy(fphip_hh *h);

extern "C" int fphip_hh_create(fphip_ctx *ctx, int batch, int d, int n, int row_expo, fphip_hh **out)
{
  if (!ctx || !out)
    return FPHIP_ERROR;
  *out = nullptr;
  if (batch <= 0 || d <= 0 || n <= 0 || !fphip_ctx_stream(ctx))
  {
    snprintf(fphip_ctx_errbuf(ctx), 512, "fphip_hh_create: bad arguments or no device");
    return FPHIP_ERROR;
  }
  if (d > 256 || n > 256)
    return FPHIP_UNSUPPORTED;
  fphip_hh *h = new fphip_hh();
  memset(h, 0, sizeof *h);
  h->ctx        = ctx;
  h->P.batch    = batch;
  h->P.d        = d;
  h->P.n        = n;
  h->P.ldn      = (n + 15) / 16 * 16;
  if (h->P.ldn > 256)
    h->P.ldn = 256;
  h->P.row_expo = row_expo ? 1 : 0;
  const int rc  = hh_allocate(h);
  if (rc != FPHIP_OK)
  {
    fphip_hh_destroy(h);
    return rc;
  }
  *out = h;
  return FPHIP_OK;
}

static int hh_allocate(fphip_hh *h)
{
  const int batch = h->P.batch, d = h->P.d;
  const size_t B = (size_t)batch, ld = h->P.ldn, pad = 4096;
  HCHK(fphip_dev_alloc((void **)&h->P.b, B * d * ld * 8 + pad, fphip_ctx_stream(h->ctx)));
  HCHK(fphip_dev_alloc((void **)&h->P.V, B * d * ld * 8 + pad, fphip_ctx_stream(h->ctx)));
  HCHK(fphip_dev_alloc((void **)&h->P.R, B * d * ld * 8 + pad, fphip_ctx_stream(h->ctx)));
  HCHK(fphip_dev_alloc((void **)&h->P.sigma, B * d * 8, fphip_ctx_stream(h->ctx)));
  HCHK(fphip_dev_alloc((void **)&h->P.rexp, B * d * 8, fphip_ctx_stream(h->ctx)));
  HCHK(fphip_dev_alloc((void **)&h->P.status, B * sizeof(int), fphip_ctx_stream(h->ctx)));
  HCHK(hipMemsetAsync(h->P.b, 0, B * d * ld * 8 + pad, fphip_ctx_stream(h->ctx)));
  HCHK(hipMemsetAsync(h->P.V, 0, B * d * ld * 8 + pad, fphip_ctx_stream(h->ctx)));
  HCHK(hipMemsetAsync(h->P.R, 0, B * d * ld * 8 + pad, fphip_ctx_stream(h->ctx)));
  HCHK(hipStreamSynchronize(fphip_ctx_stream(h->ctx)));  // uploads use blocking copies on the null stream
  HCHK(hipEventCreate(&h->ev[0]));
  HCHK(hipEventCreate(&h->ev[1]));
  return FPHIP_OK;
}

extern "C" void fphip_hh_destroy(fphip_hh *h)
{
  if (!h)
    return;
  hipStreamSynchronize(fphip_ctx_stream(h->ctx));
  fphip_dev_free(h->P.b, fphip_ctx_stream(h->ctx));
  fphip_dev_free(h->P.V, fphip_ctx_stream(h->ctx));
  fphip_dev_free(h->P.R, fphip_ctx_stream(h->ctx));
  fphip_dev_free(h->P.sigma, fphip_ctx_stream(h->ctx));
  fphip_dev_free(h->P.rexp, fphip_ctx_stream(h->ctx));
  fphip_dev_free(h->P.status, fphip_ctx_stream(h->ctx));
  if (h->P.bf)
    fphip_dev_free(h->P.bf, fphip_ctx_stream(h->ctx));
  if (h->P.info)
    fphip_dev_free(h->P.info, fphip_ctx_stream(h->ctx));
  if (h->ev[0])
    hipEventDestroy(h->ev[0]);
  if (h->ev[1])
    hipEventDestroy(h->ev[1]);
  if (h->Tbuf)
    fphip_dev_free(h->Tbuf, fphip_ctx_stream(h->ctx));
  if (h->Rlo)
    fphip_dev_free(h->Rlo, fphip_ctx_stream(h->ctx));
  if (h->Vlo)
    fphip_dev_free(h->Vlo, fphip_ctx_stream(h->ctx));
  if (h->xsc)
    fphip_dev_free(h->xsc, fphip_ctx_stream(h->ctx));
  if (h->xprevE)
    fphip_dev_free(h->xprevE, fphip_ctx_stream(h->ctx));
  if (h->xThi)
    fphip_dev_free(h->xThi, fphip_ctx_stream(h->ctx));
  if (h->xTlo)
    fphip_dev_free(h->xTlo, fphip_ctx_stream(h->ctx));
  if (h->xRx)
    fphip_dev_free(h->xRx, fphip_ctx_stream(h->ctx));
  if (h->xVx)
    fphip_dev_free(h->xVx, fphip_ctx_stream(h->ctx));
  if (h->u)
    fphip_dev_free(h->u, fphip_ctx_stream(h->ctx));
  delete h;
}

extern "C" int fphip_hh_set_basis(fphip_hh *h, int first, int count, const int64_t *b)
{
  if (!h || !b || first < 0 || count <= 0 || first + count > h->P.batch)
    return FPHIP_ERROR;
  HCHK(hipMemcpy2D(h->P.b + (size_t)first * h->P.d * h->P.ldn, (size_t)h->P.ldn * 8, b,
                   (size_t)h->P.n * 8, (size_t)h->P.n * 8, (size_t)h->P.d * count,
                   hipMemcpyHostToDevice));
  HCHK(hipStreamSynchronize(nullptr));  // (see fphip_gso_set_basis: complete on the device before a kernel may run)
  return FPHIP_OK;
}

extern "C" int fphip_hh_broadcast_basis(fphip_hh *h, int src)
{
  if (!h || src < 0 || src >= h->P.batch)
    return FPHIP_ERROR;
  const size_t per = (size_t)h->P.d * h->P.ldn;
  for (int L = 0; L < h->P.batch; ++L)
    if (L != src)
      HCHK(hipMemcpyAsync(h->P.b + (size_t)L * per, h->P.b + (size_t)src * per, per * 8,
                          hipMemcpyDeviceToDevice, fphip_ctx_stream(h->ctx)));
  if (h->u)
  {  // MatHouseholder(b, u, ...): the copies start from src's pair
    const size_t peru = (size_t)h->P.d * h->ldu;
    for (int L = 0; L < h->P.batch; ++L)
      if (L != src)
        HCHK(hipMemcpyAsync(h->u + (size_t)L * peru, h->u + (size_t)src * peru, peru * 8, hipMemcpyDeviceToDevice,
                            fphip_ctx_stream(h->ctx)));
  }
  HCHK(hipStreamSynchronize(fphip_ctx_stream(h->ctx)));
  return FPHIP_OK;
}

// MatHouseholder(b, u, u_inv, flags) with a non-empty u (householder.h:70-130): the transformation matrix on the
// device, [batch][d][ldu] with ldu padded like ldn.  From here on fphip_hh_hlll, fphip_hh_hlll_ex, fphip_hh_hlll_ladder
// and fphip_hh_size_reduce launch the u-carrying forms of their kernels (hlll_kernel_u.hip, hlll_x_u.hip,
// hh_size_reduce_u_kernel), which apply row_addmul_we (householder.cpp:522-559) and swap (:372-398) to u as to b.
// u = NULL: the identity.  A second call resets u.
extern "C" int fphip_hh_enable_transform(fphip_hh *h, const int64_t *u)
{
  if (!h)
    return FPHIP_ERROR;
  if (h->P.d > h->P.n)
  {  // the kernels' columns-per-lane count follows n alone; a row of u has d entries
    snprintf(fphip_ctx_errbuf(h->ctx), 512,
             "fphip_hh_enable_transform: d = %d rows exceed n = %d columns; the transformation matrix is carried for "
             "d <= n only", h->P.d, h->P.n);
    return FPHIP_UNSUPPORTED;
  }
  const size_t B = (size_t)h->P.batch, d = h->P.d;
  hipStream_t s  = fphip_ctx_stream(h->ctx);
  if (!h->u)
  {
    int ldu = (h->P.d + 15) / 16 * 16;
    if (ldu > 256)
      ldu = 256;
    HCHK(fphip_dev_alloc((void **)&h->u, B * d * (size_t)ldu * sizeof(long long) + 4096, s));
    h->ldu = ldu;
  }
  const size_t ldu = h->ldu;
  HCHK(hipMemsetAsync(h->u, 0, B * d * ldu * sizeof(long long) + 4096, s));
  HCHK(hipStreamSynchronize(s));
  if (u)
    HCHK(hipMemcpy2D(h->u, ldu * 8, u, d * 8, d * 8, B * d, hipMemcpyHostToDevice));
  else
  {
    std::vector<long long> id(d * ldu, 0);
    for (size_t i = 0; i < d; ++i)
      id[i * ldu + i] = 1;
    for (size_t L = 0; L < B; ++L)
      HCHK(hipMemcpy(h->u + L * d * ldu, id.data(), d * ldu * sizeof(long long), hipMemcpyHostToDevice));
  }
  HCHK(hipStreamSynchronize(nullptr));  // (see fphip_gso_set_basis)
  return FPHIP_OK;
}

extern "C" int fphip_hh_get_transform(fphip_hh *h, int first, int count, int64_t *u)
{
  if (!h || !u || first < 0 || count <= 0 || first + count > h->P.batch)
    return FPHIP_ERROR;
  if (!h->u)
  {
    snprintf(fphip_ctx_errbuf(h->ctx), 512, "fphip_hh_get_transform: no transformation matrix (fphip_hh_enable_transform)");
    return FPHIP_ERROR;
  }
  const size_t d = h->P.d, ldu = h->ldu;
  HCHK(hipMemcpy2D(u, d * 8, h->u + (size_t)first * d * ldu, ldu * 8, d * 8, d * (size_t)count, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

// refresh_R_bf() + update_R() for every lattice; status[batch] = 1
extern "C" int fphip_hh_update_R(fphip_hh *h, int *status)
{
  FPHIP_RANGE("fphip_hh_update_R");
  if (!h)
    return FPHIP_ERROR;
  const int nq  = (h->P.n + 63) / 64;
  const int wpb = 4;
  const size_t lds = (size_t)wpb * FPHIP_GSO_RING * (size_t)((nq + 1) / 2) * 1024;
  int bpc          = (int)((160 * 1024) / lds);
  if (bpc * wpb > 32)
    bpc = 32 / wpb;
  int grid = (h->P.batch + wpb - 1) / wpb;
  if (grid > fphip_ctx_num_cus(h->ctx) * bpc)
    grid = fphip_ctx_num_cus(h->ctx) * bpc;
  hipStream_t s = fphip_ctx_stream(h->ctx);
  HCHK(hipEventRecord(h->ev[0], s));
  // rows up to 192 columns: the batch across the lanes (hh_rows.hip: a lane owns a row of one lattice and runs the
  // reference's scalar loops; the same bits); FPHIP_HH_ROWS=0 keeps the lane-per-column kernel (the A/B partner)
  const char *hr = getenv("FPHIP_HH_ROWS");
  if (h->P.n <= 192 && !(hr && hr[0] == '0'))
  {
    const int nt      = h->P.n <= 64 ? 4 : (h->P.n <= 128 ? 8 : 12);
    const size_t ldsr = ((size_t)3 * 16 * (16 * nt + 2) + 3 * 16) * sizeof(double);
    int gridr         = (h->P.batch + 15) / 16;
    if (gridr > fphip_ctx_num_cus(h->ctx))
      gridr = fphip_ctx_num_cus(h->ctx);
    switch (nt)
    {
    case 4: hipLaunchKernelGGL(hh_rows_kernel<4>, dim3(gridr), dim3(256), ldsr, s, h->P); break;
    case 8: hipLaunchKernelGGL(hh_rows_kernel<8>, dim3(gridr), dim3(256), ldsr, s, h->P); break;
    default: hipLaunchKernelGGL(hh_rows_kernel<12>, dim3(gridr), dim3(256), ldsr, s, h->P); break;
    }
  }
  else
    dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL(hh_update_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, h->P); });
  HCHK(hipGetLastError());
  HCHK(hipEventRecord(h->ev[1], s));
  HCHK(hipStreamSynchronize(s));
  HCHK(hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]));
  if (status)
    HCHK(hipMemcpy(status, h->P.status, sizeof(int) * h->P.batch, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

// MatHouseholder::size_reduce(kappa, size_reduction_end, size_reduction_start) on every lattice of the batch
// (householder.cpp:402-451; kernel in hh_rows.hip).  The state must be the one fphip_hh_update_R left (or any state
// in which rows < kappa of R are final and R(kappa, c < kappa) are the values update_R(kappa, false) gives).
extern "C" int fphip_hh_size_reduce(fphip_hh *h, int kappa, int size_reduction_end, int size_reduction_start,
                                    int *reduced, int *status)
{
  FPHIP_RANGE("fphip_hh_size_reduce");
  if (!h || !reduced)
    return FPHIP_ERROR;
  if (!(kappa > 0 && kappa < h->P.d) || size_reduction_start < 0 || size_reduction_end > kappa ||
      size_reduction_start > size_reduction_end)
  {
    snprintf(fphip_ctx_errbuf(h->ctx), 512,
             "fphip_hh_size_reduce: need 0 < kappa < d and 0 <= start <= end <= kappa (got %d, %d, %d)", kappa,
             size_reduction_end, size_reduction_start);
    return FPHIP_ERROR;
  }
  hipStream_t s = fphip_ctx_stream(h->ctx);
  int *dred     = nullptr;
  HCHK(fphip_dev_alloc((void **)&dred, sizeof(int) * (size_t)h->P.batch, s));
  HCHK(hipEventRecord(h->ev[0], s));
  if (h->u)
    hipLaunchKernelGGL(hh_size_reduce_u_kernel, dim3((h->P.batch + 3) / 4), dim3(256), 0, s, h->P, kappa,
                       size_reduction_end, size_reduction_start, dred, h->u, h->ldu);
  else
  hipLaunchKernelGGL(hh_size_reduce_kernel, dim3((h->P.batch + 3) / 4), dim3(256), 0, s, h->P, kappa,
                     size_reduction_end, size_reduction_start, dred);
  hipError_t le = hipGetLastError();
  HCHK(hipEventRecord(h->ev[1], s));
  hipError_t se = hipStreamSynchronize(s);
  if (le == hipSuccess && se == hipSuccess)
  {
    hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]);
    se = hipMemcpy(reduced, dred, sizeof(int) * h->P.batch, hipMemcpyDeviceToHost);
    if (se == hipSuccess && status)
      se = hipMemcpy(status, h->P.status, sizeof(int) * h->P.batch, hipMemcpyDeviceToHost);
  }
  fphip_dev_free(dred, s);
  HCHK(le);
  HCHK(se);
  return FPHIP_OK;
}

// The same R-factor in blocked compact-WY form on the MFMA matrix cores (hh_blocked.hip): the
// opt-in fast mode — sums in another order, hence other roundings than the reference's; R / mu / r
// agree with the exact mode to ~1e-13 relative (checked to 1e-9), row exponents and signs identical.
extern "C" int fphip_hh_update_R_blocked(fphip_hh *h, int *status)
{
  FPHIP_RANGE("fphip_hh_update_R_blocked");
  if (!h)
    return FPHIP_ERROR;
  const int nq   = (h->P.n + 63) / 64;
  const int nblk = (h->P.d + 15) / 16;
  if (!h->Tbuf)
    HCHK(fphip_dev_alloc((void **)&h->Tbuf, (size_t)h->P.batch * nblk * 256 * sizeof(double), fphip_ctx_stream(h->ctx)));
  const int ldx    = ((h->P.n + 31) & ~31) + 1;
  const size_t lds = (size_t)(16 * ldx + 256) * sizeof(double);
  int bpc          = (int)((160 * 1024) / lds);
  if (bpc > 16)
    bpc = 16;
  int grid = h->P.batch;
  if (grid > fphip_ctx_num_cus(h->ctx) * bpc)
    grid = fphip_ctx_num_cus(h->ctx) * bpc;
  hipStream_t s = fphip_ctx_stream(h->ctx);
  HCHK(hipEventRecord(h->ev[0], s));
  dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL(hh_blocked_kernel<NQ>, dim3(grid), dim3(64), lds, s, h->P, h->Tbuf); });
  HCHK(hipGetLastError());
  HCHK(hipEventRecord(h->ev[1], s));
  HCHK(hipStreamSynchronize(s));
  HCHK(hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]));
  if (status)
    HCHK(hipMemcpy(status, h->P.status, sizeof(int) * h->P.batch, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

extern "C" int fphip_hh_get_basis(fphip_hh *h, int first, int count, int64_t *b)
{
  if (!h || !b || first < 0 || count <= 0 || first + count > h->P.batch)
    return FPHIP_ERROR;
  HCHK(hipMemcpy2D(b, (size_t)h->P.n * 8, h->P.b + (size_t)first * h->P.d * h->P.ldn,
                   (size_t)h->P.ldn * 8, (size_t)h->P.n * 8, (size_t)h->P.d * count,
                   hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

// HLLLReduction<Z_NR<long>, FP_NR<double>>(m, delta, eta, theta, c, LLL_DEFAULT).hlll() on a fresh
// MatHouseholder of every lattice (hlll.cpp:26-169).  eta and c are accepted for interface parity:
// the default build of the reference uses neither (eR is delta*R(k,k), hlll.h:155-159; the size
// reduction stop rule uses the constant 0.1, hlll.cpp:297).  info (nullable) [batch][2]: swaps,
// loop iterations.
extern "C" int fphip_hh_hlll(fphip_hh *h, double delta, double eta, double theta, double c,
                             int *status, int *info)
{
  FPHIP_RANGE("fphip_hh_hlll");
  (void)eta;
  (void)c;
  if (!h)
    return FPHIP_ERROR;
  const size_t B = (size_t)h->P.batch, d = h->P.d, ld = h->P.ldn;
  if (!h->P.bf)
  {
    HCHK(fphip_dev_alloc((void **)&h->P.bf, B * d * ld * 8 + 4096, fphip_ctx_stream(h->ctx)));
    HCHK(fphip_dev_alloc((void **)&h->P.info, B * 2 * sizeof(int), fphip_ctx_stream(h->ctx)));
    HCHK(hipMemsetAsync(h->P.bf, 0, B * d * ld * 8 + 4096, fphip_ctx_stream(h->ctx)));
  }
  const int nq  = (h->P.n + 63) / 64;
  const int wpb = 4;
  const size_t lds = (size_t)wpb * FPHIP_RING_REDUCE * (size_t)((nq + 1) / 2) * 1024;
  int bpc          = (int)((160 * 1024) / lds);
  if (bpc * wpb > 32)
    bpc = 32 / wpb;
  int grid = (h->P.batch + wpb - 1) / wpb;
  if (grid > fphip_ctx_num_cus(h->ctx) * bpc)
    grid = fphip_ctx_num_cus(h->ctx) * bpc;
  const long long cap = 1LL << 40;
  hipStream_t s = fphip_ctx_stream(h->ctx);
  HCHK(hipEventRecord(h->ev[0], s));
  if (h->u)  // the transformation matrix is tracked: the u-carrying kernel (hlll_kernel_u.hip), same launch shape
    dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL(hlll_u_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, h->P, delta, theta, cap, h->u, h->ldu); });
  else
    dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL(hlll_kernel<NQ>, dim3(grid), dim3(wpb * 64), lds, s, h->P, delta, theta, cap); });
  HCHK(hipGetLastError());
  HCHK(hipEventRecord(h->ev[1], s));
  HCHK(hipStreamSynchronize(s));
  HCHK(hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]));
  h->x_planes = 1;  // (the double kernel: R has its leading plane only)
  if (status)
    HCHK(hipMemcpy(status, h->P.status, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (info)
    HCHK(hipMemcpy(info, h->P.info, sizeof(int) * 2 * B, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

// HLLL in a selectable floating-point type (hlll_x.hip): precision 106 = double-double, the device
// stand-in for the reference's FP_NR<dd_real> (BASELINE config 5 as stated); precision 53 = plain
// double with the same tree-sum kernel.  Same algorithm and status / info convention as
// fphip_hh_hlll; the sums run as wave-level trees (the exact-order double kernel is fphip_hh_hlll).
static int hh_hlll_ex(fphip_hh *h, double delta, double theta, int precision, const int *d_only_failed,
                      int *status, int *info)
{
  if (!h || (precision != 53 && precision != 106 && precision != 212))
    return FPHIP_ERROR;
  if (precision == 212 && h->P.n > 64)
  {  // hlll_x_kernel<NQ >= 2, QD>: its one run (n = 72) ended in an illegal memory access whose cause is not found
    // (DESIGN.md section 4d); until it is, the quad-double type takes one column per lane only
    snprintf(fphip_ctx_errbuf(h->ctx), 512, "fphip_hh_hlll_ex: precision 212 needs n <= 64 (n = %d)", h->P.n);
    return FPHIP_ERROR;
  }
  const size_t B = (size_t)h->P.batch, d = h->P.d, ld = h->P.ldn;
  const bool wide = precision >= 106;  // a low plane of R and V
  if (!h->P.bf)
  {
    HCHK(fphip_dev_alloc((void **)&h->P.bf, B * d * ld * 8 + 4096, fphip_ctx_stream(h->ctx)));
    HCHK(fphip_dev_alloc((void **)&h->P.info, B * 2 * sizeof(int), fphip_ctx_stream(h->ctx)));
    HCHK(hipMemsetAsync(h->P.bf, 0, B * d * ld * 8 + 4096, fphip_ctx_stream(h->ctx)));
  }
  if (!h->xsc)
  {
    HCHK(fphip_dev_alloc((void **)&h->xsc, B * 20 * d * sizeof(double), fphip_ctx_stream(h->ctx)));
    HCHK(fphip_dev_alloc((void **)&h->xprevE, B * d * sizeof(long long), fphip_ctx_stream(h->ctx)));
  }
  if (wide && !h->Rlo)
  {
    HCHK(fphip_dev_alloc((void **)&h->Rlo, B * d * ld * 8 + 4096, fphip_ctx_stream(h->ctx)));
    HCHK(fphip_dev_alloc((void **)&h->Vlo, B * d * ld * 8 + 4096, fphip_ctx_stream(h->ctx)));
  }
  hipStream_t s0 = fphip_ctx_stream(h->ctx);
  HCHK(hipMemsetAsync(h->xsc, 0, B * 20 * d * sizeof(double), s0));
  HCHK(hipMemsetAsync(h->xprevE, 0, B * d * sizeof(long long), s0));
  if (wide)
  {
    HCHK(hipMemsetAsync(h->Rlo, 0, B * d * ld * 8 + 4096, s0));
    HCHK(hipMemsetAsync(h->Vlo, 0, B * d * ld * 8 + 4096, s0));
  }
  if (precision == 212)
  {  // quad-double (the device stand-in for FP_NR<qd_real>, the ladder's third stage): two more planes each
    if (!h->xRx)
    {
      HCHK(fphip_dev_alloc((void **)&h->xRx, 2 * B * d * ld * 8 + 4096, s0));
      HCHK(fphip_dev_alloc((void **)&h->xVx, 2 * B * d * ld * 8 + 4096, s0));
    }
    HCHK(hipMemsetAsync(h->xRx, 0, 2 * B * d * ld * 8 + 4096, s0));
    HCHK(hipMemsetAsync(h->xVx, 0, 2 * B * d * ld * 8 + 4096, s0));
  }
  // the reflectors sixteen at a time (compact WY with a T per block, hlll_x.hip): opt-in, FPHIP_HLLL_BLOCKED=1.
  // Built for the lone-wave latency of config 5 and measured SLOWER there (n = 256, one lattice: 60.0 s against
  // 29.7 s one by one in double, 115.4 s against 56.5 s in double-double; same basis, 146 491 swaps): the chain of
  // dependent reductions is 16 times shorter, but every block waits for its 16 rows of V, its column of T and its
  // signs out of L2, where the one-by-one loop has the next row in flight behind each tree sum.
  const char *hb     = getenv("FPHIP_HLLL_BLOCKED");
  const bool blocked = hb && hb[0] == '1' && precision != 212;
  const size_t tdbl  = B * ((d + 15) / 16) * 256;
  if (blocked)
  {
    if (!h->xThi)
      HCHK(fphip_dev_alloc((void **)&h->xThi, tdbl * 8 + 4096, s0));
    if (precision == 106 && !h->xTlo)
      HCHK(fphip_dev_alloc((void **)&h->xTlo, tdbl * 8 + 4096, s0));
    HCHK(hipMemsetAsync(h->xThi, 0, tdbl * 8, s0));
    if (precision == 106)
      HCHK(hipMemsetAsync(h->xTlo, 0, tdbl * 8, s0));
  }
  HlllX X;
  X.Thi      = blocked ? h->xThi : nullptr;
  X.Tlo      = (blocked && precision == 106) ? h->xTlo : nullptr;
  X.Rlo      = wide ? h->Rlo : nullptr;
  X.Vlo      = wide ? h->Vlo : nullptr;
  X.Rx       = precision == 212 ? h->xRx : nullptr;
  X.Vx       = precision == 212 ? h->xVx : nullptr;
  X.sc       = h->xsc;
  X.prevE    = h->xprevE;
  X.delta    = delta;
  X.theta    = theta;
  X.iter_cap = 1LL << 40;
  X.only_failed = d_only_failed;
  const int nq = (h->P.n + 63) / 64;
  int grid     = h->P.batch;
  if (grid > fphip_ctx_num_cus(h->ctx) * 8)
    grid = fphip_ctx_num_cus(h->ctx) * 8;
  hipStream_t s = fphip_ctx_stream(h->ctx);
  HCHK(hipEventRecord(h->ev[0], s));
  if (h->u)  // the transformation matrix is tracked: the u-carrying kernels (hlll_x_u.hip)
    dispatch_precision(precision, [&](auto ft) {
      using FT = typename decltype(ft)::type;
      dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL((hlll_x_u_kernel<NQ, FT>), dim3(grid), dim3(64), 0, s, h->P, X, h->u, h->ldu); });
    });
  else
    dispatch_precision(precision, [&](auto ft) {
      using FT = typename decltype(ft)::type;
      dispatch_nq(nq, [&](auto NQ) { hipLaunchKernelGGL((hlll_x_kernel<NQ, FT>), dim3(grid), dim3(64), 0, s, h->P, X); });
    });
  HCHK(hipGetLastError());
  HCHK(hipEventRecord(h->ev[1], s));
  HCHK(hipStreamSynchronize(s));
  HCHK(hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]));
  h->x_planes = precision == 212 ? 4 : (precision == 106 ? 2 : 1);
  if (status)
    HCHK(hipMemcpy(status, h->P.status, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (info)
    HCHK(hipMemcpy(info, h->P.info, sizeof(int) * 2 * B, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

extern "C" int fphip_hh_hlll_ex(fphip_hh *h, double delta, double eta, double theta, double c, int precision,
                                int *status, int *info)
{
  FPHIP_RANGE("fphip_hh_hlll_ex");
  (void)eta;
  (void)c;
  return hh_hlll_ex(h, delta, theta, precision, nullptr, status, info);
}

// The precision ladder of the reference's wrapper (hlll_reduction with LM_WRAPPER, wrapper.cpp:
// 478-529: double, then the wider types, each stage continuing from the basis the previous one
// left) on the device: stage 1 = the exact-order double kernel for the whole batch; the lattices it
// gives up on with a precision alarm (RED_HLLL_SR_FAILURE -4, RED_HLLL_NORM_FAILURE -5) go on in
// double-double, and those it gives up on in quad-double (round 6).  stage[batch] (nullable) = 53, 106 or 212:
// where each lattice ended.  A lattice that fails at 212 bits keeps its status: the caller's MPFR stage (fplll's
// CPU path) is next.
extern "C" int fphip_hh_hlll_ladder(fphip_hh *h, double delta, double eta, double theta, double c, int *status,
                                    int *info, int *stage)
{
  FPHIP_RANGE("fphip_hh_hlll_ladder");
  if (!h)
    return FPHIP_ERROR;
  const size_t B = (size_t)h->P.batch;
  std::vector<int> st(B, 0), inf(2 * B, 0);
  int rc = fphip_hh_hlll(h, delta, eta, theta, c, st.data(), inf.data());
  if (rc != FPHIP_OK)
    return rc;
  float ms = h->last_ms;
  std::vector<int> stg(B, 53);
  bool any = false;
  // FPHIP_HLLL_LADDER_TEST=1 (tests only): treat the odd lattices as if stage 1 had raised an alarm, so
  // that the escalation path runs on inputs where plain doubles never fail (row exponents make the
  // double stage very robust: no long-sized lattice tried here trips it)
  const bool force = getenv("FPHIP_HLLL_LADDER_TEST") && atoi(getenv("FPHIP_HLLL_LADDER_TEST")) >= 1;
  if (force)
    for (size_t L = 1; L < B; L += 2)
      if (st[L] == 1)
        st[L] = -4;
  for (size_t L = 0; L < B; ++L)
    any |= (st[L] == -4 || st[L] == -5);
  if (any)
  {
    // status still sits on the device (P.status): 1 = done, anything else goes on in double-double
    std::vector<int> st2(B, 0), inf2(2 * B, 0), mask(B);
    for (size_t L = 0; L < B; ++L)
      mask[L] = (st[L] == -4 || st[L] == -5) ? 0 : 1;
    int *d_mask = nullptr;
    HCHK(fphip_dev_alloc((void **)&d_mask, B * sizeof(int), fphip_ctx_stream(h->ctx)));
    hipError_t e = hipMemcpy(d_mask, mask.data(), B * sizeof(int), hipMemcpyHostToDevice);
    rc           = (e == hipSuccess) ? hh_hlll_ex(h, delta, theta, 106, d_mask, st2.data(), inf2.data()) : FPHIP_ERROR;
    fphip_dev_free(d_mask, fphip_ctx_stream(h->ctx));
    if (rc != FPHIP_OK)
      return rc;
    ms += h->last_ms;
    for (size_t L = 0; L < B; ++L)
      if (!mask[L])
      {
        st[L]  = st2[L];
        stg[L] = 106;
        inf[2 * L] += inf2[2 * L];
        inf[2 * L + 1] += inf2[2 * L + 1];
      }
    // third stage (wrapper.cpp:630-710: FT_QD behind FT_DD): the lattices double-double gave up on, in quad-double
    // (FPHIP_HLLL_LADDER_TEST=2, tests only: every fourth lattice as if stage 2 had raised an alarm)
    const bool force3 = getenv("FPHIP_HLLL_LADDER_TEST") && atoi(getenv("FPHIP_HLLL_LADDER_TEST")) == 2;
    if (force3)
      for (size_t L = 3; L < B; L += 4)
        if (!mask[L] && st[L] == 1)
          st[L] = -4;
    bool any3 = false;
    for (size_t L = 0; L < B; ++L)
      any3 |= (!mask[L] && (st[L] == -4 || st[L] == -5));
    if (any3)
    {
      std::vector<int> st3(B, 0), inf3(2 * B, 0), mask3(B);
      for (size_t L = 0; L < B; ++L)
        mask3[L] = (!mask[L] && (st[L] == -4 || st[L] == -5)) ? 0 : 1;
      int *d_mask3 = nullptr;
      HCHK(fphip_dev_alloc((void **)&d_mask3, B * sizeof(int), fphip_ctx_stream(h->ctx)));
      hipError_t e3 = hipMemcpy(d_mask3, mask3.data(), B * sizeof(int), hipMemcpyHostToDevice);
      rc = (e3 == hipSuccess) ? hh_hlll_ex(h, delta, theta, 212, d_mask3, st3.data(), inf3.data()) : FPHIP_ERROR;
      fphip_dev_free(d_mask3, fphip_ctx_stream(h->ctx));
      if (rc != FPHIP_OK)
        return rc;
      ms += h->last_ms;
      for (size_t L = 0; L < B; ++L)
        if (!mask3[L])
        {
          st[L]  = st3[L];
          stg[L] = 212;
          inf[2 * L] += inf3[2 * L];
          inf[2 * L + 1] += inf3[2 * L + 1];
        }
    }
  }
  h->last_ms = ms;
  if (status)
    memcpy(status, st.data(), B * sizeof(int));
  if (info)
    memcpy(info, inf.data(), 2 * B * sizeof(int));
  if (stage)
    memcpy(stage, stg.data(), B * sizeof(int));
  return FPHIP_OK;
}

// low plane of R after fphip_hh_hlll_ex(precision 106): R(i,j) = hi + lo (hi through fphip_hh_get_R)
extern "C" int fphip_hh_get_R_lo(fphip_hh *h, int lattice, double *Rlo)
{
  if (!h || !Rlo || !h->Rlo || lattice < 0 || lattice >= h->P.batch)
    return FPHIP_ERROR;
  HCHK(hipMemcpy2D(Rlo, (size_t)h->P.n * 8, h->Rlo + (size_t)lattice * h->P.d * h->P.ldn,
                   (size_t)h->P.ldn * 8, (size_t)h->P.n * 8, h->P.d, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

// component plane 0..3 of R after fphip_hh_hlll_ex: R(i,j) = the sum of the planes (0 = fphip_hh_get_R, 1 =
// fphip_hh_get_R_lo, 2 and 3 the quad-double run's); a plane the last run did not have reads as zeros
extern "C" int fphip_hh_get_R_plane(fphip_hh *h, int lattice, int plane, double *out)
{
  if (!h || !out || h->x_planes == 0 || plane < 0 || plane > 3 || lattice < 0 || lattice >= h->P.batch)
    return FPHIP_ERROR;
  if (plane >= h->x_planes)
  {
    memset(out, 0, (size_t)h->P.d * h->P.n * 8);
    return FPHIP_OK;
  }
  const size_t pl   = (size_t)h->P.batch * h->P.d * h->P.ldn;  // (Rx: planes 2 and 3 back to back, hlll_x.hip)
  const double *src = plane == 0 ? h->P.R : (plane == 1 ? h->Rlo : h->xRx + (plane - 2) * pl);
  HCHK(hipMemcpy2D(out, (size_t)h->P.n * 8, src + (size_t)lattice * h->P.d * h->P.ldn, (size_t)h->P.ldn * 8,
                   (size_t)h->P.n * 8, h->P.d, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

// double-double arithmetic of the device (ftx.h), element-wise on host arrays — for its unit test
// against multiprecision.  op: 0 add, 1 sub, 2 mul, 3 div, 4 sqrt(a), 5 nint(a)
extern "C" int fphip_debug_dd_op(fphip_ctx *ctx, int op, int count, const double *ahi, const double *alo,
                                 const double *bhi, const double *blo, double *ohi, double *olo)
{
  if (!ctx || count <= 0)
    return FPHIP_ERROR;
  double *dv = nullptr;
  const size_t nb = (size_t)count * sizeof(double);
  if (fphip_dev_alloc((void **)&dv, 6 * nb, fphip_ctx_stream(ctx)) != hipSuccess)
    return FPHIP_ERROR;
  hipMemcpy(dv, ahi, nb, hipMemcpyHostToDevice);
  hipMemcpy(dv + count, alo, nb, hipMemcpyHostToDevice);
  hipMemcpy(dv + 2 * (size_t)count, bhi, nb, hipMemcpyHostToDevice);
  hipMemcpy(dv + 3 * (size_t)count, blo, nb, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(dd_op_kernel, dim3((count + 255) / 256), dim3(256), 0, fphip_ctx_stream(ctx), dv, dv + count,
                     dv + 2 * (size_t)count, dv + 3 * (size_t)count, dv + 4 * (size_t)count,
                     dv + 5 * (size_t)count, op, count);
  hipStreamSynchronize(fphip_ctx_stream(ctx));
  hipMemcpy(ohi, dv + 4 * (size_t)count, nb, hipMemcpyDeviceToHost);
  hipMemcpy(olo, dv + 5 * (size_t)count, nb, hipMemcpyDeviceToHost);
  fphip_dev_free(dv, fphip_ctx_stream(ctx));
  return FPHIP_OK;
}

// either extended type of the device (ftx.h), element-wise and wave-level, on host arrays — for the unit tests against
// multiprecision and against the host build of the same header.  a, b, out: [comps][count] planes, comps 2 (DD) or
// 4 (QD); ops as ftx_op_kernel (hlll_x.hip).  The wave-level ops (10..13) take whole wavefronts only.
extern "C" int fphip_debug_ftx_op(fphip_ctx *ctx, int comps, int op, int count, const double *a, const double *b,
                                  double *out)
{
  if (!ctx || !a || !b || !out || count <= 0 || (comps != 2 && comps != 4) || op < 0 || op > 13 ||
      (op >= 10 && count % 64 != 0))
    return FPHIP_ERROR;
  hipStream_t s    = fphip_ctx_stream(ctx);
  const size_t npl = (size_t)comps * count, nb = npl * sizeof(double);
  double *dv       = nullptr;
  if (fphip_dev_alloc((void **)&dv, 3 * nb, s) != hipSuccess)
    return FPHIP_ERROR;
  bool ok = hipMemcpy(dv, a, nb, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dv + npl, b, nb, hipMemcpyHostToDevice) == hipSuccess;
  if (ok)
  {
    const dim3 grid((count + 255) / 256), block(256);
    if (comps == 2)
      hipLaunchKernelGGL((ftx_op_kernel<DD>), grid, block, 0, s, dv, dv + npl, dv + 2 * npl, op, count);
    else
      hipLaunchKernelGGL((ftx_op_kernel<QD>), grid, block, 0, s, dv, dv + npl, dv + 2 * npl, op, count);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess &&
         hipMemcpy(out, dv + 2 * npl, nb, hipMemcpyDeviceToHost) == hipSuccess;
  }
  fphip_dev_free(dv, s);
  return ok ? FPHIP_OK : FPHIP_ERROR;
}

// R as d×n row-major (only R(i, j<=i) is meaningful, as in the reference); exponents separately
extern "C" int fphip_hh_get_R(fphip_hh *h, int lattice, double *R)
{
  if (!h || !R || lattice < 0 || lattice >= h->P.batch)
    return FPHIP_ERROR;
  HCHK(hipMemcpy2D(R, (size_t)h->P.n * 8, h->P.R + (size_t)lattice * h->P.d * h->P.ldn,
                   (size_t)h->P.ldn * 8, (size_t)h->P.n * 8, h->P.d, hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

extern "C" int fphip_hh_get_row_expo(fphip_hh *h, int lattice, int64_t *row_expo)
{
  if (!h || !row_expo || lattice < 0 || lattice >= h->P.batch)
    return FPHIP_ERROR;
  HCHK(hipMemcpy(row_expo, h->P.rexp + (size_t)lattice * h->P.d, 8 * (size_t)h->P.d,
                 hipMemcpyDeviceToHost));
  return FPHIP_OK;
}

extern "C" double fphip_hh_last_kernel_ms(const fphip_hh *h) { return h ? h->last_ms : 0.0; }
