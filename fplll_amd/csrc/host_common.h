// host_common.h — private to the host translation units (*_host.hip): the dispatchers from a run-time width class or
// precision to a kernel instantiation, the accessors of fphip_ctx (enum_host.hip defines them), and the one error
// path of a failed HIP call.
#ifndef FPHIP_HOST_COMMON_H
#define FPHIP_HOST_COMMON_H

#include <type_traits>
#include <utility>

namespace fphip
{
struct DD;  // ftx.h
struct QD;

// Columns per lane (NQ = ceil(max(d, n) / 64), 1 .. 4) to the kernel instantiation: f(std::integral_constant<int,
// NQ>{}), whose value is a constant expression inside f — hipLaunchKernelGGL((bkz_kernel<NQ>), ...).  Returns what f
// returns.  Everything above 3 is the widest class, as every launch site has always had it.
template <class F> inline decltype(auto) dispatch_nq(int nq, F &&f)
{
  switch (nq)
  {
  case 1: return f(std::integral_constant<int, 1>{});
  case 2: return f(std::integral_constant<int, 2>{});
  case 3: return f(std::integral_constant<int, 3>{});
  default: return f(std::integral_constant<int, 4>{});
  }
}

// Precision in bits (53, 106, 212) to the floating-point type of lll_x / hlll_x: f(type_tag<FT>{}), FT = typename
// decltype(tag)::type.  Everything that is neither 212 nor 106 is double, as at every launch site before.
template <class T> struct type_tag
{
  using type = T;
};
template <class F> inline decltype(auto) dispatch_precision(int precision, F &&f)
{
  switch (precision)
  {
  case 212: return f(type_tag<QD>{});
  case 106: return f(type_tag<DD>{});
  default: return f(type_tag<double>{});
  }
}
}  // namespace fphip

#ifndef FPHIP_DISPATCH_HOST_TEST  // (tests/native/dispatch_host.cpp compiles the part above with a plain C++ compiler)
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/fplll_hip.h"

// enum_host.hip
hipStream_t fphip_ctx_stream(fphip_ctx *ctx);
char *fphip_ctx_errbuf(fphip_ctx *ctx);
int fphip_ctx_num_cus(fphip_ctx *ctx);
int fphip_ctx_device(fphip_ctx *ctx);
int fphip_ctx_ensure_task_buffers(fphip_ctx *ctx);
int fphip_ctx_set_task_cap(fphip_ctx *ctx, unsigned cap);
int fphip_ctx_allow_wide_target(fphip_ctx *ctx, int on);  // closest-vector calls above 64 rows
// Gaussian-heuristic node estimate of a block (the sum over the levels of what places the phase cuts), d <= 256
double fphip_enum_gh_nodes(int d, const double *rdiag, const double *pruning, double maxdist);

static inline int fail(fphip_ctx *ctx, const char *what, hipError_t e)
{
  snprintf(fphip_ctx_errbuf(ctx), 512, "%s failed: %s", what, hipGetErrorString(e));
  return FPHIP_ERROR;
}
static inline int fail_msg(fphip_ctx *ctx, const char *msg)
{
  snprintf(fphip_ctx_errbuf(ctx), 512, "%s", msg);
  return FPHIP_ERROR;
}
// a HIP call of a function that returns an fphip status: on failure the text goes to ctx and the function returns
// (GCHK / HCHK / QCHK of the host files are this macro with the context of their handle, g->ctx or h->ctx)
#define CHK(ctx, call)            \
  do                                \
  {                                 \
    hipError_t e_ = (call);         \
    if (e_ != hipSuccess)           \
      return fail(ctx, #call, e_);  \
  } while (0)

// the kernel may use more than the 64 KiB of dynamic LDS a launch gets by default
template <class K> static inline hipError_t allow_lds(K *kernel, size_t lds)
{
  return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}
#endif

#endif
