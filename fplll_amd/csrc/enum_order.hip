// enum_order.hip — the final task list of an ordered call (fphip_enum_opts::ordered) in the reference's depth-first
// order, on the device.
//
// A task is a subtree: the coefficients of the levels >= its root level.  task_order_kernel recomputes, per task, the
// centre of every such level from the coefficients above it and the rank of the coefficient among its siblings
// (enum_order.h: the reference's zig-zag, the zero chain) and packs the ranks one byte per level, the top level in
// the most significant byte of word 0.  Tasks are disjoint subtrees, so no prefix is another's prefix and the zero
// padding of short prefixes cannot tie.  order_tasks_device then sorts the task indices by that multi-word key
// with stable radix sorts from the least significant word up (the idiom and scratch layout of enum_deal.hip); a
// word that is the same in every key is skipped, and a sort only runs over the bits that differ.
// A rank that does not fit a byte raises a flag: the host orders that call with enum_order.h's comparator.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "enum_device.h"
#include "enum_order.h"

namespace fphip
{

// summary[0..8): AND of word w over all keys, [8..16): OR, [16]: some rank did not fit a byte
#define FPHIP_ORDER_WORDS 8
#define FPHIP_ORDER_SUMMARY (2 * FPHIP_ORDER_WORDS + 1)

__global__ void order_init_kernel(unsigned long long *summary)
{
  const unsigned i = threadIdx.x;
  if (i < FPHIP_ORDER_SUMMARY)
    summary[i] = i < FPHIP_ORDER_WORDS ? ~0ull : 0ull;
}

// One wavefront per task, lane = level.  The mu rows (DevShared::mu_sq, d rows of 64: 32 KB at most) are staged in LDS once per workgroup:
// every task reads all of them.  The task's coefficients are one coalesced row; the coefficient of level j reaches
// the lanes below it as a wave-uniform lane read, so the loop over j is d - 1 - Lt dependent multiply-subtracts per
// lane — the reference's own sequence for the centre of every level at once.
__global__ __launch_bounds__(256) void task_order_kernel(const DevShared *__restrict__ g, TaskBuf in, unsigned n, int d,
                                                         const unsigned *__restrict__ slots,
                                                         unsigned long long *__restrict__ keys,
                                                         unsigned long long *__restrict__ summary)
{
  __shared__ double mu_s[64 * 64];
  for (int i = threadIdx.x; i < d * 64; i += blockDim.x)
    mu_s[i] = g->mu_sq[i >> 6][i & 63];
  __syncthreads();
  const int lane      = threadIdx.x & 63;
  const unsigned w    = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const unsigned nw   = (gridDim.x * blockDim.x) >> 6;
  const double r_l    = lane < d ? g->rdiag[lane] : 0.0;
  const int nwords    = (d + 7) >> 3;
  unsigned long long k_and = ~0ull, k_or = 0ull;  // lane 8 w: word w over this wave's tasks
  bool wide = false;
  for (unsigned tp = w; tp < n; tp += nw)
  {
    const unsigned ti = slots ? slots[tp] : tp;  // (regioned buffer: the tp-th occupied slot)
    const int Lt      = __builtin_amdgcn_readfirstlane(in.level[ti]);
    const bool on     = lane >= Lt && lane < d;
    const double xk   = on ? in.x[(unsigned long long)ti * 64 + lane] : 0.0;
    double c          = 0.0;
    for (int j = d - 1; j > Lt; --j)
    {
      const double xj = __shfl(xk, j);
      if (lane < j)
        c = order_centre_step(c, xj, mu_s[j * 64 + lane]);
    }
    const double term = on ? order_term(xk, c, r_l) : 0.0;
    // the partial distance above every level, summed from the top like the reference's: is the level on the zero chain?
    double pd   = 0.0;
    bool zchain = false;
    for (int k = d - 1; k >= Lt; --k)
    {
      if (lane == k)
        zchain = pd == 0.0;
      pd = pd + __shfl(term, k);
    }
    const unsigned rk = on ? order_rank(xk, c, zchain) : 0u;
    wide              = wide || rk >= 255u;
    // byte p = d - 1 - level of the key: lane p fetches the rank of its level, eight lanes make a word
    const unsigned rp = (unsigned)__shfl((int)(rk < 255u ? rk : 255u), (d - 1 - lane) & 63);
    unsigned long long v = lane < d ? (unsigned long long)rp << (56 - 8 * (lane & 7)) : 0ull;
    v |= __shfl_xor(v, 1);
    v |= __shfl_xor(v, 2);
    v |= __shfl_xor(v, 4);
    if ((lane & 7) == 0 && (lane >> 3) < nwords)
      keys[(size_t)(lane >> 3) * n + tp] = v;
    k_and &= v;
    k_or |= v;
  }
  // one atomic per wave and word (not per task: a returning atomic on one address costs ~50 ns of its L2 channel)
  if (w < n && (lane & 7) == 0 && (lane >> 3) < nwords)
  {
    atomicAnd(&summary[lane >> 3], k_and);
    atomicOr(&summary[FPHIP_ORDER_WORDS + (lane >> 3)], k_or);
  }
  if (__builtin_amdgcn_ballot_w64(wide) != 0ull && lane == 0)
    atomicOr(&summary[2 * FPHIP_ORDER_WORDS], 1ull);
}

__global__ void order_iota_kernel(unsigned *idx, unsigned n)
{
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    idx[i] = i;
}
__global__ void order_gather_kernel(const unsigned long long *word, const unsigned *idx, unsigned long long *out, unsigned n)
{
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    out[i] = word[idx[i]];
}
// position p of the sorted list -> the task's index in its buffer
__global__ void order_scatter_kernel(const unsigned *order, const unsigned *slot_of, unsigned *list, unsigned n)
{
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n)
    list[p] = slot_of ? slot_of[order[p]] : order[p];
}

static size_t order_sort_tmp(unsigned n)
{
  size_t tmp = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                           (const unsigned *)nullptr, (unsigned *)nullptr, (int)n);
  return (tmp + 255) & ~(size_t)255;
}

// device scratch of order_tasks_device: sort storage, the key words [8][n], two key and two index arrays, the summary
size_t order_work_bytes(unsigned n)
{
  return order_sort_tmp(n) + (size_t)n * (8 * FPHIP_ORDER_WORDS + 8 + 8 + 4 + 4) + 8 * FPHIP_ORDER_SUMMARY + 1024;
}

// The n tasks of `in` (through `slots` when the buffer is regioned) -> list[n]: their buffer indices in the
// reference's depth-first order.  Synchronises the stream (the host picks the words to sort by).  Returns 0, 1 when a
// rank did not fit a byte (list is not written: the caller orders on the host), -1 on a HIP error.
int order_tasks_device(hipStream_t s, const DevShared *g, TaskBuf in, unsigned n, int d, const unsigned *slots,
                       unsigned *list, void *work, size_t work_bytes, int num_cus, int *sort_passes)
{
  if (n == 0)
    return 0;
  size_t tmp = order_sort_tmp(n);
  if (work_bytes < order_work_bytes(n) || d > 64)
    return -1;
  char *wp                    = (char *)work;
  void *d_tmp                 = wp;
  unsigned long long *keys    = (unsigned long long *)(wp + tmp);
  unsigned long long *ka      = keys + (size_t)n * FPHIP_ORDER_WORDS;
  unsigned long long *kb      = ka + n;
  unsigned long long *summary = kb + n;
  unsigned *ia                = (unsigned *)(summary + FPHIP_ORDER_SUMMARY);
  unsigned *ib                = ia + n;
  const unsigned g1           = (n + 255) / 256;
  hipLaunchKernelGGL(order_init_kernel, dim3(1), dim3(64), 0, s, summary);
  hipLaunchKernelGGL(order_iota_kernel, dim3(g1), dim3(256), 0, s, ia, n);
  // (four tasks per workgroup pass; at most four workgroups per CU: the LDS copy of mu is paid once per workgroup)
  const unsigned kgrid = std::max(1u, std::min<unsigned>((n + 3) / 4, (unsigned)num_cus * 4u));
  hipLaunchKernelGGL(task_order_kernel, dim3(kgrid), dim3(256), 0, s, g, in, n, d, slots, keys, summary);
  if (hipGetLastError() != hipSuccess)  // (before the early return below: a launch that failed is an error, not a flag)
    return -1;
  unsigned long long sum[FPHIP_ORDER_SUMMARY];
  if (hipMemcpyAsync(sum, summary, sizeof sum, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return -1;
  if (sum[2 * FPHIP_ORDER_WORDS] != 0ull)
    return 1;
  int passes = 0;
  for (int w = (d + 7) / 8 - 1; w >= 0; --w)
  {
    const unsigned long long diff = sum[w] ^ sum[FPHIP_ORDER_WORDS + w];
    if (diff == 0ull)
      continue;  // the same word in every key
    const int lo = __builtin_ctzll(diff), hi = 64 - __builtin_clzll(diff);
    hipLaunchKernelGGL(order_gather_kernel, dim3(g1), dim3(256), 0, s, keys + (size_t)w * n, ia, kb, n);
    if (hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp, kb, ka, ia, ib, (int)n, lo, hi, s) != hipSuccess)
      return -1;
    std::swap(ia, ib);
    ++passes;
  }
  hipLaunchKernelGGL(order_scatter_kernel, dim3(g1), dim3(256), 0, s, ia, slots, list, n);
  if (hipGetLastError() != hipSuccess)
    return -1;
  if (sort_passes)
    *sort_passes = passes;
  return 0;
}

}  // namespace fphip
