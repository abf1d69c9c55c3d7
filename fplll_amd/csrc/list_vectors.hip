// list_vectors.hip — from the records of a list enumeration (fphip_enum_list) to lattice vectors: for every record its
// vector v = sum_i x_i b_i (minus the integer target when there is one) and the EXACT squared norm |v|^2, in int64 with
// overflow detection.  What the integer filter of fphip_list_vectors (gso_host.hip) runs on: the enumeration's
// distances are doubles, the answer "is |v - t|^2 <= bound" is asked of integers.
//
// One record per lane, arranged as cvp_prepare.hip arranges one target per lane: the loops over rows and columns are
// the same for every lane, so the basis rows (and the target) are wave-uniform loads, and a lane's vector lives in a
// column of a workspace in global memory — element j of lane t at [j][t], consecutive lanes consecutive addresses.  No
// LDS, no cross-lane traffic: the records are independent.
// status: 1 ok; -2 a product, a partial sum or the norm left the 63-bit range — that record's outputs are zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gso_device.h"
#include "kernels.h"

namespace fphip
{
__global__ void __launch_bounds__(64) list_vectors_kernel(ListVec P)
{
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= P.m)
    return;
  const int d = P.d, n = P.n;
  const size_t ldt = (size_t)P.ldt;
  long long *wv    = P.wv + t;
  bool ok          = true;
  for (int j = 0; j < n; ++j)
  {
    long long v0 = 0;
    if (P.target && __builtin_sub_overflow(0ll, P.target[j], &v0))
      ok = false;
    wv[j * ldt] = v0;
  }
  for (int i = 0; i < d && ok; ++i)
  {
    const long long ci = P.coef[(size_t)t * d + i];
    if (ci == 0)
      continue;
    for (int j = 0; j < n; ++j)
    {
      long long p, q;
      if (__builtin_mul_overflow(ci, P.b[(size_t)i * P.ldn + j], &p) || __builtin_add_overflow(wv[j * ldt], p, &q))
      {
        ok = false;
        break;
      }
      wv[j * ldt] = q;
    }
  }
  long long nrm = 0;
  for (int j = 0; j < n && ok; ++j)
  {
    const long long v = wv[j * ldt];
    long long p, q;
    if (__builtin_mul_overflow(v, v, &p) || __builtin_add_overflow(nrm, p, &q))
    {
      ok = false;
      break;
    }
    nrm = q;
  }
  for (int j = 0; j < n; ++j)
    P.vec[(size_t)t * n + j] = ok ? wv[j * ldt] : 0;
  P.norm[t]   = ok ? nrm : 0;
  P.status[t] = ok ? 1 : -2;
}
}  // namespace fphip
