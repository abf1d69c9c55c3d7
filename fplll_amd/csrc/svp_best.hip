// svp_best.hip — the N shortest vectors of every lattice of a BATCH (at most 64 rows, at most 64 vectors kept): one
// wavefront per lattice, the whole batch in one launch.  shortest_vectors(gso, sol_coord, sol_dist, max_sols) of the
// reference (an enumeration under a BEST_N evaluator whose radius shrinks to the worst of the kept vectors,
// svpcvp.cpp:84-241, 446-454) on the state fphip_gso_update leaves, with the decision on EXACT integers:
// tests/svp_best_model.py is the model, operation by operation.  The walk loops and the LDS layout are those of
// svp_wave.hip (the text is copied, as cvp_wave.hip did: svp_wave.hip's code object does not change).
//
// Per lattice:
//   1. the exact int64 squared norm of every row, lanes = columns; a norm beyond 63 bits: status -2, outputs zero;
//   2. the bound B0: the caller's, or N0 = the shortest row below last_useful_index (get_basis_min); the walk starts at
//      the radius (double)B0 (1 + 2^-30) — INCLUSIVE, nothing is seeded: a row of norm N0 is found by the walk;
//   3. the rows cut: without a caller's bound last_useful_index as svp_wave.hip has it (r_ii <= 2 r_00 on the true r);
//      with one the threshold is max(2 r_00, radius) — a vector whose top non-zero coefficient sits on row j has norm
//      >= r_jj, so a row above the radius contributes nothing, and the 2 r_00 rule alone would drop vectors under a
//      bound above 2 r_00;
//   4. the depth-first walk of svp_wave.hip under the level bounds pruning[k] * maxdist;
//   5. the evaluator: a leaf with nd > 0 within the bound is a candidate; v = sum x_i b_i and nv = |v|^2 in int64
//      (overflow: status -2).  It is accepted iff 0 < nv <= B0 and the table holds fewer than K entries or nv < the
//      worst kept norm; it goes behind every kept entry with norm <= nv (ties stay in discovery order), the worst
//      entry leaves a full table.  Once the table is full the radius is (double)(worst - 1) (1 + 2^-30): norms are
//      integers, only norm <= worst - 1 can still enter; a full table with worst = 1 ends the walk.  The 2^-30 is the
//      heuristic margin of the other solvers, not a proved bound.
// The table costs no LDS and no scratch: the K norms sit across the lanes (lane j = rank j) next to a rank-to-slot
// map; the coefficient records go to K slots of a global record buffer; a sorted insert is a compare, a ballot and a
// one-lane shift.  At the end the records are read back in rank order and vec is recomputed exactly per kept record,
// lanes = columns.
//
// Branches in the walk are wave-uniform; level registers are read across lanes with g_rl_f64 / readlane.
#include "gso_wave.h"
#include "kernels.h"

namespace fphip
{

__device__ __forceinline__ int btri(int k) { return (k * (k - 1)) >> 1; }

// sum over the wave of non-negative addends; ovf collects a sum beyond 63 bits (svp_wave.hip)
__device__ __forceinline__ long long best_sum_nonneg(long long v, bool &ovf)
{
  for (int off = 32; off > 0; off >>= 1)
  {
    const long long o = (long long)__shfl_xor(v, off);
    long long s;
    ovf |= __builtin_add_overflow(v, o, &s);
    v = s;
  }
  return v;
}

// |row|^2 of the values a wave holds as lanes = columns; false: beyond 63 bits
template <int NQ> __device__ __forceinline__ bool best_exact_norm(const long long (&v)[NQ], long long &out)
{
  bool ovf      = false;
  long long acc = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
  {
    long long p, s;
    ovf |= __builtin_mul_overflow(v[q], v[q], &p);
    ovf |= __builtin_add_overflow(acc, p, &s);
    acc = s;
  }
  acc = ovf ? 0 : acc;
  out = g_rl_i64(best_sum_nonneg(acc, ovf), 0);
  return !__any(ovf);
}

template <int NQ> __global__ void __launch_bounds__(256) svp_best_kernel(GsoBatch P, SvpBestWave A)
{
  extern __shared__ __attribute__((aligned(16))) char svp_best_smem[];
  const int lane = threadIdx.x & 63;
  const int wpb  = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int d = P.d, n = P.n, ldd = P.ldd, ldn = P.ldn;
  const int K = A.max_sols;
  // per wave: the triangular column stack of the walk, then the scaled mu triangle
  double *stk    = (double *)svp_best_smem + (size_t)wave * (A.stack_doubles + A.mu_doubles);
  double *mu_blk = stk + A.stack_doubles;
  for (int W = blockIdx.x * wpb + wave; W < A.count; W += gridDim.x * wpb)
  {
    if (A.take && A.take[W] == 0)
      continue;
    const size_t L     = (size_t)(A.first + W);
    const long long *b = P.b + L * d * ldn;
    const double *mu   = P.mu + L * d * ldd;
    const double *rdg  = P.rdg + L * d;
    const long long *rexp = P.rexp + L * d;
    long long *rec   = A.rec + (size_t)W * K * d;  // [K][d] coefficient records by slot
    long long *o_sol = A.sol_coord + (size_t)W * K * d;
    long long *o_vec = A.vec + (size_t)W * K * n;

    int status               = P.status[L] == 1 ? 1 : 0;
    unsigned long long nodes = 0;
    long long tn             = 0;  // lane j < found: the norm of rank j
    int slot                 = 0;  // lane j < found: the record slot of rank j
    int found                = 0;

    // ---- 1. exact row norms: lane i keeps |b_i|^2 ----------------------------------------------
    long long rn = 0;
    if (status == 1)
    {
      for (int i = 0; i < d; ++i)
      {
        long long row[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
        {
          const int c = lane + 64 * q;
          row[q]      = (c < n) ? b[(size_t)i * ldn + c] : 0;
        }
        long long nr;
        if (!best_exact_norm<NQ>(row, nr))
        {
          status = -2;
          break;
        }
        rn = (lane == i) ? nr : rn;
      }
    }
    if (status == 1)
    {
      // ---- 2. the bound; 3. the rows cut, on the true r_ii --------------------------------------
      const bool in      = lane < d;
      const double rr    = in ? rdg[lane] : 0.0;
      const long long ei = (in && P.row_expo) ? rexp[lane] : 0;
      const long long e0 = g_rl_i64(ei, 0);
      const double r00x2 = g_rl_f64(rr, 0) * 2.0;
      const long long de = 2 * (ei - e0);
      const double ri    = ldexp(rr, (int)max(min(de, 4000ll), -4000ll));
      const long long bnd = A.bound ? A.bound[W] : 0;
      long long B0;
      int d_eff;
      if (bnd > 0)
      {
        B0               = bnd;
        const double thr = fmax(r00x2, ldexp((double)B0 * (1.0 + 0x1p-30), (int)max(min(-2 * e0, 4000ll), -4000ll)));
        const uint64_t um = __ballot(in && lane > 0 && ri <= thr);
        d_eff             = um ? 64 - __clzll((long long)um) : 1;
      }
      else
      {
        const uint64_t um = __ballot(in && lane > 0 && ri <= r00x2);
        d_eff             = um ? 64 - __clzll((long long)um) : 1;
        B0                = g_rl_i64(rn, 0);  // get_basis_min: the shortest row below d_eff
        for (int i = 1; i < d_eff; ++i)
        {
          const long long ni = g_rl_i64(rn, i);
          B0                 = ni < B0 ? ni : B0;
        }
      }
      const double radius0 = (double)B0 * (1.0 + 0x1p-30);
      if (radius0 > 0.0)
      {
        // ---- normalisation, enumerate.cpp:88-141 ------------------------------------------------
        const int bs     = d_eff;
        const bool inb   = lane < bs;
        const int e2     = inb ? (int)(2 * ei) : 0;
        int ne           = inb ? (int)min((long long)e2 + fexponent(rr), (long long)INT_MAX) : INT_MIN;
        ne               = max(wave_max_i32(ne), -1);  // normexp starts at -1, enumerate.cpp:88
        const double rd  = inb ? ldexp(rr, e2 - ne) : 0.0;  // lane i: rdiag[i]
        const double prn = (inb && A.pruning) ? A.pruning[lane] : 1.0;
        double maxdist   = ldexp(radius0, -ne);
        double pb        = prn * maxdist;  // lane k: the bound of level k
        for (int k = 1; k < bs; ++k)
        {
          const long long ek = g_rl_i64(ei, k);
          if (lane < k)
          {
            const double m = mu[(size_t)k * ldd + lane];
            mu_blk[btri(k) + lane] = ldexp(m, (int)(ek - ei));
          }
        }
        __threadfence_block();
        // ---- 4. the walk: enumerate_recursive, depth-first -------------------------------------
        double xs = 0.0, cs = 0.0, pds = 0.0;
        int dxs = 0, ddxs = 0;
        unsigned long long cnt = 0;
        int k     = bs;
        double S  = 0.0;
        double nd = 0.0;
        bool done = false;
        // 5. the evaluator: the leaf in xs is within the bound with nd > 0
        auto candidate = [&]()
        {
          long long v[NQ];
#pragma unroll
          for (int q = 0; q < NQ; ++q)
            v[q] = 0;
          bool ovf = false;
          for (int i = 0; i < bs; ++i)
          {
            const double xi = g_rl_f64(xs, i);
            if (xi == 0.0)
              continue;
            if (!(fabs(xi) < 9223372036854775808.0))
            {
              ovf = true;
              break;
            }
            const long long lx = (long long)xi;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
            {
              const int c        = lane + 64 * q;
              const long long bi = (c < n) ? b[(size_t)i * ldn + c] : 0;
              long long p, s;
              ovf |= __builtin_mul_overflow(lx, bi, &p);
              ovf |= __builtin_add_overflow(v[q], p, &s);
              v[q] = s;
            }
          }
          long long nv = 0;
          if (__any(ovf) || !best_exact_norm<NQ>(v, nv))
          {  // a candidate beyond 63 bits: the lattice is given up
            status = -2;
            done   = true;
            return;
          }
          const bool full = found == K;
          if (nv > 0 && nv <= B0 && (!full || nv < g_rl_i64(tn, K - 1)))
          {
            // behind every kept entry with norm <= nv: the kept norms are sorted, so those are the ranks 0 .. p - 1
            const int p  = __popcll(__ballot(lane < found && tn <= nv));
            const int sl = full ? __builtin_amdgcn_readlane(slot, K - 1) : found;  // the worst's slot, or a fresh one
            const long long tn_up = (long long)__shfl_up(tn, 1);
            const int slot_up     = __shfl_up(slot, 1);
            tn    = lane > p ? tn_up : (lane == p ? nv : tn);
            slot  = lane > p ? slot_up : (lane == p ? sl : slot);
            found = full ? K : found + 1;
            if (lane < d)
              rec[(size_t)sl * d + lane] = inb ? (long long)xs : 0;
            if (found == K)
            {
              const long long worst = g_rl_i64(tn, K - 1);
              if (worst == 1)
              {
                done = true;  // nothing non-zero is shorter
                return;
              }
              maxdist = ldexp((double)(worst - 1) * (1.0 + 0x1p-30), -ne);
              pb      = prn * maxdist;
            }
          }
        };
        while (!done)
        {
          // CHILD chain: descend while the first child survives
          for (;;)
          {
            k               = __builtin_amdgcn_readfirstlane(k);
            const int kc    = k - 1;
            const double c1 = g_rl_f64(S, kc);
            const double x1 = round(c1);  // roundto(), enumerate_base.h:33-34
            const double a1 = x1 - c1;
            const double n1 = nd + a1 * a1 * g_rl_f64(rd, kc);
            if (!(n1 <= g_rl_f64(pb, kc)))
            {
              done = k >= bs;
              break;
            }
            if (lane < k)
              stk[btri(k) + lane] = S;
            {
              const int s1  = (c1 >= x1) ? 1 : -1;
              const bool me = lane == kc;
              cs            = me ? c1 : cs;
              xs            = me ? x1 : xs;
              pds           = me ? nd : pds;
              dxs           = me ? s1 : dxs;
              ddxs          = me ? s1 : ddxs;
              cnt += me ? 1ull : 0ull;
            }
            k  = kc;
            nd = n1;
            if (k == 0)
            {
              if (nd > 0.0)
                candidate();
              break;
            }
            const double mk = mu_blk[btri(k) + min(lane, k - 1)];
            S               = S - x1 * mk;
          }
          if (done)
            break;
          // STEP loop: next sibling at level k, climbing while they fail
          for (;;)
          {
            k                = __builtin_amdgcn_readfirstlane(k);
            const double par = stk[btri(k + 1) + min(lane, k)];  // S_{k+1}
            const double mk  = mu_blk[btri(k) + max(min(lane, k - 1), 0)];
            double xk        = g_rl_f64(xs, k);
            const double ck  = g_rl_f64(cs, k);
            const double pdk = g_rl_f64(pds, k);
            int dxk = __builtin_amdgcn_readlane(dxs, k), ddxk = __builtin_amdgcn_readlane(ddxs, k);
            if (pdk != 0.0)
            {
              xk += (double)dxk;
              ddxk = -ddxk;
              dxk  = ddxk - dxk;
            }
            else
            {
              xk += 1.0;
            }
            const bool me  = lane == k;
            xs             = me ? xk : xs;
            dxs            = me ? dxk : dxs;
            ddxs           = me ? ddxk : ddxs;
            const double a = xk - ck;
            nd             = pdk + a * a * g_rl_f64(rd, k);
            if (!(nd <= g_rl_f64(pb, k)))
            {
              ++k;
              if (k >= bs)
              {
                done = true;
                break;
              }
              continue;
            }
            cnt += me ? 1ull : 0ull;
            if (k == 0)
            {
              if (nd > 0.0)
              {
                candidate();
                if (done)
                  break;
              }
              continue;
            }
            S = par - xk * mk;
            break;
          }
        }
        // node total by the fplll rule (the initial descent is compensated, enumerate_base.cpp:181)
        unsigned long long tot = cnt;
        for (int off = 32; off > 0; off >>= 1)
          tot += (unsigned long long)__shfl_xor((long long)tot, off);
        nodes = (unsigned long long)g_rl_i64((long long)tot, 0) - (unsigned long long)(bs - 1);
      }
    }
    // ---- 6. outputs, in rank order; entries beyond found are zero -----------------------------------
    const bool ok = status == 1;
    found         = ok ? found : 0;
    for (int j = 0; j < K; ++j)
    {
      long long xr = 0;
      long long v[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        v[q] = 0;
      if (j < found)
      {
        const int sl = __builtin_amdgcn_readlane(slot, j);
        xr           = (lane < d) ? rec[(size_t)sl * d + lane] : 0;  // (each lane reads what it wrote itself)
        for (int i = 0; i < d; ++i)
        {
          const long long lx = g_rl_i64(xr, i);
          if (lx == 0)
            continue;
#pragma unroll
          for (int q = 0; q < NQ; ++q)
          {
            const int c = lane + 64 * q;
            v[q] += lx * ((c < n) ? b[(size_t)i * ldn + c] : 0);  // (no overflow: the sums of the candidate, in its order)
          }
        }
      }
      if (lane < d)
        o_sol[(size_t)j * d + lane] = xr;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
      {
        const int c = lane + 64 * q;
        if (c < n)
          o_vec[(size_t)j * n + c] = v[q];
      }
    }
    if (lane < K)
      A.norm[(size_t)W * K + lane] = lane < found ? tn : 0;
    if (lane == 0)
    {
      A.found[W]  = found;
      A.nodes[W]  = ok ? nodes : 0;
      A.status[W] = status;
    }
    __threadfence_block();
  }
}

template __global__ void svp_best_kernel<1>(GsoBatch, SvpBestWave);
template __global__ void svp_best_kernel<2>(GsoBatch, SvpBestWave);
template __global__ void svp_best_kernel<3>(GsoBatch, SvpBestWave);
template __global__ void svp_best_kernel<4>(GsoBatch, SvpBestWave);

}  // namespace fphip
