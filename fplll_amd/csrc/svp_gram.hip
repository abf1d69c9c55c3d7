// svp_gram.hip — the N shortest vectors of every quadratic FORM of a batch (at most 64 variables, at most 64 vectors
// kept): one wavefront per form, the whole range in one launch.  shortest_vectors(MatGSOGram, sol_coord, sol_dist,
// max_sols) of the reference (svpcvp.cpp:276-454 reads mu, r and get_int_gram(i, i) of the GSO object only) on the state
// fphip_gram_update leaves — mu, r_ii, status, no row exponents, no basis anywhere —, with the decision on EXACT
// integers: tests/svp_gram_model.py is the model, operation by operation.  The walk loops, the LDS layout, the table
// across the lanes and the sorted insert are those of svp_best.hip (the text is copied, as cvp_wave.hip and
// svp_best.hip did: their code objects do not change).
//
// Per form, what differs from svp_best.hip:
//   1. the "row norms" are the diagonal g_ii, exact and already there; a diagonal entry <= 0: status 0;
//   2. the bound B0: the caller's, or the smallest g_ii below last_useful_index; the radius (double)B0 (1 + 2^-30),
//      inclusive, nothing seeded;
//   3. the rows cut on r_ii directly (no exponents): r_ii <= 2 r_00, with a caller's bound max(2 r_00, radius);
//      an r_ii among the rows walked that is <= 0 or not finite: status 0 (indefinite, semidefinite, rank-deficient
//      forms), as is a form whose update status is not 1;
//   4. the mu triangle in LDS: straight copies;
//   5. the evaluator: N = x G x^T as an exact integer.  Lane j forms y_j = sum_i x_i g_ij in 128 bits — every |x_i| is
//      checked to be below 2^57, so each product is below 2^120 and the 64 of them below 2^126: no step can leave the
//      128 bits.  With y_j = yh_j 2^64 + yl_j (yh signed, yl unsigned 64 bits), N = 2^64 sum_j x_j yh_j + sum_j x_j yl_j;
//      both sums are exact in 128 bits (each addend below 2^121, 64 of them).  N fits 63 bits iff the part above 2^64
//      is zero and the low word is below 2^63: that — or a coefficient of 2^57 and more — is status -2 (outputs zero),
//      a negative N (an indefinite form the doubles did not catch) is simply not accepted.  The accept, tie, shrink and
//      stop rules are svp_best.hip's.
// There is no vec: a form has no ambient space.  Outputs: found, sol_coord [K][d] by rank, norm [K], nodes, status.
//
// d <= 64: one lane per variable, no columns-per-lane template.  Branches in the walk are wave-uniform; level
// registers are read across lanes with g_rl_f64 / readlane.
#include "gso_wave.h"
#include "kernels.h"

namespace fphip
{

typedef __int128 gram_i128;

__device__ __forceinline__ int gtri(int k) { return (k * (k - 1)) >> 1; }

// the sum over the wave of 128-bit addends that cannot leave the 128 bits (see 5. above); every lane gets the total
__device__ __forceinline__ gram_i128 gram_sum_i128(gram_i128 v)
{
  for (int off = 32; off > 0; off >>= 1)
  {
    const unsigned long long lo = (unsigned long long)v, hi = (unsigned long long)(v >> 64);
    const unsigned long long ol = (unsigned long long)__shfl_xor((long long)lo, off);
    const unsigned long long oh = (unsigned long long)__shfl_xor((long long)hi, off);
    v += (gram_i128)(((unsigned __int128)oh << 64) | (unsigned __int128)ol);
  }
  return v;
}

__global__ void __launch_bounds__(256) svp_gram_kernel(GramBatch P, SvpGramWave A)
{
  extern __shared__ __attribute__((aligned(16))) char svp_gram_smem[];
  const int lane = threadIdx.x & 63;
  const int wpb  = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int d = P.d, ldd = P.ldd;
  const int K = A.max_sols;
  // per wave: the triangular column stack of the walk, then the mu triangle
  double *stk    = (double *)svp_gram_smem + (size_t)wave * (A.stack_doubles + A.mu_doubles);
  double *mu_blk = stk + A.stack_doubles;
  for (int W = blockIdx.x * wpb + wave; W < A.count; W += gridDim.x * wpb)
  {
    if (A.take && A.take[W] == 0)
      continue;
    const size_t L     = (size_t)(A.first + W);
    const long long *g = P.g + L * d * ldd;
    const double *mu   = P.mu + L * d * ldd;
    const double *rdg  = P.rdg + L * d;
    long long *rec   = A.rec + (size_t)W * K * d;  // [K][d] coefficient records by slot
    long long *o_sol = A.sol_coord + (size_t)W * K * d;

    int status               = P.status[L] == 1 ? 1 : 0;
    unsigned long long nodes = 0;
    long long tn             = 0;  // lane j < found: the norm of rank j
    int slot                 = 0;  // lane j < found: the record slot of rank j
    int found                = 0;

    // ---- 1. the diagonal: lane i keeps g_ii ------------------------------------------------------
    const bool in      = lane < d;
    const long long rn = in ? g[(size_t)lane * ldd + lane] : 1;
    if (__any(rn <= 0))
      status = 0;
    if (status == 1)
    {
      // ---- 2. the bound; 3. the rows cut ---------------------------------------------------------
      const double rr    = in ? rdg[lane] : 0.0;
      const double r00x2 = g_rl_f64(rr, 0) * 2.0;
      const long long bnd = A.bound ? A.bound[W] : 0;
      long long B0;
      int d_eff;
      if (bnd > 0)
      {
        B0               = bnd;
        const double thr = fmax(r00x2, (double)B0 * (1.0 + 0x1p-30));
        const uint64_t um = __ballot(in && lane > 0 && rr <= thr);
        d_eff             = um ? 64 - __clzll((long long)um) : 1;
      }
      else
      {
        const uint64_t um = __ballot(in && lane > 0 && rr <= r00x2);
        d_eff             = um ? 64 - __clzll((long long)um) : 1;
        B0                = g_rl_i64(rn, 0);  // get_basis_min: the smallest diagonal entry below d_eff
        for (int i = 1; i < d_eff; ++i)
        {
          const long long ni = g_rl_i64(rn, i);
          B0                 = ni < B0 ? ni : B0;
        }
      }
      const int bs   = d_eff;
      const bool inb = lane < bs;
      if (__any(inb && !(rr > 0.0 && rr <= 1.79769313486231570815e+308)))
        status = 0;  // not positive definite on the rows walked, as far as the doubles see
      const double radius0 = (double)B0 * (1.0 + 0x1p-30);
      if (status == 1 && radius0 > 0.0)
      {
        // ---- normalisation, enumerate.cpp:88-141 ------------------------------------------------
        int ne           = inb ? (int)fexponent(rr) : INT_MIN;
        ne               = max(wave_max_i32(ne), -1);  // normexp starts at -1, enumerate.cpp:88
        const double rd  = inb ? ldexp(rr, -ne) : 0.0;  // lane i: rdiag[i]
        const double prn = (inb && A.pruning) ? A.pruning[lane] : 1.0;
        double maxdist   = ldexp(radius0, -ne);
        double pb        = prn * maxdist;  // lane k: the bound of level k
        for (int k = 1; k < bs; ++k)
          if (lane < k)
            mu_blk[gtri(k) + lane] = mu[(size_t)k * ldd + lane];
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
          // every coefficient below 2^57 in absolute value (a NaN fails as well)
          if (__any(inb && !(fabs(xs) < 144115188075855872.0)))
          {
            status = -2;
            done   = true;
            return;
          }
          const long long xl = inb ? (long long)xs : 0;
          gram_i128 y        = 0;
          for (int i = 0; i < bs; ++i)
          {
            const long long lx = g_rl_i64(xl, i);
            if (lx == 0)
              continue;
            const long long gi = inb ? g[(size_t)i * ldd + lane] : 0;
            y += (gram_i128)lx * (gram_i128)gi;
          }
          const long long yh          = (long long)(y >> 64);
          const unsigned long long yl = (unsigned long long)y;
          const gram_i128 Hs = gram_sum_i128((gram_i128)xl * (gram_i128)yh);
          const gram_i128 Ls = gram_sum_i128((gram_i128)xl * (gram_i128)(unsigned __int128)yl);
          const gram_i128 T  = Hs + (Ls >> 64);  // N = T 2^64 + (the low word of Ls)
          const long long th = g_rl_i64((long long)(T >> 64), 0), tl = g_rl_i64((long long)T, 0);
          const long long nv = g_rl_i64((long long)(unsigned long long)Ls, 0);
          if (th < 0)
            return;  // N < 0: not a candidate
          if (th != 0 || tl != 0 || nv < 0)
          {  // a candidate beyond 63 bits: the form is given up
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
              rec[(size_t)sl * d + lane] = xl;
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
              stk[gtri(k) + lane] = S;
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
            const double mk = mu_blk[gtri(k) + min(lane, k - 1)];
            S               = S - x1 * mk;
          }
          if (done)
            break;
          // STEP loop: next sibling at level k, climbing while they fail
          for (;;)
          {
            k                = __builtin_amdgcn_readfirstlane(k);
            const double par = stk[gtri(k + 1) + min(lane, k)];  // S_{k+1}
            const double mk  = mu_blk[gtri(k) + max(min(lane, k - 1), 0)];
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
      if (j < found)
      {
        const int sl = __builtin_amdgcn_readlane(slot, j);
        xr           = (lane < d) ? rec[(size_t)sl * d + lane] : 0;  // (each lane reads what it wrote itself)
      }
      if (lane < d)
        o_sol[(size_t)j * d + lane] = xr;
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

}  // namespace fphip
