// kernels.h — what the host files and the kernel files of the GSO / LLL / BKZ / Householder / Gram / closest-vector
// families share: the argument structs that travel by value from host to kernel, and ONE declaration of every
// __global__ kernel a host file launches.  Each kernel file includes this header as well, so the compiler sees the
// declaration next to the definition and the explicit instantiations: a signature that drifts is a compile error
// there, not a link error (or a silently chosen overload) on the host side.  The enumeration family has its own
// header of the same kind (enum_kernels.h: its types come from enum_device.h, which no file of these families sees).
//
// The kernel files that compile one text twice (FPHIP_LLL_X_KERNEL, FPHIP_BKZ_KERNEL, ...) define their renaming
// macros after this include.
#ifndef FPHIP_KERNELS_H
#define FPHIP_KERNELS_H

#include <hip/hip_runtime.h>

#include "gram_device.h"
#include "gso_device.h"

namespace fphip
{

// lll_x.hip / lll_x_u.hip
struct LllX
{
  int batch, d, n, ldn, ldd, row_expo;
  long long *b, *b2;      // [batch][d][ldn]: rows by slot; b2: output, rows in position order
  double *bf;             // [batch][d][ldn]
  double *mu_hi, *mu_lo;  // [batch][d][ldd]: row = slot, column = position
  double *r_hi, *r_lo;
  double *gf_hi, *gf_lo;  // [batch][d][ldd]: Gram cache, entry (max slot, min slot); hi NaN = unknown
  double *mu_x, *r_x, *gf_x;  // quad-double: components 2 and 3 of the three arrays (two planes back to back each)
  long long *rexp;        // [batch][d] by slot
  int *status, *info;     // info[4]: final_kappa, n_swaps, zeros, iterations
  const int *only_failed; // precision ladder: non-null = only the lattices whose entry is not 1
  int kmin, kstart, kend;
  double delta, eta;
  int *slot_out;          // null, or [batch][d]: the slot of every position at the end (the key of the rows of mu / r)
};

// hlll_x.hip / hlll_x_u.hip
struct HlllX
{
  // R, V: [batch][d][ldn] in up to four planes each (P.R / P.V, Rlo / Vlo, and for quad-double Rx / Vx: two more
  // planes back to back); bf has no low part
  double *Rlo, *Vlo;
  // per lattice scalars, [batch][d] each: norm_square_b, dR, eR, prev_R, R(i,i) (four component planes each)
  double *sc;  // [batch][20][d]
  long long *prevE;
  double delta, theta;
  long long iter_cap;
  const int *only_failed;  // precision ladder: non-null = reduce only lattices whose entry is not 1
  // blocked application of the reflectors (compact WY, householder.cpp:151-184 sixteen reflectors at a time):
  // T of every block of 16 reflectors, [batch][ceil(d / 16)][16][16] (hi / lo planes); null = one by one
  double *Thi, *Tlo;
  double *Rx, *Vx;  // quad-double: components 2 and 3 of R and V ([2][batch][d][ldn] each)
};

// gso_kernel.hip (gso_sweep2_kernel of gso_sweep2.hip is declared in gso_sweep2.h, next to its geometry)
template <int NQ> __global__ void gso_sweep_kernel(GsoBatch P, int kmin, int kend, double eta, int mode);
template <int NQ> __global__ void hh_update_kernel(HhBatch P);
__global__ void gso_calib_kernel(const char *buf, size_t stride, int row_bytes, long long rows);  // (fphip_debug_stream)

// lll_kernel.hip; the LLL_EARLY_RED instantiations live in lll_kernel_early.hip
template <int NQ, bool EARLY>
__global__ void lll_kernel(GsoBatch P, int kmin, int kstart, int kend, double delta, double eta,
                           double logdelta);
// lll_x.hip, lll_x_u.hip (quad-double with u: NQ = 1 only)
template <int NQ, class FT> __global__ void lll_x_kernel(LllX A);
template <int NQ, class FT> __global__ void lll_x_u_kernel(LllX A, long long *Uall, long long *U2all, int ldu);

// bkz_kernel.hip, bkzs_kernel.hip
template <int NQ>
__global__ void bkz_kernel(GsoBatch P, int block_size, double delta, double eta, double logdelta,
                           int use_max_loops, int max_loops, int stack_doubles);
template <int NQ>
__global__ void bkzs_kernel(GsoBatch P, BkzStrat S, BkzMail *mailbox, int *abort_flag, int block_size,
                            int top_flags, double delta, double eta, double logdelta, int max_loops,
                            int stack_doubles);
namespace sdv
{
template <int NQ>
__global__ void bkzd_kernel(GsoBatch P, BkzStrat S, BkzMail *mailbox, int *abort_flag, int block_size,
                            int top_flags, double delta, double eta, double logdelta, int max_loops,
                            int stack_doubles, int run_mode);
}
// the same three with the transformation matrix u (FPHIP_BKZ_TRANSFORM): bkz_kernel_u.hip, bkzs_kernel_u.hip
template <int NQ>
__global__ void bkz_kernel_u(GsoBatch P, int block_size, double delta, double eta, double logdelta,
                             int use_max_loops, int max_loops, int stack_doubles, unsigned long long *ustats);
template <int NQ>
__global__ void bkzs_kernel_u(GsoBatch P, BkzStrat S, BkzMail *mailbox, int *abort_flag, int block_size,
                              int top_flags, double delta, double eta, double logdelta, int max_loops,
                              int stack_doubles, unsigned long long *ustats);
namespace sdv
{
template <int NQ>
__global__ void bkzd_kernel_u(GsoBatch P, BkzStrat S, BkzMail *mailbox, int *abort_flag, int block_size,
                              int top_flags, double delta, double eta, double logdelta, int max_loops,
                              int stack_doubles, int run_mode, unsigned long long *ustats);
}

// hlll_kernel.hip, hlll_kernel_u.hip, hh_blocked.hip, hh_rows.hip
template <int NQ> __global__ void hlll_kernel(HhBatch P, double delta, double theta, long long iter_cap);
template <int NQ>
__global__ void hlll_u_kernel(HhBatch P, double delta, double theta, long long iter_cap, long long *Uall, int ldu);
template <int NQ> __global__ void hh_blocked_kernel(HhBatch P, double *Tbuf);
template <int NT> __global__ void hh_rows_kernel(HhBatch P);
__global__ void hh_size_reduce_kernel(HhBatch P, int k, int end, int start, int *reduced);
__global__ void hh_size_reduce_u_kernel(HhBatch P, int k, int end, int start, int *reduced, long long *Uall, int ldu);
// hlll_x.hip, hlll_x_u.hip; the first also holds the unit-test kernels of ftx.h
template <int NQ, class FT> __global__ void hlll_x_kernel(HhBatch P, HlllX X);
template <int NQ, class FT> __global__ void hlll_x_u_kernel(HhBatch P, HlllX X, long long *Uall, int ldu);
__global__ void dd_op_kernel(const double *ahi, const double *alo, const double *bhi, const double *blo,
                             double *ohi, double *olo, int op, int count);
template <class FT> __global__ void ftx_op_kernel(const double *pa, const double *pb, double *po, int op, int count);

// cvp_prepare.hip: the closest-vector solver's target preparation and MatGSOInterface::babai, one target per lane
__global__ void cvp_unscale_kernel(GsoBatch P, int lattice, double *bfd, double *mu, double *rd);
__global__ void cvp_prepare_kernel(CvpPrep P);
__global__ void cvp_babai_kernel(int T, int ldt, int d, int start, int dimension, const double *mu, const double *v,
                                 long long *w, int *status, double *wx);
__global__ void list_vectors_kernel(ListVec P);  // list_vectors.hip

// svp_wave.hip: the shortest-vector solver, one wave per lattice of the range [first, first + count)
struct SvpWave
{
  int first, count;
  int stack_doubles, mu_doubles;  // per wave, in LDS: the walk's column stack (d (d + 1) / 2 + 2), the mu triangle
  const double *pruning;          // [d] or null (every coefficient 1)
  const int *take;                // [count] or null: 0 = this lattice goes another route, its outputs are left alone
  long long *sol_coord;           // [count][d]
  long long *vec;                 // [count][n]
  long long *norm;                // [count]
  unsigned long long *nodes;      // [count] fplll's counting rule
  int *status;                    // [count] 1 RED_SUCCESS, 0 update_gso failed, -2 beyond 63 bits (outputs zero)
};
template <int NQ> __global__ void svp_wave_kernel(GsoBatch P, SvpWave A);

// svp_best.hip: the max_sols shortest vectors of every lattice of the range, one wave per lattice
struct SvpBestWave
{
  int first, count;
  int stack_doubles, mu_doubles;  // per wave, in LDS: as SvpWave
  int max_sols;                   // K, 1 .. 64: the table's norms and its rank-to-slot map sit across the lanes
  const double *pruning;          // [d] or null (every coefficient 1)
  const int *take;                // [count] or null: 0 = this lattice goes another route, its outputs are left alone
  const long long *bound;         // [count] or null: the caller's bound on the squared norm; 0 = the default (N0)
  long long *rec;                 // [count][K][d] work space: the kept coefficient records by slot
  long long *sol_coord;           // [count][K][d] by rank; entries beyond found are zero
  long long *vec;                 // [count][K][n]
  long long *norm;                // [count][K]
  int *found;                     // [count] <= K
  unsigned long long *nodes;      // [count] fplll's counting rule
  int *status;                    // [count] 1 RED_SUCCESS, 0 update_gso failed, -2 beyond 63 bits (outputs zero)
};
template <int NQ> __global__ void svp_best_kernel(GsoBatch P, SvpBestWave A);

// cvp_wave.hip: the closest-vector solver, one wave per target of ONE lattice; the inputs are the device outputs of
// the preparation (CvpPrep) and the true mu / r_ii of cvp_unscale_kernel
struct CvpWave
{
  int lattice, T;
  int stack_doubles, mu_doubles;  // in LDS: per wave the walk's column stack (d (d + 1) / 2 + 2); per workgroup the mu triangle
  unsigned long long max_nodes;   // 0: no budget
  const long long *coef;          // [T][d]
  const double *tcoord;           // [T][d]
  const double *descent;          // [T]
  const int *pstatus;             // [T] the preparation's status
  const long long *targets;       // [T][n]
  const double *mu, *rd;          // [d][d], [d]: the true values
  long long *x;                   // [T][d] the best point's coefficients on the REDUCED target (the caller adds coef)
  double *dist;                   // [T] its walk distance
  long long *norm;                // [T] its exact squared distance
  unsigned long long *nodes;      // [T] accepted (level, coefficient) pairs, leaves included
  int *found;                     // [T] 0: not walked, or no candidate — the caller fills in the rounding descent
  int *status;                    // [T] the preparation's, -2 beyond 63 bits, 2 the node budget ended the walk
};
template <int NQ> __global__ void cvp_wave_kernel(GsoBatch P, CvpWave A);

// lll_gram.hip
template <int NQ> __global__ void lll_gram_kernel(GramBatch P, double delta, double eta, double logdelta, int siegel);
template <int NQ> __global__ void gram_update_kernel(GramBatch P);

// svp_gram.hip: the max_sols shortest vectors of every quadratic form of the range, one wave per form (d <= 64)
struct SvpGramWave
{
  int first, count;
  int stack_doubles, mu_doubles;  // per wave, in LDS: as SvpWave
  int max_sols;                   // K, 1 .. 64: the table's norms and its rank-to-slot map sit across the lanes
  const double *pruning;          // [d] or null (every coefficient 1)
  const int *take;                // [count] or null: 0 = this form goes another route, its outputs are left alone
  const long long *bound;         // [count] or null: the caller's bound on x G x^T; 0 = the default (min g_ii)
  long long *rec;                 // [count][K][d] work space: the kept coefficient records by slot
  long long *sol_coord;           // [count][K][d] by rank; entries beyond found are zero
  long long *norm;                // [count][K]
  int *found;                     // [count] <= K
  unsigned long long *nodes;      // [count] fplll's counting rule
  int *status;                    // [count] 1, 0 update failed / not positive definite, -2 beyond 63 bits (outputs zero)
};
__global__ void svp_gram_kernel(GramBatch P, SvpGramWave A);

}  // namespace fphip

#endif
