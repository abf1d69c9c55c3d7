/*
 * fplll_hip_debug.h — entry points of libfplll_hip.so that are NOT part of the drop-in boundary
 * (include/fplll_hip.h): the host half of two device protocols exposed on its own so that the CPU
 * test-suite can check it without a GPU, and the calibration stream of the profiling recipe.
 * Nothing here is needed to use the library.
 */
#ifndef FPLLL_HIP_DEBUG_H
#define FPLLL_HIP_DEBUG_H

#include "fplll_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the mailbox service of fphip_gso_bkz_strategies answers for a block of `bs` rows with the
 * stored r_ii `r[i]` and doubled row exponents `e2[i]`: enumeration radius (scaled like r[0]), the
 * chosen pruning set (index into coeff_off, -1 = none) and its expectation — BKZReduction::
 * svp_reduction's radius / get_pruning arithmetic (bkz.cpp:82-98, 311-323) with the host libm.
 * tests/test_bkzs_host_cpu.py compares it with the oracle bit for bit. */
int fphip_debug_bkz_radius(const fphip_strategies *S, double gh_factor, int bs, int flags, double delta,
                           const double *r, const int *e2, double *max_dist, int *prune,
                           double *expectation);
/* The plan the service draws for rerandomize_block(lo, hi, density) (bkz.cpp:43-80) from `rnd`:
 * plan[0..n_moves) = move_row(b, a) as b | a << 8, then n_ops row additions a | b << 8 | add << 16. */
int fphip_debug_bkz_plan(fphip_rand_fn rnd, void *rnd_user, int lattice, int lo, int hi, int density,
                         unsigned *plan, int *n_moves, int *n_ops);
/* FETCH_SIZE calibration (profiles/r01_fetch_size_calibration.csv): streams `rows` rows of `row_bytes`
 * bytes, `stride` bytes apart, with the sweep kernels' load instruction; milliseconds in *ms_out. */
int fphip_debug_stream(fphip_ctx *ctx, long long rows, int row_bytes, long long stride, double *ms_out);

/* The device's double-double arithmetic (csrc/ftx.h) element-wise on host arrays, for its unit test
 * against multiprecision.  op: 0 add, 1 sub, 2 mul, 3 div, 4 sqrt(a), 5 nint(a). */
int fphip_debug_dd_op(fphip_ctx *ctx, int op, int count, const double *ahi, const double *alo,
                      const double *bhi, const double *blo, double *ohi, double *olo);
/* Either extended type of the device (csrc/ftx.h) on host arrays of component planes, a, b, out: [comps][count]
 * with comps 2 (double-double) or 4 (quad-double).  op 0..5 as above; 6 f_mul_d(a, b[0]); 7 / 8 f_le / f_gt (1.0 or
 * 0.0 in component 0); 9 f_rnd_we(a, (int)b[0]); wave-level, on wavefronts of 64 consecutive elements (count must be
 * a multiple of 64, FPHIP_ERROR otherwise): 10 f_wave_sum, 11 f_bcast(a, (int)b[0] & 63), 12 f_shfl_up(a, 1),
 * 13 f_shfl_xor(a, (int)b[0] & 63) with b[0] the same in the whole wavefront. */
int fphip_debug_ftx_op(fphip_ctx *ctx, int comps, int op, int count, const double *a, const double *b,
                       double *out);

/* mu (which = 0) or r (which = 1) of the last fphip_gso_lll_ex run in the arithmetic it ran in, one component plane
 * (0 .. 3; one plane at precision 53, two at 106, four at 212, the others read as zeros) at a time: the value is the
 * sum of the planes.  out[d][d] row-major, rows and columns in position order; mu(i,j) for j < i and r(i,j) for
 * j <= i are meaningful, stored like fphip_gso_get_mu / fphip_gso_get_r (apply fphip_gso_get_row_expo the same way).
 * (Those getters hand out a GSO recomputed in double from the reduced basis, not these.)
 * Opt-in: fphip_debug_gso_lll_ex_keep(g, 1) before the run makes fphip_gso_lll_ex keep a copy of the kernel's
 * leading planes and its slot table (two [batch][d][ldd] planes of device memory and two copies per run, which the
 * production path does not pay); without it, and after _keep(g, 0), the accessor returns FPHIP_ERROR.  After
 * fphip_gso_lll_ladder the planes are those of the LAST stage that ran, and only for the lattices it ran on. */
int fphip_debug_gso_lll_ex_keep(fphip_gso *g, int on);
int fphip_debug_gso_lll_ex_plane(fphip_gso *g, int lattice, int which, int plane, double *out);

/* Reference-order mode (fphip_enum_opts::ordered), the host half without a device.
 * fphip_debug_order_key: the depth-first key of a coefficient vector x[0..dim) — rank_out[k] = position of x[k]
 * among the children of its parent in the reference's walk (zig-zag around the rounded centre, upwards only on
 * the zero chain), compared lexicographically from level dim-1 down; nd_out (nullable): the partial distances,
 * nd_out[k] including level k.  mut / rdiag as fphip_enum_run takes them.
 * fphip_debug_order_replay: the replay over n candidates (dist[i], x[i*dim .. (i+1)*dim)) in ANY order — a superset
 * of what the reference visits: sorts them by the key, calls cb for exactly those the reference's walk would
 * report under the radius history cb's return values make, in its order.  Returns the number of cb calls (or
 * FPHIP_ERROR: bad argument, or a distance that is not the reference's sum for its vector); *final_bound: the
 * radius at the end. */
int fphip_debug_order_key(int dim, const double *mut, const double *rdiag, const double *x, unsigned *rank_out,
                          double *nd_out);
int fphip_debug_order_replay(int dim, double maxdist, const double *mut, const double *rdiag, const double *pruning,
                             int n, const double *dist, const double *x, fphip_sol_cb cb, void *user,
                             double *final_bound);

#ifdef __cplusplus
}
#endif
#endif
