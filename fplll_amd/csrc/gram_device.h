// gram_device.h — device-resident state of a BATCH of integer quadratic forms (MatGSOGram<Z_NR<long>, FP_NR<double>>,
// GSO_INT_GRAM), shared by lll_gram.hip and gram_host.hip.
//
// Layout in HBM (one form after another, dense [batch][...] slabs; ldd = d rounded up to 16, at most 256):
//   g    [batch][d][ldd]  int64   the Gram matrix, BOTH triangles stored and kept equal; during a reduction it is
//                                 addressed [slot_i][slot_j] (rows never move, lll_kernel.hip), outside one the slots
//                                 are the positions
//   g2   [batch][d][ldd]  int64   the result in position order (swapped with g by the host, like b2 / b)
//   u/u2 [batch][d][ldd]  int64   the transformation rows (nullptr: not tracked), in the slots of g's rows / in order
//   gf   [batch][d][ldd]  double  (double) g, entry by entry: MatGSOGram::get_gram is f.set_z(g(i, j))
//   mu, muT, r, rdg, vc           as in gso_device.h (no row exponents: row_expo is all zero with GSO_INT_GRAM)
#ifndef FPHIP_GRAM_DEVICE_H
#define FPHIP_GRAM_DEVICE_H

namespace fphip
{
struct GramBatch
{
  int batch, d, ldd;
  long long *g, *g2;
  long long *u, *u2;
  double *gf;
  double *mu, *muT, *r, *rdg;
  int *vc;
  int *status;  // [batch] 1 ok, 0 RED_GSO_FAILURE, -1 RED_BABAI_FAILURE, -2 multiplier > 63 bits, -3 RED_LLL_FAILURE
  int *info;    // [batch][4] final_kappa, n_swaps, zeros, loop iterations (low 31 bits)
};
}  // namespace fphip
#endif
