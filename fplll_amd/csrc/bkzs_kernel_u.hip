// bkzs_kernel_u.hip — bkzs_kernel_u<NQ> and sdv::bkzd_kernel_u<NQ>: BKZ with strategies / self-dual BKZ / slide
// reduction carrying the transformation matrix u (FPHIP_BKZ_TRANSFORM).  The text of bkzs_kernel.hip compiled with
// FPHIP_BKZ_U = 1 (see the header there and lll_wave.h); nothing else lives here, so that bkzs_kernel<NQ> — a
// 256-register build — and bkzd_kernel<NQ> are the output of the same translation unit as before.
//
// Build: the flags of bkzs_kernel.hip.
#define FPHIP_BKZ_U 1
#include "bkzs_kernel.hip"
