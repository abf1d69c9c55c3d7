// bkz_kernel_u.hip — bkz_kernel_u<NQ>: the BKZ kernel that carries the transformation matrix u (FPHIP_BKZ_TRANSFORM,
// MatGSO(b, u, ...) under bkz_reduction(b, u, param), bkz.cpp:849-927).  The text of bkz_kernel.hip compiled with
// FPHIP_BKZ_U = 1 (see the header there and lll_wave.h); nothing else lives here, so that bkz_kernel<NQ> is the
// output of the same translation unit as before.
//
// Build: the flags of bkz_kernel.hip.
#define FPHIP_BKZ_U 1
#include "bkz_kernel.hip"
