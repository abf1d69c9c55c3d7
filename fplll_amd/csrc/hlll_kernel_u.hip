// hlll_kernel_u.hip — hlll_u_kernel<NQ>: the exact-order HLLL kernel that carries the transformation matrix u
// (fphip_hh_enable_transform, MatHouseholder(b, u, ...) under hlll_reduction(b, u, ...), householder.cpp:372-398 and
// :456-559).  The text of hlll_kernel.hip compiled with FPHIP_HLLL_U = 1 (see the header there); nothing else lives
// here, so that hlll_kernel<NQ> is the output of the same translation unit as before.
//
// Build: the flags of hlll_kernel.hip.
#define FPHIP_HLLL_U 1
#include "hlll_kernel.hip"
