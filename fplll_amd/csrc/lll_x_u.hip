// lll_x_u.hip — lll_x_u_kernel<NQ, FT>: the LLL kernel of the selectable floating-point types that carries the
// transformation matrix u (fphip_gso_enable_transform under fphip_gso_lll_ex and the stages of fphip_gso_lll_ladder
// behind the first).  The text of lll_x.hip compiled with FPHIP_LLL_X_U = 1 (see the header there); nothing else
// lives here, so that lll_x_kernel<NQ, FT> is the output of the same translation unit as before.
//
// Build: the flags of lll_x.hip.
#define FPHIP_LLL_X_U 1
#include "lll_x.hip"
