// hlll_x_u.hip — hlll_x_u_kernel<NQ, FT>: the HLLL kernel of the selectable floating-point types that carries the
// transformation matrix u (fphip_hh_enable_transform under fphip_hh_hlll_ex and the stages of fphip_hh_hlll_ladder
// behind the first).  The text of hlll_x.hip compiled with FPHIP_HLLL_X_U = 1 (see the header there); nothing else
// lives here, so that hlll_x_kernel<NQ, FT> is the output of the same translation unit as before.
//
// Build: the flags of hlll_x.hip.
#define FPHIP_HLLL_X_U 1
#include "hlll_x.hip"
