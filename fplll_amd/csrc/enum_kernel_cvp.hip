// enum_kernel_cvp.hip — the closest-vector variants of the split / overflow walk, of the breadth-first stage and of the
// top walk of blocks above 64 rows: enum_phase_cvp_kernel<MU_LDS, false, false>, enum_bfs_cvp_kernel<false> and
// enum_top_cvp_kernel<NQT, false, false> (NQT = 2, 4).  The text of enum_kernel.hip compiled
// with FPHIP_CVP = 1 (see the header there, and DESIGN.md section 3c); nothing else lives here, so that the kernels of
// the shortest-vector walk are the output of the same translation unit as before.
//
// Build: the flags of enum_kernel.hip.
#define FPHIP_CVP 1
#include "enum_kernel.hip"
