// enum_walk_cvp.hip — the closest-vector variants of the walk launches: enum_walk_cvp_kernel<MU_LDS, false, CHAIN>,
// both generations.  The text of enum_walk.hip compiled with FPHIP_CVP = 1 (see the header there, and DESIGN.md
// section 3c).
//
// Build: the flags of enum_walk.hip.
#define FPHIP_CVP 1
#include "enum_walk.hip"
