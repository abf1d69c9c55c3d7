// enum_walk_cvp_list.hip — the list variants of the closest-vector walk: enum_walk_cvp_list_kernel<MU_LDS, false, CHAIN>.
// The text of enum_walk.hip compiled with FPHIP_CVP = 1 and FPHIP_LIST = 1 (DESIGN.md sections 3c, 3e).
#define FPHIP_CVP 1
#define FPHIP_LIST 1
#include "enum_walk.hip"
