// enum_walk_list.hip — the list variants of the walk launches: enum_walk_list_kernel<MU_LDS, false, CHAIN>.  The text of
// enum_walk.hip compiled with FPHIP_LIST = 1 (see the header there, and DESIGN.md section 3e).  Build: its flags.
#define FPHIP_LIST 1
#include "enum_walk.hip"
