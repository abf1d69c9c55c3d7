// enum_kernel_list.hip — the list variant of the split / overflow walk: enum_phase_list_kernel<MU_LDS, false, false>.
// The text of enum_phase_kernel (enum_kernel.hip) compiled with FPHIP_LIST = 1.  Build: its flags.
#define FPHIP_LIST 1
#include "enum_kernel.hip"
