// enum_kernel_cvp_list.hip — the list variant of the closest-vector split / overflow walk:
// enum_phase_cvp_list_kernel<MU_LDS, false, false>.  enum_kernel.hip with FPHIP_CVP = 1 and FPHIP_LIST = 1.
#define FPHIP_CVP 1
#define FPHIP_LIST 1
#include "enum_kernel.hip"
