// enum_kernels.h — ONE declaration of every __global__ kernel of the enumeration family that enum_host.hip launches
// and another file defines (enum_kernel.hip, enum_walk.hip and the files that compile those two texts again).  The
// kernel files include it too, before the macros that rename their kernels, so the compiler sees each declaration
// next to its definition and explicit instantiations.  kernels.h is the same for the other families.
#ifndef FPHIP_ENUM_KERNELS_H
#define FPHIP_ENUM_KERNELS_H

#include <hip/hip_runtime.h>

#include "enum_device.h"

namespace fphip
{
template <bool MU_LDS, bool SUBS, bool DUAL>
__global__ void enum_phase_kernel(DevShared *g, HostCtl *h, TaskBuf in, TaskBuf out, int d,
                                  int Lmax, int stop, unsigned task_lo, unsigned task_hi,
                                  const unsigned *idxlist, int launch_idx, int count_nodes,
                                  unsigned budget, const double *xhi_root, double *gstk, int Tsplit,
                                  unsigned *qh, const unsigned *rcnt, unsigned rcap,
                                  unsigned long long bound_init);
template <int NQT, bool SUBS, bool DUAL>
__global__ void enum_top_kernel(DevShared *g, HostCtl *h, TopBuf in, unsigned n_in, TopBuf out_top,
                                int stop, TaskBuf out, double *xhi_root, int d, double maxdist,
                                int count_nodes, int launch_idx, double *gtop);
__global__ void task_key_kernel(TaskBuf in, unsigned n, int d, unsigned long long *keys,
                                const double *xhi_root, const unsigned *slots);
template <bool MU_LDS, bool DUAL, bool CHAIN>
__global__ void enum_walk_kernel(DevShared *g, HostCtl *h, TaskBuf in, TaskBuf out, int d, int Lmax, unsigned task_lo,
                                 unsigned task_hi, const unsigned *idxlist, int launch_idx, int count_nodes,
                                 unsigned budget, const double *xhi_root, double *gstk, int Tsplit, unsigned *qh,
                                 const unsigned *rcnt, unsigned rcap, unsigned long long bound_init);
// the fourth generation of the walk (enum_walk4.hip: ready pair siblings)
template <bool MU_LDS, bool DUAL>
__global__ void enum_walk4_kernel(DevShared *g, HostCtl *h, TaskBuf in, TaskBuf out, int d, int Lmax, unsigned task_lo,
                                  unsigned task_hi, const unsigned *idxlist, int launch_idx, int count_nodes,
                                  unsigned budget, const double *xhi_root, double *gstk, int Tsplit, unsigned *qh,
                                  const unsigned *rcnt, unsigned rcap, unsigned long long bound_init);
// the fifth generation (enum_walk5.hip: child distances straight from the vector test)
template <bool MU_LDS, bool DUAL>
__global__ void enum_walk5_kernel(DevShared *g, HostCtl *h, TaskBuf in, TaskBuf out, int d, int Lmax, unsigned task_lo,
                                  unsigned task_hi, const unsigned *idxlist, int launch_idx, int count_nodes,
                                  unsigned budget, const double *xhi_root, double *gstk, int Tsplit, unsigned *qh,
                                  const unsigned *rcnt, unsigned rcap, unsigned long long bound_init);
// closest-vector mode (fphip_enum_opts::target): the same kernel texts compiled with the zero chain switched off and
// the zero leaf reported (enum_kernel_cvp.hip, enum_walk_cvp.hip)
template <bool MU_LDS, bool SUBS, bool DUAL>
__global__ void enum_phase_cvp_kernel(DevShared *g, HostCtl *h, TaskBuf in, TaskBuf out, int d, int Lmax, int stop,
                                      unsigned task_lo, unsigned task_hi, const unsigned *idxlist, int launch_idx,
                                      int count_nodes, unsigned budget, const double *xhi_root, double *gstk, int Tsplit,
                                      unsigned *qh, const unsigned *rcnt, unsigned rcap, unsigned long long bound_init);
template <bool MU_LDS, bool DUAL, bool CHAIN>
__global__ void enum_walk_cvp_kernel(DevShared *g, HostCtl *h, TaskBuf in, TaskBuf out, int d, int Lmax, unsigned task_lo,
                                     unsigned task_hi, const unsigned *idxlist, int launch_idx, int count_nodes,
                                     unsigned budget, const double *xhi_root, double *gstk, int Tsplit, unsigned *qh,
                                     const unsigned *rcnt, unsigned rcap, unsigned long long bound_init);
// list mode (fphip_enum_list): the same kernel texts compiled with the device-resident list as their sink
// (enum_kernel_list.hip, enum_walk_list.hip and their closest-vector twins)
template <bool MU_LDS, bool SUBS, bool DUAL>
__global__ void enum_phase_list_kernel(DevShared *g, HostCtl *h, TaskBuf in, TaskBuf out, int d, int Lmax, int stop,
                                       unsigned task_lo, unsigned task_hi, const unsigned *idxlist, int launch_idx,
                                       int count_nodes, unsigned budget, const double *xhi_root, double *gstk, int Tsplit,
                                       unsigned *qh, const unsigned *rcnt, unsigned rcap, unsigned long long bound_init,
                                       ListBuf lst);
template <bool MU_LDS, bool SUBS, bool DUAL>
__global__ void enum_phase_cvp_list_kernel(DevShared *g, HostCtl *h, TaskBuf in, TaskBuf out, int d, int Lmax, int stop,
                                           unsigned task_lo, unsigned task_hi, const unsigned *idxlist, int launch_idx,
                                           int count_nodes, unsigned budget, const double *xhi_root, double *gstk,
                                           int Tsplit, unsigned *qh, const unsigned *rcnt, unsigned rcap,
                                           unsigned long long bound_init, ListBuf lst);
template <bool MU_LDS, bool DUAL, bool CHAIN>
__global__ void enum_walk_list_kernel(DevShared *g, HostCtl *h, TaskBuf in, TaskBuf out, int d, int Lmax, unsigned task_lo,
                                      unsigned task_hi, const unsigned *idxlist, int launch_idx, int count_nodes,
                                      unsigned budget, const double *xhi_root, double *gstk, int Tsplit, unsigned *qh,
                                      const unsigned *rcnt, unsigned rcap, unsigned long long bound_init, ListBuf lst);
template <bool MU_LDS, bool DUAL, bool CHAIN>
__global__ void enum_walk_cvp_list_kernel(DevShared *g, HostCtl *h, TaskBuf in, TaskBuf out, int d, int Lmax,
                                          unsigned task_lo, unsigned task_hi, const unsigned *idxlist, int launch_idx,
                                          int count_nodes, unsigned budget, const double *xhi_root, double *gstk, int Tsplit,
                                          unsigned *qh, const unsigned *rcnt, unsigned rcap, unsigned long long bound_init,
                                          ListBuf lst);
template <bool DUAL>
__global__ void enum_bfs_cvp_kernel(DevShared *g, double maxdist, QueueMem *qm, TaskBuf f0, TaskBuf f1, TaskBuf fin, int L0,
                                    int nlev, int floor_level, float heavy, int count_nodes, int compact_n, int shard_index,
                                    int shard_count);
template <int NQT, bool SUBS, bool DUAL>
__global__ void enum_top_cvp_kernel(DevShared *g, HostCtl *h, TopBuf in, unsigned n_in, TopBuf out_top, int stop,
                                    TaskBuf out, double *xhi_root, int d, double maxdist, int count_nodes, int launch_idx,
                                    double *gtop);
__global__ void task_pack_kernel(TaskBuf in, unsigned lo, unsigned n, double *rec, const double *xhi_root, int xstr);
__global__ void task_unpack_kernel(TaskBuf out, unsigned lo, unsigned n, const double *rec, double *xhi_root, int xstr,
                                   unsigned root_base);
template <bool DUAL>
__global__ void enum_bfs_kernel(DevShared *g, double maxdist, QueueMem *qm, TaskBuf f0, TaskBuf f1,
                                TaskBuf fin, int L0, int nlev, int floor_level, float heavy, int count_nodes,
                                int compact_n, int shard_index, int shard_count);
}  // namespace fphip

#endif
