// list_sort_host.cpp — a stand-alone program around the host half of the list mode (fphip_list_sort_records,
// enum_host.hip): the canonical sort and copy of the records, for a memory-checker run of that file on the host.
// Not compiled by build().  Build enum_host.hip's host side and this file with the sanitizers and link the library's
// other objects, e.g.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Xarch_host -fsanitize=address,undefined \
//         -c fplll_amd/csrc/enum_host.hip -o enum_host_san.o
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -c tests/native/list_sort_host.cpp -o list_sort_main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined list_sort_main.o enum_host_san.o \
//         <the other objects of fplll_amd/lib/obj, enum_host.hip.o left out> -pthread -o list_sort_host
// and run it: it needs no device.  Exit status 0 and no report = clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/fplll_hip.h"

int main()
{
  int bad = 0;
  for (int dim : {1, 2, 5, 24, 64})
    for (uint64_t n : {0ull, 1ull, 2ull, 63ull, 1000ull})
    {
      // exactly n records in, exactly n out: the vectors have no slack, so a read or write past them is reported
      std::vector<double> di(n), xi(n * dim), dout(n), xo(n * dim);
      unsigned s = 12345u + (unsigned)dim * 977u + (unsigned)n;
      for (uint64_t i = 0; i < n; ++i)
      {
        s     = s * 1664525u + 1013904223u;
        di[i] = (double)((s >> 24) % 3);  // three distances: long runs of ties
        for (int k = 0; k < dim; ++k)
        {
          s               = s * 1664525u + 1013904223u;
          xi[i * dim + k] = (double)((int)((s >> 20) % 7) - 3);
        }
      }
      fphip_list_sort_records(dim, n, di.data(), xi.data(), dout.data(), xo.data());
      for (uint64_t i = 1; i < n; ++i)
      {
        bool le = dout[i - 1] < dout[i];
        if (dout[i - 1] == dout[i])
        {
          le = true;
          for (int k = dim - 1; k >= 0; --k)
            if (xo[(i - 1) * dim + k] != xo[i * dim + k])
            {
              le = xo[(i - 1) * dim + k] < xo[i * dim + k];
              break;
            }
        }
        if (!le)
          ++bad;
      }
    }
  printf("list_sort_host: %d records out of order\n", bad);
  return bad ? 1 : 0;
}
