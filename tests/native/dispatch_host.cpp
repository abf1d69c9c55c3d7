// The two dispatchers of fplll_amd/csrc/host_common.h, compiled for the host (tests/test_dispatch_cpu.py): every
// width class and every precision reaches the instantiation of its own value, exactly once — the one place where a
// wrong digit could now send a launch to the wrong kernel.
#include <cstdio>
#include <type_traits>

#define FPHIP_DISPATCH_HOST_TEST
#include "../../fplll_amd/csrc/host_common.h"

using namespace fphip;

static int failures = 0;
static void check(bool ok, const char *what, int arg)
{
  printf("%s %s(%d)\n", ok ? "ok" : "FAIL", what, arg);
  failures += ok ? 0 : 1;
}

int main()
{
  // nq = 1 .. 4 call f with 1 .. 4; anything above is the widest class
  const int want_nq[][2] = {{1, 1}, {2, 2}, {3, 3}, {4, 4}, {5, 4}};
  for (const auto &w : want_nq)
  {
    int calls = 0, got = 0;
    dispatch_nq(w[0], [&](auto NQ) {
      static_assert(std::is_same<decltype(NQ), std::integral_constant<int, decltype(NQ)::value>>::value, "");
      constexpr int as_template_argument = NQ;  // (what a launch site does: kernel<NQ>)
      ++calls;
      got = as_template_argument;
    });
    check(calls == 1 && got == w[1], "dispatch_nq", w[0]);
  }
  // the value f returns comes back (the hipFuncSetAttribute sites return its hipError_t)
  check(dispatch_nq(3, [](auto NQ) { return 10 * NQ; }) == 30, "dispatch_nq returns", 3);

  // 53 -> double, 106 -> DD, 212 -> QD; anything else is double, as at every launch site
  const int want_ft[][2] = {{53, 1}, {106, 2}, {212, 4}, {0, 1}, {107, 1}};
  for (const auto &w : want_ft)
  {
    int calls = 0, got = 0;
    dispatch_precision(w[0], [&](auto ft) {
      using FT = typename decltype(ft)::type;
      ++calls;
      got = std::is_same<FT, double>::value ? 1 : std::is_same<FT, DD>::value ? 2 : std::is_same<FT, QD>::value ? 4 : -1;
    });
    check(calls == 1 && got == w[1], "dispatch_precision", w[0]);
  }
  return failures ? 1 : 0;
}
