// observer_layout_main.cpp -- stand-alone driver of h-numo_amd/csrc/observer_layout.h for
// tests/test_observer_layout.py.  Every buffer has exactly the size its layout says, so the sanitizer sees
// an index outside it; the inputs hold 1, 2, 3 ... in memory order.
//
//   observer_layout_main pairs L NP npoin    the caller's (2*NP,npoin,L) packed: one line, 2*NP*npoin*L values of
//                                            the device's [L][NP][npoin][2]; that unpacked again: a second line
//   observer_layout_main transpose V M count planar [count][V][M] -> (V,M,count): one line (empty for count 0)
//   observer_layout_main blocks n per [most] block_count(n, per[, most]): one integer
// Exit status: 0, or 2 for a usage error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../h-numo_amd/csrc/observer_layout.h"

static std::vector<double> counted(size_t n) {
  std::vector<double> v(n);
  for (size_t i = 0; i < n; i++) v[i] = (double)(i + 1);
  return v;
}

static void line(const std::vector<double> &v) {
  for (size_t i = 0; i < v.size(); i++) printf(i ? " %.0f" : "%.0f", v[i]);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 4 || argc > 5) return 2;
  const char *what = argv[1];
  const size_t a = strtoull(argv[2], nullptr, 10), b = strtoull(argv[3], nullptr, 10), c = argc == 5 ? strtoull(argv[4], nullptr, 10) : 0;
  if (!strcmp(what, "blocks")) {
    printf("%d\n", argc == 5 ? hnumo::block_count(a, b, c) : hnumo::block_count(a, b));
    return 0;
  }
  if (argc != 5) return 2;
  if (!strcmp(what, "pairs")) {
    const int L = (int)a, NP = (int)b;
    const std::vector<double> in = counted(2 * (size_t)NP * c * L);
    std::vector<double> raw(in.size(), -1.0), out(in.size(), -1.0);
    hnumo::pairs_pack(in.data(), NP, L, c, raw.data());
    line(raw);
    hnumo::pairs_unpack(raw.data(), NP, L, c, out.data());
    line(out);
    return 0;
  }
  if (!strcmp(what, "transpose")) {
    const std::vector<double> raw = counted(a * b * c);
    std::vector<double> out(raw.size(), -1.0);
    hnumo::sample_transpose(raw.data(), (int)a, b, c, out.data());
    line(out);
    return 0;
  }
  return 2;
}
