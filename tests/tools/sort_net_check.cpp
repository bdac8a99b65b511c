// Host check of csrc/sort_net.h, the comparator table cv_probe.hip sorts a pixel's D values with: by the 0-1 principle a network
// sorts every input if it sorts every input of zeros and ones.  Exhaustive for N <= 16 (2^N inputs), and for the larger instances
// random 0/1 inputs and random inputs with repeated values against std::sort.  Exit status 0 = every instance sorts.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>

#include "../../adaptive-stereo-icra-2021_amd/csrc/sort_net.h"

template <int N>
int check() {
  constexpr SortNet<N> net = make_sort_net<N>();
  const long trials = N <= 16 ? (1L << N) : 200000;
  long bad = 0;
  for (long t = 0; t < trials; ++t) {
    float v[N], w[N];
    for (int i = 0; i < N; ++i)
      v[i] = w[i] = N <= 16 ? (float)((t >> i) & 1) : ((t & 1) ? (float)(rand() & 1) : (float)(rand() % 7) - 3.f);
    for (int k = 0; k < net.n; ++k) {
      const float x = v[net.a[k]], y = v[net.b[k]];
      v[net.a[k]] = std::max(x, y);
      v[net.b[k]] = std::min(x, y);
    }
    std::sort(w, w + N, std::greater<float>());
    for (int i = 0; i < N; ++i)
      if (v[i] != w[i]) { ++bad; break; }
  }
  printf("N %d: %d comparators, %ld wrong of %ld inputs\n", N, net.n, bad, trials);
  return bad != 0;
}

int main() {
  srand(12345);
  // the kernel's four instances, and sizes around the powers of two
  return check<4>() + check<12>() + check<24>() + check<64>() + check<1>() + check<2>() + check<3>() + check<5>() + check<9>() +
         check<16>() + check<17>() + check<33>() + check<63>();
}
