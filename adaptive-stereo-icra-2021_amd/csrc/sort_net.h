// A compile-time sorting network for N values held in registers (cv_probe.hip): Batcher's odd-even merge sort over the next
// power of two P >= N with every comparator that touches an index >= N left out.  That is sound because the network sorts into
// DESCENDING order (the larger value goes to the lower index): values of -inf imagined at indices N..P-1 would never move, so
// the comparators that involve them do nothing.  The pairs are a flat table, so one fully unrolled loop over it indexes the
// register array with constants only.
#pragma once

template <int N>
struct SortNet {
  static constexpr int P = N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : N <= 8 ? 8 : N <= 16 ? 16 : N <= 32 ? 32 : 64;
  static_assert(N >= 1 && N <= 64, "SortNet: 1 <= N <= 64");
  int n = 0;
  unsigned char a[544] = {}, b[544] = {};      // 543 comparators at P = 64
};

template <int N>
constexpr SortNet<N> make_sort_net() {
  SortNet<N> net;
  constexpr int P = SortNet<N>::P;
  for (int p = 1; p < P; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j <= P - 1 - k; j += 2 * k)
        for (int i = 0; i <= k - 1 && i <= P - j - k - 1; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < N) {
            net.a[net.n] = (unsigned char)(i + j);
            net.b[net.n] = (unsigned char)(i + j + k);
            ++net.n;
          }
  return net;
}
