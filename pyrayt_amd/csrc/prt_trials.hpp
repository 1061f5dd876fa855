// prt_trials.hpp -- how the two Monte Carlo passes launch k_tol_sum (prt_tolerance.hpp), k_mtft_moments and k_mtft_sum
// (prt_mtf_tolerance.hpp): a thread holds its trials' coefficients padded with zeros to the next
// multiple of four columns, and a call's trials go in launches of whole tiles.  The kernels keep their own prologues.
#pragma once

// launch(std::integral_constant<int, CP>(), more...) for the smallest multiple of four columns that holds K, MAX at most
template <int MAX, class Launch, class... More>
static void trial_columns(int K, Launch&& launch, More... more) {
  static_assert(MAX == 16 || MAX == 20, "the ladder ends at 16 or at 20 columns");
  if (K <= 4) launch(std::integral_constant<int, 4>(), more...);
  else if (K <= 8) launch(std::integral_constant<int, 8>(), more...);
  else if (K <= 12) launch(std::integral_constant<int, 12>(), more...);
  else if (MAX == 16 || K <= 16) launch(std::integral_constant<int, 16>(), more...);
  else if constexpr (MAX == 20) launch(std::integral_constant<int, 20>(), more...);
}

// the M trials of a call in launches of at most `most`: launch(first, n)
template <class Launch>
static void trial_launches(int M, int64_t most, Launch&& launch) {
  for (int first = 0; first < M; first += (int)most) launch(first, M - first < most ? M - first : (int)most);
}
