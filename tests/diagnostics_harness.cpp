// Host build of exoplanet_amd/csrc/exo_diagnostics_core.hpp -- the arithmetic of the rank-normalised split diagnostics -- in
// double and in long double, for tests/test_diagnostics_host.py and tests/make_diagnostics_golden.py: the whole summary of P
// parameters given as x [P][N][C] (draws, then chains), in the steps and the summation order of the kernels of
// exo_diagnostics.hip (the sorts are std::stable_sort here).  Results: out [P][diag::kOut].
// Compiled on its own (-DDIAGNOSTICS_HARNESS_MAIN) it is a program that runs a few small inputs, every array at its exact size:
// what an address / undefined-behaviour sanitizer build checks.
#define EXO_HOST_BUILD
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../exoplanet_amd/csrc/exo_diagnostics_core.hpp"

namespace {

using namespace diag;

bool before(double a, double b) { return a != a ? false : (b != b ? true : a < b); }      // NaN last, as torch.sort has it

std::vector<int64_t> order_of(const std::vector<double>& v) {
  std::vector<int64_t> idx(v.size());
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return before(v[a], v[b]); });
  return idx;
}

template <typename T>
void rank_into(const std::vector<double>& values, T* set) {
  const int64_t S = (int64_t)values.size();
  const std::vector<int64_t> perm = order_of(values);
  std::vector<double> sorted(S);
  for (int64_t i = 0; i < S; ++i) sorted[i] = values[perm[i]];
  for (int64_t i = 0; i < S; ++i) set[perm[i]] = z_of_rank<T>(rank2_of(sorted.data(), S, i), S);
}

template <typename T>
void one_parameter(const double* x, int64_t N, int64_t C, double* out) {
  for (int k = 0; k < kOut; ++k) out[k] = NAN;
  out[oMaxTBulk] = out[oMaxTLow] = out[oMaxTHigh] = out[oMaxTMean] = -1.0;
  if (N < 4 || C < 1) return;
  const int64_t L = N / 2, M = 2 * C, S = M * L, n_full = N * C;
  std::vector<double> xs(S), full(x, x + n_full);
  for (int64_t n = 0; n < L; ++n)
    for (int64_t m = 0; m < M; ++m) xs[n * M + m] = m < C ? x[n * C + m] : x[(N - L + n) * C + (m - C)];
  std::vector<double> sorted(xs);
  std::stable_sort(sorted.begin(), sorted.end(), before);
  std::stable_sort(full.begin(), full.end(), before);
  // moments
  std::vector<T> mom(kMoments);
  const double pivot_full = full[n_full / 2];
  T a = T(0);
  for (int64_t i = 0; i < n_full; ++i) a = a + (T(full[i]) - T(pivot_full));
  const T mean_rel = a / T(n_full);
  T b = T(0);
  for (int64_t i = 0; i < n_full; ++i) {
    const T d = (T(full[i]) - T(pivot_full)) - mean_rel;
    b = b + d * d;
  }
  mom[mMean] = T(pivot_full) + mean_rel;
  mom[mSd] = sqrt_of(b / T(n_full - 1));
  mom[mQ05] = quantile_sorted<T>(full.data(), n_full, 5);
  mom[mQ50] = quantile_sorted<T>(full.data(), n_full, 50);
  mom[mQ95] = quantile_sorted<T>(full.data(), n_full, 95);
  mom[mBad] = finite(full[0]) && finite(full[n_full - 1]) ? T(0) : T(1);
  mom[mConst] = full[0] == full[n_full - 1] ? T(1) : T(0);
  // the five sets, [set][n][m]
  std::vector<T> sets(kSets * S);
  const T pivot = T(sorted[S / 2]);
  std::vector<double> folded(S);
  for (int64_t j = 0; j < S; ++j) {
    const T v = T(xs[j]);
    folded[j] = (double)folded_of<T>(v, sorted.data(), S);
    sets[kLow * S + j] = v <= mom[mQ05] ? T(1) : T(0);
    sets[kHigh * S + j] = v <= mom[mQ95] ? T(1) : T(0);
    sets[kRaw * S + j] = v - pivot;
  }
  rank_into<T>(xs, sets.data() + kZ * S);
  rank_into<T>(folded, sets.data() + kZFold * S);
  // autocovariances in lag blocks, as the kernels form them
  const int64_t Lp = (L + kLagBlock - 1) / kLagBlock * kLagBlock;
  std::vector<T> state(kSets * kState), rho(Lp), means(M), lane(M);
  for (int set = 0; set < kSets; ++set) {
    const T* y = sets.data() + set * S;
    T* st = state.data() + set * kState;
    for (int64_t m = 0; m < M; ++m) {
      T sum = T(0);
      for (int64_t n = 0; n < L; ++n) sum = sum + y[n * M + m];
      means[m] = sum / T(L);
    }
    bool done = false;
    for (int64_t block = 0; block * kLagBlock < Lp && !done; ++block) {
      T sums[kLagBlock];
      for (int k = 0; k < kLagBlock; ++k) {
        const int64_t t = block * kLagBlock + k;
        for (int64_t m = 0; m < M; ++m) {
          T acc = T(0);
          for (int64_t n = t; n < L; ++n) acc = acc + (y[n * M + m] - means[m]) * (y[(n - t) * M + m] - means[m]);
          lane[m] = acc;
        }
        sums[k] = wave_order_sum(lane.data(), M);
      }
      if (block == 0) begin_set<T>(sums[0], means.data(), M, L, st);
      for (int k = 0; k < kLagBlock; ++k) rho[block * kLagBlock + k] = rho_of<T>(sums[k], M, L, st);
      if (block == 0) {
        rho[0] = T(1);
        st[sRo] = rho[1];
      }
      done = set == kZFold || advance_set<T>(rho.data(), (block + 1) * kLagBlock, M, L, st);
    }
  }
  std::vector<T> res(kOut);
  assemble<T>(state.data(), mom.data(), M, L, res.data());
  for (int k = 0; k < kOut; ++k) out[k] = (double)res[k];
}

}  // namespace

extern "C" {

int harness_n_out() { return kOut; }
int harness_lag_block() { return kLagBlock; }

void harness_summary(int long_double, const double* x, int64_t P, int64_t N, int64_t C, double* out) {
  for (int64_t p = 0; p < P; ++p) {
    if (long_double) one_parameter<long double>(x + p * N * C, N, C, out + p * kOut);
    else one_parameter<double>(x + p * N * C, N, C, out + p * kOut);
  }
}

double harness_ndtri(int long_double, int64_t rank2, int64_t S) {
  return long_double ? (double)z_of_rank<long double>(rank2, S) : z_of_rank<double>(rank2, S);
}

}  // extern "C"

#ifdef DIAGNOSTICS_HARNESS_MAIN
#include <stdio.h>

// an AR(1) series with ties, a constant one and one with a NaN, at an odd number of draws and at a length that takes
// several lag blocks
int main() {
  const int64_t shapes[3][2] = {{37, 3}, {8, 1}, {120, 2}};
  for (int long_double = 0; long_double < 2; ++long_double)
    for (const auto& shape : shapes) {
      const int64_t N = shape[0], C = shape[1], P = 3;
      std::vector<double> x(P * N * C), out(P * kOut);
      uint64_t s = 12345;
      for (int64_t c = 0; c < C; ++c) {
        double v = 0.0;
        for (int64_t n = 0; n < N; ++n) {
          s = s * 6364136223846793005ull + 1442695040888963407ull;
          const double u = (double)(s >> 11) / 9007199254740992.0 - 0.5;
          if (n % 3 != 2) v = 0.95 * v + u;                 // every third draw repeats the one before
          x[n * C + c] = v;
          x[N * C + n * C + c] = 2.5;
          x[2 * N * C + n * C + c] = n == 2 && c == 0 ? NAN : u;
        }
      }
      harness_summary(long_double, x.data(), P, N, C, out.data());
      printf("%s %ldx%ld: ess_bulk %.6g r_hat %.6g max_t %g | constant: ess %.6g | nan: %g\n", long_double ? "long double" : "double",
             (long)C, (long)N, out[oEssBulk], out[oRhat], out[oMaxTBulk], out[kOut + oEssBulk], out[2 * kOut + oEssBulk]);
      if (!(out[oEssBulk] > 0) || out[kOut + oEssBulk] != (double)(2 * C * (N / 2)) || out[2 * kOut + oEssBulk] == out[2 * kOut + oEssBulk])
        return 1;
    }
  return 0;
}
#endif
