// Host build of exoplanet_amd/csrc/exo_predictive_core.hpp for tests/test_predictive_host.py (g++, no GPU): the strided column
// accessor, the whole-number rank rule and the per-column routine, exactly as the kernel calls them.
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_predictive_core.hpp"

using namespace predictive;

namespace {

template <int Q, int B>
void run(const double* x, int64_t n_rows, int64_t n_cols, int64_t row_stride, const int64_t* num, const int64_t* den, int n_q,
         double* out, int32_t* n_valid, int32_t* n_pass) {
  int64_t a[Q], b[Q];
  for (int q = 0; q < Q; ++q) {
    a[q] = num[q < n_q ? q : n_q - 1];
    b[q] = den[q < n_q ? q : n_q - 1];
  }
  for (int64_t c = 0; c < n_cols; ++c) {
    double res[Q];
    int passes = 0;
    const int32_t m = column_quantiles<Q, B>(Column{x + c, row_stride}, n_rows, a, b, res, 1, &passes);
    for (int q = 0; q < n_q; ++q) out[q * n_cols + c] = res[q];
    if (n_valid) n_valid[c] = m;
    if (n_pass) n_pass[c] = passes;
  }
}

}  // namespace

extern "C" {

void harness_rank(int64_t m, int64_t a, int64_t b, int64_t* lo, int64_t* rem) {
  const Rank r = rank_of(m, a, b);
  *lo = r.lo;
  *rem = r.rem;
}

// the columns of x (n_rows, n_cols; rows row_stride doubles apart) one after the other, with the Q and the bits per pass the library picks
int harness_column_quantiles(const double* x, int64_t n_rows, int64_t n_cols, int64_t row_stride, const int64_t* num,
                             const int64_t* den, int n_q, double* out, int32_t* n_valid, int32_t* n_pass) {
  if (n_q < 1 || n_q > kMaxQ) return 1;
  if (n_q == 1) run<1, 3>(x, n_rows, n_cols, row_stride, num, den, n_q, out, n_valid, n_pass);
  else if (n_q <= 3) run<3, 2>(x, n_rows, n_cols, row_stride, num, den, n_q, out, n_valid, n_pass);
  else run<kMaxQ, 1>(x, n_rows, n_cols, row_stride, num, den, n_q, out, n_valid, n_pass);
  return 0;
}

}  // extern "C"
