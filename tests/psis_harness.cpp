// Host build of exoplanet_amd/csrc/exo_psis_core.hpp for tests/test_psis_host.py (g++, no GPU): the per-column routine, one
// lane owning the column, on the strided column accessor the kernel uses.
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_psis_core.hpp"

extern "C" {

// the columns of x (n_rows, n_cols; rows row_stride doubles apart) one after the other
int harness_column_psis(const double* x, int64_t n_rows, int64_t n_cols, int64_t row_stride, int32_t n_tail_max, double* out_elpd,
                        double* out_k, double* out_lppd, double* out_var, int32_t* out_n_tail) {
  if (n_tail_max < 1 || n_tail_max > psis::kMaxTail) return 1;
  double tail[psis::kMaxTail];
  for (int64_t c = 0; c < n_cols; ++c) {
    const psis::Result r = psis::column_psis(psis::Column{x + c, row_stride}, n_rows, n_tail_max, tail);
    out_elpd[c] = r.elpd;
    out_k[c] = r.k;
    out_lppd[c] = r.lppd;
    out_var[c] = r.var;
    out_n_tail[c] = r.n_tail;
  }
  return 0;
}

}  // extern "C"
