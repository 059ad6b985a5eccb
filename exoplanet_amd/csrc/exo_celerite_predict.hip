// exo_celerite_predict.hip -- the predictive variance of a celerite GP (celerite2's GaussianProcess.predict(return_var=True),
// and of one component of the kernel): one lane per draw runs the forward factorisation and the backward smoother of
// exo_celerite_predict.hpp.  A utility beside the likelihood, not part of the per-step path: a translation unit of its own,
// so that none of the likelihood's kernels changes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <utility>

#include "../../include/exoplanet_amd.h"
#include "exo_celerite_predict.hpp"

namespace {

using namespace gp;

constexpr int kWave = 64;

template <int J>
__global__ __launch_bounds__(kWave) void celerite_predict_var_kernel(const double* __restrict__ t,
                                                                     const double* __restrict__ diag, int64_t n_diag, int64_t n,
                                                                     Coefs cf, const int32_t* __restrict__ slot_mask,
                                                                     int64_t n_draw, const double* __restrict__ tq, int64_t m,
                                                                     double* __restrict__ var, double* __restrict__ work) {
  const int64_t draw = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (draw >= n_draw) return;
  predict_var_lane<J>(t, diag, n_diag, n, cf, slot_mask, tq, m, var, work, n_draw, draw);
}

template <int J>
__global__ __launch_bounds__(kWave) void celerite_solve_kernel(const double* __restrict__ t, const double* __restrict__ diag,
                                                               int64_t n_diag, int64_t n, Coefs cf, int64_t n_draw,
                                                               const double* __restrict__ y, double* __restrict__ alpha,
                                                               double* __restrict__ work) {
  const int64_t draw = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (draw >= n_draw) return;
  solve_lane<J>(t, diag, n_diag, n, cf, y, alpha, work, n_draw, draw);
}

// (the next three: as in exo_celerite.hip)
inline int launch_status() { return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH; }

inline bool gp_args_ok(int64_t n, int64_t n_diag, int32_t n_real, int32_t n_complex, int64_t n_draw) {
  const int J = n_real + 2 * n_complex;
  return n >= 1 && n_draw >= 1 && n_real >= 0 && n_complex >= 0 && J >= 1 && J <= EXO_GP_MAX_J &&
         (n_diag == 1 || n_diag == n_draw);
}

template <int V>
using IntK = std::integral_constant<int, V>;
template <int Lo, class F, int... I>
bool with_J_seq(int J, F&& f, std::integer_sequence<int, I...>) {
  return ((J == Lo + I ? (f(IntK<Lo + I>{}), true) : false) || ...);
}
template <int Lo, int Hi, class F>
bool with_J(int J, F&& f) {
  return with_J_seq<Lo>(J, f, std::make_integer_sequence<int, Hi - Lo + 1>{});
}

}  // namespace

extern "C" {

int64_t exo_celerite_predict_var_work_doubles(int64_t n, int64_t m, int32_t n_real, int32_t n_complex, int64_t n_draw) {
  const int J = n_real + 2 * n_complex;
  if (n < 1 || m < 0 || n_draw < 0 || n_real < 0 || n_complex < 0 || J < 1 || J > EXO_GP_MAX_J) return -1;
  return predict_var_work_doubles(n, m, J, n_draw);
}

int exo_celerite_predict_var_f64(const double* t, const double* diag, int64_t n_diag, int64_t n, const double* coef_real,
                                 int32_t n_real, const double* coef_complex, int32_t n_complex, const int32_t* pair_kind,
                                 const int32_t* slot_mask, int64_t n_draw, const double* tq, int64_t m, double* var, double* work,
                                 int64_t work_doubles, void* stream) {
  if (n_draw == 0 || m == 0) return EXO_OK;
  if (!gp_args_ok(n, n_diag, n_real, n_complex, n_draw) || m < 0 || !t || !diag || !tq || !var || !work ||
      (n_real > 0 && !coef_real) || (n_complex > 0 && !coef_complex))
    return EXO_ERR_INVALID_ARGUMENT;
  if (work_doubles < predict_var_work_doubles(n, m, n_real + 2 * n_complex, n_draw)) return EXO_ERR_WORKSPACE;
  const Coefs cf{coef_real, coef_complex, pair_kind, n_real, n_complex, t};
  const dim3 grid((unsigned)((n_draw + kWave - 1) / kWave)), block(kWave);
  if (!with_J<1, EXO_GP_MAX_J>(cf.J(), [&](auto jj) {
        hipLaunchKernelGGL((celerite_predict_var_kernel<decltype(jj)::value>), grid, block, 0, (hipStream_t)stream, t, diag, n_diag,
                           n, cf, slot_mask, n_draw, tq, m, var, work);
      }))
    return EXO_ERR_INVALID_ARGUMENT;
  return launch_status();
}

int64_t exo_celerite_solve_work_doubles(int64_t n, int32_t n_real, int32_t n_complex, int64_t n_draw) {
  const int J = n_real + 2 * n_complex;
  if (n < 1 || n_draw < 0 || n_real < 0 || n_complex < 0 || J < 1 || J > EXO_GP_MAX_J) return -1;
  return solve_work_doubles(n, J, n_draw);
}

int exo_celerite_solve_f64(const double* t, const double* diag, int64_t n_diag, int64_t n, const double* coef_real, int32_t n_real,
                           const double* coef_complex, int32_t n_complex, const int32_t* pair_kind, int64_t n_draw, const double* y,
                           double* alpha, double* work, int64_t work_doubles, void* stream) {
  if (n_draw == 0) return EXO_OK;
  if (!gp_args_ok(n, n_diag, n_real, n_complex, n_draw) || !t || !diag || !y || !alpha || !work || y == alpha ||
      (n_real > 0 && !coef_real) || (n_complex > 0 && !coef_complex))
    return EXO_ERR_INVALID_ARGUMENT;
  if (work_doubles < solve_work_doubles(n, n_real + 2 * n_complex, n_draw)) return EXO_ERR_WORKSPACE;
  const Coefs cf{coef_real, coef_complex, pair_kind, n_real, n_complex, t};
  const dim3 grid((unsigned)((n_draw + kWave - 1) / kWave)), block(kWave);
  if (!with_J<1, EXO_GP_MAX_J>(cf.J(), [&](auto jj) {
        hipLaunchKernelGGL((celerite_solve_kernel<decltype(jj)::value>), grid, block, 0, (hipStream_t)stream, t, diag, n_diag, n, cf,
                           n_draw, y, alpha, work);
      }))
    return EXO_ERR_INVALID_ARGUMENT;
  return launch_status();
}

}  // extern "C"
