// exo_optimize.hip -- batched L-BFGS on (chains, parameters) arrays that stay on the device (exoplanet_amd/optimize.py:
// LBFGS; exo_lbfgs_f64).  The chains of a batch are the draw dimension of the likelihood kernels; between two batched
// evaluations of value and gradient every chain makes its own decision -- Armijo test, history update, two-loop
// direction, convergence, the next trial point -- in ONE launch, one thread per chain (a chain moves a few hundred bytes:
// the cost is the launch).  The arithmetic is exo_optimize_core.hpp, shared with the host harness of the tests.
// A translation unit of its own: nothing else in the library is compiled differently.  Definition, layout and
// resources: DESIGN.md section 15.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_optimize_core.hpp"

namespace {

static_assert(lbfgs::kMaxHistory == EXO_LBFGS_MAX_HISTORY, "the header's bound is the core's");
constexpr int kLbfgsPtrs = 22;

struct LbfgsBatch {
  double *x, *g, *xt, *gt, *d;       // [D][n]
  const double* free;                // [D][n]
  double *hs, *hy;                   // [n_hist][n][D]
  double *hsy, *coef;                // [n_hist][D]
  double* logp;                      // [D]
  const double* lpt;                 // [D]
  double *alpha, *gamma, *grad_max;  // [D]
  int32_t *status, *n_iter, *n_eval, *m, *head, *n_rej, *n_small;   // [D]
  int64_t D;
  lbfgs::Rules<double> rules;
};

__device__ __forceinline__ lbfgs::Chain<double> chain_of(const LbfgsBatch& a, int64_t d) {
  const int64_t row = d * a.rules.n;
  lbfgs::Chain<double> c;
  c.x = a.x + row; c.g = a.g + row; c.xt = a.xt + row; c.d = a.d + row; c.gt = a.gt + row; c.free = a.free + row;
  c.hs = a.hs + d; c.hy = a.hy + d; c.hsy = a.hsy + d; c.coef = a.coef + d;
  c.stride = a.D;
  c.logp = a.logp + d; c.lpt = a.lpt + d; c.alpha = a.alpha + d; c.gamma = a.gamma + d; c.grad_max = a.grad_max + d;
  c.status = a.status + d; c.n_iter = a.n_iter + d; c.n_eval = a.n_eval + d; c.m = a.m + d; c.head = a.head + d;
  c.n_rej = a.n_rej + d; c.n_small = a.n_small + d;
  return c;
}

__global__ __launch_bounds__(64) void lbfgs_start_kernel(LbfgsBatch a) {
  const int64_t d = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (d >= a.D) return;
  lbfgs::start(chain_of(a, d), a.rules);
}

__global__ __launch_bounds__(64) void lbfgs_decide_kernel(LbfgsBatch a) {
  const int64_t d = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (d >= a.D) return;
  lbfgs::decide(chain_of(a, d), a.rules);
}

}  // namespace

extern "C" {

// ptrs: kLbfgsPtrs device pointers in the order of LbfgsBatch's pointer members
int exo_lbfgs_f64(const void* const* ptrs, int64_t n_chain, int32_t n_param, int32_t n_hist, int32_t max_linesearch, double c1,
                  double gtol, double ftol, int32_t phase, void* stream) {
  if (!ptrs || n_chain < 0 || n_param < 1 || n_hist < 1 || n_hist > EXO_LBFGS_MAX_HISTORY || max_linesearch < 1 || phase < 0 ||
      phase > 1)
    return EXO_ERR_INVALID_ARGUMENT;
  if (n_chain == 0) return EXO_OK;
  for (int k = 0; k < kLbfgsPtrs; ++k)
    if (!ptrs[k]) return EXO_ERR_INVALID_ARGUMENT;
  LbfgsBatch a;
  int k = 0;
  auto dp = [&]() { return (double*)ptrs[k++]; };
  auto ip = [&]() { return (int32_t*)ptrs[k++]; };
  a.x = dp(); a.g = dp(); a.xt = dp(); a.gt = dp(); a.d = dp(); a.free = dp(); a.hs = dp(); a.hy = dp(); a.hsy = dp();
  a.coef = dp(); a.logp = dp(); a.lpt = dp(); a.alpha = dp(); a.gamma = dp(); a.grad_max = dp();
  a.status = ip(); a.n_iter = ip(); a.n_eval = ip(); a.m = ip(); a.head = ip(); a.n_rej = ip(); a.n_small = ip();
  a.D = n_chain;
  a.rules = lbfgs::Rules<double>{n_param, n_hist, max_linesearch, c1, gtol, ftol};
  const dim3 grid((unsigned)((n_chain + 63) / 64)), block(64);
  if (phase == 0) hipLaunchKernelGGL(lbfgs_start_kernel, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(lbfgs_decide_kernel, grid, block, 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH;
}

}  // extern "C"
