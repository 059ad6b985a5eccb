// exo_priors.hip -- priors and constrained parameters of a ParameterSpace (exoplanet_amd/distributions.py): ONE kernel from the
// samplers' unconstrained array z[n_chain][n_free] to every named parameter and the chains' log prior, ONE kernel back.
// ABI: include/exoplanet_amd.h (exo_prior_transform_f64 / _vjp_f64); arithmetic: exo_priors_core.hpp; DESIGN.md section 10.
//
// A lane is a chain and walks the block table.  The table and the output pointers are kernel arguments (by value): they are
// the same for every lane, so the switch on a block's kind does not diverge and the table is read through the scalar unit.
// The chain's log prior is summed in a register in table order: no reduction across lanes, no atomics, and the result does
// not depend on the launch geometry (eager launch and graph replay agree bit for bit).  z is n_chain x n_free x 8 bytes --
// 245 KB at 1024 chains of 30 coordinates -- and a lane touches its own row only: the kernels are latency-bound (a handful of
// exp / log1p / sqrt chains per coordinate behind one strided load), not bandwidth-bound.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_priors_core.hpp"

namespace {

struct PriorTable {
  exo_prior_block b[EXO_PRIOR_MAX_BLOCKS];
  int32_t n_block, n_free;
};

struct PriorOutputs {
  double* p[EXO_PRIOR_MAX_OUTPUTS];
};

struct PriorCotangents {
  const double* p[EXO_PRIOR_MAX_OUTPUTS];
};

inline int launch_status() { return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH; }

__global__ __launch_bounds__(64) void exo_prior_transform_kernel(const double* __restrict__ z, int64_t n_chain, PriorTable t,
                                                                 PriorOutputs out, double* __restrict__ log_prior) {
  const int64_t d = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (d >= n_chain) return;
  log_prior[d] = pri::chain_fwd(t.b, t.n_block, z + d * t.n_free, out.p, d);
}

__global__ __launch_bounds__(64) void exo_prior_transform_vjp_kernel(const double* __restrict__ z, int64_t n_chain, PriorTable t,
                                                                     PriorCotangents gout, const double* __restrict__ glog_prior,
                                                                     double* __restrict__ gz) {
  const int64_t d = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (d >= n_chain) return;
  pri::chain_vjp(t.b, t.n_block, t.n_free, z + d * t.n_free, gout.p, glog_prior ? glog_prior[d] : 0.0, d, gz + d * t.n_free);
}

// the checks the two entry points share; fills `t`; returns the number of outputs, or -1
int prepare(const double* z, int64_t n_chain, int32_t n_free, const exo_prior_block* table, int32_t n_block, PriorTable* t) {
  if (n_chain < 0) return -1;
  const int n_outputs = pri::check_table(table, n_block, n_free);
  if (n_outputs < 0 || (n_chain > 0 && !z)) return -1;
  for (int k = 0; k < n_block; ++k) t->b[k] = table[k];
  t->n_block = n_block;
  t->n_free = n_free;
  return n_outputs;
}

}  // namespace

extern "C" {

int exo_prior_transform_f64(const double* z, int64_t n_chain, int32_t n_free, const exo_prior_block* table, int32_t n_block,
                            double* const* theta, double* log_prior, void* stream) {
  PriorTable t{};
  const int n_outputs = prepare(z, n_chain, n_free, table, n_block, &t);
  if (n_outputs < 0) return EXO_ERR_INVALID_ARGUMENT;
  if (n_chain == 0) return EXO_OK;
  if (!theta || !log_prior) return EXO_ERR_INVALID_ARGUMENT;
  PriorOutputs out{};
  for (int k = 0; k < n_block; ++k)
    for (int o = table[k].out; o < table[k].out + pri::n_out(table[k].kind); ++o) {
      if (!theta[o]) return EXO_ERR_INVALID_ARGUMENT;
      out.p[o] = theta[o];
    }
  hipLaunchKernelGGL(exo_prior_transform_kernel, dim3((unsigned)((n_chain + 63) / 64)), dim3(64), 0, (hipStream_t)stream, z, n_chain,
                     t, out, log_prior);
  return launch_status();
}

int exo_prior_transform_vjp_f64(const double* z, int64_t n_chain, int32_t n_free, const exo_prior_block* table, int32_t n_block,
                                const double* const* gtheta, const double* glog_prior, double* gz, void* stream) {
  PriorTable t{};
  const int n_outputs = prepare(z, n_chain, n_free, table, n_block, &t);
  if (n_outputs < 0) return EXO_ERR_INVALID_ARGUMENT;
  if (n_chain == 0) return EXO_OK;
  if (!gtheta || !gz) return EXO_ERR_INVALID_ARGUMENT;
  PriorCotangents gout{};
  for (int o = 0; o < n_outputs; ++o) gout.p[o] = gtheta[o];
  hipLaunchKernelGGL(exo_prior_transform_vjp_kernel, dim3((unsigned)((n_chain + 63) / 64)), dim3(64), 0, (hipStream_t)stream, z,
                     n_chain, t, gout, glog_prior, gz);
  return launch_status();
}

}  // extern "C"
