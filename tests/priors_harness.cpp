// Host build of exoplanet_amd/csrc/exo_priors_core.hpp: the loop over chains that the kernels of exo_priors.hip spread over
// lanes, with the same table, pointer lists and argument checks (tests/test_distributions_host.py).
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_priors_core.hpp"

extern "C" {

int harness_prior_transform(const double* z, int64_t n_chain, int32_t n_free, const exo_prior_block* table, int32_t n_block,
                            double* const* theta, double* log_prior) {
  if (pri::check_table(table, n_block, n_free) < 0) return EXO_ERR_INVALID_ARGUMENT;
  for (int64_t d = 0; d < n_chain; ++d) log_prior[d] = pri::chain_fwd(table, n_block, z + d * n_free, theta, d);
  return EXO_OK;
}

int harness_prior_transform_vjp(const double* z, int64_t n_chain, int32_t n_free, const exo_prior_block* table, int32_t n_block,
                                const double* const* gtheta, const double* glog_prior, double* gz) {
  if (pri::check_table(table, n_block, n_free) < 0) return EXO_ERR_INVALID_ARGUMENT;
  for (int64_t d = 0; d < n_chain; ++d)
    pri::chain_vjp(table, n_block, n_free, z + d * n_free, gtheta, glog_prior ? glog_prior[d] : 0.0, d, gz + d * n_free);
  return EXO_OK;
}

double harness_digamma(double x) { return pri::digamma(x); }

}  // extern "C"
