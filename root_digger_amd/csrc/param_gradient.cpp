// rdamd_gradient_from_pair_sums and rdamd_gradient_from_adjoints (include/root_digger_amd.h): the C
// entries of param_gradient.hpp.
#include "../../include/root_digger_amd.h"
#include "common.hpp"
#include "param_gradient.hpp"

extern "C" int rdamd_gradient_from_pair_sums(unsigned int states, unsigned int rate_cats, unsigned int rate_matrices,
                                             unsigned int n_ops, const double *pair, const double *root, const double *cat,
                                             const double *lengths, const double *subst, const double *freqs,
                                             const unsigned int *params_indices, const unsigned int *freqs_indices,
                                             const double *rates, const double *weights, double *d_subst, double *d_freqs,
                                             double *d_rates, double *d_weights) {
  rdamd::clear_error();
  const int e = rdamd::pgrad::gradient_from_pair_sums(states, rate_cats, rate_matrices, n_ops, pair, root, cat, lengths, subst,
                                                      freqs, params_indices, freqs_indices, rates, weights, d_subst, d_freqs,
                                                      d_rates, d_weights);
  if (e == 64)
    rdamd::set_error(64, "rdamd_gradient_from_pair_sums: a null input, or %u states / %u rate categories / %u rate matrices "
                         "out of range (2 .. 64 states, at least one category and matrix)", states, rate_cats, rate_matrices);
  else if (e == 7)
    rdamd::set_error(7, "rdamd_gradient_from_pair_sums: params or freqs index out of range");
  return e == 0 ? RDAMD_SUCCESS : RDAMD_FAILURE;
}

extern "C" int rdamd_gradient_from_adjoints(unsigned int states, unsigned int rate_cats, unsigned int rate_matrices,
                                            unsigned int n_ops, const double *adjoint, const double *root, const double *cat,
                                            const double *lengths, const double *subst, const double *freqs,
                                            const unsigned int *params_indices, const unsigned int *freqs_indices,
                                            const double *rates, const double *weights, double *d_subst, double *d_freqs,
                                            double *d_rates, double *d_weights) {
  rdamd::clear_error();
  const int e = rdamd::pgrad::gradient_from_adjoints(states, rate_cats, rate_matrices, n_ops, adjoint, root, cat, lengths,
                                                     subst, freqs, params_indices, freqs_indices, rates, weights, d_subst,
                                                     d_freqs, d_rates, d_weights);
  if (e == 64)
    rdamd::set_error(64, "rdamd_gradient_from_adjoints: a null input, or %u states / %u rate categories / %u rate matrices "
                         "out of range (2 .. 64 states, at least one category and matrix)", states, rate_cats, rate_matrices);
  else if (e == 7)
    rdamd::set_error(7, "rdamd_gradient_from_adjoints: params or freqs index out of range");
  return e == 0 ? RDAMD_SUCCESS : RDAMD_FAILURE;
}
