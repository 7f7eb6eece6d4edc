// rdamd_substitution_counts_from_pair_sums and rdamd_substitution_counts_from_adjoints
// (include/root_digger_amd.h): the C entries of subst_map.hpp.
#include "../../include/root_digger_amd.h"
#include "common.hpp"
#include "subst_map.hpp"

extern "C" int rdamd_substitution_counts_from_pair_sums(unsigned int states, unsigned int rate_cats, unsigned int rate_matrices,
                                                        unsigned int n_ops, const double *pair, const double *lengths,
                                                        const double *subst, const double *freqs,
                                                        const unsigned int *params_indices, const double *rates,
                                                        double *typed_out) {
  rdamd::clear_error();
  const int e = rdamd::smap::counts_from_pair_sums(states, rate_cats, rate_matrices, n_ops, pair, lengths, subst, freqs,
                                                   params_indices, rates, typed_out);
  if (e == 64)
    rdamd::set_error(64, "rdamd_substitution_counts_from_pair_sums: a null argument, %u states / %u rate categories / %u rate "
                         "matrices out of range (2 .. 64 states, at least one category and matrix), or a branch length that "
                         "is negative or not finite", states, rate_cats, rate_matrices);
  else if (e == 7)
    rdamd::set_error(7, "rdamd_substitution_counts_from_pair_sums: params index out of range");
  return e == 0 ? RDAMD_SUCCESS : RDAMD_FAILURE;
}

extern "C" int rdamd_substitution_counts_from_adjoints(unsigned int states, unsigned int rate_cats, unsigned int rate_matrices,
                                                       unsigned int n_ops, const double *adjoint, const double *lengths,
                                                       const double *subst, const double *freqs,
                                                       const unsigned int *params_indices, const double *rates,
                                                       double *typed_out) {
  rdamd::clear_error();
  const int e = rdamd::smap::counts_from_adjoints(states, rate_cats, rate_matrices, n_ops, adjoint, lengths, subst, freqs,
                                                  params_indices, rates, typed_out);
  if (e == 64)
    rdamd::set_error(64, "rdamd_substitution_counts_from_adjoints: a null argument, %u states / %u rate categories / %u rate "
                         "matrices out of range (2 .. 64 states, at least one category and matrix), or a branch length that "
                         "is negative or not finite", states, rate_cats, rate_matrices);
  else if (e == 7)
    rdamd::set_error(7, "rdamd_substitution_counts_from_adjoints: params index out of range");
  return e == 0 ? RDAMD_SUCCESS : RDAMD_FAILURE;
}
