// rdamd_pair_sum_adjoints (include/root_digger_amd.h): the adjoints of the pair sums, on the host for
// any state count (pgrad::adjoints) or, for 20 states, on the matrix cores (kernels_block_exp.hip).
// Host pointers in and out; the device route owns its device memory, its stream and its events, as
// rdamd_rell_bootstrap does.
#include <cmath>
#include <vector>

#include "../../include/root_digger_amd.h"
#include "common.hpp"
#include "k20_block_exp.hpp"
#include "param_gradient.hpp"

namespace rdamd {
hipError_t launch_k20_block_exp(const double *q, const double *pair, const k20x_problem_t *problems, size_t n_problems,
                                double *adjoint, hipStream_t stream);
}

namespace {

thread_local double g_adjoints_ms = 0.0;

// A call's device allocations, its stream and its events: released on every way out.
template <class T> struct device_array_t {
  T *p = nullptr;
  device_array_t() = default;
  device_array_t(const device_array_t &) = delete;
  device_array_t &operator=(const device_array_t &) = delete;
  ~device_array_t() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t count) { return hipMalloc((void **)&p, count * sizeof(T)); }
  operator T *() const { return p; }
};
template <class T, hipError_t (*DESTROY)(T)> struct owned_t {
  T h = nullptr;
  owned_t() = default;
  owned_t(const owned_t &) = delete;
  owned_t &operator=(const owned_t &) = delete;
  ~owned_t() { if (h) (void)DESTROY(h); }
  operator T() const { return h; }
};
using stream_t = owned_t<hipStream_t, hipStreamDestroy>;
using event_t = owned_t<hipEvent_t, hipEventDestroy>;

bool device_present() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return n > 0;
}

// the 20-state device route: one copy of Q per rate-matrix set, one problem per (branch, rate)
int adjoints_on_device(unsigned R, unsigned sets, unsigned n_ops, const double *pair, const double *lengths,
                       const double *subst, const double *freqs, const unsigned *pidx, const double *rates,
                       double *adjoint_out) {
  using namespace rdamd;
  constexpr unsigned K = kBx20States;
  constexpr size_t n = (size_t)K * K, nsub = n - K;
  const size_t count = (size_t)n_ops * 2 * R;
  std::vector<double> raw(n), q(sets * n), xt(n);
  for (unsigned m = 0; m < sets; ++m) pgrad::build_q(K, subst + m * nsub, freqs + (size_t)m * K, raw.data(), q.data() + m * n);
  std::vector<k20x_problem_t> problems(count);
  for (size_t b = 0; b < (size_t)n_ops * 2; ++b)
    for (unsigned r = 0; r < R; ++r) {
      k20x_problem_t &pr = problems[b * R + r];
      pr.set = pidx[r];
      pr.rho_tau = rates[r] * lengths[b];
      const double *qm = q.data() + (size_t)pr.set * n;
      for (unsigned i = 0; i < K; ++i)
        for (unsigned j = 0; j < K; ++j) xt[i * K + j] = pr.rho_tau * qm[j * K + i];   // (rho tau Q)^T, as pgrad::adjoints forms it
      pgrad::block_scaling(K, xt.data(), &pr.squarings, &pr.scale);
    }
  stream_t stream;
  event_t t0, t1;
  device_array_t<double> d_q, d_pair, d_adjoint;
  device_array_t<k20x_problem_t> d_problems;
  RDAMD_HIP_TRY(hipStreamCreateWithFlags(&stream.h, hipStreamNonBlocking), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventCreate(&t0.h), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventCreate(&t1.h), RDAMD_FAILURE);
  RDAMD_HIP_TRY(d_q.alloc(sets * n), RDAMD_FAILURE);
  RDAMD_HIP_TRY(d_pair.alloc(count * n), RDAMD_FAILURE);
  RDAMD_HIP_TRY(d_adjoint.alloc(count * n), RDAMD_FAILURE);
  RDAMD_HIP_TRY(d_problems.alloc(count), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(d_q, q.data(), sets * n * sizeof(double), hipMemcpyHostToDevice), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(d_pair, pair, count * n * sizeof(double), hipMemcpyHostToDevice), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(d_problems, problems.data(), count * sizeof(k20x_problem_t), hipMemcpyHostToDevice),
                RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventRecord(t0, stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(launch_k20_block_exp(d_q, d_pair, d_problems, count, d_adjoint, stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipEventRecord(t1, stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipStreamSynchronize(stream), RDAMD_FAILURE);
  RDAMD_HIP_TRY(hipMemcpy(adjoint_out, d_adjoint, count * n * sizeof(double), hipMemcpyDeviceToHost), RDAMD_FAILURE);
  float ms = 0.0f;   // (a call that fails reports no time)
  if (hipEventElapsedTime(&ms, t0, t1) == hipSuccess) g_adjoints_ms = ms;
  return RDAMD_SUCCESS;
}

}  // namespace

extern "C" {

double rdamd_pair_sum_adjoints_last_ms(void) { return g_adjoints_ms; }

int rdamd_pair_sum_adjoints(unsigned int states, unsigned int rate_cats, unsigned int rate_matrices, unsigned int n_ops,
                            const double *pair, const double *lengths, const double *subst, const double *freqs,
                            const unsigned int *params_indices, const double *rates, int where, double *adjoint_out) {
  using rdamd::set_error;
  const char *who = "rdamd_pair_sum_adjoints";
  rdamd::clear_error();
  g_adjoints_ms = 0.0;
  const auto number_ok = [](double v) { return v >= 0.0 && std::isfinite(v); };
  bool ok = pair && lengths && subst && freqs && params_indices && rates && adjoint_out && states >= 2 && states <= 64 &&
            rate_cats > 0 && rate_matrices > 0 &&
            (where == RDAMD_ADJOINTS_AUTO || where == RDAMD_ADJOINTS_HOST || where == RDAMD_ADJOINTS_DEVICE);
  for (size_t b = 0; ok && b < (size_t)n_ops * 2; ++b) ok = number_ok(lengths[b]);
  for (unsigned r = 0; ok && r < rate_cats; ++r) ok = number_ok(rates[r]);
  if (!ok) {
    set_error(64, "%s: a null argument, %u states / %u rate categories / %u rate matrices out of range (2 .. 64 states, at "
                  "least one category and matrix), a branch length or category rate that is negative or not finite, or "
                  "an unknown route %d", who, states, rate_cats, rate_matrices, where);
    return RDAMD_FAILURE;
  }
  for (unsigned r = 0; r < rate_cats; ++r)
    if (params_indices[r] >= rate_matrices) {
      set_error(7, "%s: params index out of range", who);
      return RDAMD_FAILURE;
    }
  bool on_device = false;
  if (where == RDAMD_ADJOINTS_DEVICE) {
    if (states != rdamd::kBx20States) {
      set_error(63, "%s: the device route takes 20 states, not %u", who, states);
      return RDAMD_FAILURE;
    }
    if (!device_present()) {
      set_error(63, "%s: the device route was asked for and no device is present", who);
      return RDAMD_FAILURE;
    }
    on_device = true;
  } else if (where == RDAMD_ADJOINTS_AUTO) {
    on_device = states == rdamd::kBx20States && device_present();
  }
  if (n_ops == 0) return RDAMD_SUCCESS;
  if (on_device)
    return adjoints_on_device(rate_cats, rate_matrices, n_ops, pair, lengths, subst, freqs, params_indices, rates, adjoint_out);
  rdamd::pgrad::adjoints(states, rate_cats, rate_matrices, n_ops, pair, lengths, subst, freqs, params_indices, rates,
                         adjoint_out);
  return RDAMD_SUCCESS;
}

}  // extern "C"
