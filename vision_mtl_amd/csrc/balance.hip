// Task-loss balancing (opt-in): how the T <= 4 scalar task losses of one step become the loss that is differentiated,
// in place of the reference's two host floats (lit_module.py:120-131: loss = w_segm * loss_segm + w_depth * loss_depth).
//
//   vmtl_task_balance_fwd   total and weights_k = d total / d L_k of one of three schemes (VMTL_BALANCE_*)
//   vmtl_task_balance_bwd   g_k = grad_out * weights_k, and the gradient of the log-variances
//   vmtl_dwa_epoch_update   Dynamic Weight Average: the epoch's mean losses -> history -> next epoch's weights
//
// Everything is read by pointer - the losses, the parameters (log-variances or DWA weights), grad_out - so a launch
// captured into a hipGraph sees the values of the replay, not of the capture.  The work is a few dozen flops: each
// kernel is one wavefront whose lane 0 does plain C++ in fp64 and rounds once on the way out.  No atomics, no LDS.
//
// DWA state: VMTL_BALANCE_STATE_DOUBLES(T) = 3 T + 2 doubles
//   [0, T)          sum of L_k over the accumulated steps of the running epoch
//   [T]             number of accumulated steps        [T + 1]  number of completed (accepted) epochs
//   [T + 2, 2T + 2) prev:  mean losses of the last completed epoch
//   [2T + 2, 3T + 2) prev2: mean losses of the epoch before it
// The first T + 1 doubles are what a data-parallel run sum-reduces over its ranks before the epoch update.
#include "common.h"
#include "../../include/vmtl.h"

#define BAL_MAX_T 4
#define BAL_THREADS 64

struct BalLosses {
  const float* p[BAL_MAX_T];
};
struct BalGrads {
  float* p[BAL_MAX_T];
};

__global__ __launch_bounds__(BAL_THREADS) void task_balance_fwd_kernel(BalLosses losses, int T, int mode,
                                                                       const float* __restrict__ param,
                                                                       double* __restrict__ state, int accumulate,
                                                                       float* __restrict__ total,
                                                                       float* __restrict__ weights) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float L[BAL_MAX_T];
  for (int k = 0; k < T; ++k) L[k] = *losses.p[k];
  double sum = 0.0;
  if (mode == VMTL_BALANCE_UNCERTAINTY) {  // Kendall et al. 2018 with s = log sigma^2: sum_k exp(-s_k) L_k + s_k
    for (int k = 0; k < T; ++k) {
      const double s = (double)param[k];
      const float w = (float)exp(-s);
      weights[k] = w;
      sum += (double)w * (double)L[k] + s;
    }
    *total = (float)sum;
  } else if (mode == VMTL_BALANCE_DWA) {  // Liu et al. 2019: the weights are data of the epoch, not of the step
    bool finite = true;
    for (int k = 0; k < T; ++k) {
      const float w = param[k];
      weights[k] = w;
      sum += (double)w * (double)L[k];
      finite = finite && isfinite(L[k]);
    }
    *total = (float)sum;
    if (accumulate && finite) {  // one bad batch must not poison the epoch's means
      for (int k = 0; k < T; ++k) state[k] += (double)L[k];
      state[T] += 1.0;
    }
  } else {  // Chennupati et al. 2019: the geometric mean, exp(mean_k log L_k); defined for positive losses only
    bool positive = true;
    for (int k = 0; k < T; ++k) {
      positive = positive && L[k] > 0.f;
      sum += log((double)L[k]);
    }
    const double nan = __builtin_nan("");
    const double gm = positive ? exp(sum / T) : nan;
    *total = (float)gm;
    for (int k = 0; k < T; ++k) weights[k] = positive ? (float)(gm / ((double)T * (double)L[k])) : (float)nan;
  }
}

__global__ __launch_bounds__(BAL_THREADS) void task_balance_bwd_kernel(const float* __restrict__ grad_out,
                                                                       const float* __restrict__ weights,
                                                                       BalLosses losses, const float* __restrict__ param,
                                                                       int mode, int T, BalGrads grads,
                                                                       float* __restrict__ dparam) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float go = *grad_out;
  for (int k = 0; k < T; ++k) {
    const float w = weights[k];
    if (grads.p[k] != nullptr) *grads.p[k] = go * w;  // the arithmetic of vmtl_axpby's backward, bit for bit
    if (dparam != nullptr) {
      // d total / d s_k = 1 - exp(-s_k) L_k; the other two schemes have nothing to learn
      dparam[k] = mode == VMTL_BALANCE_UNCERTAINTY ? (float)((double)go * (1.0 - (double)w * (double)*losses.p[k])) : 0.f;
    }
  }
}

__global__ __launch_bounds__(BAL_THREADS) void dwa_epoch_update_kernel(double* __restrict__ state,
                                                                       float* __restrict__ param, int T,
                                                                       float temperature) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double* sum = state;
  double* prev = state + T + 2;
  double* prev2 = state + 2 * T + 2;
  const double steps = state[T];
  if (!(steps > 0.0)) return;  // an epoch without an accumulated step: nothing moves
  double mean[BAL_MAX_T], e[BAL_MAX_T];
  for (int k = 0; k < T; ++k) {
    mean[k] = sum[k] / steps;
    sum[k] = 0.0;
  }
  state[T] = 0.0;
  const double epochs = state[T + 1];
  if (epochs >= 1.0) {  // this epoch is at least the second: w_k = T softmax_k(r / tau), r_k = mean_k / prev_k
    double rmax = 0.0, den = 0.0;
    for (int k = 0; k < T; ++k) {
      const double r = mean[k] / prev[k];
      if (!(isfinite(r) && r > 0.0)) return;  // the epoch is dropped: weights and history stay, its sums are gone
      e[k] = r / (double)temperature;
      rmax = k == 0 || e[k] > rmax ? e[k] : rmax;
    }
    for (int k = 0; k < T; ++k) {
      e[k] = exp(e[k] - rmax);
      den += e[k];
    }
    for (int k = 0; k < T; ++k) param[k] = (float)((double)T * e[k] / den);
  } else {
    for (int k = 0; k < T; ++k) param[k] = 1.f;
  }
  for (int k = 0; k < T; ++k) {
    prev2[k] = prev[k];
    prev[k] = mean[k];
  }
  state[T + 1] = epochs + 1.0;
}

static inline bool bal_mode_ok(int mode) {
  return mode == VMTL_BALANCE_UNCERTAINTY || mode == VMTL_BALANCE_DWA || mode == VMTL_BALANCE_GEOMETRIC;
}

// the first T loss pointers must be there; the others are ignored
static inline bool bal_losses(BalLosses& out, const float* l0, const float* l1, const float* l2, const float* l3, int T) {
  const float* l[BAL_MAX_T] = {l0, l1, l2, l3};
  for (int k = 0; k < BAL_MAX_T; ++k) {
    out.p[k] = k < T ? l[k] : nullptr;
    if (k < T && !l[k]) return false;
  }
  return true;
}

extern "C" long long vmtl_task_balance_state_bytes(int T) {
  if (T < 1 || T > BAL_MAX_T) return 0;
  return (long long)sizeof(double) * (3 * T + 2);
}

extern "C" int vmtl_task_balance_fwd(const float* l0, const float* l1, const float* l2, const float* l3, int T, int mode,
                                     const float* param, void* state, int accumulate, float* total, float* weights,
                                     void* stream) {
  VMTL_ENTER();
  BalLosses losses;
  if (T < 1 || T > BAL_MAX_T || !bal_mode_ok(mode) || !bal_losses(losses, l0, l1, l2, l3, T)) return VMTL_ERR_ARG;
  if (!total || !weights || (mode != VMTL_BALANCE_GEOMETRIC && !param)) return VMTL_ERR_ARG;
  const bool acc = mode == VMTL_BALANCE_DWA && accumulate;
  if (acc && (!state || ((uintptr_t)state & 7))) return VMTL_ERR_ARG;
  hipLaunchKernelGGL(task_balance_fwd_kernel, dim3(1), dim3(BAL_THREADS), 0, (hipStream_t)stream, losses, T, mode, param,
                     (double*)state, acc ? 1 : 0, total, weights);
  return vmtl_check_launch();
}

extern "C" int vmtl_task_balance_bwd(const float* grad_out, const float* weights, const float* l0, const float* l1,
                                     const float* l2, const float* l3, const float* param, int mode, int T, float* g0,
                                     float* g1, float* g2, float* g3, float* dparam, void* stream) {
  VMTL_ENTER();
  BalLosses losses;
  if (T < 1 || T > BAL_MAX_T || !bal_mode_ok(mode) || !bal_losses(losses, l0, l1, l2, l3, T)) return VMTL_ERR_ARG;
  if (!grad_out || !weights || (mode != VMTL_BALANCE_GEOMETRIC && !param)) return VMTL_ERR_ARG;
  float* g[BAL_MAX_T] = {g0, g1, g2, g3};
  BalGrads grads;
  bool any = dparam != nullptr;
  for (int k = 0; k < BAL_MAX_T; ++k) {
    grads.p[k] = k < T ? g[k] : nullptr;
    any = any || grads.p[k] != nullptr;
  }
  if (!any) return VMTL_ERR_ARG;
  hipLaunchKernelGGL(task_balance_bwd_kernel, dim3(1), dim3(BAL_THREADS), 0, (hipStream_t)stream, grad_out, weights,
                     losses, param, mode, T, grads, dparam);
  return vmtl_check_launch();
}

extern "C" int vmtl_dwa_epoch_update(void* state, float* param, int T, float temperature, void* stream) {
  VMTL_ENTER();
  if (T < 1 || T > BAL_MAX_T || !state || ((uintptr_t)state & 7) || !param || !(temperature > 0.f))
    return VMTL_ERR_ARG;
  hipLaunchKernelGGL(dwa_epoch_update_kernel, dim3(1), dim3(BAL_THREADS), 0, (hipStream_t)stream, (double*)state, param,
                     T, temperature);
  return vmtl_check_launch();
}
