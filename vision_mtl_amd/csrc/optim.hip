// Global-norm gradient clipping and the extended fused Adam / AdamW update over flat fp32 buffers
// (dp.FlatArena: flat_param, flat_grad and the two moment buffers).
//
//   vmtl_grad_sumsq      sum over i of (g[i] * grad_scale)^2 as per-workgroup fp64 partials in a caller workspace
//   vmtl_optim_control   partials -> control block (norm, clip coefficient, non-finite / skip flags, bias corrections)
//                        and the step counter, incremented on the device unless the step is skipped
//   vmtl_adam_step_ex    torch.optim.Adam / AdamW arithmetic driven by the control block; g is read only
//   vmtl_grad_clip_      g *= grad_scale * clip coefficient in place (every workgroup re-derives the coefficient from
//                        the partials, so norm + clip are two launches)
//
// Determinism: the grid of vmtl_grad_sumsq is a function of n alone, every thread adds its elements in a fixed order,
// block_sum (reduce.h) combines the threads of a workgroup in a fixed order and partials_sum below combines the
// workgroups in a fixed order.  No atomics anywhere: the same g at the same address gives the same bits on every run.
//
// Pointers need 4-byte alignment only.  A kernel peels the elements in front of the first 16-byte boundary (at most 3) and
// behind the last one (at most 3) and streams the body as float4; the update does so when p, g, m and v share their
// offset inside a 16-byte line (slices of one arena layout do) and falls back to scalar accesses otherwise.
//
// Control block: VMTL_OPTIM_CTL_FLOATS floats
//   [0] total norm of g * grad_scale (NaN: no norm was computed)   [1] clip coefficient   [2] norm is not finite (0 / 1)
//   [3] this step is skipped (0 / 1)   [4] running count of skipped steps   [5] 1 / (1 - b1^step)
//   [6] 1 / sqrt(1 - b2^step)   [7] b1   [8] 1 - b1   [9] b2   [10] 1 - b2   [11..15] unused
// The betas arrive as a float pair (hi + lo): the C ABI carries no double, and 1 - b2 taken from the fp32 0.999 alone is off
// by 3e-5 of its value - that much of every second-moment increment.
#include "optim.h"
#include "reduce.h"

// fixed-order fp64 sum of the nparts partials; every thread of the 256-thread workgroup returns the total
__device__ __forceinline__ double partials_sum(const double* __restrict__ partials, int nparts, double* sh) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += OPT_THREADS) s += partials[i];
  return block_sum(s, sh);
}

// torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0) in fp32; a NaN stays a NaN
__device__ __forceinline__ float clip_coef(float norm, float max_norm) {
  if (!(max_norm > 0.f)) return 1.f;
  const float c = max_norm / (norm + 1e-6f);
  return c < 1.f ? c : (c != c ? c : 1.f);
}

// ------------------------------------------------------------------ sum of squares
__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, float gscale,
                                                                 long long n, double* __restrict__ partials) {
  __shared__ double sh[4];
  const int head = opt_head(g, n);
  const long long nvec = (n - head) >> 2;
  const int tail = (int)(n - head - (nvec << 2));
  const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + head);
  const double sc = (double)gscale;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < nvec;
       i += (long long)gridDim.x * OPT_THREADS) {
    const f32x4 x = gv[i];
    const double a = (double)x.x * sc, b = (double)x.y * sc, c = (double)x.z * sc, d = (double)x.w * sc;
    acc += a * a;
    acc += b * b;
    acc += c * c;
    acc += d * d;
  }
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    if (t < head) {
      const double a = (double)g[t] * sc;
      acc += a * a;
    } else if (t >= 64 && t - 64 < tail) {
      const double a = (double)g[head + (nvec << 2) + (t - 64)] * sc;
      acc += a * a;
    }
  }
  const double s = block_sum(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

extern "C" long long vmtl_grad_sumsq_workspace_bytes(long long n) {
  return (long long)opt_blocks(n) * (long long)sizeof(double);
}

extern "C" int vmtl_grad_sumsq(const float* g, float grad_scale, void* workspace, long long n, void* stream) {
  VMTL_ENTER();
  if (!g || !workspace || n <= 0 || ((uintptr_t)g & 3) || ((uintptr_t)workspace & 7)) return VMTL_ERR_ARG;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(opt_blocks(n)), dim3(OPT_THREADS), 0, (hipStream_t)stream, g, grad_scale,
                     n, (double*)workspace);
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ control step
__global__ __launch_bounds__(OPT_THREADS) void optim_control_kernel(const double* __restrict__ partials, int nparts,
                                                                    float max_norm, int skip_nonfinite,
                                                                    float* __restrict__ step_ptr, float b1, float b1_lo,
                                                                    float b2, float b2_lo, float* __restrict__ ctl) {
  __shared__ double sh[4];
  const double ss = nparts > 0 ? partials_sum(partials, nparts, sh) : 0.0;
  if (threadIdx.x != 0) return;
  const float norm = nparts > 0 ? (float)sqrt(ss) : __builtin_nanf("");
  const bool nonfinite = nparts > 0 && !(fabsf(norm) <= 3.402823466e38f);
  const bool skip = skip_nonfinite != 0 && nonfinite;
  ctl[0] = norm;
  ctl[1] = nparts > 0 ? clip_coef(norm, max_norm) : 1.f;
  ctl[2] = nonfinite ? 1.f : 0.f;
  ctl[3] = skip ? 1.f : 0.f;
  const double d1 = (double)b1 + (double)b1_lo, d2 = (double)b2 + (double)b2_lo;
  ctl[7] = (float)d1;
  ctl[8] = (float)(1.0 - d1);
  ctl[9] = (float)d2;
  ctl[10] = (float)(1.0 - d2);
  if (skip) {
    ctl[4] += 1.f;
    return;
  }
  const float step = step_ptr[0] + 1.f;
  step_ptr[0] = step;
  ctl[5] = (float)(1.0 / (1.0 - pow(d1, (double)step)));
  ctl[6] = (float)(1.0 / sqrt(1.0 - pow(d2, (double)step)));
}

extern "C" int vmtl_optim_control(const void* workspace, long long n, float max_norm, int skip_nonfinite,
                                  float* step_ptr, float b1, float b1_lo, float b2, float b2_lo, float* ctl,
                                  void* stream) {
  VMTL_ENTER();
  // n: the element count vmtl_grad_sumsq filled `workspace` for; 0 (workspace may be null): no norm - then nothing can
  // be clipped or found non-finite
  if (!step_ptr || !ctl || n < 0 || (n > 0 && (!workspace || ((uintptr_t)workspace & 7)))) return VMTL_ERR_ARG;
  if (n == 0 && (max_norm > 0.f || skip_nonfinite)) return VMTL_ERR_ARG;
  if (!(max_norm >= 0.f)) return VMTL_ERR_ARG;
  hipLaunchKernelGGL(optim_control_kernel, dim3(1), dim3(OPT_THREADS), 0, (hipStream_t)stream,
                     (const double*)workspace, n > 0 ? opt_blocks(n) : 0, max_norm, skip_nonfinite, step_ptr, b1, b1_lo,
                     b2, b2_lo, ctl);
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ fused update
// AdamConsts / adam_consts / adam_elem: optim.h (weight_avg.hip runs the same element update)
template <bool VEC>
__global__ __launch_bounds__(OPT_THREADS) void adam_ex_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                              float* __restrict__ m, float* __restrict__ v,
                                                              const float* __restrict__ ctl, float lr,
                                                              const float* __restrict__ lr_ptr, float eps, float wd,
                                                              int decoupled, float gscale, long long n) {
  if (ctl[3] != 0.f) return;  // skipped step: p, m and v keep their bits
  if (lr_ptr) lr = lr_ptr[0];
  const AdamConsts c = adam_consts(ctl, lr, eps, wd, decoupled, gscale);
  if (VEC) {
    const int head = opt_head(p, n);  // the host checked that g, m and v share p's offset in a 16-byte line
    const long long nvec = (n - head) >> 2;
    const int tail = (int)(n - head - (nvec << 2));
    f32x4* __restrict__ pv = reinterpret_cast<f32x4*>(p + head);
    const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + head);
    f32x4* __restrict__ mv = reinterpret_cast<f32x4*>(m + head);
    f32x4* __restrict__ vv = reinterpret_cast<f32x4*>(v + head);
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < nvec;
         i += (long long)gridDim.x * OPT_THREADS) {
      const f32x4 p4 = pv[i], g4 = gv[i], m4 = mv[i], v4 = vv[i];
      float pi[4] = {p4.x, p4.y, p4.z, p4.w}, mi[4] = {m4.x, m4.y, m4.z, m4.w}, vi[4] = {v4.x, v4.y, v4.z, v4.w};
      const float gi[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) adam_elem(pi[k], gi[k], mi[k], vi[k], c);
      mv[i] = (f32x4){mi[0], mi[1], mi[2], mi[3]};
      vv[i] = (f32x4){vi[0], vi[1], vi[2], vi[3]};
      pv[i] = (f32x4){pi[0], pi[1], pi[2], pi[3]};
    }
    if (blockIdx.x == 0) {
      const int t = threadIdx.x;
      long long j = -1;
      if (t < head)
        j = t;
      else if (t >= 64 && t - 64 < tail)
        j = head + (nvec << 2) + (t - 64);
      if (j >= 0) {
        float pi = p[j], mi = m[j], vi = v[j];
        adam_elem(pi, g[j], mi, vi, c);
        m[j] = mi;
        v[j] = vi;
        p[j] = pi;
      }
    }
  } else {
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n;
         i += (long long)gridDim.x * OPT_THREADS) {
      float pi = p[i], mi = m[i], vi = v[i];
      adam_elem(pi, g[i], mi, vi, c);
      m[i] = mi;
      v[i] = vi;
      p[i] = pi;
    }
  }
}

extern "C" int vmtl_adam_step_ex(float* p, const float* g, float* m, float* v, const float* ctl, float lr,
                                 const float* lr_ptr, float eps, float weight_decay, int decoupled, float grad_scale,
                                 long long n, void* stream) {
  VMTL_ENTER();
  if (!p || !g || !m || !v || !ctl || n <= 0) return VMTL_ERR_ARG;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)g, c = (uintptr_t)m, d = (uintptr_t)v;
  if ((a | b | c | d) & 3) return VMTL_ERR_ARG;
  if ((((a ^ b) | (a ^ c) | (a ^ d)) & 15) == 0) {
    hipLaunchKernelGGL(adam_ex_kernel<true>, dim3(opt_blocks(n)), dim3(OPT_THREADS), 0, (hipStream_t)stream, p, g, m,
                       v, ctl, lr, lr_ptr, eps, weight_decay, decoupled, grad_scale, n);
  } else {
    const int nb = opt_blocks_scalar(n);
    hipLaunchKernelGGL(adam_ex_kernel<false>, dim3(nb), dim3(OPT_THREADS), 0, (hipStream_t)stream, p, g, m, v,
                       ctl, lr, lr_ptr, eps, weight_decay, decoupled, grad_scale, n);
  }
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ in-place clip
__global__ __launch_bounds__(OPT_THREADS) void grad_clip_kernel(float* __restrict__ g,
                                                                const double* __restrict__ partials, int nparts,
                                                                float gscale, float max_norm, float* __restrict__ ctl,
                                                                long long n) {
  __shared__ double sh[4];
  const float norm = (float)sqrt(partials_sum(partials, nparts, sh));  // the same bits in every workgroup
  const float coef = clip_coef(norm, max_norm);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctl[0] = norm;
    ctl[1] = coef;
    ctl[2] = fabsf(norm) <= 3.402823466e38f ? 0.f : 1.f;
  }
  if (gscale == 1.f && coef == 1.f) return;  // nothing to clip: spare the read and the write of g
  const int head = opt_head(g, n);
  const long long nvec = (n - head) >> 2;
  const int tail = (int)(n - head - (nvec << 2));
  f32x4* __restrict__ gv = reinterpret_cast<f32x4*>(g + head);
  for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < nvec;
       i += (long long)gridDim.x * OPT_THREADS)
    gv[i] = gv[i] * gscale * coef;
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    if (t < head)
      g[t] = g[t] * gscale * coef;
    else if (t >= 64 && t - 64 < tail) {
      const long long j = head + (nvec << 2) + (t - 64);
      g[j] = g[j] * gscale * coef;
    }
  }
}

extern "C" int vmtl_grad_clip_(float* g, const void* workspace, float grad_scale, float max_norm, float* ctl,
                               long long n, void* stream) {
  VMTL_ENTER();
  if (!g || !workspace || !ctl || n <= 0 || ((uintptr_t)g & 3) || ((uintptr_t)workspace & 7)) return VMTL_ERR_ARG;
  if (!(max_norm >= 0.f)) return VMTL_ERR_ARG;
  hipLaunchKernelGGL(grad_clip_kernel, dim3(opt_blocks(n)), dim3(OPT_THREADS), 0, (hipStream_t)stream, g,
                     (const double*)workspace, opt_blocks(n), grad_scale, max_norm, ctl, n);
  return vmtl_check_launch();
}
