// What the flat-buffer passes of optim.hip and weight_avg.hip share: the launch shape, the head / tail peeling of a
// 4-byte-aligned pointer and the Adam element update, stated once so that both files compute the same bits.
#pragma once
#include "common.h"

#define OPT_THREADS 256
#define OPT_MAX_BLOCKS 1024  // 4 workgroups per CU: 64 KiB of 16-byte loads in flight per CU in the four-stream update
#define VMTL_OPTIM_CTL_FLOATS 16

static inline int opt_blocks(long long n) {  // float4 per thread and trip; a function of n alone (see Determinism)
  return grid_1d(n, 4 * OPT_THREADS, OPT_MAX_BLOCKS);
}

// blocks of the scalar fall-back (buffers at different offsets inside a 16-byte line): one element per thread and trip
static inline int opt_blocks_scalar(long long n) { return grid_1d(n, OPT_THREADS, 4 * OPT_MAX_BLOCKS); }

// elements in front of the first 16-byte boundary of a 4-byte-aligned pointer, at most n
__host__ __device__ static inline int opt_head(const void* ptr, long long n) {
  const int h = (int)((16 - ((uintptr_t)ptr & 15)) & 15) >> 2;
  return (long long)h < n ? h : (int)n;
}

struct AdamConsts {
  float gscale, coef, b1, omb1, b2, omb2, step_size, inv_sqrt_bc2, eps, wd, decay;
  int decoupled;
};

// the constants of one extended update from the control block (optim.hip lists its fields) and the launch arguments
__device__ __forceinline__ AdamConsts adam_consts(const float* __restrict__ ctl, float lr, float eps, float wd,
                                                  int decoupled, float gscale) {
  AdamConsts c;
  c.gscale = gscale;
  c.coef = ctl[1];
  c.b1 = ctl[7];
  c.omb1 = ctl[8];
  c.b2 = ctl[9];
  c.omb2 = ctl[10];
  c.step_size = lr * ctl[5];
  c.inv_sqrt_bc2 = ctl[6];
  c.eps = eps;
  c.wd = wd;
  c.decoupled = decoupled;
  c.decay = (float)(1.0 - (double)lr * (double)wd);
  return c;
}

// torch/optim/adam.py _single_tensor_adam, element by element
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamConsts& c) {
  float gi = g * c.gscale * c.coef;
  if (c.decoupled)
    p *= c.decay;
  else if (c.wd != 0.f)
    gi += c.wd * p;
  m = c.b1 * m + c.omb1 * gi;
  v = c.b2 * v + c.omb2 * gi * gi;
  const float denom = sqrtf(v) * c.inv_sqrt_bc2 + c.eps;
  p -= c.step_size * (m / denom);
}
