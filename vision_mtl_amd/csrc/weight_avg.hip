// An averaged copy of the flat parameter buffer (dp.ArenaAverage): exponential moving average (timm ModelEmaV2,
// torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn) and the equal average of SWA.
//
//   vmtl_wavg_control     state block: the weight of this update, copy / skip flags, the update counter (one workgroup)
//   vmtl_wavg_update      e[i] += w * (p[i] - e[i]), or e[i] = p[i] on the copy flag; p is read only
//   vmtl_adam_step_wavg   vmtl_adam_step_ex and vmtl_wavg_update in one pass: the freshly updated p goes into e
//   vmtl_wavg_buffers     the same update over a descriptor table of small buffers (BatchNorm running statistics)
//   vmtl_swap_            exchange two flat buffers in place, bit for bit
//   vmtl_swap_table_      the same exchange over the descriptor table
//
// Conventions are optim.hip's: 4-byte-aligned pointers, head and tail peeled and the body streamed as 16-byte vectors when
// all buffers share their offset inside a 16-byte line (a scalar fall-back otherwise), grids that are a function of n
// alone, grid-stride loops, no atomics.  Every element is owned by one thread, so the same inputs give the same bits.
//
// State block: VMTL_WAVG_STATE_FLOATS 4-byte words, 8-byte aligned, zeroed once by the caller
//   [0..1] n_averaged, a 64-bit integer (torch's AveragedModel keeps a long)   [2] w, the weight of this update (fp32)
//   [3] this update copies (0 / 1)   [4] this update is skipped (0 / 1)   [5] running count of skipped updates
//   [6..7] unused
// Everything that changes from update to update lives there, so a captured control + update pair advances by itself.
#include "optim.h"

#define VMTL_WAVG_STATE_FLOATS 8
#define VMTL_WAVG_EMA 0
#define VMTL_WAVG_SWA 1
#define WAVG_TABLE_THREADS 128
#define WAVG_TABLE_MAX_BLOCKS 64  // per record; the records are BatchNorm statistics, a few hundred floats each

struct WavgConsts {
  float w;
  bool copy;
};

__device__ __forceinline__ WavgConsts wavg_consts(const float* __restrict__ state) {
  WavgConsts c;
  c.w = state[2];
  c.copy = state[3] != 0.f;
  return c;
}

// one fused multiply-add: the same two roundings in every kernel of this file, whatever the compiler would contract
__device__ __forceinline__ float wavg_elem(float e, float p, const WavgConsts& c) {
  return c.copy ? p : __fmaf_rn(c.w, p - e, e);
}

// ------------------------------------------------------------------ control step
__global__ __launch_bounds__(64) void wavg_control_kernel(float* __restrict__ state, const float* __restrict__ ctl,
                                                          int mode, float decay, float decay_lo, int warmup) {
  if (threadIdx.x != 0) return;
  if (ctl && ctl[3] != 0.f) {  // the optimizer skipped its step: the counter stays and the average keeps its bits
    state[4] = 1.f;
    state[5] += 1.f;
    return;
  }
  long long* __restrict__ count = reinterpret_cast<long long*>(state);
  const long long n = count[0];
  double w = 1.0;  // n == 0: a copy, what AveragedModel does on its first update
  if (n > 0) {
    if (mode == VMTL_WAVG_SWA) {
      w = 1.0 / (double)(n + 1);
    } else {
      double d = (double)decay + (double)decay_lo;
      if (warmup) d = fmin(d, (1.0 + (double)n) / (10.0 + (double)n));  // timm's rule
      w = 1.0 - d;
    }
  }
  state[2] = (float)w;
  state[3] = n == 0 ? 1.f : 0.f;
  state[4] = 0.f;
  count[0] = n + 1;
}

extern "C" int vmtl_wavg_control(float* state, const float* ctl, int mode, float decay, float decay_lo, int warmup,
                                 void* stream) {
  VMTL_ENTER();
  if (!state || ((uintptr_t)state & 7) || ((uintptr_t)ctl & 3)) return VMTL_ERR_ARG;
  if (mode != VMTL_WAVG_EMA && mode != VMTL_WAVG_SWA) return VMTL_ERR_ARG;
  const double d = (double)decay + (double)decay_lo;
  if (mode == VMTL_WAVG_EMA && !(d >= 0.0 && d <= 1.0)) return VMTL_ERR_ARG;
  hipLaunchKernelGGL(wavg_control_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, ctl, mode, decay, decay_lo,
                     warmup);
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ stand-alone update
template <bool VEC>
__global__ __launch_bounds__(OPT_THREADS) void wavg_update_kernel(float* __restrict__ e, const float* __restrict__ p,
                                                                  const float* __restrict__ state, long long n) {
  if (state[4] != 0.f) return;  // skipped update: e keeps its bits
  const WavgConsts c = wavg_consts(state);
  if (VEC) {
    const int head = opt_head(e, n);  // the host checked that p shares e's offset in a 16-byte line
    const long long nvec = (n - head) >> 2;
    const int tail = (int)(n - head - (nvec << 2));
    f32x4* __restrict__ ev = reinterpret_cast<f32x4*>(e + head);
    const f32x4* __restrict__ pv = reinterpret_cast<const f32x4*>(p + head);
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < nvec;
         i += (long long)gridDim.x * OPT_THREADS) {
      const f32x4 p4 = pv[i];
      if (c.copy) {
        ev[i] = p4;
      } else {
        const f32x4 e4 = ev[i];
        ev[i] = (f32x4){wavg_elem(e4.x, p4.x, c), wavg_elem(e4.y, p4.y, c), wavg_elem(e4.z, p4.z, c),
                        wavg_elem(e4.w, p4.w, c)};
      }
    }
    if (blockIdx.x == 0) {
      const int t = threadIdx.x;
      long long j = -1;
      if (t < head)
        j = t;
      else if (t >= 64 && t - 64 < tail)
        j = head + (nvec << 2) + (t - 64);
      if (j >= 0) e[j] = wavg_elem(e[j], p[j], c);
    }
  } else {
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n;
         i += (long long)gridDim.x * OPT_THREADS)
      e[i] = wavg_elem(e[i], p[i], c);
  }
}

extern "C" int vmtl_wavg_update(float* e, const float* p, const float* state, long long n, void* stream) {
  VMTL_ENTER();
  if (!e || !p || !state || n <= 0) return VMTL_ERR_ARG;
  const uintptr_t a = (uintptr_t)e, b = (uintptr_t)p;
  if (((a | b) & 3) || ((uintptr_t)state & 7)) return VMTL_ERR_ARG;
  if (((a ^ b) & 15) == 0)
    hipLaunchKernelGGL(wavg_update_kernel<true>, dim3(opt_blocks(n)), dim3(OPT_THREADS), 0, (hipStream_t)stream, e, p,
                       state, n);
  else
    hipLaunchKernelGGL(wavg_update_kernel<false>, dim3(opt_blocks_scalar(n)), dim3(OPT_THREADS), 0, (hipStream_t)stream,
                       e, p, state, n);
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ Adam / AdamW update with the average in the same pass
// What vmtl_adam_step_ex followed by vmtl_wavg_update compute, element by element and bit for bit: each half honours its
// own skip flag (ctl[3] / state[4]; vmtl_wavg_control sets the second whenever it is given a control block with the first).
template <bool VEC>
__global__ __launch_bounds__(OPT_THREADS) void adam_wavg_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                float* __restrict__ m, float* __restrict__ v,
                                                                float* __restrict__ e, const float* __restrict__ ctl,
                                                                const float* __restrict__ state, float lr,
                                                                const float* __restrict__ lr_ptr, float eps, float wd,
                                                                int decoupled, float gscale, long long n) {
  const bool step = ctl[3] == 0.f, avg = state[4] == 0.f;
  if (!step && !avg) return;  // both skipped: p, m, v and e keep their bits
  if (lr_ptr) lr = lr_ptr[0];
  const AdamConsts c = adam_consts(ctl, lr, eps, wd, decoupled, gscale);
  const WavgConsts a = wavg_consts(state);
  if (VEC) {
    const int head = opt_head(p, n);  // the host checked that g, m, v and e share p's offset in a 16-byte line
    const long long nvec = (n - head) >> 2;
    const int tail = (int)(n - head - (nvec << 2));
    f32x4* __restrict__ pv = reinterpret_cast<f32x4*>(p + head);
    const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + head);
    f32x4* __restrict__ mv = reinterpret_cast<f32x4*>(m + head);
    f32x4* __restrict__ vv = reinterpret_cast<f32x4*>(v + head);
    f32x4* __restrict__ ev = reinterpret_cast<f32x4*>(e + head);
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < nvec;
         i += (long long)gridDim.x * OPT_THREADS) {
      const f32x4 p4 = pv[i];
      float pi[4] = {p4.x, p4.y, p4.z, p4.w};
      if (step) {
        const f32x4 g4 = gv[i], m4 = mv[i], v4 = vv[i];
        float mi[4] = {m4.x, m4.y, m4.z, m4.w}, vi[4] = {v4.x, v4.y, v4.z, v4.w};
        const float gi[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) adam_elem(pi[k], gi[k], mi[k], vi[k], c);
        mv[i] = (f32x4){mi[0], mi[1], mi[2], mi[3]};
        vv[i] = (f32x4){vi[0], vi[1], vi[2], vi[3]};
        pv[i] = (f32x4){pi[0], pi[1], pi[2], pi[3]};
      }
      if (avg) {
        if (a.copy) {
          ev[i] = (f32x4){pi[0], pi[1], pi[2], pi[3]};
        } else {
          const f32x4 e4 = ev[i];
          ev[i] = (f32x4){wavg_elem(e4.x, pi[0], a), wavg_elem(e4.y, pi[1], a), wavg_elem(e4.z, pi[2], a),
                          wavg_elem(e4.w, pi[3], a)};
        }
      }
    }
    if (blockIdx.x == 0) {
      const int t = threadIdx.x;
      long long j = -1;
      if (t < head)
        j = t;
      else if (t >= 64 && t - 64 < tail)
        j = head + (nvec << 2) + (t - 64);
      if (j >= 0) {
        float pi = p[j];
        if (step) {
          float mi = m[j], vi = v[j];
          adam_elem(pi, g[j], mi, vi, c);
          m[j] = mi;
          v[j] = vi;
          p[j] = pi;
        }
        if (avg) e[j] = wavg_elem(e[j], pi, a);
      }
    }
  } else {
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n;
         i += (long long)gridDim.x * OPT_THREADS) {
      float pi = p[i];
      if (step) {
        float mi = m[i], vi = v[i];
        adam_elem(pi, g[i], mi, vi, c);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
      }
      if (avg) e[i] = wavg_elem(e[i], pi, a);
    }
  }
}

extern "C" int vmtl_adam_step_wavg(float* p, const float* g, float* m, float* v, float* e, const float* ctl,
                                   const float* state, float lr, const float* lr_ptr, float eps, float weight_decay,
                                   int decoupled, float grad_scale, long long n, void* stream) {
  VMTL_ENTER();
  if (!p || !g || !m || !v || !e || !ctl || !state || n <= 0) return VMTL_ERR_ARG;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)g, c = (uintptr_t)m, d = (uintptr_t)v, f = (uintptr_t)e;
  if (((a | b | c | d | f) & 3) || ((uintptr_t)state & 7)) return VMTL_ERR_ARG;
  if ((((a ^ b) | (a ^ c) | (a ^ d) | (a ^ f)) & 15) == 0)
    hipLaunchKernelGGL(adam_wavg_kernel<true>, dim3(opt_blocks(n)), dim3(OPT_THREADS), 0, (hipStream_t)stream, p, g, m,
                       v, e, ctl, state, lr, lr_ptr, eps, weight_decay, decoupled, grad_scale, n);
  else
    hipLaunchKernelGGL(adam_wavg_kernel<false>, dim3(opt_blocks_scalar(n)), dim3(OPT_THREADS), 0, (hipStream_t)stream, p,
                       g, m, v, e, ctl, state, lr, lr_ptr, eps, weight_decay, decoupled, grad_scale, n);
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ descriptor table of small buffers
struct WavgDesc {
  float* src;  // the live buffer: read by vmtl_wavg_buffers, exchanged by vmtl_swap_table_
  float* avg;
  long long n;
};

static inline int wavg_table_blocks(long long max_n) {
  return grid_1d(max_n, WAVG_TABLE_THREADS, WAVG_TABLE_MAX_BLOCKS);
}

__global__ __launch_bounds__(WAVG_TABLE_THREADS) void wavg_buffers_kernel(const WavgDesc* __restrict__ descs,
                                                                          const float* __restrict__ state) {
  if (state[4] != 0.f) return;
  const WavgConsts c = wavg_consts(state);
  const WavgDesc d = descs[blockIdx.y];
  VMTL_GRID_STRIDE(i, d.n) d.avg[i] = wavg_elem(d.avg[i], d.src[i], c);
}

__global__ __launch_bounds__(WAVG_TABLE_THREADS) void swap_table_kernel(const WavgDesc* __restrict__ descs) {
  const WavgDesc d = descs[blockIdx.y];
  unsigned* a = reinterpret_cast<unsigned*>(d.src);
  unsigned* b = reinterpret_cast<unsigned*>(d.avg);
  VMTL_GRID_STRIDE(i, d.n) {
    const unsigned x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
}

extern "C" int vmtl_wavg_desc_bytes(void) { return (int)sizeof(WavgDesc); }

// descs: device array of n WavgDesc records (vmtl_wavg_desc_bytes() each, validated by the host that wrote them: non-null
// 4-byte-aligned pointers to disjoint buffers of 0 < n <= max_n elements); max_n sizes the grid.
static int wavg_table_args(const void* descs, int n, long long max_n) {
  return (!descs || ((uintptr_t)descs & 7) || n <= 0 || n > 65535 || max_n <= 0) ? VMTL_ERR_ARG : VMTL_OK;
}

extern "C" int vmtl_wavg_buffers(const void* descs, int n, long long max_n, const float* state, void* stream) {
  VMTL_ENTER();
  if (wavg_table_args(descs, n, max_n) != VMTL_OK || !state || ((uintptr_t)state & 7)) return VMTL_ERR_ARG;
  hipLaunchKernelGGL(wavg_buffers_kernel, dim3(wavg_table_blocks(max_n), n), dim3(WAVG_TABLE_THREADS), 0,
                     (hipStream_t)stream, (const WavgDesc*)descs, state);
  return vmtl_check_launch();
}

extern "C" int vmtl_swap_table_(const void* descs, int n, long long max_n, void* stream) {
  VMTL_ENTER();
  if (wavg_table_args(descs, n, max_n) != VMTL_OK) return VMTL_ERR_ARG;
  hipLaunchKernelGGL(swap_table_kernel, dim3(wavg_table_blocks(max_n), n), dim3(WAVG_TABLE_THREADS), 0,
                     (hipStream_t)stream, (const WavgDesc*)descs);
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ in-place exchange
// The words travel as integers: no arithmetic touches them, so NaN payloads and signed zeros survive.
template <bool VEC>
__global__ __launch_bounds__(OPT_THREADS) void swap_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b,
                                                           long long n) {
  if (VEC) {
    const int head = opt_head(a, n);  // the host checked that b shares a's offset in a 16-byte line
    const long long nvec = (n - head) >> 2;
    const int tail = (int)(n - head - (nvec << 2));
    u32x4* __restrict__ av = reinterpret_cast<u32x4*>(a + head);
    u32x4* __restrict__ bv = reinterpret_cast<u32x4*>(b + head);
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < nvec;
         i += (long long)gridDim.x * OPT_THREADS) {
      const u32x4 x = av[i], y = bv[i];
      av[i] = y;
      bv[i] = x;
    }
    if (blockIdx.x == 0) {
      const int t = threadIdx.x;
      long long j = -1;
      if (t < head)
        j = t;
      else if (t >= 64 && t - 64 < tail)
        j = head + (nvec << 2) + (t - 64);
      if (j >= 0) {
        const unsigned x = a[j], y = b[j];
        a[j] = y;
        b[j] = x;
      }
    }
  } else {
    for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n;
         i += (long long)gridDim.x * OPT_THREADS) {
      const unsigned x = a[i], y = b[i];
      a[i] = y;
      b[i] = x;
    }
  }
}

extern "C" int vmtl_swap_(float* a, float* b, long long n, void* stream) {
  VMTL_ENTER();
  if (!a || !b || n <= 0) return VMTL_ERR_ARG;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  if ((x | y) & 3) return VMTL_ERR_ARG;
  const uintptr_t bytes = (uintptr_t)n * 4, lo = x < y ? x : y, hi = x < y ? y : x;
  if (hi - lo < bytes) return VMTL_ERR_ARG;  // the two ranges overlap (a == b included)
  if (((x ^ y) & 15) == 0)
    hipLaunchKernelGGL(swap_kernel<true>, dim3(opt_blocks(n)), dim3(OPT_THREADS), 0, (hipStream_t)stream, (unsigned*)a,
                       (unsigned*)b, n);
  else
    hipLaunchKernelGGL(swap_kernel<false>, dim3(opt_blocks_scalar(n)), dim3(OPT_THREADS), 0, (hipStream_t)stream,
                       (unsigned*)a, (unsigned*)b, n);
  return vmtl_check_launch();
}
