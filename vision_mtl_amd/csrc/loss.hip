// Per-pixel losses of the multi-task step, forward and backward.
//
//   cross entropy : torch.nn.CrossEntropyLoss() as used at reference lit_module.py:31,123
//                   (mean over B*H*W); the *_ex entry points add torch's `weight` and `ignore_index`:
//                   sum_valid w[t] nll / sum_valid w[t], valid = (t != ignore_index).  No smoothing.
//   SILog         : reference vision_mtl/losses.py:14-36 on already-sigmoided predictions
//                   (mask = target > min_depth, or the caller's uint8 mask in the *_mask entry points;
//                   unbiased variance, 10*sqrt(var + 0.15*mean^2))
//   L1 / MAE      : the depth metric of reference lit_module.py:68,112 (mean |p - t|)
//
// Reductions are two-stage: per-workgroup partials in fp64, summed in a fixed order by a
// single finalize workgroup, so results are run-to-run reproducible.
//
// Every cross-entropy kernel is written once as a template over `bool EX` and compiled twice.  EX = false is the plain
// mean over all pixels; EX = true takes the operands of CeEx<true>: class weights, an ignore index and, in the backward,
// the denominator the forward left on the device.  What the two variants do differently is stated once, in the ce_*<EX>
// helpers in front of the kernels; everything else - thread-to-pixel maps, strides, launch shapes, the log-softmax - is
// the one kernel body.  The plain instantiations compile to the instruction sequence a kernel without the parameter
// compiles to, so the default step pays nothing for the variant.  The SILog kernels take their
// validity test (target > min_depth, or the caller's mask) as a functor in the same way.
//
// These kernels spell the pixel pass and the three gradient layouts themselves instead of taking them from ce_pixel.h,
// as the OHEM and region criteria do: built from the header's inlined pieces, the plain instantiations hold the same
// operations but come out in another block and scheduling order, 1 - 2 % slower on the default step's path (DESIGN.md
// section 16d).  What is shared with the header is what does not touch their code: the NaN constant, the rule for
// labels, the layout decision, the Q dispatch and the block count.  A change to the rows kernel's tail or to the
// label rule is made here and in ce_pixel.h.
//
// The weighted / ignoring cross entropy divides by a sum that depends on the targets.  Its forward reduces
// (numerator, denominator) pairs and leaves the denominator in a two-float `stats` buffer on the device
// (stats[0] = sum of weights over valid pixels, stats[1] = the weighted nll sum); the backward reads stats[0], so the
// step never waits for the host.
#include "ce_pixel.h"
#include "reduce.h"

// ------------------------------------------------------------------ cross entropy: what the variants do differently
// The operands only the weighted / ignoring variant has.  weight: C floats or null (all ones); ignore: VMTL_NO_IGNORE
// for none; stats: what the forward left for the backward (null in the forward itself).  The plain variant's struct is
// empty and never read, but as a kernel argument it still takes 8 bytes: the backward kernels take it LAST, so that
// the plain ones find their arguments where they were without it (behind `tgt` the gap split their one load of the
// four pointers in two).  The forward kernels take it behind `tgt`, where the gap costs the plain ones nothing.
template <bool EX>
struct CeEx {};
template <>
struct CeEx<true> {
  const float* __restrict__ weight;
  long long ignore;
  const float* __restrict__ stats;
};

// Forward, before the pixel's sum of exponentials: false when the pixel adds no nll (the rule for labels, ce_pixel.h).
// The plain variant skips nothing and applies the rule in ce_add.
template <bool EX>
__device__ __forceinline__ bool ce_counts(long long t, int C, CeEx<EX> ex, double& num) {
  if constexpr (EX) {
    if (t == ex.ignore) return false;
    if (!ce_label_inside(t, C)) {
      num += (double)ce_nan();
      return false;
    }
  }
  return true;
}

// What a pixel that counts adds: w[t] * nll and w[t] to (numerator, denominator), or nll to the plain variant's single
// sum (kept in num; den stays unused).  nll() is only evaluated for a target inside [0, C).
template <bool EX, class Nll>
__device__ __forceinline__ void ce_add(double& num, double& den, long long t, int C, CeEx<EX> ex, Nll nll) {
  if constexpr (EX) {
    const float wt = ex.weight != nullptr ? ex.weight[t] : 1.f;
    num += (double)wt * (double)nll();
    den += (double)wt;
  } else {
    if (!ce_label_inside(t, C)) num += (double)ce_nan();  // see ce_counts
    else num += (double)nll();
  }
}

// partial: one double per block, or (numerator, denominator) per block
template <bool EX>
__device__ __forceinline__ void ce_store_partials(double num, double den, double* __restrict__ partial, double* shd) {
  const double bn = block_sum(num, shd);
  if constexpr (EX) {
    const double bd = block_sum(den, shd);
    if (threadIdx.x == 0) {
      partial[2 * blockIdx.x] = bn;
      partial[2 * blockIdx.x + 1] = bd;
    }
  } else {
    if (threadIdx.x == 0) partial[blockIdx.x] = bn;
  }
}

// Backward: the gradient of one pixel is dz_c = (softmax_c - 1[c == t]) * k + bad, with k = g = gout / P in the plain
// variant and k = w[t] * g, g = gout / stats[0] in the other.  bad: NaN for a target outside [0, C) that is not the
// ignore index - as the forward: NaN, never a silent 0 - and such a target never indexes w.  An ignored pixel sets
// `zero`, and the kernels then store 0.0f in every lane they own (a select, never a product with g, which is inf when
// every pixel is ignored).
template <bool EX>
__device__ __forceinline__ float ce_grad_unit(const float* __restrict__ gout, long long P, CeEx<EX> ex) {
  if constexpr (EX) return gout[0] / ex.stats[0];
  else return gout[0] / (float)P;
}

template <bool EX>
__device__ __forceinline__ float ce_scale(long long t, int C, float g, CeEx<EX> ex, float& bad, bool& zero) {
  if constexpr (EX) {
    zero = t == ex.ignore;
    const bool oob = !ce_label_inside(t, C);
    bad = (oob && !zero) ? ce_nan() : 0.f;
    return (!oob && ex.weight != nullptr) ? ex.weight[t] * g : g;
  } else {
    zero = false;
    bad = (!ce_label_inside(t, C)) ? ce_nan() : 0.f;
    return g;
  }
}

// ------------------------------------------------------------------ cross entropy: kernels
// Element (b, c, hw) of the logits sits at z[b*sb + c*sc + hw*sp] (layouts: ce_pixel.h).  One thread per pixel; the
// (few) channels are reduced in registers.  The log-softmax subtracts the max first (the numerics note of ce_pixel.h).
// The argmax is written for ignored pixels too (the prediction does not depend on the target).
template <bool EX>
__global__ __launch_bounds__(CE_THREADS) void ce_fwd_kernel(const float* __restrict__ z,
                                                            const long long* __restrict__ tgt, CeEx<EX> ex,
                                                            double* __restrict__ partial,
                                                            long long* __restrict__ amax, long long P, int HW,
                                                            int C, long long sb, long long sc, long long sp) {
  __shared__ double shd[4];
  double num = 0.0, den = 0.0;
  VMTL_GRID_STRIDE(i, P) {
    const long long b = i / HW, hw = i - b * HW;
    const float* r = z + b * sb + hw * sp;
    float m = r[0];
    int am = 0;
    for (int c = 1; c < C; ++c) {
      const float v = r[c * sc];
      if (v > m) { m = v; am = c; }  // first maximum wins, like torch.argmax on ties
    }
    if (amax != nullptr) amax[i] = am;
    if (!ce_counts<EX>(tgt[i], C, ex, num)) continue;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(r[c * sc] - m);
    const long long t = tgt[i];
    ce_add<EX>(num, den, t, C, ex, [&] { return logf(s) - (r[t * sc] - m); });
  }
  ce_store_partials<EX>(num, den, partial, shd);
}

// The same pass with the pixel's logits held in registers (C <= 32: one load per logit instead of three sweeps over
// the channel planes for max / sum-exp / target): 44 -> ~30 us for 32x19x128x256.
template <int Q, bool EX>
__global__ __launch_bounds__(CE_THREADS) void ce_fwd_regs_kernel(const float* __restrict__ z,
                                                                 const long long* __restrict__ tgt, CeEx<EX> ex,
                                                                 double* __restrict__ partial,
                                                                 long long* __restrict__ amax, long long P, int HW,
                                                                 int C, long long sb, long long sc, long long sp) {
  __shared__ double shd[4];
  double num = 0.0, den = 0.0;
  VMTL_GRID_STRIDE(i, P) {
    const long long b = i / HW, hw = i - b * HW;
    const float* r = z + b * sb + hw * sp;
    float v[4 * Q];
#pragma unroll
    for (int c = 0; c < 4 * Q; ++c) v[c] = c < C ? r[c * sc] : 0.f;
    const long long t = tgt[i];
    float m = v[0];
    int am = 0;
#pragma unroll
    for (int c = 1; c < 4 * Q; ++c)
      if (c < C && v[c] > m) { m = v[c]; am = c; }  // first maximum wins, like torch.argmax on ties
    if (amax != nullptr) amax[i] = am;
    if (!ce_counts<EX>(t, C, ex, num)) continue;
    float s = 0.f, zt = 0.f;
#pragma unroll
    for (int c = 0; c < 4 * Q; ++c) {
      if (c < C) s += expf(v[c] - m);
      if (c == t) zt = v[c];
    }
    ce_add<EX>(num, den, t, C, ex, [&] { return logf(s) - (zt - m); });
  }
  ce_store_partials<EX>(num, den, partial, shd);
}

// err (may be null): the result becomes NaN when the flag is set.
__global__ void sum_finalize_kernel(const double* __restrict__ partial, int n, double scale, float* out,
                                    const int* __restrict__ err) {
  __shared__ double shd[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += partial[i];
  const double t = block_sum(s, shd);
  if (threadIdx.x == 0) out[0] = (err != nullptr && err[0] != 0) ? ce_nan() : (float)(t * scale);
}

// The (numerator, denominator) pairs summed in the fixed order of sum_finalize_kernel.
// loss = num / den: NaN (0/0) when every pixel is ignored, as torch.  stats[0] = den, stats[1] = num.
__global__ void ce_ex_finalize_kernel(const double* __restrict__ partial, int n, float* loss, float* stats) {
  __shared__ double shd[4];
  double num = 0.0, den = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    num += partial[2 * i];
    den += partial[2 * i + 1];
  }
  num = block_sum(num, shd);
  den = block_sum(den, shd);
  if (threadIdx.x == 0) {
    loss[0] = (float)(num / den);
    stats[0] = (float)den;
    stats[1] = (float)num;
  }
}

// dz = (softmax(z) - onehot(y)) * k + bad (see ce_scale), written with its own strides.  The softmax is
// recomputed from the logits (max-subtracted, see above); nothing but the denominator is saved by the forward pass.
template <bool EX>
__global__ __launch_bounds__(CE_THREADS) void ce_bwd_kernel(const float* __restrict__ z,
                                                            const long long* __restrict__ tgt,
                                                            const float* __restrict__ gout, float* __restrict__ dz,
                                                            long long P, int HW, int C, long long sb, long long sc,
                                                            long long sp, long long dsb, long long dsc, long long dsp,
                                                            CeEx<EX> ex) {
  const float g = ce_grad_unit<EX>(gout, P, ex);
  VMTL_GRID_STRIDE(i, P) {
    const long long b = i / HW, hw = i - b * HW;
    const long long off = b * sb + hw * sp, doff = b * dsb + hw * dsp;
    float m = z[off];
    for (int c = 1; c < C; ++c) m = fmaxf(m, z[off + c * sc]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(z[off + c * sc] - m);
    const float inv = 1.f / s;
    const long long t = tgt[i];
    float bad;
    bool zero;
    const float k = ce_scale<EX>(t, C, g, ex, bad, zero);
    for (int c = 0; c < C; ++c)  // "EX &&": the plain variant's `zero` is gone before the loop is laid out
      dz[doff + c * dsc] = (EX && zero) ? 0.f : (expf(z[off + c * sc] - m) * inv - (c == t ? 1.f : 0.f)) * k + bad;
  }
}

// The same gradient, channel-contiguous (NHWC rows of ld >= ceil4(C) floats, of which the first ceil4(C) are written):
// one thread per (pixel, channel quad), so a wave writes 1 KB of CONTIGUOUS gradient (one thread per pixel left every
// store instruction touching 64 lanes x 16 bytes at an 80-byte stride: 2-4x slower than the NCHW form).  The softmax
// statistics of a pixel are recomputed by its Q = ceil(C/4) threads (reads hit L1; ~2*C expf each).
template <bool EX>
__global__ __launch_bounds__(CE_THREADS) void ce_bwd_nhwc_kernel(const float* __restrict__ z,
                                                                 const long long* __restrict__ tgt,
                                                                 const float* __restrict__ gout, float* __restrict__ dz,
                                                                 long long P, int HW, int C, long long sb, long long sc,
                                                                 long long sp, int ld, CeEx<EX> ex) {
  const float g = ce_grad_unit<EX>(gout, P, ex);
  const int Q = (C + 3) >> 2;
  const long long total = P * Q;
  VMTL_GRID_STRIDE(idx, total) {
    const long long i = idx / Q;
    const int q = (int)(idx - i * Q);
    const long long b = i / HW, hw = i - b * HW;
    const long long off = b * sb + hw * sp;
    float m = z[off];
    for (int c = 1; c < C; ++c) m = fmaxf(m, z[off + c * sc]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(z[off + c * sc] - m);
    const float inv = 1.f / s;
    const long long t = tgt[i];
    float bad;
    bool zero;
    const float k = ce_scale<EX>(t, C, g, ex, bad, zero);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * q + e;
      v[e] = (c < C && !zero) ? (expf(z[off + c * sc] - m) * inv - (c == t ? 1.f : 0.f)) * k + bad : 0.f;
    }
    *reinterpret_cast<f32x4*>(dz + i * ld + 4 * q) = v;
  }
}

// The same gradient when the NHWC rows are exactly the Q = ceil(C/4) quads (ld == 4*Q, the layout
// ops._CrossEntropy.backward allocates): one thread per PIXEL - logits read once, coalesced along the pixel axis of
// each channel plane, softmax evaluated once - and the wave's 64 finished rows (64*ld contiguous floats) turned
// through LDS so every store instruction writes 1 KB of consecutive gradient.  138 -> ~60 us for 32x19x128x256 on
// MI355X (the quad-per-thread form above re-reads the pixel's logits and re-evaluates 2*C expf in each of its Q threads).
template <int Q, bool EX>
__global__ __launch_bounds__(256) void ce_bwd_nhwc_rows_kernel(const float* __restrict__ z,
                                                               const long long* __restrict__ tgt,
                                                               const float* __restrict__ gout, float* __restrict__ dz,
                                                               long long P, int HW, int C, long long sb, long long sc,
                                                               long long sp, CeEx<EX> ex) {
  __shared__ f32x4 sm[4][64 * Q];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float g = ce_grad_unit<EX>(gout, P, ex);
  for (long long wg0 = (long long)blockIdx.x * 256; wg0 < P; wg0 += (long long)gridDim.x * 256) {  // uniform trip count
    const long long base = wg0 + wave * 64, i = base + lane;
    if (i < P) {
      const long long b = i / HW, hw = i - b * HW;
      const float* r = z + b * sb + hw * sp;
      float v[4 * Q];
#pragma unroll
      for (int c = 0; c < 4 * Q; ++c) v[c] = c < C ? r[c * sc] : 0.f;
      float m = v[0];
#pragma unroll
      for (int c = 1; c < 4 * Q; ++c) m = c < C ? fmaxf(m, v[c]) : m;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < 4 * Q; ++c) {
        v[c] = c < C ? expf(v[c] - m) : 0.f;
        s += v[c];
      }
      const float inv = 1.f / s;
      const long long t = tgt[i];
      float bad;
      bool zero;
      const float k = ce_scale<EX>(t, C, g, ex, bad, zero);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 4 * q + e;
          o[e] = (c < C && !zero) ? (v[c] * inv - (c == t ? 1.f : 0.f)) * k + bad : 0.f;
        }
        sm[wave][lane * Q + q] = o;
      }
    }
    __syncthreads();
    if (base < P) {
      const int nf4 = (int)(P - base < 64 ? P - base : 64) * Q;
      f32x4* out = reinterpret_cast<f32x4*>(dz + base * (4 * Q));
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        const int idx = j * 64 + lane;
        if (idx < nf4) out[idx] = sm[wave][idx];
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ cross entropy: launchers and entry points
// The per-block partials of the loss into `partial` (ce_blocks(P) entries): logits in registers for C <= 32.
template <bool EX>
static void ce_fwd_launch(const float* logits, const long long* target, CeEx<EX> ex, double* partial, long long* amax,
                          long long P, int HW, int C, long long sb, long long sc, long long sp, hipStream_t st) {
  const int nblk = ce_blocks(P);
  ce_dispatch_q(
      C <= 32 ? (C + 3) >> 2 : 0,
      [&](auto q) {
        hipLaunchKernelGGL((ce_fwd_regs_kernel<decltype(q)::value, EX>), dim3(nblk), dim3(CE_THREADS), 0, st, logits,
                           target, ex, partial, amax, P, HW, C, sb, sc, sp);
      },
      [&] {
        hipLaunchKernelGGL(ce_fwd_kernel<EX>, dim3(nblk), dim3(CE_THREADS), 0, st, logits, target, ex, partial, amax, P,
                           HW, C, sb, sc, sp);
      });
}

// The gradient in `layout`: ce_grad_layout's answer (ce_pixel.h, which also says what the three layouts are), or
// CE_GRAD_STRIDED for any strides.
template <bool EX>
static void ce_bwd_launch(CeGradLayout layout, const float* logits, const long long* target, const float* grad_out,
                          float* dlogits, CeEx<EX> ex, long long P, int HW, int C, long long sb, long long sc,
                          long long sp, long long dsb, long long dsc, long long dsp, hipStream_t st) {
  if (layout == CE_GRAD_ROWS) {
    const int nb = grid_1d(P, 256, 8192);
    auto launch = [&](auto q) {
      hipLaunchKernelGGL((ce_bwd_nhwc_rows_kernel<decltype(q)::value, EX>), dim3(nb), dim3(256), 0, st, logits, target,
                         grad_out, dlogits, P, HW, C, sb, sc, sp, ex);
    };
    ce_dispatch_q((int)dsp >> 2, launch, [&] { launch(std::integral_constant<int, 8>{}); });
  } else if (layout == CE_GRAD_WIDE) {
    const int nb = grid_1d(P * ((C + 3) >> 2), CE_THREADS, 8192);
    hipLaunchKernelGGL(ce_bwd_nhwc_kernel<EX>, dim3(nb), dim3(CE_THREADS), 0, st, logits, target, grad_out, dlogits,
                       P, HW, C, sb, sc, sp, (int)dsp, ex);
  } else {
    hipLaunchKernelGGL(ce_bwd_kernel<EX>, dim3(ce_blocks(P)), dim3(CE_THREADS), 0, st, logits, target, grad_out, dlogits,
                       P, HW, C, sb, sc, sp, dsb, dsc, dsp, ex);
  }
}

extern "C" long long vmtl_ce_workspace_bytes(long long P) { return ((long long)ce_blocks(P) + 1) * (long long)sizeof(double); }

// (numerator, denominator) per block
extern "C" long long vmtl_ce_ex_workspace_bytes(long long P) { return 2 * (long long)ce_blocks(P) * (long long)sizeof(double); }

// workspace: vmtl_ce_workspace_bytes(P) bytes, 8-byte aligned (per-block partial sums).  A target outside [0, C)
// makes the loss NaN.
static int ce_fwd_impl(const float* logits, const long long* target, float* loss, void* workspace, long long* amax,
                       int B, int HW, int C, long long sb, long long sc, long long sp, void* stream) {
  if (!logits || !target || !loss || !workspace || B <= 0 || HW <= 0 || C <= 0) return VMTL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long long P = (long long)B * HW;
  double* partial = (double*)workspace;
  ce_fwd_launch<false>(logits, target, {}, partial, amax, P, HW, C, sb, sc, sp, st);
  hipLaunchKernelGGL(sum_finalize_kernel, dim3(1), dim3(256), 0, st, partial, ce_blocks(P), 1.0 / (double)P, loss,
                     (const int*)nullptr);
  return vmtl_check_launch();
}

extern "C" int vmtl_ce_fwd(const float* logits, const long long* target, float* loss, void* workspace, int B, int HW,
                           int C, long long sb, long long sc, long long sp, void* stream) {
  VMTL_ENTER();
  return ce_fwd_impl(logits, target, loss, workspace, nullptr, B, HW, C, sb, sc, sp, stream);
}

// vmtl_ce_fwd that also emits argmax_c logits (= the segmentation prediction of lit_module.py:137-138): the loss
// pass finds every pixel's maximum anyway, so the prediction costs one 8-byte store instead of a second sweep
// over the logits in its own launch
extern "C" int vmtl_ce_fwd_argmax(const float* logits, const long long* target, float* loss, void* workspace,
                                  long long* argmax, int B, int HW, int C, long long sb, long long sc, long long sp,
                                  void* stream) {
  VMTL_ENTER();
  if (!argmax) return VMTL_ERR_ARG;
  return ce_fwd_impl(logits, target, loss, workspace, argmax, B, HW, C, sb, sc, sp, stream);
}

// weight = C floats or null (all ones), ignore_index = VMTL_NO_IGNORE for none, argmax = null or the prediction output.
// Writes loss and stats (2 floats); workspace: vmtl_ce_ex_workspace_bytes(P) bytes, 8-byte aligned.
extern "C" int vmtl_ce_fwd_ex(const float* logits, const long long* target, const float* weight, long long ignore_index,
                              float* loss, float* stats, void* workspace, long long* argmax, int B, int HW, int C,
                              long long sb, long long sc, long long sp, void* stream) {
  VMTL_ENTER();
  if (!logits || !target || !loss || !stats || !workspace || B <= 0 || HW <= 0 || C <= 0) return VMTL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long long P = (long long)B * HW;
  double* partial = (double*)workspace;
  ce_fwd_launch<true>(logits, target, {weight, ignore_index, nullptr}, partial, argmax, P, HW, C, sb, sc, sp, st);
  hipLaunchKernelGGL(ce_ex_finalize_kernel, dim3(1), dim3(256), 0, st, partial, ce_blocks(P), loss, stats);
  return vmtl_check_launch();
}

// The gradient with the strides of the logits (generic-stride kernel, C lanes per pixel, whatever the strides are).
extern "C" int vmtl_ce_bwd(const float* logits, const long long* target, const float* grad_out, float* dlogits, int B,
                           int HW, int C, long long sb, long long sc, long long sp, void* stream) {
  VMTL_ENTER();
  if (!logits || !target || !grad_out || !dlogits || B <= 0 || HW <= 0 || C <= 0) return VMTL_ERR_ARG;
  ce_bwd_launch<false>(CE_GRAD_STRIDED, logits, target, grad_out, dlogits, {}, (long long)B * HW, HW, C, sb, sc, sp, sb,
                       sc, sp, (hipStream_t)stream);
  return vmtl_check_launch();
}

// vmtl_ce_bwd with its own strides for dlogits, in the layout ce_grad_layout (ce_pixel.h) finds for them
extern "C" int vmtl_ce_bwd_strided(const float* logits, const long long* target, const float* grad_out, float* dlogits,
                                   int B, int HW, int C, long long sb, long long sc, long long sp, long long dsb,
                                   long long dsc, long long dsp, void* stream) {
  VMTL_ENTER();
  if (!logits || !target || !grad_out || !dlogits || B <= 0 || HW <= 0 || C <= 0) return VMTL_ERR_ARG;
  ce_bwd_launch<false>(ce_grad_layout(C, HW, dsb, dsc, dsp), logits, target, grad_out, dlogits, {}, (long long)B * HW,
                       HW, C, sb, sc, sp, dsb, dsc, dsp, (hipStream_t)stream);
  return vmtl_check_launch();
}

// dz_c = w[t] (softmax_c - 1[c == t]) gout / stats[0], 0.0f in every written lane of an ignored pixel; stats as
// vmtl_ce_fwd_ex left it.  The three layouts of vmtl_ce_bwd_strided, chosen by the same tests, writing the same lanes.
extern "C" int vmtl_ce_bwd_ex(const float* logits, const long long* target, const float* weight, long long ignore_index,
                              const float* stats, const float* grad_out, float* dlogits, int B, int HW, int C,
                              long long sb, long long sc, long long sp, long long dsb, long long dsc, long long dsp,
                              void* stream) {
  VMTL_ENTER();
  if (!logits || !target || !stats || !grad_out || !dlogits || B <= 0 || HW <= 0 || C <= 0) return VMTL_ERR_ARG;
  ce_bwd_launch<true>(ce_grad_layout(C, HW, dsb, dsc, dsp), logits, target, grad_out, dlogits,
                      {weight, ignore_index, stats}, (long long)B * HW, HW, C, sb, sc, sp, dsb, dsc, dsp,
                      (hipStream_t)stream);
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ SILog
#define SL_BLOCKS_MAX 1024

// Which pixels count: those with target > min_depth, or those of the caller's uint8 mask (reference losses.py:29-31
// with `mask` given; min_depth is then not applied).  The kernels take either as their `valid` operand; partials,
// finalize and the closed-form backward are the same, and with mask == (target > min_depth) the two agree bit for bit.
struct SlAboveMinDepth {
  float min_depth;
  __device__ __forceinline__ bool operator()(const float* __restrict__ tgt, long long i) const { return tgt[i] > min_depth; }
};
struct SlMasked {
  const unsigned char* __restrict__ mask;
  __device__ __forceinline__ bool operator()(const float* __restrict__, long long i) const { return mask[i] != 0; }
};

template <class Valid>
__global__ __launch_bounds__(256) void silog_fwd_kernel(const float* __restrict__ pred,
                                                        const float* __restrict__ tgt, Valid valid, long long P,
                                                        double* __restrict__ partial) {
  __shared__ double shd[4];
  double n = 0.0, s1 = 0.0, s2 = 0.0;
  VMTL_GRID_STRIDE(i, P) {
    if (valid(tgt, i)) {
      const float g = logf(pred[i]) - logf(tgt[i]);
      n += 1.0;
      s1 += (double)g;
      s2 += (double)g * (double)g;
    }
  }
  const double bn = block_sum(n, shd);
  const double b1 = block_sum(s1, shd);
  const double b2 = block_sum(s2, shd);
  if (threadIdx.x == 0) {
    partial[blockIdx.x * 3 + 0] = bn;
    partial[blockIdx.x * 3 + 1] = b1;
    partial[blockIdx.x * 3 + 2] = b2;
  }
}

// stats[0] = N, stats[1] = mean(g), stats[2] = Dg ; loss = 10*sqrt(Dg)
__global__ void silog_finalize_kernel(const double* __restrict__ partial, int nblk, float* loss, float* stats) {
  __shared__ double shd[4];
  double n = 0.0, s1 = 0.0, s2 = 0.0;
  for (int i = threadIdx.x; i < nblk; i += blockDim.x) {
    n += partial[i * 3 + 0];
    s1 += partial[i * 3 + 1];
    s2 += partial[i * 3 + 2];
  }
  n = block_sum(n, shd);
  s1 = block_sum(s1, shd);
  s2 = block_sum(s2, shd);
  if (threadIdx.x == 0) {
    const double mu = s1 / n;                          // n == 0 -> NaN, as torch.mean of an empty tensor
    const double var = (s2 - n * mu * mu) / (n - 1.0); // n == 1 -> NaN (unbiased variance), as torch.var
    const double dg = var + 0.15 * mu * mu;
    loss[0] = (float)(10.0 * sqrt(dg));
    stats[0] = (float)n;
    stats[1] = (float)mu;
    stats[2] = (float)dg;
  }
}

// dL/dpred_i = gout * (5/sqrt(Dg)) * (2 (g_i - mu)/(N-1) + 0.3 mu / N) / pred_i   on valid pixels, else 0
template <class Valid>
__global__ __launch_bounds__(256) void silog_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                        const float* __restrict__ stats,
                                                        const float* __restrict__ gout, Valid valid, long long P,
                                                        float* __restrict__ dpred) {
  const float n = stats[0], mu = stats[1], dg = stats[2];
  const float k = gout[0] * 5.f / sqrtf(dg);
  const float a = 2.f / (n - 1.f), b = 0.3f * mu / n;
  VMTL_GRID_STRIDE(i, P) {
    float r = 0.f;
    if (valid(tgt, i)) {
      const float p = pred[i];
      const float g = logf(p) - logf(tgt[i]);
      r = k * (a * (g - mu) + b) / p;
    }
    dpred[i] = r;
  }
}

static inline int sl_blocks(long long P) {
  return grid_1d(P, 1024, SL_BLOCKS_MAX);
}

extern "C" long long vmtl_silog_workspace_bytes(long long P) { return (long long)sl_blocks(P) * 3 * sizeof(double); }

template <class Valid>
static int silog_fwd_launch(const float* pred, const float* target, Valid valid, float* loss, float* stats,
                            void* workspace, long long P, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nblk = sl_blocks(P);
  hipLaunchKernelGGL(silog_fwd_kernel<Valid>, dim3(nblk), dim3(256), 0, st, pred, target, valid, P, (double*)workspace);
  hipLaunchKernelGGL(silog_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, nblk, loss, stats);
  return vmtl_check_launch();
}

template <class Valid>
static int silog_bwd_launch(const float* pred, const float* target, Valid valid, const float* stats,
                            const float* grad_out, float* dpred, long long P, void* stream) {
  hipLaunchKernelGGL(silog_bwd_kernel<Valid>, dim3(sl_blocks(P)), dim3(256), 0, (hipStream_t)stream, pred, target, stats,
                     grad_out, valid, P, dpred);
  return vmtl_check_launch();
}

extern "C" int vmtl_silog_fwd(const float* pred, const float* target, float min_depth, float* loss, float* stats,
                              void* workspace, long long P, void* stream) {
  VMTL_ENTER();
  if (!pred || !target || !loss || !stats || !workspace || P <= 0) return VMTL_ERR_ARG;
  return silog_fwd_launch(pred, target, SlAboveMinDepth{min_depth}, loss, stats, workspace, P, stream);
}

extern "C" int vmtl_silog_bwd(const float* pred, const float* target, const float* stats, const float* grad_out,
                              float min_depth, float* dpred, long long P, void* stream) {
  VMTL_ENTER();
  if (!pred || !target || !stats || !grad_out || !dpred || P <= 0) return VMTL_ERR_ARG;
  return silog_bwd_launch(pred, target, SlAboveMinDepth{min_depth}, stats, grad_out, dpred, P, stream);
}

extern "C" int vmtl_silog_fwd_mask(const float* pred, const float* target, const unsigned char* mask, float* loss,
                                   float* stats, void* workspace, long long P, void* stream) {
  VMTL_ENTER();
  if (!pred || !target || !mask || !loss || !stats || !workspace || P <= 0) return VMTL_ERR_ARG;
  return silog_fwd_launch(pred, target, SlMasked{mask}, loss, stats, workspace, P, stream);
}

extern "C" int vmtl_silog_bwd_mask(const float* pred, const float* target, const unsigned char* mask, const float* stats,
                                   const float* grad_out, float* dpred, long long P, void* stream) {
  VMTL_ENTER();
  if (!pred || !target || !mask || !stats || !grad_out || !dpred || P <= 0) return VMTL_ERR_ARG;
  return silog_bwd_launch(pred, target, SlMasked{mask}, stats, grad_out, dpred, P, stream);
}

// ------------------------------------------------------------------ L1 (mean absolute error)
__global__ __launch_bounds__(256) void l1_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                     long long P, double* __restrict__ partial) {
  __shared__ double shd[4];
  double s = 0.0;
  VMTL_GRID_STRIDE(i, P)
    s += (double)fabsf(pred[i] - tgt[i]);
  const double b = block_sum(s, shd);
  if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

__global__ __launch_bounds__(256) void l1_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                     const float* __restrict__ gout, long long P,
                                                     float* __restrict__ dpred) {
  const float g = gout[0] / (float)P;
  VMTL_GRID_STRIDE(i, P) {
    const float d = pred[i] - tgt[i];
    dpred[i] = d > 0.f ? g : (d < 0.f ? -g : 0.f);
  }
}

extern "C" int vmtl_l1_fwd(const float* pred, const float* target, float* loss, void* workspace, long long P,
                           void* stream) {
  VMTL_ENTER();
  if (!pred || !target || !loss || !workspace || P <= 0) return VMTL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = sl_blocks(P);
  hipLaunchKernelGGL(l1_fwd_kernel, dim3(nblk), dim3(256), 0, st, pred, target, P, (double*)workspace);
  hipLaunchKernelGGL(sum_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, nblk, 1.0 / (double)P,
                     loss, (const int*)nullptr);
  return vmtl_check_launch();
}

extern "C" int vmtl_l1_bwd(const float* pred, const float* target, const float* grad_out, float* dpred, long long P,
                           void* stream) {
  VMTL_ENTER();
  if (!pred || !target || !grad_out || !dpred || P <= 0) return VMTL_ERR_ARG;
  hipLaunchKernelGGL(l1_bwd_kernel, dim3(sl_blocks(P)), dim3(256), 0, (hipStream_t)stream, pred, target, grad_out, P,
                     dpred);
  return vmtl_check_launch();
}
