// The softmax pixel pass and the gradient layouts of the segmentation criteria.  OHEM (ce_ohem.hip) and cross entropy +
// region term (ce_region.hip) are built from the pieces here: a criterion supplies what its forward accumulates from a
// pixel's (max, argmax, sum of exponentials, z_t), and a GRADIENT POLICY (below) that turns a pixel's softmax into its
// output lanes.  The plain and the weighted / ignoring cross entropy (loss.hip) share the constants, the rule for
// labels, the layout decision and the Q dispatch, but keep their own kernels: loss.hip says why.
#pragma once
#include <type_traits>

#include "common.h"

#define CE_THREADS 256

__device__ __forceinline__ float ce_nan() { return __int_as_float(0x7fc00000); }

// The rule for labels, in every criterion and in both directions: a pixel whose label is the ignore index contributes
// nothing (no nll, +0.0f in every gradient lane it owns); any OTHER label outside [0, C) contributes NaN - to the
// numerator of the loss, and to every gradient lane of the pixel - and never indexes the class weights or any other
// per-class table.  torch raises on an out-of-range class index; raising here would need a host sync on the step path,
// so the step fails VISIBLY instead of silently adding 0.  (The plain cross entropy has no ignore index: the second half
// of the rule is all of it.)
__device__ __forceinline__ bool ce_label_inside(long long t, int C) { return t >= 0 && t < C; }

// Element (b, c, hw) of the logits sits at z[b*sb + c*sc + hw*sp]:
//   NCHW (the reference's layout at the boundary): sb = C*HW, sc = HW, sp = 1  -> every channel
//   read of a wave is 256 contiguous bytes;  NHWC: sb = HW*ld, sc = 1, sp = ld.
// Channel 0 of pixel i = b*HW + hw; the gradient's strides (dsb, dsp) address the same way.
template <class T>
__device__ __forceinline__ T* ce_pixel(T* z, long long i, int HW, long long sb, long long sp) {
  const long long b = i / HW, hw = i - b * HW;
  return z + b * sb + hw * sp;
}

// ------------------------------------------------------------------ the pixel pass
// One thread per pixel.  Numerics: log-softmax is evaluated as (z - max) - log(sum exp(z - max)), subtracting the max
// FIRST (exact for nearby floats).  Forming lse = max + log(sum) and then z - lse would lose ~ulp(max) per pixel when the
// logits are large, a systematic error the backward pass of a deep net amplifies.  Every sum runs in channel order
// c = 0, 1, ..: the association is part of the results' bits.
//
// Register form (C <= 32): the pixel's logits in v[4*Q], 4*Q >= C, one load per logit; lanes c >= C hold 0.f and take
// part in nothing.
template <int Q>
__device__ __forceinline__ void ce_load(float (&v)[4 * Q], const float* r, int C, long long sc) {
#pragma unroll
  for (int c = 0; c < 4 * Q; ++c) v[c] = c < C ? r[c * sc] : 0.f;
}

// max_c v_c and its index, the segmentation prediction (forward kernels)
struct CeMax {
  float m;
  int am;
};
template <int Q>
__device__ __forceinline__ CeMax ce_max_argmax(const float (&v)[4 * Q], int C) {
  float m = v[0];
  int am = 0;
#pragma unroll
  for (int c = 1; c < 4 * Q; ++c)
    if (c < C && v[c] > m) { m = v[c]; am = c; }  // first maximum wins, like torch.argmax on ties
  return {m, am};
}

// max_c v_c alone (backward kernels)
template <int Q>
__device__ __forceinline__ float ce_max(const float (&v)[4 * Q], int C) {
  float m = v[0];
#pragma unroll
  for (int c = 1; c < 4 * Q; ++c) m = c < C ? fmaxf(m, v[c]) : m;
  return m;
}

// sum_c exp(v_c - m), for a caller that needs nothing but the sum
template <int Q>
__device__ __forceinline__ float ce_sum_exp(const float (&v)[4 * Q], int C, float m) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 4 * Q; ++c)
    if (c < C) s += expf(v[c] - m);
  return s;
}

// the same sum, v_c replaced by exp(v_c - m): softmax_c = v_c / sum
template <int Q>
__device__ __forceinline__ float ce_exp_sum(float (&v)[4 * Q], int C, float m) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 4 * Q; ++c) {
    v[c] = c < C ? expf(v[c] - m) : 0.f;
    s += v[c];
  }
  return s;
}

// v_t by selects (0.f for a label outside [0, 4*Q)): a runtime index would put v into scratch
template <int Q>
__device__ __forceinline__ float ce_pick(const float (&v)[4 * Q], long long t) {
  float zt = 0.f;
#pragma unroll
  for (int c = 0; c < 4 * Q; ++c)
    if (c == t) zt = v[c];
  return zt;
}

// Sweep form (any C): one pass over the channel planes per statistic.
__device__ __forceinline__ CeMax ce_sweep_max_argmax(const float* r, int C, long long sc) {
  float m = r[0];
  int am = 0;
  for (int c = 1; c < C; ++c) {
    const float v = r[c * sc];
    if (v > m) { m = v; am = c; }  // as ce_max_argmax
  }
  return {m, am};
}

__device__ __forceinline__ float ce_sweep_max(const float* r, int C, long long sc) {
  float m = r[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, r[c * sc]);
  return m;
}

// each(v) sees every logit of the sweep (OHEM's finiteness flag rides on it)
template <class Each>
__device__ __forceinline__ float ce_sweep_sum_exp(const float* r, int C, long long sc, float m, Each each) {
  float s = 0.f;
  for (int c = 0; c < C; ++c) {
    const float v = r[c * sc];
    s += expf(v - m);
    each(v);
  }
  return s;
}
__device__ __forceinline__ float ce_sweep_sum_exp(const float* r, int C, long long sc, float m) {
  return ce_sweep_sum_exp(r, C, sc, m, [](float) {});
}

// ------------------------------------------------------------------ gradient policies
// The gradient kernels below recompute a pixel's softmax from the logits (max-subtracted, see above) and leave the rest
// to a policy, passed by value as the last kernel argument.  A policy has
//
//   template <int Q> Wg begin(gout, P, C) const     in front of the pixel loop: the scale of the gradient and whatever
//                                                   per-class state the criterion keeps (Q = 0 in the sweep kernels: no
//                                                   register form).  It may declare __shared__ state and hold a
//                                                   barrier, so EVERY thread of the block calls it exactly once, before
//                                                   any thread leaves the kernel or enters divergent code.
//   Wg::pixel(i, t, C) -> Px                        the pixel's scale / flags.  Px::zero: every lane the kernel owns at
//                                                   this pixel is +0.0f, stored without evaluating the softmax (a store,
//                                                   never a product with the scale, which is inf when the forward's
//                                                   denominator is 0).
//   Wg::lanes<Q>(px, e, inv, t, C, put)             the Q output quads of a pixel that is not zeroed, each handed to
//                                                   put(q, quad), from e_c = exp(z_c - max) and inv = 1 / sum e (not
//                                                   from the normalised softmax: a criterion's expression keeps its own
//                                                   shape, which decides where a multiply-add is fused, i.e. the last bit)
//   Wg::lane(px, e, inv, hit) -> float              one lane of a LINEAR policy, dz_c = (softmax_c - 1[c == t]) k + bad;
//                                                   the sweep kernels take only those.
//
// A linear policy's pixel: k = w[t] * g (g without weights, or for a label that may not index them), bad = NaN for a
// label outside [0, C) of a pixel that is not zeroed (see ce_label_inside), zero as the criterion decides.
struct CeLinearPx {
  float k, bad;
  bool zero;
};

__device__ __forceinline__ CeLinearPx ce_linear_px(long long t, int C, float g, const float* __restrict__ weight,
                                                   bool zero) {
  const bool oob = !ce_label_inside(t, C);
  return {(!oob && weight != nullptr) ? weight[t] * g : g, (oob && !zero) ? ce_nan() : 0.f, zero};
}

// what a linear policy's Wg derives from: the lane, and the quads built from it
struct CeLinearWg {
  static __device__ __forceinline__ float lane(const CeLinearPx& px, float e, float inv, bool hit) {
    return (e * inv - (hit ? 1.f : 0.f)) * px.k + px.bad;
  }
  template <int Q, class Put>
  static __device__ __forceinline__ void lanes(const CeLinearPx& px, const float (&e)[4 * Q], float inv, long long t, int C,
                                               Put put) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * q + j;
        o[j] = c < C ? lane(px, e[c], inv, c == t) : 0.f;
      }
      put(q, o);
    }
  }
};

// The gradient of pixel i, logits in registers: put(q, quad) takes channel quad q = 0 .. Q-1 (lanes c >= C are +0.0f).
template <int Q, class Wg, class Put>
__device__ __forceinline__ void ce_grad_pixel(const Wg& wg, const float* z, const long long* tgt, long long i, int HW,
                                              int C, long long sb, long long sc, long long sp, Put put) {
  const long long t = tgt[i];
  const auto px = wg.pixel(i, t, C);
  if (px.zero) {
#pragma unroll
    for (int q = 0; q < Q; ++q) put(q, (f32x4){0.f, 0.f, 0.f, 0.f});
  } else {
    float e[4 * Q];
    ce_load<Q>(e, ce_pixel(z, i, HW, sb, sp), C, sc);
    const float m = ce_max<Q>(e, C);
    const float inv = 1.f / ce_exp_sum<Q>(e, C, m);
    wg.template lanes<Q>(px, e, inv, t, C, put);
  }
}

// ------------------------------------------------------------------ the three gradient layouts
// Element (b, c, hw) of the gradient goes to dz[b*dsb + c*dsc + hw*dsp].  With (HW*ld, 1, ld) the gradient lands in the
// NHWC storage the head's data-gradient conv reads (one 76-byte run per pixel) and the NCHW -> NHWC relayout of an 80 MB
// tensor disappears from the step.
//   rows    : NHWC rows of exactly ceil4(C) <= 32 floats, all written, turned through LDS
//   wide    : NHWC rows of ld > ceil4(C) floats (or C > 32), of which the first ceil4(C) are written
//   strided : anything else; C lanes per pixel
enum CeGradLayout { CE_GRAD_ROWS, CE_GRAD_WIDE, CE_GRAD_STRIDED };

static inline CeGradLayout ce_grad_layout(int C, int HW, long long dsb, long long dsc, long long dsp) {
  const int c4 = (C + 3) & ~3;
  if (dsc == 1 && dsp == c4 && dsp <= 32 && dsb == dsp * HW) return CE_GRAD_ROWS;
  if (dsc == 1 && (dsp & 3) == 0 && dsp >= c4 && dsb == dsp * HW) return CE_GRAD_WIDE;
  return CE_GRAD_STRIDED;
}

// rows, ld == 4*Q with Q = ceil(C/4) (the layout the autograd nodes of ops.py allocate when C + 1 fits): one thread per
// PIXEL - logits read once, coalesced along the pixel axis of each channel plane, softmax evaluated once - and the
// wave's 64 finished rows (64*ld contiguous floats) turned through LDS so every store instruction writes 1 KB of
// consecutive gradient.  138 -> ~60 us for 32x19x128x256 on MI355X against the quad-per-thread form below, which
// re-reads the pixel's logits and re-evaluates 2*C expf in each of its Q threads.
template <int Q, class Pol>
__global__ __launch_bounds__(256) void ce_grad_rows_kernel(const float* __restrict__ z,
                                                           const long long* __restrict__ tgt,
                                                           const float* __restrict__ gout, float* __restrict__ dz,
                                                           long long P, int HW, int C, long long sb, long long sc,
                                                           long long sp, Pol pol) {
  __shared__ f32x4 sm[4][64 * Q];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const auto wg = pol.template begin<Q>(gout, P, C);
  for (long long wg0 = (long long)blockIdx.x * 256; wg0 < P; wg0 += (long long)gridDim.x * 256) {  // uniform trip count
    const long long base = wg0 + wave * 64, i = base + lane;
    if (i < P) {
      ce_grad_pixel<Q>(wg, z, tgt, i, HW, C, sb, sc, sp, [&](int q, f32x4 o) { sm[wave][lane * Q + q] = o; });
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

// The softmax statistics of the sweep kernels: max and 1 / sum exp over the channel planes.
__device__ __forceinline__ void ce_sweep_softmax(const float* r, int C, long long sc, float& m, float& inv) {
  m = ce_sweep_max(r, C, sc);
  inv = 1.f / ce_sweep_sum_exp(r, C, sc, m);
}

// wide: one thread per (pixel, channel quad), so a wave writes 1 KB of CONTIGUOUS gradient (one thread per pixel left
// every store instruction touching 64 lanes x 16 bytes at an 80-byte stride: 2-4x slower than the NCHW form).  The
// softmax statistics of a pixel are recomputed by its Q = ceil(C/4) threads (reads hit L1; ~2*C expf each).
template <class Pol>
__global__ __launch_bounds__(CE_THREADS) void ce_grad_wide_kernel(const float* __restrict__ z,
                                                                  const long long* __restrict__ tgt,
                                                                  const float* __restrict__ gout, float* __restrict__ dz,
                                                                  long long P, int HW, int C, long long sb, long long sc,
                                                                  long long sp, int ld, Pol pol) {
  const auto wg = pol.template begin<0>(gout, P, C);
  const int Q = (C + 3) >> 2;
  const long long total = P * Q;
  VMTL_GRID_STRIDE(idx, total) {
    const long long i = idx / Q;
    const int q = (int)(idx - i * Q);
    const float* r = ce_pixel(z, i, HW, sb, sp);
    const long long t = tgt[i];
    const auto px = wg.pixel(i, t, C);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!px.zero) {
      float m, inv;
      ce_sweep_softmax(r, C, sc, m, inv);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * q + e;
        v[e] = c < C ? wg.lane(px, expf(r[c * sc] - m), inv, c == t) : 0.f;
      }
    }
    *reinterpret_cast<f32x4*>(dz + i * ld + 4 * q) = v;
  }
}

// strided: one thread per pixel, C lanes, whatever the strides are
template <class Pol>
__global__ __launch_bounds__(CE_THREADS) void ce_grad_strided_kernel(const float* __restrict__ z,
                                                                     const long long* __restrict__ tgt,
                                                                     const float* __restrict__ gout,
                                                                     float* __restrict__ dz, long long P, int HW, int C,
                                                                     long long sb, long long sc, long long sp,
                                                                     long long dsb, long long dsc, long long dsp, Pol pol) {
  const auto wg = pol.template begin<0>(gout, P, C);
  VMTL_GRID_STRIDE(i, P) {
    const float* r = ce_pixel(z, i, HW, sb, sp);
    float* d = ce_pixel(dz, i, HW, dsb, dsp);
    const long long t = tgt[i];
    const auto px = wg.pixel(i, t, C);
    if (px.zero) {
      for (int c = 0; c < C; ++c) d[c * dsc] = 0.f;
      continue;
    }
    float m, inv;
    ce_sweep_softmax(r, C, sc, m, inv);
    for (int c = 0; c < C; ++c) d[c * dsc] = wg.lane(px, expf(r[c * sc] - m), inv, c == t);
  }
}

// ------------------------------------------------------------------ host side
// f(std::integral_constant<int, Q>) for Q = q in 1 .. 8, otherwise() for any other q.
template <class F, class G>
static inline void ce_dispatch_q(int q, F f, G otherwise) {
  switch (q) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: otherwise();
  }
}

// blocks of the one-thread-per-pixel kernels that leave per-block partials, and of the strided gradient
static inline int ce_blocks(long long P) {
  return grid_1d(P, CE_THREADS, 2048);
}

template <class Pol>
static void ce_grad_rows_launch(const float* logits, const long long* target, const float* grad_out, float* dlogits,
                                Pol pol, long long P, int HW, int C, long long sb, long long sc, long long sp,
                                hipStream_t st) {
  const int nb = grid_1d(P, 256, 8192);
  auto launch = [&](auto q) {
    hipLaunchKernelGGL((ce_grad_rows_kernel<decltype(q)::value, Pol>), dim3(nb), dim3(256), 0, st, logits, target,
                       grad_out, dlogits, P, HW, C, sb, sc, sp, pol);
  };
  ce_dispatch_q((C + 3) >> 2, launch, [&] { launch(std::integral_constant<int, 8>{}); });
}

// The gradient of a linear policy in `layout` (ce_grad_layout's answer, or CE_GRAD_STRIDED for any strides).
template <class Pol>
static void ce_grad_launch(CeGradLayout layout, const float* logits, const long long* target, const float* grad_out,
                           float* dlogits, Pol pol, long long P, int HW, int C, long long sb, long long sc, long long sp,
                           long long dsb, long long dsc, long long dsp, hipStream_t st) {
  if (layout == CE_GRAD_ROWS) {
    ce_grad_rows_launch(logits, target, grad_out, dlogits, pol, P, HW, C, sb, sc, sp, st);
  } else if (layout == CE_GRAD_WIDE) {
    const int nb = grid_1d(P * ((C + 3) >> 2), CE_THREADS, 8192);
    hipLaunchKernelGGL(ce_grad_wide_kernel<Pol>, dim3(nb), dim3(CE_THREADS), 0, st, logits, target, grad_out, dlogits, P,
                       HW, C, sb, sc, sp, (int)dsp, pol);
  } else {
    hipLaunchKernelGGL(ce_grad_strided_kernel<Pol>, dim3(ce_blocks(P)), dim3(CE_THREADS), 0, st, logits, target, grad_out,
                       dlogits, P, HW, C, sb, sc, sp, dsb, dsc, dsp, pol);
  }
}
