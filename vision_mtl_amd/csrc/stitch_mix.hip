// Full 2x2 cross-stitch unit (Misra et al., "Cross-stitch Networks for Multi-task Learning"): the opt-in mix of the two
// task networks' activations, y_a = sum_b w[a,b,(c)] * x_b.  The reference's einsum (models/cross_stitch_model.py:32-37)
// only ever uses the diagonal of this matrix - that default lives in eltwise.hip (stitch_kernel) and is folded into the
// next conv; the full mix cannot be folded (conv(W_a, sum_b w_ab x_b) is not a rescaling of W_a), hence these kernels.
//
// Two tasks only.  Layout: padded NHWC [M][Cs], Cs % 4 == 0, lanes c >= C are written as exact zeros.  The weights
// are the parameter as stored: entry (a,b,c) at (a*2+b)*C + c (wstride 1, channel-wise) or (a,b) at a*2+b (wstride 0).
#include "common.h"

#include "reduce.h"

namespace {

// the four weights of a thread's channel quad; lanes c >= C hold 0
struct MixW {
  f32x4 w[4];  // w[a*2+b]
  int valid;   // channels of the quad below C (0..4)
};

__device__ __forceinline__ MixW mix_weights(const float* __restrict__ w, int q, int C, int wstride) {
  MixW s;
  const int wb = wstride ? C : 1;  // distance between the (a,b) blocks
  s.valid = min(4, max(0, C - q * 4));
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = q * 4 + e;
      s.w[k][e] = c < C ? w[(size_t)k * wb + (size_t)c * wstride] : 0.f;
    }
  return s;
}

// zero a quad's lanes at c >= C whatever they hold (a padded input lane may carry anything, 0 * NaN included)
__device__ __forceinline__ f32x4 mix_mask(f32x4 v, int valid) {
  if (valid < 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e >= valid) v[e] = 0.f;
  }
  return v;
}

// wa * a + wb * b with the rounding spelled out (one product rounded, then one fused multiply-add): the forward, the
// data-gradient-only launch and the one-sweep backward give the same bits, and a zero wb leaves exactly round(wa * a),
// what the diagonal kernel computes
__device__ __forceinline__ f32x4 mix2(f32x4 wa, f32x4 a, f32x4 wb, f32x4 b) {
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = __fmaf_rn(wb[e], b[e], __fmul_rn(wa[e], a[e]));
  return v;
}

struct Mix2 {
  f32x4 a, b;
};
struct Mix4 {
  f32x4 x0, x1, g0, g1;
};

}  // namespace

// y0 = wA*x0 + wB*x1, y1 = wC*x0 + wD*x1 with (A,B,C,D) = (00,01,10,11), or (00,10,01,11) when `transpose`
// (the data gradient: dx_b = sum_a w[a,b] * dy_a).  One float4 column per thread, two rows' loads in flight.
__global__ __launch_bounds__(RED_THREADS) void stitch_mix_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                                                 const float* __restrict__ w, float* __restrict__ y0,
                                                                 float* __restrict__ y1, int M, int C, int Cs, int wstride,
                                                                 int transpose) {
  const int CQ = Cs >> 2;
  column_sweep2(
      M, CQ,
      [&](int q) {
        MixW s = mix_weights(w, q, C, wstride);
        if (transpose) {
          const f32x4 t = s.w[1];
          s.w[1] = s.w[2];
          s.w[2] = t;
        }
        return s;
      },
      [&](int r, int q) {
        const size_t off = (size_t)r * Cs + (size_t)q * 4;
        return Mix2{*reinterpret_cast<const f32x4*>(x0 + off), *reinterpret_cast<const f32x4*>(x1 + off)};
      },
      [&](const Mix2& l, int r, int q, const MixW& s) {
        const size_t off = (size_t)r * Cs + (size_t)q * 4;
        *reinterpret_cast<f32x4*>(y0 + off) = mix_mask(mix2(s.w[0], l.a, s.w[1], l.b), s.valid);
        *reinterpret_cast<f32x4*>(y1 + off) = mix_mask(mix2(s.w[2], l.a, s.w[3], l.b), s.valid);
      });
}

// Backward in one sweep: dx0 = w00*dy0 + w10*dy1, dx1 = w01*dy0 + w11*dy1 (both nullable together) and the partial
// column sums of dy_a * x_b, k = a*2+b - every operand is read once.
__global__ __launch_bounds__(RED_THREADS) void stitch_mix_bwd_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                                                     const float* __restrict__ dy0,
                                                                     const float* __restrict__ dy1,
                                                                     const float* __restrict__ w, float* __restrict__ dx0,
                                                                     float* __restrict__ dx1, int M, int C, int Cs,
                                                                     int wstride, float* partial) {
  const int CQ = Cs >> 2;
  column_reduce_init2<4>(
      M, CQ, Cs, partial, [&](int q) { return mix_weights(w, q, C, wstride); },
      [&](int r, int q) {
        const size_t off = (size_t)r * Cs + (size_t)q * 4;
        return Mix4{*reinterpret_cast<const f32x4*>(x0 + off), *reinterpret_cast<const f32x4*>(x1 + off),
                    *reinterpret_cast<const f32x4*>(dy0 + off), *reinterpret_cast<const f32x4*>(dy1 + off)};
      },
      [&](const Mix4& l, int r, int q, const MixW& s, f32x4* acc) {
        acc[0] += l.g0 * l.x0;
        acc[1] += l.g0 * l.x1;
        acc[2] += l.g1 * l.x0;
        acc[3] += l.g1 * l.x1;
        if (dx0 != nullptr) {
          const size_t off = (size_t)r * Cs + (size_t)q * 4;
          *reinterpret_cast<f32x4*>(dx0 + off) = mix_mask(mix2(s.w[0], l.g0, s.w[2], l.g1), s.valid);
          *reinterpret_cast<f32x4*>(dx1 + off) = mix_mask(mix2(s.w[1], l.g0, s.w[3], l.g1), s.valid);
        }
      });
}

// colsum_finalize_kernel (bn.hip) for K interleaved partial rows per block: workgroup (c, k) sums partial[(b*K+k)*Cs + c]
// over b in fp64 in a fixed order and writes out[k*ostride + c]
__global__ __launch_bounds__(256) void stitch_mix_finalize_kernel(const float* __restrict__ partial, int nblk, int K, int Cs,
                                                                  float* out, int ostride) {
  __shared__ double sh[4];
  const int c = blockIdx.x, k = blockIdx.y;
  const double s = block_rows_sum(partial, nblk, K, k, Cs, c, sh);
  if (threadIdx.x == 0) out[(size_t)k * ostride + c] = (float)s;
}

// layer-wise weights: out[k] = sum over the C channels of row k of the finalize's output (one workgroup per k)
__global__ __launch_bounds__(256) void stitch_mix_sum_channels_kernel(const float* __restrict__ v, int C, int vstride,
                                                                      float* out) {
  __shared__ double sh[4];
  const float* row = v + (size_t)blockIdx.x * vstride;
  double a = 0.0;
  for (int c = threadIdx.x; c < C; c += 256) a += (double)row[c];
  a = block_sum(a, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)a;
}

// [p, p + n) and [q, q + n) overlap
static inline bool mix_overlap(const float* p, const float* q, size_t n) {
  return p != nullptr && q != nullptr && p < q + n && q < p + n;
}

extern "C" int vmtl_stitch_mix(const float* x0, const float* x1, const float* w, float* y0, float* y1, int M, int C, int Cs,
                               int wstride, void* stream) {
  VMTL_ENTER();
  if (!x0 || !x1 || !w || !y0 || !y1 || (Cs & 3) || M <= 0 || C <= 0 || C > Cs || (wstride != 0 && wstride != 1))
    return VMTL_ERR_ARG;
  const size_t n = (size_t)M * Cs;
  if (mix_overlap(y0, y1, n) || mix_overlap(y0, x0, n) || mix_overlap(y0, x1, n) || mix_overlap(y1, x0, n) ||
      mix_overlap(y1, x1, n))
    return VMTL_ERR_ARG;
  hipLaunchKernelGGL(stitch_mix_kernel, dim3(sweep_blocks(M, Cs)), dim3(RED_THREADS), 0, (hipStream_t)stream, x0, x1, w, y0,
                     y1, M, C, Cs, wstride, 0);
  return vmtl_check_launch();
}

// dw (nullable): the whole gradient in parameter layout - 4*C floats (wstride 1) or 4 (wstride 0), overwritten.
// dw NULL: data gradients only, no reduction is launched (the forward kernel on the transposed matrix).
// partial: (4 * vmtl_reduce_rows(M) + 4) * Cs floats (the last four rows are scratch for the layer-wise sum).
extern "C" int vmtl_stitch_mix_bwd(const float* x0, const float* x1, const float* dy0, const float* dy1, const float* w,
                                   float* dx0, float* dx1, float* partial, float* dw, int M, int C, int Cs, int wstride,
                                   void* stream) {
  VMTL_ENTER();
  if (!dy0 || !dy1 || !w || (Cs & 3) || M <= 0 || C <= 0 || C > Cs || (wstride != 0 && wstride != 1)) return VMTL_ERR_ARG;
  if ((dx0 == nullptr) != (dx1 == nullptr) || (!dx0 && !dw)) return VMTL_ERR_ARG;
  if (dw && (!x0 || !x1 || !partial)) return VMTL_ERR_ARG;
  const size_t n = (size_t)M * Cs;
  if (dx0) {
    const float* in[4] = {x0, x1, dy0, dy1};
    if (mix_overlap(dx0, dx1, n)) return VMTL_ERR_ARG;
    for (const float* p : in)
      if (mix_overlap(dx0, p, n) || mix_overlap(dx1, p, n)) return VMTL_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (!dw) {
    hipLaunchKernelGGL(stitch_mix_kernel, dim3(sweep_blocks(M, Cs)), dim3(RED_THREADS), 0, st, dy0, dy1, w, dx0, dx1, M, C, Cs,
                       wstride, 1);
    return vmtl_check_launch();
  }
  const int nblk = red_blocks(M);
  hipLaunchKernelGGL(stitch_mix_bwd_kernel, dim3(nblk), dim3(RED_THREADS), 0, st, x0, x1, dy0, dy1, w, dx0, dx1, M, C, Cs,
                     wstride, partial);
  if (wstride) {
    hipLaunchKernelGGL(stitch_mix_finalize_kernel, dim3(C, 4), dim3(256), 0, st, partial, nblk, 4, Cs, dw, C);
  } else {
    float* per_channel = partial + (size_t)4 * nblk * Cs;
    hipLaunchKernelGGL(stitch_mix_finalize_kernel, dim3(C, 4), dim3(256), 0, st, partial, nblk, 4, Cs, per_channel, Cs);
    hipLaunchKernelGGL(stitch_mix_sum_channels_kernel, dim3(4), dim3(256), 0, st, per_channel, C, Cs, dw);
  }
  return vmtl_check_launch();
}
