// The three kernels a torchvision BasicBlock ResNet encoder (smp ResNetEncoder "resnet18" / "resnet34", reference
// vision_mtl/utils/model_utils.py:10-31 with encoder_name set) needs beyond the MobileNet path:
//
//  1. the data gradient of a stride-2 dense conv by PHASE DECOMPOSITION: the input pixels of one phase
//     (ih mod 2, iw mod 2) receive a stride-1 correlation of dy with that phase's subset of the flipped taps (3x3 / pad 1:
//     2x2, 2x1, 1x2 and 1x1 taps, the forward's 9 taps in all; no zero insertion).  Each phase is one launch of the
//     implicit-GEMM conv (vmtl_conv2d_fwd_ws_p: split-K where the stride-1 data gradient splits too; single-tap unpadded
//     phases in fp32 on the pointwise GEMM vmtl_conv1x1_fwd) into a workspace, and one gather interleaves them into dx.
//  2. BatchNorm + activation + MaxPool2d(3, stride 2, pad 1) of the ResNet stem as one node that writes both the activated
//     map (a decoder skip) and the pooled map, with a gather backward (no atomics).
//  3. the residual close y = act(BN_a(z) + r), r = the block input or BN_b(z_ds) (downsample branch).
//
// NHWC fp32 [B][H][W][Cs], Cs = round_up(C, 4), pad channels are written as 0.  Per-channel reductions are two-stage and
// deterministic (reduce.h partial rows, fp64 finalize in a fixed order).
#include "common.h"

#include "reduce.h"
#include "../../include/vmtl.h"

#define RES_ACT_SWITCH(act, CALL)                           \
  switch (act) {                                            \
    case VMTL_ACT_NONE: CALL(VMTL_ACT_NONE); break;         \
    case VMTL_ACT_RELU: CALL(VMTL_ACT_RELU); break;         \
    case VMTL_ACT_HSWISH: CALL(VMTL_ACT_HSWISH); break;     \
    case VMTL_ACT_HSIGMOID: CALL(VMTL_ACT_HSIGMOID); break; \
    case VMTL_ACT_SIGMOID: CALL(VMTL_ACT_SIGMOID); break;   \
    default: return VMTL_ERR_ARG;                           \
  }

// ---------------------------------------------------------------- 1. stride-2 data gradient
struct S2Phase {
  int T[2];    // taps along h / w (0: the phase receives no tap, its pixels are exact zeros)
  int k0[2];   // first (smallest) forward tap index of the phase along h / w
  int pad;     // pad of the phase correlation as launched (phase pad + e)
  int e;       // leading rows / columns of the launch output that lie before pixel 0 of the phase
  int Hp, Wp;  // extent of the launch output
  int Ha, Wa;  // pixels of the phase inside the input
  long long woff, poff;  // float offsets of the phase in the workspace / in the packed weights
};
struct S2Geo {
  S2Phase ph[4];
  long long ws, pk;  // workspace / packed-weight floats
  long long split_off;  // the split-K slabs of the phase launches (shared: the phases run in stream order)
};

// per-dimension phase a of a K-tap / pad conv: (taps, first tap, correlation pad); false when that pad is negative
static bool s2_dim(int a, int K, int pad, int& T, int& k0, int& p) {
  k0 = (a + pad) & 1;
  T = k0 < K ? (K - k0 + 1) / 2 : 0;
  p = 0;
  if (T == 0) return true;
  p = (T - 1) - (a + pad - k0) / 2;
  return p >= 0;
}

// phase geometry of dx [B][H][W][Cs] from dy [B][Ho][Wo][ldy]; false: unsupported (K, pad)
static bool s2_geometry(int B, int H, int W, int Cs, int Ho, int Wo, int K, int pad, int ldy, int Cin, S2Geo& g) {
  if (K <= 0 || pad < 0 || H <= 0 || W <= 0) return false;
  int T[2], k0[2], p[2];
  for (int a = 0; a < 2; ++a)
    if (!s2_dim(a, K, pad, T[a], k0[a], p[a])) return false;
  if (T[0] > 0 && T[1] > 0 && p[0] != p[1]) return false;  // the implicit GEMM takes one pad for both axes
  const int pc = T[0] > 0 ? p[0] : p[1];
  g.ws = g.pk = 0;
  long long split = 0;
  for (int ph = 0; ph < 4; ++ph) {
    const int a = ph >> 1, b = ph & 1;
    S2Phase& s = g.ph[ph];
    s.T[0] = T[a]; s.T[1] = T[b];
    s.k0[0] = k0[a]; s.k0[1] = k0[b];
    s.Ha = (H - a + 1) / 2;
    s.Wa = (W - b + 1) / 2;
    s.woff = g.ws;
    s.poff = g.pk;
    s.e = s.pad = s.Hp = s.Wp = 0;
    if (s.T[0] == 0 || s.T[1] == 0) {
      s.T[0] = s.T[1] = 0;
      continue;
    }
    g.pk += (long long)Cin * s.T[0] * s.T[1] * ldy;  // the packed operand does not depend on the extent
    if (s.Ha == 0 || s.Wa == 0) continue;           // H or W == 1: the phase has no pixels (Hp = 0: no launch)
    // output row r of the launch is phase row r - e: grow the pad until the launch covers all Ha (Wa) rows (columns)
    int e = 0;
    e = max(e, s.Ha + s.T[0] - 1 - Ho - 2 * pc);
    e = max(e, s.Wa + s.T[1] - 1 - Wo - 2 * pc);
    s.e = e;
    s.pad = pc + e;
    s.Hp = Ho + 2 * s.pad - s.T[0] + 1;
    s.Wp = Wo + 2 * s.pad - s.T[1] + 1;
    g.ws += (long long)B * Cs * s.Hp * s.Wp;
    // tile-starved phases split K exactly as the stride-1 data gradient does (vmtl_conv2d_fwd_ws_p)
    const int ks = vmtl_conv2d_ksplit(B, s.Hp, s.Wp, Cs, s.T[0] * s.T[1] * ldy);
    if (ks > 1) split = max(split, (long long)ks * B * s.Hp * s.Wp * Cs);
  }
  g.split_off = g.ws;
  g.ws += split;
  return true;
}

// packed data-gradient operand, phase by phase: [Cin][T0*T1][ldy], tap (th, tw) = forward tap
// (k0h + 2*(T0-1-th), k0w + 2*(T1-1-tw)) (flipped), channels >= Cout zero
__global__ __launch_bounds__(256) void pack_dgrad_s2_kernel(const float* __restrict__ w, float* __restrict__ dst, S2Geo g,
                                                            int Cout, int Cin, int ldy, int K) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.pk) return;
  int ph = 3;
  while (ph > 0 && (g.ph[ph].T[0] == 0 || i < g.ph[ph].poff)) --ph;
  const S2Phase& s = g.ph[ph];
  const long long j = i - s.poff;
  const int co = (int)(j % ldy);
  const long long rest = j / ldy;
  const int ntap = s.T[0] * s.T[1];
  const int t = (int)(rest % ntap), ci = (int)(rest / ntap);
  const int th = t / s.T[1], tw = t % s.T[1];
  const int kh = s.k0[0] + 2 * (s.T[0] - 1 - th), kw = s.k0[1] + 2 * (s.T[1] - 1 - tw);
  dst[i] = co < Cout ? w[(((size_t)co * Cin + ci) * K + kh) * K + kw] : 0.f;
}

// dx[b][ih][iw][:] = phase (ih & 1, iw & 1) output at (ih >> 1, iw >> 1) (+ e), or 0 for a phase without taps
__global__ __launch_bounds__(256) void dgrad_s2_interleave_kernel(const float* __restrict__ ws, float* __restrict__ dx,
                                                                  S2Geo g, int B, int H, int W, int Cs) {
  const int CQ = Cs >> 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * H * W * CQ) return;
  const int q = (int)(i % CQ);
  const long long pix = i / CQ;
  const int iw = (int)(pix % W);
  const long long t = pix / W;
  const int ih = (int)(t % H), b = (int)(t / H);
  const S2Phase& s = g.ph[(ih & 1) * 2 + (iw & 1)];
  f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (s.T[0] > 0) {
    const size_t src = (((size_t)b * s.Hp + (ih >> 1) + s.e) * s.Wp + (iw >> 1) + s.e) * Cs + (size_t)q * 4;
    v = *reinterpret_cast<const f32x4*>(ws + s.woff + src);
  }
  *reinterpret_cast<f32x4*>(dx + (size_t)pix * Cs + (size_t)q * 4) = v;
}

extern "C" int vmtl_conv2d_dgrad_s2_supported(int K, int pad) {
  S2Geo g;
  return s2_geometry(1, 2 * K + 2, 2 * K + 2, 4, K + 1, K + 1, K, pad, 4, 1, g) ? 1 : 0;
}

extern "C" long long vmtl_conv2d_dgrad_s2_ws(int B, int H, int W, int Cs, int Ho, int Wo, int ldy, int K, int pad) {
  S2Geo g;
  if (B <= 0 || Cs <= 0 || ldy <= 0 || !s2_geometry(B, H, W, Cs, Ho, Wo, K, pad, ldy, 1, g)) return -1;
  return g.ws;
}

extern "C" long long vmtl_pack_dgrad_s2_size(int Cin, int ldy, int K, int pad) {
  S2Geo g;
  if (!s2_geometry(1, 2 * K + 2, 2 * K + 2, 4, K + 1, K + 1, K, pad, ldy, Cin, g)) return -1;
  return g.pk;
}

extern "C" int vmtl_pack_dgrad_s2(const float* w, float* dst, int Cout, int Cin, int ldy, int K, int pad, void* stream) {
  VMTL_ENTER();
  if (!w || !dst || Cout <= 0 || Cin <= 0 || ldy < Cout || (ldy & 3)) return VMTL_ERR_ARG;
  S2Geo g;
  if (!s2_geometry(1, 2 * K + 2, 2 * K + 2, 4, K + 1, K + 1, K, pad, ldy, Cin, g)) return VMTL_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pack_dgrad_s2_kernel, dim3((unsigned)cdivll(g.pk, 256)), dim3(256), 0, (hipStream_t)stream, w, dst, g,
                     Cout, Cin, ldy, K);
  return vmtl_check_launch();
}

extern "C" int vmtl_conv2d_dgrad_s2_p(const float* dy, const float* wp, float* dx, float* ws, int B, int H, int W, int Cs,
                                      int Ho, int Wo, int ldy, int Cin, int K, int pad, int precision, void* stream) {
  VMTL_ENTER();
  if (!valid_prec(precision) || !dy || !wp || !dx || !ws || B <= 0 || Cin <= 0 || Cin > Cs || (Cs & 3) || (ldy & 3) ||
      ldy <= 0)
    return VMTL_ERR_ARG;
  if ((H + 2 * pad - K) / 2 + 1 != Ho || (W + 2 * pad - K) / 2 + 1 != Wo || Ho <= 0 || Wo <= 0) return VMTL_ERR_ARG;
  if ((long long)B * H * W > 0x7fffffffLL) return VMTL_ERR_ARG;
  S2Geo g;
  if (!s2_geometry(B, H, W, Cs, Ho, Wo, K, pad, ldy, Cin, g)) return VMTL_ERR_UNSUPPORTED;
  for (int ph = 0; ph < 4; ++ph) {
    const S2Phase& s = g.ph[ph];
    if (s.T[0] == 0 || s.Hp == 0) continue;
    if ((long long)B * s.Hp * s.Wp > 0x7fffffffLL) return VMTL_ERR_ARG;
    int rc;
    if (s.T[0] == 1 && s.T[1] == 1 && s.pad == 0 && precision == VMTL_PREC_FP32 &&
        (long long)B * s.Hp * s.Wp <= (1LL << 21)) {
      // a single-tap phase without padding (1x1 / pad 0; the (even, even) phase of 3x3 / pad 1) is a plain GEMM over the
      // pixels of dy: the pointwise kernel, as the stride-1 route takes for 1x1 convs (ops.conv_plan)
      rc = vmtl_conv1x1_fwd(dy, wp + s.poff, nullptr, ws + s.woff, nullptr, B * s.Hp * s.Wp, ldy, Cs, Cin, Cin, stream);
    } else {
      rc = vmtl_conv2d_fwd_ws_p(dy, wp + s.poff, nullptr, ws + s.woff, ws + g.split_off, B, Ho, Wo, ldy, s.Hp, s.Wp, Cs,
                                Cin, Cin, s.T[0], s.T[1], 1, s.pad, precision, stream);
    }
    if (rc != 0) return rc;
  }
  const long long n = (long long)B * H * W * (Cs >> 2);
  hipLaunchKernelGGL(dgrad_s2_interleave_kernel, dim3((unsigned)cdivll(n, 256)), dim3(256), 0, (hipStream_t)stream, ws, dx,
                     g, B, H, W, Cs);
  return vmtl_check_launch();
}

extern "C" int vmtl_conv2d_dgrad_s2(const float* dy, const float* wp, float* dx, float* ws, int B, int H, int W, int Cs,
                                    int Ho, int Wo, int ldy, int Cin, int K, int pad, void* stream) {
  return vmtl_conv2d_dgrad_s2_p(dy, wp, dx, ws, B, H, W, Cs, Ho, Wo, ldy, Cin, K, pad, VMTL_PREC_FP32, stream);
}

// ---------------------------------------------------------------- shared per-channel coefficients
// v = act(gamma * (x - mean) * invstd + beta) on valid channels; mean == nullptr: no BatchNorm (v = act(x))
struct ChanCoef {
  f32x4 mean, invstd, gamma, beta, valid;
};

__device__ __forceinline__ ChanCoef chan_coef(int q, int C, const float* mean, const float* invstd, const float* gamma,
                                              const float* beta) {
  ChanCoef k;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = q * 4 + e;
    const bool ok = c < C;
    k.valid[e] = ok ? 1.f : 0.f;
    k.mean[e] = (ok && mean) ? mean[c] : 0.f;
    k.invstd[e] = (ok && mean) ? invstd[c] : 1.f;
    k.gamma[e] = (ok && gamma) ? gamma[c] : 1.f;
    k.beta[e] = (ok && beta) ? beta[c] : 0.f;
  }
  return k;
}

// ---------------------------------------------------------------- 2. BatchNorm + activation + MaxPool2d(3, 2, 1)
// Row r of the forward sweep is one pooled pixel (b, oh, ow).  Its window covers input rows 2oh-1..2oh+1 and columns
// 2ow-1..2ow+1; the 2x2 block (2oh..2oh+1, 2ow..2ow+1) inside it is "owned" by the row, and the owned blocks of all rows
// tile the input (Ho = floor((H-1)/2) + 1 >= H/2), so the activated map is written once with no extra loads.  The arg-max
// follows torch's CPU max_pool2d: start at -inf with the first in-range element, take v when v > max or v is NaN
// (first maximum in row-major window order wins, the last NaN wins).  idx keeps the window position (0..8) per element.
template <int ACT>
__global__ __launch_bounds__(RED_THREADS) void bn_act_pool3s2_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ a_out, float* __restrict__ y,
    unsigned char* __restrict__ idx, int B, int H, int W, int Ho, int Wo, int C, int Cs) {
  const int Mp = B * Ho * Wo;
  column_sweep(Mp, Cs >> 2, [&](int q) { return chan_coef(q, C, mean, invstd, gamma, beta); },
               [&](int r, int q, const ChanCoef& k) {
                 const int ow = r % Wo, t = r / Wo;
                 const int oh = t % Ho, b = t / Ho;
                 f32x4 m;
                 unsigned pos[4];
                 const int h0 = max(2 * oh - 1, 0), w0 = max(2 * ow - 1, 0);
#pragma unroll
                 for (int e = 0; e < 4; ++e) {
                   m[e] = -__builtin_inff();
                   pos[e] = (unsigned)((h0 - (2 * oh - 1)) * 3 + (w0 - (2 * ow - 1)));
                 }
#pragma unroll
                 for (int kh = 0; kh < 3; ++kh) {
                   const int ih = 2 * oh - 1 + kh;
                   if (ih < 0 || ih >= H) continue;
#pragma unroll
                   for (int kw = 0; kw < 3; ++kw) {
                     const int iw = 2 * ow - 1 + kw;
                     if (iw < 0 || iw >= W) continue;
                     const size_t off = (((size_t)b * H + ih) * W + iw) * Cs + (size_t)q * 4;
                     const f32x4 xv = *reinterpret_cast<const f32x4*>(x + off);
                     f32x4 v;
#pragma unroll
                     for (int e = 0; e < 4; ++e) {
                       v[e] = k.valid[e] != 0.f ? act_fwd(k.gamma[e] * ((xv[e] - k.mean[e]) * k.invstd[e]) + k.beta[e], ACT)
                                                : 0.f;
                       if (v[e] > m[e] || v[e] != v[e]) {
                         m[e] = v[e];
                         pos[e] = (unsigned)(kh * 3 + kw);
                       }
                     }
                     if (a_out != nullptr && kh >= 1 && kw >= 1) *reinterpret_cast<f32x4*>(a_out + off) = v;
                   }
                 }
                 f32x4 o;
                 unsigned packed = 0;
#pragma unroll
                 for (int e = 0; e < 4; ++e) {
                   o[e] = k.valid[e] != 0.f ? m[e] : 0.f;
                   packed |= (pos[e] & 0xffu) << (8 * e);
                 }
                 *reinterpret_cast<f32x4*>(y + (size_t)r * Cs + (size_t)q * 4) = o;
                 *reinterpret_cast<unsigned*>(idx + (size_t)r * Cs + (size_t)q * 4) = packed;
               });
}

// gradient reaching input pixel r = (b, ih, iw) through the pool: the skip gradient plus dyp of every window (at most 2x2,
// fixed order) whose arg-max is this pixel
__device__ __forceinline__ f32x4 pool3s2_gather(const float* __restrict__ dskip, const float* __restrict__ dyp,
                                                const unsigned char* __restrict__ idx, int r, int q, int H, int W, int Ho,
                                                int Wo, int Cs) {
  const int iw = r % W, t = r / W;
  const int ih = t % H, b = t / H;
  f32x4 g = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (dskip != nullptr) g = *reinterpret_cast<const f32x4*>(dskip + (size_t)r * Cs + (size_t)q * 4);
  const int oh0 = ih >> 1, oh1 = min((ih + 1) >> 1, Ho - 1);
  const int ow0 = iw >> 1, ow1 = min((iw + 1) >> 1, Wo - 1);
  for (int oh = oh0; oh <= oh1; ++oh)
    for (int ow = ow0; ow <= ow1; ++ow) {
      const unsigned want = (unsigned)((ih - 2 * oh + 1) * 3 + (iw - 2 * ow + 1));
      const size_t o = (((size_t)b * Ho + oh) * Wo + ow) * Cs + (size_t)q * 4;
      const unsigned p = *reinterpret_cast<const unsigned*>(idx + o);
      const f32x4 d = *reinterpret_cast<const f32x4*>(dyp + o);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (((p >> (8 * e)) & 0xffu) == want) g[e] += d[e];
    }
  return g;
}

// BatchNorm form: dz = g * act'(z) (written for the apply sweep) and the partial rows (sum dz, sum dz*xhat)
template <int ACT>
__global__ __launch_bounds__(RED_THREADS) void bn_pool3s2_bwd_reduce_kernel(
    const float* __restrict__ x, const float* __restrict__ dskip, const float* __restrict__ dyp,
    const unsigned char* __restrict__ idx, const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ dz, float* partial, int B, int H,
    int W, int Ho, int Wo, int C, int Cs) {
  column_reduce_init<2>(B * H * W, Cs >> 2, Cs, partial, [&](int q) { return chan_coef(q, C, mean, invstd, gamma, beta); },
                        [&](int r, int q, const ChanCoef& k, f32x4* acc) {
                          const f32x4 g = pool3s2_gather(dskip, dyp, idx, r, q, H, W, Ho, Wo, Cs);
                          const size_t off = (size_t)r * Cs + (size_t)q * 4;
                          const f32x4 xh = (*reinterpret_cast<const f32x4*>(x + off) - k.mean) * k.invstd;
                          f32x4 d;
#pragma unroll
                          for (int e = 0; e < 4; ++e) d[e] = k.valid[e] * g[e] * act_grad(k.gamma[e] * xh[e] + k.beta[e], ACT);
                          *reinterpret_cast<f32x4*>(dz + off) = d;
                          acc[0] += d;
                          acc[1] += d * xh;
                        });
}

// plain form (no BatchNorm): dx = g * act'(x)
template <int ACT>
__global__ __launch_bounds__(RED_THREADS) void pool3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dskip,
                                                                  const float* __restrict__ dyp,
                                                                  const unsigned char* __restrict__ idx,
                                                                  float* __restrict__ dx, int B, int H, int W, int Ho, int Wo,
                                                                  int C, int Cs) {
  column_sweep(B * H * W, Cs >> 2, [&](int q) { return chan_coef(q, C, nullptr, nullptr, nullptr, nullptr); },
               [&](int r, int q, const ChanCoef& k) {
                 const f32x4 g = pool3s2_gather(dskip, dyp, idx, r, q, H, W, Ho, Wo, Cs);
                 const size_t off = (size_t)r * Cs + (size_t)q * 4;
                 const f32x4 xv = *reinterpret_cast<const f32x4*>(x + off);
                 f32x4 d;
#pragma unroll
                 for (int e = 0; e < 4; ++e) d[e] = k.valid[e] * g[e] * act_grad(xv[e], ACT);
                 *reinterpret_cast<f32x4*>(dx + off) = d;
               });
}

static bool pool3s2_args(int B, int H, int W, int C, int Cs) {
  return B > 0 && H > 0 && W > 0 && C > 0 && C <= Cs && !(Cs & 3) && (long long)B * H * W * Cs <= 0x7fffffffLL;
}

extern "C" int vmtl_bn_act_pool3s2_fwd(const float* x, const float* mean, const float* invstd, const float* gamma,
                                       const float* beta, float* a_out, float* y, unsigned char* idx, int B, int H, int W,
                                       int C, int Cs, int act, void* stream) {
  VMTL_ENTER();
  if (!x || !y || !idx || !pool3s2_args(B, H, W, C, Cs) || ((mean == nullptr) != (invstd == nullptr))) return VMTL_ERR_ARG;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int nb = sweep_blocks((long long)B * Ho * Wo, Cs);
  hipStream_t st = (hipStream_t)stream;
#define CALL(A)                                                                                                         \
  hipLaunchKernelGGL((bn_act_pool3s2_fwd_kernel<A>), dim3(nb), dim3(RED_THREADS), 0, st, x, mean, invstd, gamma, beta, \
                     a_out, y, idx, B, H, W, Ho, Wo, C, Cs)
  RES_ACT_SWITCH(act, CALL)
#undef CALL
  return vmtl_check_launch();
}

extern "C" int vmtl_bn_act_pool3s2_bwd(const float* x, const float* dskip, const float* dyp, const unsigned char* idx,
                                       const float* mean, const float* invstd, const float* gamma, const float* beta,
                                       float* dz, float* partial, float* sum_dz, float* sum_dzx, float* dx, int B, int H,
                                       int W, int C, int Cs, int act, int training, void* stream) {
  VMTL_ENTER();
  if (!x || !dyp || !idx || !dx || !pool3s2_args(B, H, W, C, Cs) || ((mean == nullptr) != (invstd == nullptr)))
    return VMTL_ERR_ARG;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int M = B * H * W;
  hipStream_t st = (hipStream_t)stream;
  if (mean == nullptr) {
    const int nb = sweep_blocks(M, Cs);
#define CALL(A)                                                                                                       \
  hipLaunchKernelGGL((pool3s2_bwd_kernel<A>), dim3(nb), dim3(RED_THREADS), 0, st, x, dskip, dyp, idx, dx, B, H, W, Ho, \
                     Wo, C, Cs)
    RES_ACT_SWITCH(act, CALL)
#undef CALL
    return vmtl_check_launch();
  }
  if (!dz || !partial || !sum_dz || !sum_dzx) return VMTL_ERR_ARG;
  const int nblk = red_blocks(M);
#define CALL(A)                                                                                                          \
  hipLaunchKernelGGL((bn_pool3s2_bwd_reduce_kernel<A>), dim3(nblk), dim3(RED_THREADS), 0, st, x, dskip, dyp, idx, mean, \
                     invstd, gamma, beta, dz, partial, B, H, W, Ho, Wo, C, Cs)
  RES_ACT_SWITCH(act, CALL)
#undef CALL
  int rc = vmtl_check_launch();
  if (rc != 0) return rc;
  rc = vmtl_bn_bwd_finalize(partial, nblk, M, C, Cs, sum_dz, sum_dzx, nullptr, nullptr, nullptr, training, nullptr,
                            nullptr, nullptr, stream);
  if (rc != 0) return rc;
  return vmtl_bn_bwd_apply(x, dz, mean, invstd, gamma, sum_dz, sum_dzx, dx, M, C, Cs, training, stream);
}

// ---------------------------------------------------------------- 3. residual close act(BN_a(z) + r)
// r = res (identity branch) or BN_b(zd) (downsample branch: res == nullptr, zd != nullptr)
template <int ACT>
__global__ __launch_bounds__(RED_THREADS) void bn_add_act_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ mean_a, const float* __restrict__ invstd_a,
    const float* __restrict__ gamma_a, const float* __restrict__ beta_a, const float* __restrict__ res,
    const float* __restrict__ zd, const float* __restrict__ mean_b, const float* __restrict__ invstd_b,
    const float* __restrict__ gamma_b, const float* __restrict__ beta_b, float* __restrict__ y, int M, int C, int Cs) {
  struct K2 { ChanCoef a, b; };
  column_sweep(M, Cs >> 2,
               [&](int q) {
                 K2 k;
                 k.a = chan_coef(q, C, mean_a, invstd_a, gamma_a, beta_a);
                 k.b = chan_coef(q, C, mean_b, invstd_b, gamma_b, beta_b);
                 return k;
               },
               [&](int r, int q, const K2& k) {
                 const size_t off = (size_t)r * Cs + (size_t)q * 4;
                 const f32x4 zv = *reinterpret_cast<const f32x4*>(z + off);
                 f32x4 rv;
                 if (res != nullptr) {
                   rv = *reinterpret_cast<const f32x4*>(res + off);
                 } else {
                   const f32x4 dv = *reinterpret_cast<const f32x4*>(zd + off);
                   rv = k.b.gamma * ((dv - k.b.mean) * k.b.invstd) + k.b.beta;
                 }
                 const f32x4 pre = k.a.gamma * ((zv - k.a.mean) * k.a.invstd) + k.a.beta + rv;
                 f32x4 o;
#pragma unroll
                 for (int e = 0; e < 4; ++e) o[e] = k.a.valid[e] != 0.f ? act_fwd(pre[e], ACT) : 0.f;
                 *reinterpret_cast<f32x4*>(y + off) = o;
               });
}

// g = dy * act'(pre) (the gradient of the residual operand and of both BatchNorm outputs) and the partial rows
// [nblk][3][Cs] = (sum g, sum g*xhat_a, sum g*xhat_b)
template <int ACT>
__global__ __launch_bounds__(RED_THREADS) void bn_add_act_bwd_reduce_kernel(
    const float* __restrict__ z, const float* __restrict__ mean_a, const float* __restrict__ invstd_a,
    const float* __restrict__ gamma_a, const float* __restrict__ beta_a, const float* __restrict__ res,
    const float* __restrict__ zd, const float* __restrict__ mean_b, const float* __restrict__ invstd_b,
    const float* __restrict__ gamma_b, const float* __restrict__ beta_b, const float* __restrict__ dy,
    float* __restrict__ g, float* partial, int M, int C, int Cs) {
  struct K2 { ChanCoef a, b; };
  column_reduce_init<3>(M, Cs >> 2, Cs, partial,
                        [&](int q) {
                          K2 k;
                          k.a = chan_coef(q, C, mean_a, invstd_a, gamma_a, beta_a);
                          k.b = chan_coef(q, C, mean_b, invstd_b, gamma_b, beta_b);
                          return k;
                        },
                        [&](int r, int q, const K2& k, f32x4* acc) {
                          const size_t off = (size_t)r * Cs + (size_t)q * 4;
                          const f32x4 xa = (*reinterpret_cast<const f32x4*>(z + off) - k.a.mean) * k.a.invstd;
                          f32x4 rv, xb = (f32x4){0.f, 0.f, 0.f, 0.f};
                          if (res != nullptr) {
                            rv = *reinterpret_cast<const f32x4*>(res + off);
                          } else {
                            xb = (*reinterpret_cast<const f32x4*>(zd + off) - k.b.mean) * k.b.invstd;
                            rv = k.b.gamma * xb + k.b.beta;
                          }
                          const f32x4 pre = k.a.gamma * xa + k.a.beta + rv;
                          const f32x4 d = *reinterpret_cast<const f32x4*>(dy + off);
                          f32x4 gv;
#pragma unroll
                          for (int e = 0; e < 4; ++e) gv[e] = k.a.valid[e] * d[e] * act_grad(pre[e], ACT);
                          *reinterpret_cast<f32x4*>(g + off) = gv;
                          acc[0] += gv;
                          acc[1] += gv * xa;
                          acc[2] += gv * xb;
                        });
}

// one workgroup per channel: fp64 sums of the partial rows in a fixed order; exactly C entries of each output
__global__ __launch_bounds__(256) void bn_add_act_finalize_kernel(const float* __restrict__ partial, int nblk, int Cs,
                                                                  float* sum_dz_a, float* sum_dzx_a, float* sum_dz_b,
                                                                  float* sum_dzx_b) {
  __shared__ double sh[4];
  const int c = blockIdx.x;
  const double s0 = block_rows_sum(partial, nblk, 3, 0, Cs, c, sh);
  const double s1 = block_rows_sum(partial, nblk, 3, 1, Cs, c, sh);
  const double s2 = sum_dz_b != nullptr ? block_rows_sum(partial, nblk, 3, 2, Cs, c, sh) : 0.0;
  if (threadIdx.x != 0) return;
  sum_dz_a[c] = (float)s0;
  sum_dzx_a[c] = (float)s1;
  if (sum_dz_b != nullptr) {
    sum_dz_b[c] = (float)s0;
    sum_dzx_b[c] = (float)s2;
  }
}

static bool add_act_args(const float* z, const float* mean_a, const float* invstd_a, const float* res, const float* zd,
                         const float* mean_b, const float* invstd_b, int M, int C, int Cs) {
  if (!z || !mean_a || !invstd_a || M <= 0 || C <= 0 || C > Cs || (Cs & 3)) return false;
  if ((long long)M * Cs > 0x7fffffffLL) return false;
  if ((res == nullptr) == (zd == nullptr)) return false;  // exactly one residual form
  if (zd != nullptr && (!mean_b || !invstd_b)) return false;
  return true;
}

extern "C" int vmtl_bn_add_act_fwd(const float* z, const float* mean_a, const float* invstd_a, const float* gamma_a,
                                   const float* beta_a, const float* res, const float* zd, const float* mean_b,
                                   const float* invstd_b, const float* gamma_b, const float* beta_b, float* y, int M, int C,
                                   int Cs, int act, void* stream) {
  VMTL_ENTER();
  if (!y || !add_act_args(z, mean_a, invstd_a, res, zd, mean_b, invstd_b, M, C, Cs)) return VMTL_ERR_ARG;
  const int nb = sweep_blocks(M, Cs);
  hipStream_t st = (hipStream_t)stream;
#define CALL(A)                                                                                                            \
  hipLaunchKernelGGL((bn_add_act_fwd_kernel<A>), dim3(nb), dim3(RED_THREADS), 0, st, z, mean_a, invstd_a, gamma_a, beta_a, \
                     res, zd, mean_b, invstd_b, gamma_b, beta_b, y, M, C, Cs)
  RES_ACT_SWITCH(act, CALL)
#undef CALL
  return vmtl_check_launch();
}

extern "C" int vmtl_bn_add_act_bwd(const float* z, const float* mean_a, const float* invstd_a, const float* gamma_a,
                                   const float* beta_a, const float* res, const float* zd, const float* mean_b,
                                   const float* invstd_b, const float* gamma_b, const float* beta_b, const float* dy,
                                   float* g, float* partial, float* sum_dz_a, float* sum_dzx_a, float* sum_dz_b,
                                   float* sum_dzx_b, float* dz, float* dzd, int M, int C, int Cs, int act, int training,
                                   void* stream) {
  VMTL_ENTER();
  if (!dy || !g || !partial || !sum_dz_a || !sum_dzx_a ||
      !add_act_args(z, mean_a, invstd_a, res, zd, mean_b, invstd_b, M, C, Cs))
    return VMTL_ERR_ARG;
  if (zd != nullptr && (!sum_dz_b || !sum_dzx_b)) return VMTL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = red_blocks(M);
#define CALL(A)                                                                                                          \
  hipLaunchKernelGGL((bn_add_act_bwd_reduce_kernel<A>), dim3(nblk), dim3(RED_THREADS), 0, st, z, mean_a, invstd_a,      \
                     gamma_a, beta_a, res, zd, mean_b, invstd_b, gamma_b, beta_b, dy, g, partial, M, C, Cs)
  RES_ACT_SWITCH(act, CALL)
#undef CALL
  hipLaunchKernelGGL(bn_add_act_finalize_kernel, dim3(C), dim3(256), 0, st, partial, nblk, Cs, sum_dz_a, sum_dzx_a,
                     zd != nullptr ? sum_dz_b : nullptr, sum_dzx_b);
  int rc = vmtl_check_launch();
  if (rc != 0) return rc;
  if (dz != nullptr) {
    rc = vmtl_bn_bwd_apply(z, g, mean_a, invstd_a, gamma_a, sum_dz_a, sum_dzx_a, dz, M, C, Cs, training, stream);
    if (rc != 0) return rc;
  }
  if (zd != nullptr && dzd != nullptr)
    rc = vmtl_bn_bwd_apply(zd, g, mean_b, invstd_b, gamma_b, sum_dz_b, sum_dzx_b, dzd, M, C, Cs, training, stream);
  return rc;
}
