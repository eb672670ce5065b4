// Cross entropy plus a Dice / Jaccard / Tversky region-overlap term for the segmentation criterion, forward and backward
// (DESIGN.md section 24).  No reference call site: segmentation_models_pytorch's DiceLoss / JaccardLoss / TverskyLoss
// in their multiclass form, fused with the weighted / ignoring cross entropy (loss.hip's, restated here on the shared
// pixel pass of ce_pixel.h).
//
// Semantics.  Logits z (B,C,H,W), int64 target t, optional class weights w (cross entropy only), optional ignore index:
//   valid    : t_i != ignore_index; every sum runs over the valid pixels of the whole batch.  p_ic = softmax(z_i)_c.
//   TP_c     = sum p_ic 1[t_i = c],  S_c = sum p_ic,  N_c = #{i valid : t_i = c} (an integer, exact).
//   D_c      = TP_c + alpha (S_c - TP_c) + beta (N_c - TP_c) + smooth,   T_c = (TP_c + smooth) / D_c
//   L_region = (1/C) sum_{c : N_c > 0} (1 - T_c)     (an absent class adds 0; the mean is over C).  alpha = beta = 0.5 is
//              Dice, alpha = beta = 1 Jaccard.  For a present class D_c >= min(1, beta) N_c > 0: nothing is clamped.
//   loss     = ce_weight CE + region_weight L_region, CE = sum_valid w[t] nll / sum_valid w[t] as vmtl_ce_fwd_ex.
//              ce_weight == 0: the cross entropy is neither evaluated nor differentiated.
//   gradient : dL_region/dp_ic = b_c + a_c 1[t_i = c] on valid pixels, m_c = [N_c > 0],
//                b_c = m_c alpha (TP_c + smooth) / (C D_c^2),
//                a_c = -m_c (1/D_c - (1 - alpha - beta)(TP_c + smooth) / D_c^2) / C,
//              and through the softmax dz_ic = p_ic (g_ic - sum_k p_ik g_ik).
//   A valid pixel whose label is outside [0, C) makes the loss, both terms and the whole coefficient table NaN.  With
//   every pixel ignored L_region is exactly 0 and CE is NaN (0/0).
//
// Forward, two launches.  The pixel pass reads each logit once (held in registers, C <= 32), keeps S_c and TP_c in
// per-thread registers (the class match is a select), counts N_c, V and the bad labels as integers in LDS, and leaves
// one row of per-block partials: fp64 sums reduced over the wave in wave_sum's xor-tree order (the 2 * 4Q class sums by
// cr_wave_spread_sum, which spends a sixth of the shuffles: the first version, wave_sum per value, took 53.5 us against
// 46.1 at 32x19x128x256) and over the waves pairwise, as block_sum_n adds them, integers exact.
// The finalize workgroup sums the rows column by column in a fixed order, forms T_c, a_c, b_c,
// the terms, stats and the loss in fp64 and rounds each to fp32 once.  No atomics on global memory at all (so nothing
// to clear), no allocation, no sync; the grid depends on the shape only: bit-identical run to run, and it captures.
// The backward recomputes the softmax as every criterion of ce_pixel.h does and writes, in the three layouts of
// ce_grad_layout and exactly their lanes,
//   dz_c = grad_out [ce_weight w[t] (p_c - 1[c = t]) / stats[0] + region_weight p_c (g_c - sum_k p_k g_k)],
// +0.0f in every written lane of an ignored pixel.
#include "../../include/vmtl.h"
#include "ce_pixel.h"
#include "reduce.h"

// Forward: 512 blocks of 512 threads at most.  Measured at 32x19x128x256 / 16x14x256x256 (us per forward): 1024 x 256
// threads 46.1 / 44.6, 512 x 256 46.3 / 42.2, 256 x 256 53.9 / 46.8, 512 x 512 42.6 / 42.5, 256 x 512 44.2 / 40.2, and
// 2048 x 256 56.0 / 58.1: the single finalize workgroup pulls every row through one compute unit, so rows cost time
// there, while the pixel pass wants at least four waves per SIMD in flight.
#define CR_THREADS 512
#define CR_BLOCKS_MAX 512
#define CR_BWD_THREADS 256
#define CR_FIN_THREADS 1024
#define CR_MAXC VMTL_CE_REGION_MAX_CLASSES
static_assert(CR_MAXC == 32, "the register forms hold 4 * Q <= 32 logits");

// One row of the workspace per block of the pixel pass, 8 bytes per column:
//   doubles [0] sum w nll  [1] sum w  [2 .. 2+C) S_c  [2+C .. 2+2C) TP_c;  uint64 [2+2C .. 2+3C) N_c  [2+3C] V  [3+3C] bad
#define CR_COLS(C) (3 * (C) + 4)
static inline int cr_blocks(long long P) { return grid_1d(P, CR_THREADS, CR_BLOCKS_MAX); }

// The wave's sums of NP (a power of two, 8 .. 64) per-lane values in NP - 1 + log2(64 / NP) shuffles instead of 6 * NP:
// at the step with xor mask m (32, 16, ..) a lane keeps the half of its values that its lane bit m selects and adds the
// partner's copy of that half, so the values a lane carries halve until one is left - value number lane >> log2(64 / NP)
// - and the remaining masks are plain xor steps.  Every total is the xor tree 32, 16, .., 1 over the lanes, as
// wave_sum's: a fixed association.  The first step shuffles the fp32 values and adds them in fp64.
template <int NP>
__device__ __forceinline__ double cr_wave_spread_sum(const float (&f)[NP], int lane) {
  constexpr int H = NP / 2;
  double d[H];
  {
    const bool up = (lane & 32) != 0;
#pragma unroll
    for (int j = 0; j < H; ++j) {
      const float keep = up ? f[j + H] : f[j], send = up ? f[j] : f[j + H];
      d[j] = (double)keep + (double)__shfl_xor(send, 32, 64);
    }
  }
  int m = 16;
#pragma unroll
  for (int n = H; n > 1; n >>= 1, m >>= 1) {
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int j = 0; j < n / 2; ++j) {
      const double keep = up ? d[j + n / 2] : d[j], send = up ? d[j] : d[j + n / 2];
      d[j] = keep + __shfl_xor(send, m, 64);
    }
  }
  for (; m > 0; m >>= 1) d[0] += __shfl_xor(d[0], m, 64);
  return d[0];
}

// ------------------------------------------------------------------ forward: pixel pass
// One thread per pixel, the pixel pass of ce_pixel.h in its register form (4*Q >= C logits).  The argmax is written for
// ignored pixels too.  ce_on == 0: no nll, no weight read.
template <int Q>
__global__ __launch_bounds__(CR_THREADS) void cr_pixel_kernel(const float* __restrict__ z,
                                                              const long long* __restrict__ tgt,
                                                              const float* __restrict__ weight, long long ignore,
                                                              int ce_on, double* __restrict__ ws,
                                                              long long* __restrict__ amax, long long P, int HW, int C,
                                                              long long sb, long long sc, long long sp) {
  __shared__ double shd[CR_THREADS / 64][2 + 8 * Q];
  __shared__ unsigned cnt[4 * Q + 2];  // N_c, V at [4Q], bad labels at [4Q + 1]: at most P < 2^31 each
  for (int j = threadIdx.x; j < 4 * Q + 2; j += CR_THREADS) cnt[j] = 0u;
  __syncthreads();
  float S[4 * Q], TP[4 * Q];
#pragma unroll
  for (int c = 0; c < 4 * Q; ++c) S[c] = TP[c] = 0.f;
  double num = 0.0, den = 0.0;
  unsigned nv = 0;
  VMTL_GRID_STRIDE(i, P) {
    float v[4 * Q];
    ce_load<Q>(v, ce_pixel(z, i, HW, sb, sp), C, sc);
    const long long t = tgt[i];
    const CeMax mx = ce_max_argmax<Q>(v, C);
    const float m = mx.m;
    if (amax != nullptr) amax[i] = mx.am;
    if (t == ignore) continue;
    const bool inside = ce_label_inside(t, C);
    const float zt = ce_pick<Q>(v, t), s = ce_exp_sum<Q>(v, C, m);
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < 4 * Q; ++c) {
      const float p = v[c] * inv;
      S[c] += p;
      TP[c] += c == t ? p : 0.f;
    }
    ++nv;
    atomicAdd(&cnt[inside ? (int)t : 4 * Q + 1], 1u);
    if (ce_on) {
      if (inside) {
        const float wt = weight != nullptr ? weight[t] : 1.f;
        num += (double)wt * (double)(logf(s) - (zt - m));
        den += (double)wt;
      } else {
        num += (double)ce_nan();  // the rule for labels (ce_pixel.h)
      }
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  nv = wave_sum(nv);
  if (lane == 0 && nv != 0u) atomicAdd(&cnt[4 * Q], nv);
  num = wave_sum(num);
  den = wave_sum(den);
  if (lane == 0) {
    shd[wave][0] = num;
    shd[wave][1] = den;
  }
  {  // S_0 .. S_{4Q-1}, TP_0 .. TP_{4Q-1}, zeros up to a power of two: value j ends up in lane j << SH
    constexpr int NP = Q <= 1 ? 8 : (Q <= 2 ? 16 : (Q <= 4 ? 32 : 64)), SH = NP == 8 ? 3 : (NP == 16 ? 2 : (NP == 32 ? 1 : 0));
    float f[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) f[j] = j < 4 * Q ? S[j < 4 * Q ? j : 0] : (j < 8 * Q ? TP[j < 8 * Q ? j - 4 * Q : 0] : 0.f);
    const double tot = cr_wave_spread_sum<NP>(f, lane);
    const int idx = lane >> SH;
    if ((lane & ((1 << SH) - 1)) == 0 && idx < 8 * Q) shd[wave][2 + idx] = tot;
  }
  __syncthreads();
  double* row = ws + (long long)blockIdx.x * CR_COLS(C);
  const int k = threadIdx.x;
  if (k < 2 + 2 * C) {  // the waves' totals pairwise: ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7))
    const int j = k < 2 ? k : (k < 2 + C ? k : 2 + 4 * Q + (k - 2 - C));
    double t[CR_THREADS / 64];
#pragma unroll
    for (int w = 0; w < CR_THREADS / 64; ++w) t[w] = shd[w][j];
#pragma unroll
    for (int st = 1; st < CR_THREADS / 64; st <<= 1) {
#pragma unroll
      for (int w = 0; w < CR_THREADS / 64; w += 2 * st) t[w] += t[w + st];
    }
    row[k] = t[0];
  } else if (k < 4 + 3 * C) {
    const int j = k - 2 - 2 * C;  // N_0 .. N_{C-1}, V, bad
    reinterpret_cast<unsigned long long*>(row)[k] = (unsigned long long)cnt[j < C ? j : 4 * Q + (j - C)];
  }
}

// ------------------------------------------------------------------ forward: finalize
// Thread (column, row group) sums its rows top-down, the row groups of a column are added in their order: one fixed
// association per column.  Then thread c forms class c's T_c, a_c, b_c and thread 0 adds the C terms in class order.
__global__ __launch_bounds__(CR_FIN_THREADS) void cr_finalize_kernel(const double* __restrict__ ws, int nblk, int C,
                                                                     float alpha, float beta, float smooth,
                                                                     float ce_weight, float region_weight,
                                                                     float* __restrict__ loss, float* __restrict__ terms,
                                                                     float* __restrict__ stats, float* __restrict__ coef,
                                                                     long long* __restrict__ counts) {
  __shared__ unsigned long long red[CR_FIN_THREADS];
  __shared__ unsigned long long tot[3 * CR_MAXC + 4];
  __shared__ double term[CR_MAXC];
  const int ncol = CR_COLS(C), rpt = CR_FIN_THREADS / ncol;
  const int col = threadIdx.x % ncol, ro = threadIdx.x / ncol;
  const bool isint = col >= 2 + 2 * C;
  const unsigned long long* wsi = reinterpret_cast<const unsigned long long*>(ws);
  double ds = 0.0;
  unsigned long long is = 0;
  if (ro < rpt) {
#pragma unroll 8
    for (int r = ro; r < nblk; r += rpt) {
      const unsigned long long bits = wsi[(long long)r * ncol + col];
      if (isint) is += bits;
      else ds += __longlong_as_double((long long)bits);
    }
  }
  red[threadIdx.x] = isint ? is : (unsigned long long)__double_as_longlong(ds);
  __syncthreads();
  if (threadIdx.x < ncol) {
    if (isint) {
      unsigned long long s = red[col];
      for (int j = 1; j < rpt; ++j) s += red[col + j * ncol];
      tot[col] = s;
    } else {
      double s = __longlong_as_double((long long)red[col]);
      for (int j = 1; j < rpt; ++j) s += __longlong_as_double((long long)red[col + j * ncol]);
      tot[col] = (unsigned long long)__double_as_longlong(s);
    }
  }
  __syncthreads();
  const bool bad = tot[3 + 3 * C] != 0ull;
  const double nan = (double)ce_nan();
  if (threadIdx.x < C) {
    const int c = threadIdx.x;
    const double Sc = __longlong_as_double((long long)tot[2 + c]), TPc = __longlong_as_double((long long)tot[2 + C + c]);
    const unsigned long long Nc = tot[2 + 2 * C + c];
    const double al = (double)alpha, be = (double)beta, tps = TPc + (double)smooth;
    const double D = TPc + al * (Sc - TPc) + be * ((double)Nc - TPc) + (double)smooth;
    const bool present = Nc != 0ull;  // a select, never a product with 1/D of an absent class
    double a = present ? -(1.0 / D - (1.0 - al - be) * tps / (D * D)) / (double)C : 0.0;
    double b = present ? al * tps / ((double)C * D * D) : 0.0;
    term[c] = present ? 1.0 - tps / D : 0.0;
    if (bad) a = b = nan;
    coef[c] = (float)a;
    coef[C + c] = (float)b;
    counts[c] = (long long)Nc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double lr = 0.0;
    for (int c = 0; c < C; ++c) lr += term[c];
    lr = bad ? nan : lr / (double)C;
    const double num = __longlong_as_double((long long)tot[0]), den = __longlong_as_double((long long)tot[1]);
    const bool ce_on = ce_weight != 0.f;
    const double ce = ce_on ? num / den : 0.0;  // NaN (0/0) when every pixel is ignored, as vmtl_ce_fwd_ex
    terms[0] = (float)ce;
    terms[1] = (float)lr;
    stats[0] = (float)den;
    stats[1] = (float)num;
    loss[0] = (float)(ce_on ? (double)ce_weight * ce + (double)region_weight * lr : (double)region_weight * lr);
    counts[C] = (long long)tot[2 + 3 * C];
  }
}

// ------------------------------------------------------------------ backward
// The gradient policy (ce_pixel.h): b_c in registers, a_t from LDS, and the cross entropy's k as a linear policy forms
// it.  The term needs the pixel's whole softmax (the dot), so it has no per-lane form: the rows layout is the shared
// ce_grad_rows_kernel, and the two other layouts are the one-thread-per-pixel kernel below instead of the sweep kernels.
// An ignored pixel is skipped with a branch.
// One lane: the cross entropy's product and the region term's, each rounded, then their sum, then bad.  Stated with
// contraction off: fused, the compiler would pick the product a multiply-add swallows, and with it the last bit.
__device__ __forceinline__ float cr_lane(float p, float hit, float k, float grg, float g, float dot, float bad) {
#pragma clang fp contract(off)
  const float ce = (p - hit) * k, rg = (grg * p) * (g - dot);
  return (ce + rg) + bad;
}

struct CrGrad {
  const float* __restrict__ weight;
  long long ignore;
  const float* __restrict__ stats;
  const float* __restrict__ coef;
  float ce_weight, region_weight;

  struct Px {
    bool zero, inside;
  };
  template <int Q>
  struct Wg {
    const float* __restrict__ weight;
    long long ignore;
    const float* sa;  // a_c, in LDS
    float cb[4 * Q];  // b_c
    float gce, grg;
    __device__ __forceinline__ Px pixel(long long, long long t, int C) const { return {t == ignore, ce_label_inside(t, C)}; }
    template <int, class Put>
    __device__ __forceinline__ void lanes(const Px& px, float (&v)[4 * Q], float inv, long long t, int C, Put put) const {
      const float bad = px.inside ? 0.f : ce_nan();  // the rule for labels: such a label never indexes w or the table
      const float at = px.inside ? sa[t] : 0.f;
      const float k = (px.inside && weight != nullptr) ? weight[t] * gce : gce;
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < 4 * Q; ++c) {
        v[c] *= inv;
        dot += v[c] * (cb[c] + (c == t ? at : 0.f));
      }
      float o[4 * Q];
#pragma unroll
      for (int c = 0; c < 4 * Q; ++c) {
        const float hit = c == t ? 1.f : 0.f;
        o[c] = c < C ? cr_lane(v[c], hit, k, grg, cb[c] + hit * at, dot, bad) : 0.f;
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) put(q, (f32x4){o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]});
    }
  };
  template <int Q>
  __device__ __forceinline__ Wg<Q> begin(const float* __restrict__ gout, long long, int C) const {
    __shared__ float sa[4 * Q];
    Wg<Q> wg;
    wg.weight = weight;
    wg.ignore = ignore;
    wg.sa = sa;
    if (threadIdx.x < 4 * Q) sa[threadIdx.x] = threadIdx.x < C ? coef[threadIdx.x] : 0.f;
#pragma unroll
    for (int c = 0; c < 4 * Q; ++c) wg.cb[c] = c < C ? coef[C + c] : 0.f;
    // the cross entropy's unit as the weighted / ignoring policy's; a select when it is off (stats[0] is then 0)
    wg.gce = ce_weight != 0.f ? gout[0] * ce_weight / stats[0] : 0.f;
    wg.grg = gout[0] * region_weight;
    __syncthreads();
    return wg;
  }
};

// One thread per pixel, logits in registers.  WIDE: NHWC rows of ld > 4*Q floats, of which the first ceil4(C) are
// written (Q quad stores per pixel); otherwise generic strides, C lanes per pixel.
template <int Q, bool WIDE>
__global__ __launch_bounds__(CR_BWD_THREADS) void cr_bwd_kernel(const float* __restrict__ z,
                                                                const long long* __restrict__ tgt,
                                                                const float* __restrict__ gout, float* __restrict__ dz,
                                                                long long P, int HW, int C, long long sb, long long sc,
                                                                long long sp, long long dsb, long long dsc, long long dsp,
                                                                CrGrad pol) {
  const auto wg = pol.template begin<Q>(gout, P, C);
  VMTL_GRID_STRIDE(i, P) {
    ce_grad_pixel<Q>(wg, z, tgt, i, HW, C, sb, sc, sp, [&](int q, f32x4 o) {
      if constexpr (WIDE) {
        reinterpret_cast<f32x4*>(dz + i * dsp)[q] = o;
      } else {
        float* out = ce_pixel(dz, i, HW, dsb, dsp);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * q + j < C) out[(4 * q + j) * dsc] = o[j];
      }
    });
  }
}

// ------------------------------------------------------------------ entry points
static inline bool cr_classes_ok(int C) { return C >= 2 && C <= CR_MAXC; }
static inline bool cr_finite(float v) { return v - v == 0.f; }

// one row of CR_COLS(C) 8-byte columns per block of the pixel pass; 0 for a class count the kernels do not take
extern "C" long long vmtl_ce_region_workspace_bytes(long long P, int C) {
  if (!cr_classes_ok(C) || P <= 0) return 0;
  return (long long)cr_blocks(P) * CR_COLS(C) * (long long)sizeof(double);
}

extern "C" int vmtl_ce_region_fwd(const float* logits, const long long* target, const float* weight,
                                  long long ignore_index, float alpha, float beta, float smooth, float ce_weight,
                                  float region_weight, float* loss, float* terms, float* stats, float* coef,
                                  long long* counts, void* workspace, long long* argmax, int B, int HW, int C,
                                  long long sb, long long sc, long long sp, void* stream) {
  VMTL_ENTER();
  if (!logits || !target || !loss || !terms || !stats || !coef || !counts || !workspace || B <= 0 || HW <= 0 || C <= 0 ||
      !cr_finite(alpha) || !(alpha > 0.f) || !cr_finite(beta) || !(beta > 0.f) || !cr_finite(smooth) ||
      !(smooth >= 0.f) || !cr_finite(ce_weight) || !(ce_weight >= 0.f) || !cr_finite(region_weight) ||
      !(region_weight > 0.f))
    return VMTL_ERR_ARG;
  const long long P = (long long)B * HW;
  if (!cr_classes_ok(C) || P >= (1LL << 31)) return VMTL_ERR_UNSUPPORTED;  // register form; 32-bit block counters
  hipStream_t st = (hipStream_t)stream;
  const int nblk = cr_blocks(P);
  double* ws = (double*)workspace;
  auto pixel = [&](auto q) {
    hipLaunchKernelGGL((cr_pixel_kernel<decltype(q)::value>), dim3(nblk), dim3(CR_THREADS), 0, st, logits, target, weight,
                       ignore_index, ce_weight != 0.f ? 1 : 0, ws, argmax, P, HW, C, sb, sc, sp);
  };
  ce_dispatch_q((C + 3) >> 2, pixel, [&] { pixel(std::integral_constant<int, 8>{}); });
  hipLaunchKernelGGL(cr_finalize_kernel, dim3(1), dim3(CR_FIN_THREADS), 0, st, (const double*)ws, nblk, C, alpha, beta,
                     smooth, ce_weight, region_weight, loss, terms, stats, coef, counts);
  return vmtl_check_launch();
}

extern "C" int vmtl_ce_region_bwd(const float* logits, const long long* target, const float* weight,
                                  long long ignore_index, const float* stats, const float* coef, const float* grad_out,
                                  float ce_weight, float region_weight, float* dlogits, int B, int HW, int C,
                                  long long sb, long long sc, long long sp, long long dsb, long long dsc, long long dsp,
                                  void* stream) {
  VMTL_ENTER();
  if (!logits || !target || !stats || !coef || !grad_out || !dlogits || B <= 0 || HW <= 0 || C <= 0 ||
      !cr_finite(ce_weight) || !(ce_weight >= 0.f) || !cr_finite(region_weight) || !(region_weight > 0.f))
    return VMTL_ERR_ARG;
  if (!cr_classes_ok(C)) return VMTL_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const long long P = (long long)B * HW;
  const CrGrad pol = {weight, ignore_index, stats, coef, ce_weight, region_weight};
  const CeGradLayout layout = ce_grad_layout(C, HW, dsb, dsc, dsp);
  if (layout == CE_GRAD_ROWS) {
    ce_grad_rows_launch(logits, target, grad_out, dlogits, pol, P, HW, C, sb, sc, sp, st);
  } else {
    const int nb = grid_1d(P, CR_BWD_THREADS, 8192);
    ce_dispatch_q((C + 3) >> 2,
                  [&](auto q) {
                    constexpr int Q = decltype(q)::value;
                    if (layout == CE_GRAD_WIDE)
                      hipLaunchKernelGGL((cr_bwd_kernel<Q, true>), dim3(nb), dim3(CR_BWD_THREADS), 0, st, logits, target,
                                         grad_out, dlogits, P, HW, C, sb, sc, sp, dsb, dsc, dsp, pol);
                    else
                      hipLaunchKernelGGL((cr_bwd_kernel<Q, false>), dim3(nb), dim3(CR_BWD_THREADS), 0, st, logits, target,
                                         grad_out, dlogits, P, HW, C, sb, sc, sp, dsb, dsc, dsp, pol);
                  },
                  [] {});
  }
  return vmtl_check_launch();
}
