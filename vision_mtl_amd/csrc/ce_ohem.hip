// Online hard example mining (OHEM, "bootstrapped" cross entropy) for the segmentation criterion, forward and backward.
//
// Semantics.  Logits z (B,C,H,W), int64 target t, optional class weights w, optional ignore index:
//   valid   : t_i != ignore_index; V = number of valid pixels.
//   nll_i   : -log softmax(z_i)[t_i], UNWEIGHTED - the ranking key (mmseg's OHEMPixelSampler ranks by probability).
//             Evaluated as (max_c z - z_t) + log(sum_c exp(z_c - max_c z)): >= +0.0f by construction, clamped to +0.0f
//             anyway.  A valid pixel whose label is outside [0, C), or whose logits are not all finite, has nll = NaN:
//             it ranks as the hardest, is kept, and makes the loss NaN (as the *_ex kernels fail a bad label visibly).
//   K       : min(min_kept_total, V); the host passes min_kept * B, the device clamps it to V.
//   tau     : -log(thresh), a float >= +0.0f from the host; +inf is pure top-K.
//   kappa   : the K-th largest nll among the valid pixels (NaN ranks above +inf).  cut = min(tau, kappa); when kappa is
//             NaN (K or more NaN pixels) or K = 0, cut = tau.
//   kept    : valid and not (nll_i < cut).  Every tie at the cut is kept, at least K pixels are kept, the set does not
//             depend on the order of the pixels, and a NaN pixel stays in.
//   loss    : sum_kept w[t] nll / sum_kept w[t] (w = 1 without weights); NaN (0/0) when V = 0, as vmtl_ce_fwd_ex.
//   gradient: dz_c = w[t] (softmax_c - 1[c == t]) grad_out / sum_kept w[t] on kept pixels, +0.0f in every written lane
//             of every other pixel.  No gradient flows through the selection.
//   thresh = 1 (tau = +0.0f) or min_kept_total >= V keeps every valid pixel: the *_ex loss.
//
// Selection.  nll >= +0.0f, so its fp32 bit pattern orders like an unsigned integer; NaN maps to 0xFFFFFFFF.  kappa is
// found EXACTLY by a three-round most-significant-digit radix select over that key (11 / 11 / 10 bits):
//   1. pixel pass : reads the logits once, writes nll[i] (ignored pixels: the sentinel -1.0f, which no cut can select)
//                   and the optional argmax, counts V and the pixels with not (nll < tau), and histograms the top 11 key
//                   bits (per block in LDS, then ONE integer atomic per non-empty bin: exact, order independent).
//   2. two rounds : grid-stride passes over nll[P] only (4 bytes per pixel).  Each block first scans the previous global
//                   histogram(s) from the top bin down to the bin that holds rank K - no pick launch in between - and
//                   histograms the next digit of the keys inside that bin.  When count(not nll < tau) >= K the cut is
//                   tau and both rounds return at once (the common case early in training).
//   3. sum pass   : resolves the cut the same way, accumulates (sum w nll, sum w, count) over the kept pixels as fp64
//                   per-block partials; one finalize block sums them in a fixed order and writes loss, stats, counts.
// The backward reads the SAVED nll and stats[2] = cut to decide membership - a recomputed nll need not reproduce the
// forward's bits at the cut - and is otherwise vmtl_ce_bwd_ex: the three gradient kernels of ce_pixel.h under OHEM's
// policy, so the same three layouts and the same written lanes.
//
// No allocation, no sync, everything on the caller's stream (the counters and histograms are cleared in-stream by a
// memset node), so the node captures into a graph: K and tau are host constants, V, the cut and the denominator never
// leave the device.
#include "ce_pixel.h"
#include "reduce.h"

#define OH_THREADS CE_THREADS
#define OH_BINS0 2048  // key >> 21
#define OH_BINS1 2048  // (key >> 10) & 0x7ff
#define OH_BINS2 1024  // key & 0x3ff

// The head of the workspace (cleared by the entry point); 3 doubles per block of the sum pass follow it.
struct OhemWs {
  unsigned long long valid;   // V
  unsigned long long ge_tau;  // valid pixels with not (nll < tau)
  float cut;                  // written by block 0 of the sum pass for the finalize block
  float pad_[3];
  unsigned long long pad2_[4];
  unsigned hist[OH_BINS0 + OH_BINS1 + OH_BINS2];
};
static_assert(sizeof(OhemWs) % 8 == 0, "the partials behind the head are doubles");

__device__ __forceinline__ unsigned oh_key(float nll) { return nll != nll ? 0xFFFFFFFFu : __float_as_uint(nll); }

// The bin that holds the rank-th largest entry of hist[nbins] (rank is 1-based and at most the histogram's total), and
// the rank inside that bin.  Thread t owns the nbins/256 bins below nbins - t*per, so thread order is top-down bin
// order; an exclusive scan over the threads' sums places the rank.  Every thread returns the result.  sh: 6 entries.
__device__ __forceinline__ void oh_find(const unsigned* __restrict__ hist, int nbins, unsigned long long rank,
                                        unsigned long long* sh, int& bin, unsigned long long& within) {
  const int per = nbins / OH_THREADS;  // 8 or 4
  const int hi = nbins - (int)threadIdx.x * per;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned c[8];
  unsigned long long local = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c[j] = j < per ? hist[hi - 1 - j] : 0u;
    local += c[j];
  }
  unsigned long long inc = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  __syncthreads();  // the previous call's readers are done with sh
  if (lane == 63) sh[wave] = inc;
  if (threadIdx.x == 0) {
    sh[4] = 0;
    sh[5] = 0;
  }
  __syncthreads();
  unsigned long long before = inc - local;
  for (int w = 0; w < wave; ++w) before += sh[w];
  if (before < rank && rank <= before + local) {  // exactly one thread
    unsigned long long acc = before;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (rank > acc && rank <= acc + c[j]) {
        sh[4] = (unsigned long long)(hi - 1 - j);
        sh[5] = rank - acc;
      }
      acc += c[j];
    }
  }
  __syncthreads();
  bin = (int)sh[4];
  within = sh[5];
}

// K = min(min_kept_total, V).  True when the cut is tau and nothing needs selecting: K or more valid pixels are not
// below tau (then kappa >= tau, or kappa is NaN), or K = 0.
__device__ __forceinline__ bool oh_cut_is_tau(const OhemWs* __restrict__ ws, long long kmin, unsigned long long& K) {
  const unsigned long long V = ws->valid;
  K = (unsigned long long)kmin < V ? (unsigned long long)kmin : V;
  return ws->ge_tau >= K;
}

__device__ __forceinline__ void oh_flush(const unsigned* lh, unsigned* __restrict__ gh, int nbins) {
  for (int j = threadIdx.x; j < nbins; j += OH_THREADS) {
    const unsigned n = lh[j];
    if (n != 0u) atomicAdd(gh + j, n);
  }
}

// ------------------------------------------------------------------ forward: pixel pass
// One thread per pixel, the pixel pass of ce_pixel.h: Q > 0 holds the pixel's 4*Q >= C logits in registers (C <= 32),
// Q = 0 sweeps the channel planes.  The argmax is written for ignored pixels too.
template <int Q>
__global__ __launch_bounds__(OH_THREADS) void oh_pixel_kernel(const float* __restrict__ z,
                                                              const long long* __restrict__ tgt, long long ignore,
                                                              float tau, float* __restrict__ nll,
                                                              long long* __restrict__ amax, OhemWs* __restrict__ ws,
                                                              long long P, int HW, int C, long long sb, long long sc,
                                                              long long sp) {
  __shared__ unsigned lh[OH_BINS0];
  __shared__ unsigned lc[2];
  for (int j = threadIdx.x; j < OH_BINS0; j += OH_THREADS) lh[j] = 0u;
  if (threadIdx.x < 2) lc[threadIdx.x] = 0u;
  __syncthreads();
  unsigned nv = 0, nt = 0;
  VMTL_GRID_STRIDE(i, P) {
    const float* r = ce_pixel(z, i, HW, sb, sp);
    const long long t = tgt[i];
    const bool valid = t != ignore, inside = ce_label_inside(t, C);
    CeMax mx;
    float s = 0.f, zt = 0.f;
    bool fin = true;
    if constexpr (Q > 0) {
      float v[4 * Q];
      ce_load<Q>(v, r, C, sc);
      mx = ce_max_argmax<Q>(v, C);
      if (valid) {
        s = ce_sum_exp<Q>(v, C, mx.m);
#pragma unroll
        for (int c = 0; c < 4 * Q; ++c)
          if (c < C) fin = fin && fabsf(v[c]) < HUGE_VALF;
        zt = ce_pick<Q>(v, t);
      }
    } else {
      mx = ce_sweep_max_argmax(r, C, sc);
      if (valid) {
        s = ce_sweep_sum_exp(r, C, sc, mx.m, [&](float v) { fin = fin && fabsf(v) < HUGE_VALF; });
        if (inside) zt = r[t * sc];
      }
    }
    const float m = mx.m;
    if (amax != nullptr) amax[i] = mx.am;
    float v = -1.f;  // ignored: below every cut
    if (valid) {
      v = ce_nan();  // the rule for labels (ce_pixel.h); non-finite logits rank the same way
      if (inside && fin) {
        v = (m - zt) + logf(s);
        v = v > 0.f ? v : 0.f;  // finite logits: never NaN here; -0.0f and any rounding below zero become +0.0f
      }
      ++nv;
      nt += !(v < tau) ? 1u : 0u;
      atomicAdd(&lh[oh_key(v) >> 21], 1u);
    }
    nll[i] = v;
  }
  // wave_sum's tree for the two counts together: two wave_sum calls put one tree behind the other
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nv += __shfl_xor(nv, o, 64);
    nt += __shfl_xor(nt, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&lc[0], nv);
    atomicAdd(&lc[1], nt);
  }
  __syncthreads();
  oh_flush(lh, ws->hist, OH_BINS0);
  if (threadIdx.x == 0) {
    if (lc[0] != 0u) atomicAdd(&ws->valid, (unsigned long long)lc[0]);
    if (lc[1] != 0u) atomicAdd(&ws->ge_tau, (unsigned long long)lc[1]);
  }
}

// ------------------------------------------------------------------ forward: radix rounds 1 and 2 over nll[P]
// R = 1: the keys inside the rank-K bin of histogram 0 are counted by their next 11 bits into histogram 1.
// R = 2: the keys inside the rank-K bins of histograms 0 and 1 by their last 10 bits into histogram 2.
template <int R>
__global__ __launch_bounds__(OH_THREADS) void oh_round_kernel(const float* __restrict__ nll, OhemWs* __restrict__ ws,
                                                              long long kmin, long long P) {
  constexpr int NB = R == 1 ? OH_BINS1 : OH_BINS2;
  __shared__ unsigned lh[NB];
  __shared__ unsigned long long sh[6];
  unsigned long long K, rank;
  if (oh_cut_is_tau(ws, kmin, K)) return;  // uniform over the grid
  int b0, b1 = 0;
  oh_find(ws->hist, OH_BINS0, K, sh, b0, rank);
  if (R == 2) oh_find(ws->hist + OH_BINS0, OH_BINS1, rank, sh, b1, rank);
  const unsigned prefix = R == 1 ? (unsigned)b0 : ((unsigned)b0 << 11) | (unsigned)b1;
  for (int j = threadIdx.x; j < NB; j += OH_THREADS) lh[j] = 0u;
  __syncthreads();
  VMTL_GRID_STRIDE(i, P) {
    const float v = nll[i];
    if (v < 0.f) continue;  // the sentinel of an ignored pixel (a valid nll is >= +0.0f or NaN)
    const unsigned key = oh_key(v);
    if (R == 1) {
      if ((key >> 21) == prefix) atomicAdd(&lh[(key >> 10) & 0x7ffu], 1u);
    } else {
      if ((key >> 10) == prefix) atomicAdd(&lh[key & 0x3ffu], 1u);
    }
  }
  __syncthreads();
  oh_flush(lh, ws->hist + (R == 1 ? OH_BINS0 : OH_BINS0 + OH_BINS1), NB);
}

// ------------------------------------------------------------------ forward: sum pass and finalize
// partial: (sum w nll, sum w, kept count) per block; the count is exact in a double (P < 2^31).
__global__ __launch_bounds__(OH_THREADS) void oh_sum_kernel(const float* __restrict__ nll,
                                                            const long long* __restrict__ tgt,
                                                            const float* __restrict__ weight, OhemWs* __restrict__ ws,
                                                            long long kmin, float tau, double* __restrict__ partial,
                                                            long long P, int C) {
  __shared__ unsigned long long sh[6];
  __shared__ double shd[4];
  unsigned long long K, rank;
  float cut = tau;
  if (!oh_cut_is_tau(ws, kmin, K)) {  // fewer than K pixels reach tau: kappa < tau, and kappa is no NaN
    int b0, b1, b2;
    oh_find(ws->hist, OH_BINS0, K, sh, b0, rank);
    oh_find(ws->hist + OH_BINS0, OH_BINS1, rank, sh, b1, rank);
    oh_find(ws->hist + OH_BINS0 + OH_BINS1, OH_BINS2, rank, sh, b2, rank);
    cut = __uint_as_float(((unsigned)b0 << 21) | ((unsigned)b1 << 10) | (unsigned)b2);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) ws->cut = cut;
  double num = 0.0, den = 0.0, cnt = 0.0;
  VMTL_GRID_STRIDE(i, P) {
    const float v = nll[i];
    if (v < 0.f || v < cut) continue;  // ignored, or easier than the cut; NaN stays in
    float w = 1.f;
    if (weight != nullptr) {
      const long long t = tgt[i];
      if (ce_label_inside(t, C)) w = weight[t];  // a label outside [0, C) never indexes w (its nll is NaN)
    }
    num += (double)w * (double)v;
    den += (double)w;
    cnt += 1.0;
  }
  num = block_sum(num, shd);
  den = block_sum(den, shd);
  cnt = block_sum(cnt, shd);
  if (threadIdx.x == 0) {
    partial[3 * blockIdx.x] = num;
    partial[3 * blockIdx.x + 1] = den;
    partial[3 * blockIdx.x + 2] = cnt;
  }
}

// loss = num / den: NaN (0/0) when every pixel is ignored.  stats = {den, num, cut, 0}, counts = {V, kept}.
__global__ void oh_finalize_kernel(const double* __restrict__ partial, int n, const OhemWs* __restrict__ ws, float* loss,
                                   float* stats, long long* counts) {
  __shared__ double shd[4];
  double num = 0.0, den = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    num += partial[3 * i];
    den += partial[3 * i + 1];
    cnt += partial[3 * i + 2];
  }
  num = block_sum(num, shd);
  den = block_sum(den, shd);
  cnt = block_sum(cnt, shd);
  if (threadIdx.x == 0) {
    loss[0] = (float)(num / den);
    stats[0] = (float)den;
    stats[1] = (float)num;
    stats[2] = ws->cut;
    stats[3] = 0.f;
    counts[0] = (long long)ws->valid;
    counts[1] = (long long)cnt;
  }
}

// ------------------------------------------------------------------ backward
// A linear policy of ce_pixel.h: dz_c = (softmax_c - 1[c == t]) * k + bad with k = w[t] * g, g = gout / stats[0].  Its
// operands beside the logits: stats as the forward left it ({den, num, cut, 0}) and nll as it saved it.  A pixel is
// zeroed when it is ignored or below the cut; most are, so the kernels skip a zeroed pixel's softmax with a branch.
struct OhGrad {
  const float* __restrict__ weight;
  long long ignore;
  const float* __restrict__ stats;
  const float* __restrict__ nll;

  struct Wg : CeLinearWg {
    const float* __restrict__ weight;
    long long ignore;
    const float* __restrict__ nll;
    float g, cut;
    __device__ __forceinline__ CeLinearPx pixel(long long i, long long t, int C) const {
      return ce_linear_px(t, C, g, weight, t == ignore || nll[i] < cut);
    }
  };
  template <int>
  __device__ __forceinline__ Wg begin(const float* __restrict__ gout, long long, int) const {
    return {{}, weight, ignore, nll, gout[0] / stats[0], stats[2]};
  }
};

// ------------------------------------------------------------------ entry points
static inline int oh_blocks(long long P) { return ce_blocks(P); }

// the cleared head (counters, three histograms) and (sum w nll, sum w, kept) per block of the sum pass
extern "C" long long vmtl_ce_ohem_workspace_bytes(long long P) {
  return (long long)sizeof(OhemWs) + 3 * (long long)oh_blocks(P) * (long long)sizeof(double);
}

// weight = C floats or null (all ones), ignore_index = VMTL_NO_IGNORE for none, nll_thresh = tau = -log(thresh) >= 0
// (+inf: pure top-K), min_kept_total = min_kept * B >= 1, argmax = null or the prediction output.  Writes loss, stats
// (4 floats: den, num, cut, 0), counts (2 int64: V, kept) and nll (P floats, what the backward reads); workspace:
// vmtl_ce_ohem_workspace_bytes(P) bytes, 8-byte aligned.
extern "C" int vmtl_ce_ohem_fwd(const float* logits, const long long* target, const float* weight, long long ignore_index,
                                float nll_thresh, long long min_kept_total, float* loss, float* stats, long long* counts,
                                float* nll, void* workspace, long long* argmax, int B, int HW, int C, long long sb,
                                long long sc, long long sp, void* stream) {
  VMTL_ENTER();
  if (!logits || !target || !loss || !stats || !counts || !nll || !workspace || B <= 0 || HW <= 0 || C <= 0 ||
      min_kept_total < 1 || !(nll_thresh >= 0.f))
    return VMTL_ERR_ARG;
  const long long P = (long long)B * HW;
  if (P >= (1LL << 31)) return VMTL_ERR_UNSUPPORTED;  // 32-bit histogram bins
  hipStream_t st = (hipStream_t)stream;
  OhemWs* ws = (OhemWs*)workspace;
  double* partial = (double*)((char*)workspace + sizeof(OhemWs));
  const int nblk = oh_blocks(P);
  const float tau = nll_thresh + 0.f;  // -0.0f -> +0.0f
  if (hipMemsetAsync(ws, 0, sizeof(OhemWs), st) != hipSuccess) return VMTL_ERR_LAUNCH;
  auto pixel = [&](auto q) {
    hipLaunchKernelGGL((oh_pixel_kernel<decltype(q)::value>), dim3(nblk), dim3(OH_THREADS), 0, st, logits, target,
                       ignore_index, tau, nll, argmax, ws, P, HW, C, sb, sc, sp);
  };
  ce_dispatch_q(C <= 32 ? (C + 3) >> 2 : 0, pixel, [&] { pixel(std::integral_constant<int, 0>{}); });
  hipLaunchKernelGGL(oh_round_kernel<1>, dim3(nblk), dim3(OH_THREADS), 0, st, (const float*)nll, ws, min_kept_total, P);
  hipLaunchKernelGGL(oh_round_kernel<2>, dim3(nblk), dim3(OH_THREADS), 0, st, (const float*)nll, ws, min_kept_total, P);
  hipLaunchKernelGGL(oh_sum_kernel, dim3(nblk), dim3(OH_THREADS), 0, st, (const float*)nll, target, weight, ws,
                     min_kept_total, tau, partial, P, C);
  hipLaunchKernelGGL(oh_finalize_kernel, dim3(1), dim3(OH_THREADS), 0, st, (const double*)partial, nblk,
                     (const OhemWs*)ws, loss, stats, counts);
  return vmtl_check_launch();
}

// dz_c = w[t] (softmax_c - 1[c == t]) grad_out / stats[0] on the pixels the forward kept (valid and not nll < stats[2]),
// 0.0f in every written lane of every other pixel.  stats and nll as vmtl_ce_ohem_fwd left them.  The layout is
// ce_grad_layout's (ce_pixel.h), as for vmtl_ce_bwd_strided.
extern "C" int vmtl_ce_ohem_bwd(const float* logits, const long long* target, const float* weight, long long ignore_index,
                                const float* stats, const float* nll, const float* grad_out, float* dlogits, int B,
                                int HW, int C, long long sb, long long sc, long long sp, long long dsb, long long dsc,
                                long long dsp, void* stream) {
  VMTL_ENTER();
  if (!logits || !target || !stats || !nll || !grad_out || !dlogits || B <= 0 || HW <= 0 || C <= 0) return VMTL_ERR_ARG;
  ce_grad_launch(ce_grad_layout(C, HW, dsb, dsc, dsp), logits, target, grad_out, dlogits,
                 OhGrad{weight, ignore_index, stats, nll}, (long long)B * HW, HW, C, sb, sc, sp, dsb, dsc, dsp,
                 (hipStream_t)stream);
  return vmtl_check_launch();
}
