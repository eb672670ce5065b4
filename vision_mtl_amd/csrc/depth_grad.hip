// Depth loss with a multi-scale gradient-matching term (MegaDepth, Li & Snavely 2018; MiDaS' GradientLoss with
// batch-based reduction, on log depth):
//
//   R      = log(pred) - log(target) on the valid pixels (target > min_depth, or the caller's uint8 mask), 0 elsewhere;
//            evaluated as log(pred / target)
//   G_k    = pixels with y % s == 0 and x % s == 0, s = 2^k, k = 0 .. scales-1
//   N_k    = #{valid pixels of G_k}, whole batch
//   S_k    = sum over G_k of |R(y,x+s) - R(y,x)| (x+s < W, both valid) + |R(y+s,x) - R(y,x)| (y+s < H, both valid)
//   L_grad = sum_k (N_k > 0 ? S_k / N_k : 0)
//   loss   = silog_weight * SILog + grad_weight * L_grad          (SILog: reference losses.py:29-36, as loss.hip)
//
// Forward, three launches: dg_resid_kernel (the one sweep over pred / target: writes R for every pixel and the SILog
// partials), dg_stencil_kernel (reads R written by the launch before it - a neighbour's residual crosses workgroups only
// over that kernel boundary - and writes per-block S_k / N_k partials), dg_finalize_kernel (one workgroup folds all
// partials in a fixed order).  Backward, one launch: every pixel GATHERS its up to 4 * scales signed 1/N_k contributions,
// signs taken from the saved R.  fp64 partials, no floating-point atomics, nothing visits the host.
#include "common.h"

#define DG_BLOCKS_MAX 1024
#define DG_PIX_PER_BLOCK 1024
#define DG_BWD_BLOCKS_MAX 4096
#define DG_SCALES_MAX 6

struct DgAboveMinDepth {
  float min_depth;
  template <typename I>
  __device__ __forceinline__ bool operator()(const float* __restrict__ tgt, I i) const { return tgt[i] > min_depth; }
};
struct DgMasked {
  const unsigned char* __restrict__ mask;
  template <typename I>
  __device__ __forceinline__ bool operator()(const float* __restrict__, I i) const { return mask[i] != 0; }
};

// The sweeps are instantiated for a pixel index type I: int while every index and every neighbour offset fits
// (dg_small), long long otherwise.  pixel i of [B][H][W] -> (y, x)
template <typename I>
__device__ __forceinline__ void dg_yx(I i, int H, int W, int& y, int& x) {
  if constexpr (sizeof(I) == 4) {
    const unsigned u = (unsigned)i, row = u / (unsigned)W;
    x = (int)(u - row * (unsigned)W);
    y = (int)(row % (unsigned)H);
  } else {
    const long long row = i / W;
    x = (int)(i - row * W);
    y = (int)(row % H);
  }
}

// sign as torch's: 0 at 0 (and at NaN)
__device__ __forceinline__ float dg_sgn(float d) { return (float)((d > 0.f) - (d < 0.f)); }

// The loads of a pixel never depend on a loaded value (validity selects, it does not branch), so all of them are in
// flight together: these sweeps are latency-bound, not bandwidth-bound, at a few pixels per thread.  Counts come from
// ballots (wave-uniform integers), sums from fp64 shuffles; the block's waves are folded in a fixed order behind one
// barrier.  partial[0 / 1 / 2][blk] = N, sum g, sum g^2 of the block's valid pixels
template <typename I, class Valid>
__global__ __launch_bounds__(256) void dg_resid_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                       Valid valid, I P, float* __restrict__ resid,
                                                       double* __restrict__ partial) {
  __shared__ double shd[4 * 3];
  double s1 = 0.0, s2 = 0.0;
  int n = 0;
  for (I i = (I)(blockIdx.x * blockDim.x + threadIdx.x); i < P; i += (I)(gridDim.x * blockDim.x)) {
    const bool v = valid(tgt, i);
    const float p = pred[i], t = tgt[i];
    // one log of the correctly rounded quotient: |R| is small, so its rounding (an ulp of R, plus 2^-24 from the
    // division) is several times below that of a difference of two logs of magnitude 1..3, and the stencil's sums are
    // sums of small differences of R.  A non-positive prediction keeps its own log (NaN or -inf), whatever the target.
    const float g = v ? logf(p > 0.f ? p / t : p) : 0.f;
    n += __popcll(__ballot(v));
    s1 += (double)g;
    s2 += (double)g * (double)g;
    resid[i] = g;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    shd[w * 3 + 0] = (double)n;
    shd[w * 3 + 1] = s1;
    shd[w * 3 + 2] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 3)
    partial[threadIdx.x * gridDim.x + blockIdx.x] =
        ((shd[threadIdx.x] + shd[3 + threadIdx.x]) + shd[6 + threadIdx.x]) + shd[9 + threadIdx.x];
}

// partial[2 * k][blk] = S_k, [2 * k + 1][blk] = N_k of the block's pixels.  A neighbour outside the image, or of a pixel
// off the scale's grid, is read at the pixel's own index and selected away; a wave with no pixel on a scale's grid (the
// rows with y % s != 0) skips that scale - a test on indices, not on loaded values.
template <int SCALES, typename I, class Valid>
__global__ __launch_bounds__(256) void dg_stencil_kernel(const float* __restrict__ resid, const float* __restrict__ tgt,
                                                         Valid valid, I P, int H, int W, double* __restrict__ partial) {
  __shared__ double shd[4 * 2 * SCALES];
  double S[SCALES];
  int N[SCALES];
#pragma unroll
  for (int k = 0; k < SCALES; ++k) {
    S[k] = 0.0;
    N[k] = 0;
  }
  for (I i = (I)(blockIdx.x * blockDim.x + threadIdx.x); i < P; i += (I)(gridDim.x * blockDim.x)) {
    const bool v = valid(tgt, i);
    const float r = resid[i];
    int y, x;
    dg_yx(i, H, W, y, x);
    const int yx = y | x;
#pragma unroll
    for (int k = 0; k < SCALES; ++k) {
      const int s = 1 << k;
      const bool on = !(yx & (s - 1));
      if (k > 0 && !__any(on)) continue;
      const bool hr = on && x + s < W, hd = on && y + s < H;
      const I jr = hr ? i + (I)s : i, jd = hd ? i + (I)s * (I)W : i;
      const bool vr = valid(tgt, jr), vd = valid(tgt, jd);
      const float rr = resid[jr], rd = resid[jd];
      float a = 0.f;
      a += hr && vr ? fabsf(rr - r) : 0.f;
      a += hd && vd ? fabsf(rd - r) : 0.f;
      S[k] += v && on ? (double)a : 0.0;
      N[k] += __popcll(__ballot(v && on));
    }
  }
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < SCALES; ++k) {
    const double sk = wave_sum(S[k]);
    if ((threadIdx.x & 63) == 0) {
      shd[w * 2 * SCALES + 2 * k] = sk;
      shd[w * 2 * SCALES + 2 * k + 1] = (double)N[k];  // a count: exact in fp64
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * SCALES) {
    const int j = threadIdx.x;
    partial[j * gridDim.x + blockIdx.x] =
        ((shd[j] + shd[2 * SCALES + j]) + shd[4 * SCALES + j]) + shd[6 * SCALES + j];
  }
}

// One workgroup of 1024: wave j sums value j (3 of SILog, then S_k, N_k per scale: at most 15) over the blocks, lane l
// taking blocks l, l + 64, ..; every load is independent of every other.  silog_weight == 0: the SILog term is not
// evaluated (terms[0], stats[1], stats[2] are 0), so fewer than two valid pixels leave the stand-alone term finite.
__global__ __launch_bounds__(1024) void dg_finalize_kernel(const double* __restrict__ partial, int nblk, int scales,
                                                           float silog_weight, float grad_weight, float* loss,
                                                           float* terms, float* stats, long long* counts) {
  __shared__ double tot[16];
  const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double s = 0.0;
  if (j < 3 + 2 * scales)
    for (int i = lane; i < nblk; i += 64) s += partial[(long long)j * nblk + i];
  s = wave_sum(s);
  if (lane == 0) tot[j] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = tot[0], s1 = tot[1], s2 = tot[2];
    double lgrad = 0.0;
    for (int k = 0; k < scales; ++k) {
      const double sk = tot[3 + 2 * k], nk = tot[4 + 2 * k];
      if (nk > 0.0) lgrad += sk / nk;
      counts[k] = (long long)nk;  // sums of integers below 2^53: exact
    }
    double silog = 0.0, mu = 0.0, dg = 0.0;
    if (silog_weight != 0.f) {
      mu = s1 / n;                                        // n == 0 -> NaN, as torch.mean of an empty tensor
      const double var = (s2 - n * mu * mu) / (n - 1.0);  // n == 1 -> NaN (unbiased variance), as torch.var
      dg = var + 0.15 * mu * mu;
      silog = 10.0 * sqrt(dg);
    }
    double l = (double)grad_weight * lgrad;
    if (silog_weight != 0.f) l += (double)silog_weight * silog;
    loss[0] = (float)l;
    terms[0] = (float)silog;
    terms[1] = (float)lgrad;
    stats[0] = (float)n;
    stats[1] = (float)mu;
    stats[2] = (float)dg;
  }
}

// dL/dR_i = silog_weight * (5/sqrt(Dg)) (2 (R_i - mu)/(N-1) + 0.3 mu/N)
//         + grad_weight * sum_k [i in G_k] (1/N_k) ( sgn(R_i - R_left) - sgn(R_right - R_i) + sgn(R_i - R_up) - sgn(R_down - R_i) )
// over the neighbours at distance 2^k that are inside the image and valid; dpred_i = grad_out * dL/dR_i / pred_i on
// valid pixels, +0.0f elsewhere.  Loads and the per-scale skip as in the stencil.
template <int SCALES, typename I, class Valid>
__global__ __launch_bounds__(256) void dg_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                     const float* __restrict__ resid, const float* __restrict__ stats,
                                                     const long long* __restrict__ counts,
                                                     const float* __restrict__ gout, Valid valid, I P, int H, int W,
                                                     float silog_weight, float grad_weight, float* __restrict__ dpred) {
  const float go = gout[0];
  float ks = 0.f, a = 0.f, b = 0.f, mu = 0.f;
  if (silog_weight != 0.f) {
    const float n = stats[0];
    mu = stats[1];
    ks = silog_weight * 5.f / sqrtf(stats[2]);
    a = 2.f / (n - 1.f);
    b = 0.3f * mu / n;
  }
  float inv[SCALES];
#pragma unroll
  for (int k = 0; k < SCALES; ++k) inv[k] = counts[k] > 0 ? grad_weight / (float)counts[k] : 0.f;
  for (I i = (I)(blockIdx.x * blockDim.x + threadIdx.x); i < P; i += (I)(gridDim.x * blockDim.x)) {
    const bool v = valid(tgt, i);
    const float r = resid[i], p = pred[i];
    int y, x;
    dg_yx(i, H, W, y, x);
    const int yx = y | x;
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < SCALES; ++k) {
      const int s = 1 << k;
      const bool on = !(yx & (s - 1));
      if (k > 0 && !__any(on)) continue;
      const I sw = (I)s * (I)W;
      const bool hl = on && x >= s, hr = on && x + s < W, hu = on && y >= s, hd = on && y + s < H;
      const I jl = hl ? i - (I)s : i, jr = hr ? i + (I)s : i, ju = hu ? i - sw : i, jd = hd ? i + sw : i;
      const bool vl = valid(tgt, jl), vr = valid(tgt, jr), vu = valid(tgt, ju), vd = valid(tgt, jd);
      const float rl = resid[jl], rr = resid[jr], ru = resid[ju], rd = resid[jd];
      float c = 0.f;
      c += hl && vl ? dg_sgn(r - rl) : 0.f;
      c -= hr && vr ? dg_sgn(rr - r) : 0.f;
      c += hu && vu ? dg_sgn(r - ru) : 0.f;
      c -= hd && vd ? dg_sgn(rd - r) : 0.f;
      g += inv[k] * c;
    }
    if (silog_weight != 0.f) g += ks * (a * (r - mu) + b);
    dpred[i] = v ? go * g / p : 0.f;
  }
}

// forward sweeps: a block per 1024 pixels, at most 1024 blocks (their partials are what the finalize reads)
static inline int dg_blocks(long long P) {
  return grid_1d(P, DG_PIX_PER_BLOCK, DG_BLOCKS_MAX);
}

// backward sweep: no reduction, a pixel per thread while the grid allows it
static inline int dg_bwd_blocks(long long P) {
  return grid_1d(P, 256, DG_BWD_BLOCKS_MAX);
}

// int pixel indices: i + grid stride, 4 * i (a byte offset) and 32 * W (the farthest neighbour's offset) all fit
static inline bool dg_small(long long P, int W) { return P <= (1LL << 29) && W <= (1 << 24); }

static inline bool dg_geometry_ok(int B, int H, int W, int scales) {
  return B > 0 && H > 0 && W > 0 && scales >= 1 && scales <= DG_SCALES_MAX;
}

static inline bool dg_weight_ok(float w) { return w >= 0.f && w <= 3.0e38f; }  // finite, not negative, not NaN

extern "C" long long vmtl_depth_grad_workspace_bytes(int B, int H, int W, int scales) {
  if (!dg_geometry_ok(B, H, W, scales)) return 0;
  return (long long)dg_blocks((long long)B * H * W) * (3 + 2 * scales) * (long long)sizeof(double);
}

template <int SCALES, class Valid>
static void dg_stencil_launch(const float* resid, const float* target, Valid valid, double* partial, long long P, int H,
                              int W, int nblk, hipStream_t st) {
  if (dg_small(P, W))
    hipLaunchKernelGGL((dg_stencil_kernel<SCALES, int, Valid>), dim3(nblk), dim3(256), 0, st, resid, target, valid, (int)P,
                       H, W, partial);
  else
    hipLaunchKernelGGL((dg_stencil_kernel<SCALES, long long, Valid>), dim3(nblk), dim3(256), 0, st, resid, target, valid,
                       P, H, W, partial);
}

template <class Valid>
static int dg_fwd_launch(const float* pred, const float* target, Valid valid, int B, int H, int W, int scales,
                         float silog_weight, float grad_weight, float* loss, float* terms, float* stats,
                         long long* counts, float* resid, void* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const long long P = (long long)B * H * W;
  const int nblk = dg_blocks(P);
  double* ws = (double*)workspace;
  double* pg = ws + (long long)nblk * 3;  // [3][nblk] of SILog, then [2 * scales][nblk]
  if (dg_small(P, W))
    hipLaunchKernelGGL((dg_resid_kernel<int, Valid>), dim3(nblk), dim3(256), 0, st, pred, target, valid, (int)P, resid, ws);
  else
    hipLaunchKernelGGL((dg_resid_kernel<long long, Valid>), dim3(nblk), dim3(256), 0, st, pred, target, valid, P, resid, ws);
  switch (scales) {
    case 1: dg_stencil_launch<1>(resid, target, valid, pg, P, H, W, nblk, st); break;
    case 2: dg_stencil_launch<2>(resid, target, valid, pg, P, H, W, nblk, st); break;
    case 3: dg_stencil_launch<3>(resid, target, valid, pg, P, H, W, nblk, st); break;
    case 4: dg_stencil_launch<4>(resid, target, valid, pg, P, H, W, nblk, st); break;
    case 5: dg_stencil_launch<5>(resid, target, valid, pg, P, H, W, nblk, st); break;
    default: dg_stencil_launch<6>(resid, target, valid, pg, P, H, W, nblk, st); break;
  }
  hipLaunchKernelGGL(dg_finalize_kernel, dim3(1), dim3(1024), 0, st, (const double*)ws, nblk, scales, silog_weight,
                     grad_weight, loss, terms, stats, counts);
  return vmtl_check_launch();
}

template <int SCALES, class Valid>
static void dg_bwd_scales(const float* pred, const float* target, Valid valid, const float* resid, const float* stats,
                          const long long* counts, const float* grad_out, long long P, int H, int W, float silog_weight,
                          float grad_weight, float* dpred, hipStream_t st) {
  const int nblk = dg_bwd_blocks(P);
  if (dg_small(P, W))
    hipLaunchKernelGGL((dg_bwd_kernel<SCALES, int, Valid>), dim3(nblk), dim3(256), 0, st, pred, target, resid, stats,
                       counts, grad_out, valid, (int)P, H, W, silog_weight, grad_weight, dpred);
  else
    hipLaunchKernelGGL((dg_bwd_kernel<SCALES, long long, Valid>), dim3(nblk), dim3(256), 0, st, pred, target, resid,
                       stats, counts, grad_out, valid, P, H, W, silog_weight, grad_weight, dpred);
}

template <class Valid>
static int dg_bwd_launch(const float* pred, const float* target, Valid valid, const float* resid, const float* stats,
                         const long long* counts, const float* grad_out, int B, int H, int W, int scales,
                         float silog_weight, float grad_weight, float* dpred, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const long long P = (long long)B * H * W;
  switch (scales) {
    case 1: dg_bwd_scales<1>(pred, target, valid, resid, stats, counts, grad_out, P, H, W, silog_weight, grad_weight, dpred, st); break;
    case 2: dg_bwd_scales<2>(pred, target, valid, resid, stats, counts, grad_out, P, H, W, silog_weight, grad_weight, dpred, st); break;
    case 3: dg_bwd_scales<3>(pred, target, valid, resid, stats, counts, grad_out, P, H, W, silog_weight, grad_weight, dpred, st); break;
    case 4: dg_bwd_scales<4>(pred, target, valid, resid, stats, counts, grad_out, P, H, W, silog_weight, grad_weight, dpred, st); break;
    case 5: dg_bwd_scales<5>(pred, target, valid, resid, stats, counts, grad_out, P, H, W, silog_weight, grad_weight, dpred, st); break;
    default: dg_bwd_scales<6>(pred, target, valid, resid, stats, counts, grad_out, P, H, W, silog_weight, grad_weight, dpred, st); break;
  }
  return vmtl_check_launch();
}

// (tests hand the entry points dummy addresses with bad arguments: keep every argument check ahead of the first launch)
extern "C" int vmtl_depth_grad_fwd(const float* pred, const float* target, const unsigned char* mask, float min_depth,
                                   int B, int H, int W, int scales, float silog_weight, float grad_weight, float* loss,
                                   float* terms, float* stats, long long* counts, float* resid, void* workspace,
                                   void* stream) {
  VMTL_ENTER();
  if (!pred || !target || !loss || !terms || !stats || !counts || !resid || !workspace) return VMTL_ERR_ARG;
  if (!dg_geometry_ok(B, H, W, scales) || !dg_weight_ok(silog_weight) || !dg_weight_ok(grad_weight)) return VMTL_ERR_ARG;
  if (mask)
    return dg_fwd_launch(pred, target, DgMasked{mask}, B, H, W, scales, silog_weight, grad_weight, loss, terms, stats,
                         counts, resid, workspace, stream);
  return dg_fwd_launch(pred, target, DgAboveMinDepth{min_depth}, B, H, W, scales, silog_weight, grad_weight, loss, terms,
                       stats, counts, resid, workspace, stream);
}

extern "C" int vmtl_depth_grad_bwd(const float* pred, const float* target, const unsigned char* mask, float min_depth,
                                   const float* resid, const float* stats, const long long* counts,
                                   const float* grad_out, int B, int H, int W, int scales, float silog_weight,
                                   float grad_weight, float* dpred, void* stream) {
  VMTL_ENTER();
  if (!pred || !target || !resid || !stats || !counts || !grad_out || !dpred) return VMTL_ERR_ARG;
  if (!dg_geometry_ok(B, H, W, scales) || !dg_weight_ok(silog_weight) || !dg_weight_ok(grad_weight)) return VMTL_ERR_ARG;
  if (mask)
    return dg_bwd_launch(pred, target, DgMasked{mask}, resid, stats, counts, grad_out, B, H, W, scales, silog_weight, grad_weight,
                         dpred, stream);
  return dg_bwd_launch(pred, target, DgAboveMinDepth{min_depth}, resid, stats, counts, grad_out, B, H, W, scales, silog_weight,
                       grad_weight, dpred, stream);
}
