// Test-time augmentation and output-size predictions: the inference-side counterpart of
// augment.hip.  The model is run on resized / mirrored views of a batch; three forward-only kernels do the rest:
//
//   tta_view_kernel        image batch -> the model's NHWC input storage of one view (resample, then mirror in x)
//   tta_accumulate_kernel  one view's logits (NCHW) and depth logits -> un-mirrored, resampled to the base size and
//                          merged into the accumulators (softmax probabilities or logits; sigmoid depth)
//   tta_finish_*_kernel    merged map -> arg-max / depth / confidence at ANY output size, channel by channel with a
//                          running best: the (B, C, Ho, Wo) map is never written
//
// All three are gathers: one thread per output pixel (the resampling finish: per output column and four rows), x
// fastest, so the four taps of every channel plane are read from (nearly) consecutive addresses by consecutive lanes
// and every store is coalesced.  No atomics, no
// workspace, every output element written by exactly one thread: bit-identical from run to run.
//
// Resampling everywhere is F.interpolate(mode="bilinear", align_corners=False, antialias=False) as ATen evaluates it:
// scale = (float)in / out, src = scale * (dst + 0.5) - 0.5 clamped below at 0, i0 = (int)src, i1 = i0 + (i0 < in - 1),
// lambda1 = src - i0.  Equal sizes take an explicit copy branch (SAME): l0 * v + 0 * v' is not v for an infinite v'.
#include "common.h"

#include "../../include/vmtl.h"

#define TTA_MAX_C 32

// pixel i of [B][H][W] -> (b, y, x); the 32-bit form is the one that runs (uniform switch: 64-bit divisions are ~100
// instructions each), the 64-bit one takes over when B * H * W passes 2^31
__device__ __forceinline__ void tta_byx(long long i, int H, int W, bool small, int& b, int& y, int& x) {
  if (small) {
    const unsigned u = (unsigned)i, row = u / (unsigned)W, img = row / (unsigned)H;
    x = (int)(u - row * (unsigned)W);
    y = (int)(row - img * (unsigned)H);
    b = (int)img;
  } else {
    const long long row = i / W, img = row / H;
    x = (int)(i - row * W);
    y = (int)(row - img * H);
    b = (int)img;
  }
}

// ATen's area_pixel_compute_source_index (align_corners=False, cubic=False) + guard_index_and_lambda
__device__ __forceinline__ void tta_coord(int o, int in_size, float scale, int& i0, int& i1, float& l1) {
  float s = scale * ((float)o + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

// The four taps of an output pixel inside one [h][w] plane, and their weights.  SAME: o00 alone is used.
struct TtaTaps {
  int o00, o01, o10, o11;
  float ly, lx;
};

// (y, x) of the (H, W) output -> taps in the (h, w) source; flip: the source is mirrored in x, so column x' of the
// un-mirrored map is read from w - 1 - x'
template <bool SAME>
__device__ __forceinline__ TtaTaps tta_taps(int y, int x, int h, int w, float sh, float sw, int flip) {
  TtaTaps t;
  if (SAME) {
    t.o00 = t.o01 = t.o10 = t.o11 = y * w + (flip ? w - 1 - x : x);
    t.ly = t.lx = 0.f;
  } else {
    int y0, y1, x0, x1;
    tta_coord(y, h, sh, y0, y1, t.ly);
    tta_coord(x, w, sw, x0, x1, t.lx);
    if (flip) {
      x0 = w - 1 - x0;
      x1 = w - 1 - x1;
    }
    t.o00 = y0 * w + x0;
    t.o01 = y0 * w + x1;
    t.o10 = y1 * w + x0;
    t.o11 = y1 * w + x1;
  }
  return t;
}

__device__ __forceinline__ float tta_mix(float v00, float v01, float v10, float v11, float ly, float lx) {
  // hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11) with the fused operations spelled out: left to the
  // compiler's contraction, the scalar and the 16-byte paths of the view kernel came out an ulp apart
  const float hy = 1.f - ly, hx = 1.f - lx;
  const float top = fmaf(lx, v01, hx * v00), bottom = fmaf(lx, v11, hx * v10);
  return fmaf(ly, bottom, hy * top);
}

template <bool SAME>
__device__ __forceinline__ float tta_sample(const float* __restrict__ plane, const TtaTaps& t) {
  if (SAME) return plane[t.o00];
  return tta_mix(plane[t.o00], plane[t.o01], plane[t.o10], plane[t.o11], t.ly, t.lx);
}

// ------------------------------------------------------------------ view
// LD: pixel stride of the input (3: dataset sample layout, scalar loads; 4: NHWC input storage, 16-byte loads).
// out[b][y][x] = resized[b][y][flip ? Wo - 1 - x : x], pad lane +0.0f; one 16-byte store per thread.
template <int LD, bool SAME>
__global__ __launch_bounds__(256) void tta_view_kernel(const float* __restrict__ img, f32x4* __restrict__ out, int H,
                                                       int W, int Ho, int Wo, float sh, float sw, int flip,
                                                       long long P, bool small) {
  VMTL_GRID_STRIDE(i, P) {
    int b, y, x;
    tta_byx(i, Ho, Wo, small, b, y, x);
    // resample first, mirror after: output column x shows column Wo - 1 - x of the resized image
    const TtaTaps t = tta_taps<SAME>(y, flip ? Wo - 1 - x : x, H, W, sh, sw, 0);
    const float* base = img + (size_t)b * H * W * LD;
    f32x4 o;
    if (LD == 4) {
      if (SAME) {
        o = *reinterpret_cast<const f32x4*>(base + (size_t)t.o00 * 4);
      } else {
        const f32x4 v00 = *reinterpret_cast<const f32x4*>(base + (size_t)t.o00 * 4);
        const f32x4 v01 = *reinterpret_cast<const f32x4*>(base + (size_t)t.o01 * 4);
        const f32x4 v10 = *reinterpret_cast<const f32x4*>(base + (size_t)t.o10 * 4);
        const f32x4 v11 = *reinterpret_cast<const f32x4*>(base + (size_t)t.o11 * 4);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = tta_mix(v00[c], v01[c], v10[c], v11[c], t.ly, t.lx);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (SAME)
          o[c] = base[(size_t)t.o00 * 3 + c];
        else
          o[c] = tta_mix(base[(size_t)t.o00 * 3 + c], base[(size_t)t.o01 * 3 + c], base[(size_t)t.o10 * 3 + c],
                         base[(size_t)t.o11 * 3 + c], t.ly, t.lx);
      }
    }
    o[3] = 0.f;
    out[i] = o;
  }
}

// ------------------------------------------------------------------ accumulate
// MODE: VMTL_TTA_PROB / VMTL_TTA_LOGIT, a compile-time variant.  PROB keeps the pixel's C resampled logits in
// registers (the loops are unrolled over TTA_MAX_C with a uniform c < C guard: constant indices, no scratch), so
// every tap is read once: maximum, exponentials, sum, then C stores.  LOGIT streams: one channel at a time.
template <int MODE, bool SAME>
__global__ __launch_bounds__(256) void tta_accumulate_kernel(const float* __restrict__ logits,
                                                             const float* __restrict__ depth_logits,
                                                             float* __restrict__ acc, float* __restrict__ acc_depth,
                                                             int C, int h, int w, int H, int W, float sh, float sw,
                                                             int flip, float weight, float depth_weight, int first,
                                                             long long P, bool small) {
  const size_t hw = (size_t)h * w, HW = (size_t)H * W;
  VMTL_GRID_STRIDE(i, P) {
    int b, y, x;
    tta_byx(i, H, W, small, b, y, x);
    const TtaTaps t = tta_taps<SAME>(y, x, h, w, sh, sw, flip);
    const float* src = logits + (size_t)b * C * hw;
    float* dst = acc + (size_t)b * C * HW + ((size_t)y * W + x);
    if (MODE == VMTL_TTA_LOGIT) {
      for (int c = 0; c < C; ++c) {
        const float v = weight * tta_sample<SAME>(src + c * hw, t);
        dst[c * HW] = first ? v : dst[c * HW] + v;
      }
    } else {
      float v[TTA_MAX_C];
      float m = -INFINITY;
#pragma unroll
      for (int c = 0; c < TTA_MAX_C; ++c)
        if (c < C) {
          v[c] = tta_sample<SAME>(src + c * hw, t);
          m = fmaxf(m, v[c]);
        }
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < TTA_MAX_C; ++c)
        if (c < C) {
          v[c] = expf(v[c] - m);
          s += v[c];
        }
#pragma unroll
      for (int c = 0; c < TTA_MAX_C; ++c)
        if (c < C) {
          const float p = weight * (v[c] / s);
          dst[c * HW] = first ? p : dst[c * HW] + p;
        }
    }
    if (depth_logits != nullptr) {
      const float* d = depth_logits + (size_t)b * hw;
      float r;
      if (SAME)
        r = sigmoid_exact(d[t.o00]);
      else
        r = tta_mix(sigmoid_exact(d[t.o00]), sigmoid_exact(d[t.o01]), sigmoid_exact(d[t.o10]), sigmoid_exact(d[t.o11]),
                    t.ly, t.lx);
      r *= depth_weight;
      acc_depth[i] = first ? r : acc_depth[i] + r;
    }
  }
}

// ------------------------------------------------------------------ finish
// One pass over the channels per output pixel: resample plane c, keep the running best (strict >: the first maximum
// wins, as argmax_kernel).  Confidence, PROB: best / sum of the resampled probabilities (inv_weight cancels).  LOGIT:
// the merged logits are inv_weight * acc (the mean over the views); online softmax - the running maximum m and
// s = sum exp(z - m), rescaled when m moves - so confidence = exp(best - m) / s = 1 / s.
template <int MODE>
__device__ __forceinline__ void tta_keep(float v, int c, float inv_weight, bool conf, float& best, int& am, float& s) {
  if (c == 0) {
    best = v;
    am = 0;
    s = MODE == VMTL_TTA_PROB ? v : 1.f;  // LOGIT: exp(z_0 - m) with m = z_0
  } else if (MODE == VMTL_TTA_PROB || !conf) {
    s += v;
    if (v > best) { best = v; am = c; }
  } else if (v > best) {
    s = s * expf(inv_weight * (best - v)) + 1.f;
    best = v;
    am = c;
  } else {
    s += expf(inv_weight * (v - best));
  }
}

template <int MODE>
__device__ __forceinline__ float tta_confidence(float best, float s) {
  return MODE == VMTL_TTA_PROB ? best / s : 1.f / s;
}

// equal sizes: a copy, one load per channel and pixel
template <int MODE>
__global__ __launch_bounds__(256) void tta_finish_same_kernel(const float* __restrict__ acc,
                                                              const float* __restrict__ acc_depth, float inv_weight,
                                                              long long* __restrict__ segm, float* __restrict__ depth,
                                                              float* __restrict__ confidence, int C, long long HW,
                                                              long long P, bool small) {
  const bool conf = confidence != nullptr;
  VMTL_GRID_STRIDE(i, P) {
    long long b, pix;
    if (small) {
      const unsigned u = (unsigned)i, q = u / (unsigned)HW;
      b = q;
      pix = u - q * (unsigned)HW;
    } else {
      b = i / HW;
      pix = i - b * HW;
    }
    const float* src = acc + (size_t)b * C * HW + pix;
    float best, s;
    int am;
    for (int c = 0; c < C; ++c) tta_keep<MODE>(src[c * HW], c, inv_weight, conf, best, am, s);
    segm[i] = am;
    if (conf) confidence[i] = tta_confidence<MODE>(best, s);
    if (acc_depth != nullptr) depth[i] = inv_weight * acc_depth[i];
  }
}

// Resampling: one thread per output column x and group of TTA_ROWS consecutive output rows.  The column taps are the
// group's; when the rows of the group fall between the same two source rows (any up-sampling by 2 * TTA_ROWS or more,
// and most groups of a smaller one) the four taps of a channel are loaded ONCE and mixed in x once, and every row adds
// only its own y weight - at 128x256 -> 1024x2048 that is a quarter of the loads, which is what the pixel-per-thread
// form of this kernel was bound by (76 tap loads for 12 bytes written).  Otherwise every row loads its own taps.  The
// arithmetic per pixel is tta_mix's either way.
#define TTA_ROWS 4
template <int MODE>
__global__ __launch_bounds__(256) void tta_finish_rows_kernel(const float* __restrict__ acc,
                                                              const float* __restrict__ acc_depth, float inv_weight,
                                                              long long* __restrict__ segm, float* __restrict__ depth,
                                                              float* __restrict__ confidence, int C, int H, int W,
                                                              int Ho, int Wo, int G, float sh, float sw, long long PG,
                                                              bool small) {
  const size_t HW = (size_t)H * W;
  const bool conf = confidence != nullptr;
  VMTL_GRID_STRIDE(i, PG) {
    int b, g, x;
    tta_byx(i, G, Wo, small, b, g, x);
    int x0, x1;
    float lx;
    tta_coord(x, W, sw, x0, x1, lx);
    const float hx = 1.f - lx;
    int r0[TTA_ROWS], r1[TTA_ROWS];  // row offsets y0 * W, y1 * W; a row past the end repeats the last one (not stored)
    float ly[TTA_ROWS];
#pragma unroll
    for (int k = 0; k < TTA_ROWS; ++k) {
      int y0, y1;
      tta_coord(min(g * TTA_ROWS + k, Ho - 1), H, sh, y0, y1, ly[k]);
      r0[k] = y0 * W;
      r1[k] = y1 * W;
    }
    const bool shared = r0[0] == r0[TTA_ROWS - 1] && r1[0] == r1[TTA_ROWS - 1];  // both are monotone in the row
    float best[TTA_ROWS], s[TTA_ROWS], v[TTA_ROWS];
    int am[TTA_ROWS];
    // plane C is the depth accumulator: the same taps, no arg-max
    for (int c = 0; c <= C; ++c) {
      if (c == C && acc_depth == nullptr) break;
      const float* p = c < C ? acc + ((size_t)b * C + c) * HW : acc_depth + (size_t)b * HW;
      if (shared) {
        const float top = fmaf(lx, p[r0[0] + x1], hx * p[r0[0] + x0]);
        const float bottom = fmaf(lx, p[r1[0] + x1], hx * p[r1[0] + x0]);
#pragma unroll
        for (int k = 0; k < TTA_ROWS; ++k) v[k] = fmaf(ly[k], bottom, (1.f - ly[k]) * top);
      } else {
#pragma unroll
        for (int k = 0; k < TTA_ROWS; ++k)
          v[k] = tta_mix(p[r0[k] + x0], p[r0[k] + x1], p[r1[k] + x0], p[r1[k] + x1], ly[k], lx);
      }
      if (c < C) {
#pragma unroll
        for (int k = 0; k < TTA_ROWS; ++k) tta_keep<MODE>(v[k], c, inv_weight, conf, best[k], am[k], s[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < TTA_ROWS; ++k) {
      const int y = g * TTA_ROWS + k;
      if (y < Ho) {
        const size_t o = ((size_t)b * Ho + y) * Wo + x;
        segm[o] = am[k];
        if (conf) confidence[o] = tta_confidence<MODE>(best[k], s[k]);
        if (acc_depth != nullptr) depth[o] = inv_weight * v[k];
      }
    }
  }
}

// ------------------------------------------------------------------ entry points
static inline float tta_scale(int in_size, int out_size) { return (float)in_size / (float)out_size; }
static inline bool tta_small(long long P) { return P < (1LL << 31); }
// the tap offsets inside one plane (and 4 * offset inside one image of the view kernel) are ints
static inline bool tta_plane_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= (1LL << 28); }

extern "C" int vmtl_tta_view(const float* img, int ld, float* out, int B, int H, int W, int Ho, int Wo, int flip,
                             void* stream) {
  VMTL_ENTER();
  if (!img || !out || B <= 0 || !tta_plane_ok(H, W) || !tta_plane_ok(Ho, Wo) || (ld != 3 && ld != 4)) return VMTL_ERR_ARG;
  if (((uintptr_t)out & 15) || (ld == 4 && ((uintptr_t)img & 15))) return VMTL_ERR_ARG;
  const long long P = (long long)B * Ho * Wo;
  const bool same = H == Ho && W == Wo, small = tta_small(P);
  const float sh = tta_scale(H, Ho), sw = tta_scale(W, Wo);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(grid_1d(P, 256, 8192)), block(256);
#define TTA_VIEW(LD, SAME) \
  hipLaunchKernelGGL((tta_view_kernel<LD, SAME>), grid, block, 0, st, img, (f32x4*)out, H, W, Ho, Wo, sh, sw, flip, P, small)
  if (ld == 4) {
    if (same) TTA_VIEW(4, true); else TTA_VIEW(4, false);
  } else {
    if (same) TTA_VIEW(3, true); else TTA_VIEW(3, false);
  }
#undef TTA_VIEW
  return vmtl_check_launch();
}

static inline bool tta_mode_ok(int mode) { return mode == VMTL_TTA_PROB || mode == VMTL_TTA_LOGIT; }

// (tests hand the entry points dummy addresses with bad arguments: keep every argument check ahead of the first launch)
extern "C" int vmtl_tta_accumulate(const float* logits, const float* depth_logits, float* acc, float* acc_depth, int B,
                                   int C, int h, int w, int H, int W, int flip, float weight, float depth_gain, int mode,
                                   int first, void* stream) {
  VMTL_ENTER();
  if (!logits || !acc || B <= 0 || !tta_plane_ok(h, w) || !tta_plane_ok(H, W) || !tta_mode_ok(mode)) return VMTL_ERR_ARG;
  if ((depth_logits == nullptr) != (acc_depth == nullptr)) return VMTL_ERR_ARG;
  if (C < 1 || C > TTA_MAX_C) return VMTL_ERR_UNSUPPORTED;
  const long long P = (long long)B * H * W;
  const bool same = h == H && w == W, small = tta_small(P);
  const float sh = tta_scale(h, H), sw = tta_scale(w, W), dw = weight * depth_gain;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(grid_1d(P, 256, 8192)), block(256);
#define TTA_ACC(MODE, SAME)                                                                                          \
  hipLaunchKernelGGL((tta_accumulate_kernel<MODE, SAME>), grid, block, 0, st, logits, depth_logits, acc, acc_depth, C, \
                     h, w, H, W, sh, sw, flip, weight, dw, first, P, small)
  if (mode == VMTL_TTA_PROB) {
    if (same) TTA_ACC(VMTL_TTA_PROB, true); else TTA_ACC(VMTL_TTA_PROB, false);
  } else {
    if (same) TTA_ACC(VMTL_TTA_LOGIT, true); else TTA_ACC(VMTL_TTA_LOGIT, false);
  }
#undef TTA_ACC
  return vmtl_check_launch();
}

extern "C" int vmtl_tta_finish(const float* acc, const float* acc_depth, float inv_weight, long long* segm, float* depth,
                               float* confidence, int B, int C, int H, int W, int Ho, int Wo, int mode, void* stream) {
  VMTL_ENTER();
  if (!acc || !segm || B <= 0 || !tta_plane_ok(H, W) || !tta_plane_ok(Ho, Wo) || !tta_mode_ok(mode)) return VMTL_ERR_ARG;
  if ((acc_depth == nullptr) != (depth == nullptr)) return VMTL_ERR_ARG;
  if (!(inv_weight > 0.f && inv_weight <= 3.0e38f)) return VMTL_ERR_ARG;  // the arg-max is taken on acc itself
  if (C < 1 || C > TTA_MAX_C) return VMTL_ERR_UNSUPPORTED;
  const long long P = (long long)B * Ho * Wo;
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(256);
  if (H == Ho && W == Wo) {
    const long long HW = (long long)H * W;
#define TTA_FIN(MODE)                                                                                            \
  hipLaunchKernelGGL((tta_finish_same_kernel<MODE>), dim3(grid_1d(P, 256, 8192)), block, 0, st, acc, acc_depth, \
                     inv_weight, segm, depth, confidence, C, HW, P, tta_small(P))
    if (mode == VMTL_TTA_PROB) TTA_FIN(VMTL_TTA_PROB); else TTA_FIN(VMTL_TTA_LOGIT);
#undef TTA_FIN
    return vmtl_check_launch();
  }
  const int G = cdiv(Ho, TTA_ROWS);
  const long long PG = (long long)B * G * Wo;
  const float sh = tta_scale(H, Ho), sw = tta_scale(W, Wo);
#define TTA_FIN(MODE)                                                                                             \
  hipLaunchKernelGGL((tta_finish_rows_kernel<MODE>), dim3(grid_1d(PG, 256, 8192)), block, 0, st, acc, acc_depth, \
                     inv_weight, segm, depth, confidence, C, H, W, Ho, Wo, G, sh, sw, PG, tta_small(PG))
  if (mode == VMTL_TTA_PROB) TTA_FIN(VMTL_TTA_PROB); else TTA_FIN(VMTL_TTA_LOGIT);
#undef TTA_FIN
  return vmtl_check_launch();
}
