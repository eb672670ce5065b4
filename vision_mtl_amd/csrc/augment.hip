// Joint training augmentation on the device: MTAN's recipe of the multi-task literature, random
// scale-crop + horizontal flip (+ an optional brightness gain), applied to image, class-id mask and depth together on a
// batch that is already on the GPU.  The reference trains without augmentation (cfg.py:103-155: train_transform ==
// test_transform), so there is no reference code to mirror; the definition is torch's CPU F.interpolate, restated:
//   image : bilinear, align_corners=True, of the crop window [top, top+h) x [left, left+w) back to H x W
//           (scale = (float)(h-1) / (float)(H-1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < h-1),
//           l1 = src - i0, l0 = 1 - l1, v = ly0*(lx0*p00 + lx1*p01) + ly1*(lx0*p10 + lx1*p11))
//   mask, depth : nearest (scale = (float)h / (float)H, i = min((int)floorf(dst * scale), h-1)), depth / s (IEEE divide)
//   then the image gain with a clamp to [0,1] (only when gain != 1), then the flip.
// Nearest sampling never blends labels: ignore_index pixels and invalid (zero) depth pixels stay what the loss kernels
// of csrc/loss.hip expect.
//
// Two launches, neither allocates nor synchronises (both are captured by graphed.GraphedStep):
//   augment_draw_kernel  : ONE workgroup draws params[B][8] from the device state {seed, counter} with a counter-based
//                          generator and then advances the counter, so every replay of a captured graph draws afresh.
//   augment_apply_kernel : a plain gather, one thread per DESTINATION pixel.  A wavefront owns 64 consecutive x of one
//                          output row, a workgroup 4 rows: whatever the flip, its stores are contiguous (64 x 16 bytes of
//                          image, 64 x 8 of mask, 64 x 4 of depth); the flip only reverses the order of the reads.  The
//                          per-sample parameters and the scale tables are wave-uniform loads.
#include <stdint.h>

#include "../../include/vmtl.h"
#include "common.h"

namespace {

constexpr int AUG_NT = 256;     // threads per workgroup
constexpr int AUG_TW = 64;      // output columns per workgroup: one wavefront per row segment
constexpr int AUG_TH = AUG_NT / AUG_TW;
constexpr int AUG_MAX_S = 8;    // scales
constexpr int AUG_NP = 8;       // int32 words per parameter row
constexpr unsigned long long AUG_G = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// r24(b, k) = mix(mix(seed + G*(counter+1)) + G*(8*b + k + 1)) >> 40; every range reduction is (r24 * n) >> 24 in
// integers (a float product u * n can round up to n)
__global__ __launch_bounds__(AUG_NT) void augment_draw_kernel(long long* state, int* __restrict__ params,
                                                              const int* __restrict__ crop_hw, int B, int H, int W, int S,
                                                              int flip_threshold, float brightness) {
  const unsigned long long seed = (unsigned long long)state[0], counter = (unsigned long long)state[1];
  const unsigned long long base = mix64(seed + AUG_G * (counter + 1ull));
  for (int b = threadIdx.x; b < B; b += AUG_NT) {
    unsigned long long r[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) r[k] = mix64(base + AUG_G * (8ull * (unsigned long long)b + (unsigned long long)k + 1ull)) >> 40;
    const int si = (int)((r[0] * (unsigned long long)S) >> 24);
    const int h = clampi(crop_hw[2 * si], 1, H), w = clampi(crop_hw[2 * si + 1], 1, W);
    const int top = (int)((r[1] * (unsigned long long)(H - h + 1)) >> 24);
    const int left = (int)((r[2] * (unsigned long long)(W - w + 1)) >> 24);
    const int flip = r[3] < (unsigned long long)flip_threshold ? 1 : 0;
    const float u = (float)(unsigned)r[4] * 0x1p-24f;
    const float gain = 1.0f + (2.0f * u - 1.0f) * brightness;
    int4* row = reinterpret_cast<int4*>(params + (long long)b * AUG_NP);
    row[0] = make_int4(si, top, left, flip);
    row[1] = make_int4(__float_as_int(gain), 0, 0, 0);
  }
  __syncthreads();  // every thread has read the counter: one thread advances it for the next launch / replay
  if (threadIdx.x == 0) state[1] = (long long)(counter + 1ull);
}

struct AugP {
  const float* img;
  const long long* mask;
  const float* depth;
  const int* params;
  const float* scales;
  const int* crop_hw;
  float* img_out;
  long long* mask_out;
  float* depth_out;
  int H, W, S;
};

// source index and weights of one axis of the bilinear resample (torch's guard_index_and_lambda, align_corners=True)
__device__ __forceinline__ void lin_axis(int dst, int n_in, int n_out, int& i0, int& i1, float& l0, float& l1) {
  // the product is rounded before the subtraction below, as on the host: contracted into one FMA (hipcc's default),
  // src - i0 differs from torch's weight by up to an ulp of src (4e-6 at src = 36), and the pixel with it - measured
  // 1.7e-6 on a 37x70 batch
#pragma clang fp contract(off)
  const float scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
  const float src = scale * (float)dst;
  i0 = (int)src;
  i0 = i0 < n_in - 1 ? i0 : n_in - 1;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
  l0 = 1.f - l1;
}

__device__ __forceinline__ int near_axis(int dst, int n_in, int n_out) {
  const int i = (int)floorf((float)dst * ((float)n_in / (float)n_out));
  return i < n_in - 1 ? i : n_in - 1;
}

template <int LD>
__device__ __forceinline__ void load_px(const float* p, float& r, float& g, float& b) {
  if (LD == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    r = v.x, g = v.y, b = v.z;
  } else {
    r = p[0], g = p[1], b = p[2];
  }
}

template <int LD>
__global__ __launch_bounds__(AUG_NT) void augment_apply_kernel(AugP p) {
  const int H = p.H, W = p.W, b = blockIdx.z;
  const int xd = blockIdx.x * AUG_TW + (threadIdx.x & (AUG_TW - 1));  // destination column: stores stay contiguous
  const int y = blockIdx.y * AUG_TH + threadIdx.x / AUG_TW;
  // the sample's row, clamped: a hand-made parameter row cannot send a read out of bounds
  const int* pr = p.params + (long long)b * AUG_NP;
  const int si = clampi(pr[0], 0, p.S - 1);
  const int h = clampi(p.crop_hw[2 * si], 1, H), w = clampi(p.crop_hw[2 * si + 1], 1, W);
  const int top = clampi(pr[1], 0, H - h), left = clampi(pr[2], 0, W - w);
  const bool flip = pr[3] != 0;
  const float gain = __int_as_float(pr[4]);
  const float s = p.scales[si];
  if (xd >= W || y >= H) return;
  const int x = flip ? W - 1 - xd : xd;

  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  lin_axis(y, h, H, y0, y1, ly0, ly1);
  lin_axis(x, w, W, x0, x1, lx0, lx1);
  const long long plane = (long long)b * H * W;
  const float* r0 = p.img + (plane + (long long)(top + y0) * W + left) * LD;
  const float* r1 = p.img + (plane + (long long)(top + y1) * W + left) * LD;
  float a[3], c[3], d[3], e[3];
  load_px<LD>(r0 + (long long)x0 * LD, a[0], a[1], a[2]);
  load_px<LD>(r0 + (long long)x1 * LD, c[0], c[1], c[2]);
  load_px<LD>(r1 + (long long)x0 * LD, d[0], d[1], d[2]);
  load_px<LD>(r1 + (long long)x1 * LD, e[0], e[1], e[2]);
  const long long near = plane + (long long)(top + near_axis(y, h, H)) * W + left + near_axis(x, w, W);
  const long long m = p.mask[near];
  const float dep = p.depth[near];

  float v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = ly0 * (lx0 * a[k] + lx1 * c[k]) + ly1 * (lx0 * d[k] + lx1 * e[k]);
    if (gain != 1.0f) v[k] = fminf(fmaxf(v[k] * gain, 0.f), 1.f);
  }
  const long long o = plane + (long long)y * W + xd;
  const f32x4 px = {v[0], v[1], v[2], 0.f};
  *reinterpret_cast<f32x4*>(p.img_out + 4 * o) = px;
  p.mask_out[o] = m;
  p.depth_out[o] = dep / s;
}

static bool overlaps(const void* a, long long na, const void* b, long long nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

}  // namespace

extern "C" int vmtl_augment_draw(long long* state, int* params, const int* crop_hw, int B, int H, int W, int S,
                                 int flip_threshold, float brightness, void* stream) {
  if (!state || !params || !crop_hw || B <= 0 || H <= 0 || W <= 0 || S < 1 || S > AUG_MAX_S || flip_threshold < 0 ||
      flip_threshold > (1 << 24) || !(brightness >= 0.f && brightness < 1.f))
    return VMTL_ERR_ARG;
  if (((uintptr_t)params & 15) || ((uintptr_t)state & 7)) return VMTL_ERR_ARG;
  VMTL_ENTER();
  hipLaunchKernelGGL(augment_draw_kernel, dim3(1), dim3(AUG_NT), 0, (hipStream_t)stream, state, params, crop_hw, B, H, W,
                     S, flip_threshold, brightness);
  return vmtl_check_launch();
}

extern "C" int vmtl_augment_apply(const float* img, int ld, const long long* mask, const float* depth, const int* params,
                                  const float* scales, const int* crop_hw, float* img_out, long long* mask_out,
                                  float* depth_out, int B, int H, int W, int S, void* stream) {
  if (!img || !mask || !depth || !params || !scales || !crop_hw || !img_out || !mask_out || !depth_out ||
      (ld != 3 && ld != 4) || B <= 0 || H <= 0 || W <= 0 || S < 1 || S > AUG_MAX_S)
    return VMTL_ERR_ARG;
  if (B > 65535 || cdiv(H, AUG_TH) > 65535) return VMTL_ERR_ARG;
  if (((uintptr_t)img_out & 15) || (ld == 4 && ((uintptr_t)img & 15)) || ((uintptr_t)mask & 7) ||
      ((uintptr_t)mask_out & 7))
    return VMTL_ERR_ARG;
  const long long P = (long long)B * H * W;
  // the gather reads pixels other workgroups write: an output may not alias its input
  if (overlaps(img, 4 * P * ld, img_out, 16 * P) || overlaps(mask, 8 * P, mask_out, 8 * P) ||
      overlaps(depth, 4 * P, depth_out, 4 * P))
    return VMTL_ERR_ARG;
  VMTL_ENTER();
  AugP p;
  p.img = img, p.mask = mask, p.depth = depth, p.params = params, p.scales = scales, p.crop_hw = crop_hw;
  p.img_out = img_out, p.mask_out = mask_out, p.depth_out = depth_out;
  p.H = H, p.W = W, p.S = S;
  const dim3 grid(cdiv(W, AUG_TW), cdiv(H, AUG_TH), B);
  if (ld == 4)
    hipLaunchKernelGGL(augment_apply_kernel<4>, grid, dim3(AUG_NT), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(augment_apply_kernel<3>, grid, dim3(AUG_NT), 0, (hipStream_t)stream, p);
  return vmtl_check_launch();
}
