// NYUv2 sample transform on the device: the reference's per-sample host chain ToTensor() + Resize(size, antialias=True)
// (cfg.py:144-155, applied by data_modules/nyuv2.py:100-141 to the image, the class-id mask and the uint16 depth PNG),
// followed by the value rules of data.prepare_sample(dataset="nyuv2").
//
// The filter is PyTorch's CPU _upsample_bilinear2d_aa, reproduced operation by operation so that the result is the same
// float32 value, not merely a close one (the mask and depth are rounded back to integers, where one ulp can flip k+0.5):
//   * per axis: scale = (float)in / out, support = scale >= 1 ? scale : 1, invscale = (float)(1.0 / scale) (or 1),
//     center = (float)(scale * (i + 0.5)), xmin = max((long)((center - support) + 0.5), 0),
//     xsize = min((long)((center + support) + 0.5), in) - xmin, with the float / double promotions of the C++ source;
//   * tap weight tri(((float)(xmin + j) - center + 0.5) * invscale), tri(t) = max(0, 1 - |t|), normalised by the float
//     sum of the taps;
//   * separable, WIDTH FIRST, then height (the CPU kernel resamples the contiguous dimension first; the other order
//     differs from it in the last bit for most downscaled pixels), each pass accumulating
//     acc = x0*w0, acc = fma(xj, wj, acc) in tap order (the vectorised CPU build contracts the accumulation into FMAs).
//
// One workgroup per (sample, TH x TW output tile).  Its input window rows are staged chunk by chunk: raw uint8 / uint16 /
// int32 bytes of every plane arrive in LDS by 16-byte loads, the width pass writes an fp32 [5][rows][TW] tile, and each
// thread accumulates the height pass of its two output pixels over the chunk's taps.  Outputs: the image straight into the
// model's NHWC input storage [B][Ho][Wo][4] (one 16-byte store per pixel, pad channel 0), the mask as int64 class ids
// (round half to even of m*255), the depth as rint(counts) / 1e4 plus one per-tile maximum.  A second launch takes each
// sample's maximum over its tiles (max is exact and order-free) and applies the `/ max_depth when > 1` rule in place.
#include <stdint.h>

#include "../../include/vmtl.h"
#include "common.h"

namespace {

constexpr int RS_NT = 256;          // threads per workgroup
constexpr int RS_TH = 8;            // output rows per tile
constexpr int RS_SLOTS = 2;         // output pixels per thread: TH * TW <= RS_NT * RS_SLOTS
constexpr int RS_LDS = 52 * 1024;   // dynamic LDS cap: with the static 1 KB, three workgroups per CU (160 KB)
constexpr int RS_SG = 4;           // staging loads in flight per thread
constexpr int RS_MIN_ROWS = 8;      // a tile width is taken when its chunk holds >= min(window rows, this)

__host__ __device__ inline int imin(int a, int b) { return a < b ? a : b; }

struct AxisAA {
  float scale, support, invscale;
  int n_in, K;  // K: taps per output (PyTorch's max_interp_size)
};

__host__ __device__ inline AxisAA axis_aa(int n_in, int n_out) {
  AxisAA a;
  a.scale = (float)n_in / (float)n_out;
  a.support = a.scale >= 1.0f ? a.scale : 1.0f;
  a.invscale = a.scale >= 1.0f ? (float)(1.0 / (double)a.scale) : 1.0f;
  a.n_in = n_in;
  a.K = (int)ceil((double)a.support) * 2 + 1;
  return a;
}

// taps [xmin, xmin + xsize) of output index i
__host__ __device__ inline void aa_range(const AxisAA& a, int i, float& center, int& xmin, int& xsize) {
  center = (float)((double)a.scale * (i + 0.5));
  const long long lo = (long long)((double)(center - a.support) + 0.5);
  const long long hi = (long long)((double)(center + a.support) + 0.5);
  xmin = (int)(lo > 0 ? lo : 0);
  xsize = (int)(hi < a.n_in ? hi : a.n_in) - xmin;
  xsize = xsize < 0 ? 0 : (xsize > a.K ? a.K : xsize);
}

__device__ inline void aa_weights(const AxisAA& a, int i, int& xmin, int& xsize, float* w) {
  float center;
  aa_range(a, i, center, xmin, xsize);
  float total = 0.f;
  for (int j = 0; j < xsize; ++j) {
    float t = (float)(((double)((float)(j + xmin) - center) + 0.5) * (double)a.invscale);
    t = fabsf(t);
    const float v = t < 1.0f ? (float)(1.0 - (double)t) : 0.f;
    w[j] = v;
    total += v;
  }
  if (total != 0.f)
    for (int j = 0; j < xsize; ++j) w[j] = w[j] / total;
}

struct ResizeP {
  const uint8_t* plane[3];  // img (3 B/px), mask (1 B/px), depth (2 or 4 B/px)
  long long plane_bytes[3];
  int bpp[3];
  float* img_out;
  long long* mask_out;
  float* depth_out;
  float* part;  // [B][tiles_y][tiles_x] per-tile depth maxima
  int B, Hi, Wi, Ho, Wo;
  AxisAA ax, ay;
  int TW, R;            // tile width, input rows per staged chunk
  int tiles_x, tiles_y;
  int seg16[3];         // LDS granules per staged row and plane
  int row_bytes;        // LDS bytes per staged row (all planes)
  int off_wy, off_idx, off_raw, off_h;  // LDS byte offsets
};

struct Plan {
  int TW, R, seg16[3], row_bytes, off_wy, off_idx, off_raw, off_h, lds;
};

// the widest tile whose LDS fits: wx [TW][Kx], wy [TH][Ky], xmin/xsize/ymin/ysize, then R staged rows of raw bytes and
// of width-pass output [5][R][TW]
static bool make_plan(const AxisAA& ax, const AxisAA& ay, int Ho, int Wo, const int bpp[3], Plan& pl) {
  int yspan = 0;
  for (int t0 = 0; t0 < Ho; t0 += RS_TH) {
    const int t1 = (t0 + RS_TH < Ho ? t0 + RS_TH : Ho) - 1;
    float c;
    int a0, s0, a1, s1;
    aa_range(ay, t0, c, a0, s0);
    aa_range(ay, t1, c, a1, s1);
    if (a1 + s1 - a0 > yspan) yspan = a1 + s1 - a0;
  }
  static const int widths[] = {64, 32, 16, 8, 4, 2, 1};
  for (int TW : widths) {
    int xspan = 0;
    for (int t0 = 0; t0 < Wo; t0 += TW) {
      const int t1 = (t0 + TW < Wo ? t0 + TW : Wo) - 1;
      float c;
      int a0, s0, a1, s1;
      aa_range(ax, t0, c, a0, s0);
      aa_range(ax, t1, c, a1, s1);
      if (a1 + s1 - a0 > xspan) xspan = a1 + s1 - a0;
    }
    Plan p;
    p.TW = TW;
    p.row_bytes = 0;
    for (int k = 0; k < 3; ++k) {
      p.seg16[k] = (xspan * bpp[k] + 30) / 16 + 1;  // the span plus the 16-byte alignment of both of its ends
      p.row_bytes += 16 * p.seg16[k];
    }
    p.off_wy = 4 * TW * ax.K;
    p.off_idx = p.off_wy + 4 * RS_TH * ay.K;
    p.off_raw = (p.off_idx + 4 * 2 * (TW + RS_TH) + 15) / 16 * 16;
    const int per_row = p.row_bytes + 4 * 5 * TW;
    const int fit = (RS_LDS - p.off_raw) / per_row;
    p.R = fit < yspan ? fit : yspan;
    if (p.R >= (yspan < RS_MIN_ROWS ? yspan : RS_MIN_ROWS) || (TW == 1 && p.R >= 1)) {
      p.off_h = p.off_raw + p.R * p.row_bytes;
      p.lds = p.off_h + 4 * 5 * p.R * TW;
      pl = p;
      return true;
    }
  }
  return false;
}

__global__ __launch_bounds__(RS_NT) void nyuv2_resize_kernel(ResizeP p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rs_smem[];
  float* wx = reinterpret_cast<float*>(rs_smem);
  float* wy = reinterpret_cast<float*>(rs_smem + p.off_wy);
  int* xmin = reinterpret_cast<int*>(rs_smem + p.off_idx);
  int* xsz = xmin + p.TW;
  int* ymin = xsz + p.TW;
  int* ysz = ymin + RS_TH;
  uint8_t* raw = rs_smem + p.off_raw;
  float* hb = reinterpret_cast<float*>(rs_smem + p.off_h);
  __shared__ unsigned tile_max;
  __shared__ float u8f[256];  // u8 / 255.0f: ToTensor's division, once per workgroup

  const int tid = threadIdx.x, TW = p.TW, R = p.R;
  const int txi = blockIdx.x % p.tiles_x, tyi = blockIdx.x / p.tiles_x, b = blockIdx.y;
  const int ox0 = txi * TW, oy0 = tyi * RS_TH;
  const int nx = (imin(p.Wo - ox0, TW)), ny = (imin(p.Ho - oy0, RS_TH));

  // per-axis taps of this tile
  for (int i = tid; i < nx + ny; i += RS_NT) {
    if (i < nx) aa_weights(p.ax, ox0 + i, xmin[i], xsz[i], wx + i * p.ax.K);
    else aa_weights(p.ay, oy0 + i - nx, ymin[i - nx], ysz[i - nx], wy + (i - nx) * p.ay.K);
  }
  u8f[tid] = (float)tid / 255.0f;
  if (tid == 0) tile_max = 0u;
  __syncthreads();
  const int X0 = xmin[0], X1 = xmin[nx - 1] + xsz[nx - 1], Y0 = ymin[0], Y1 = ymin[ny - 1] + ysz[ny - 1];

  float acc[RS_SLOTS][5];
#pragma unroll
  for (int s = 0; s < RS_SLOTS; ++s)
#pragma unroll
    for (int c = 0; c < 5; ++c) acc[s][c] = 0.f;

  const int seg_all = p.seg16[0] + p.seg16[1] + p.seg16[2];
  for (int r0 = Y0; r0 < Y1; r0 += R) {
    const int nr = Y1 - r0 < R ? Y1 - r0 : R;
    // 1. stage the raw bytes of rows [r0, r0 + nr), columns [X0, X1) of every plane: 16-byte loads of the aligned
    //    granules that cover them (byte loads for a granule that would cross the end of the buffer), RS_SG loads in
    //    flight per thread before the first LDS store
    for (int i0 = 0; i0 < nr * seg_all; i0 += RS_SG * RS_NT) {
      uint4 v[RS_SG];
      int dst[RS_SG];
#pragma unroll
      for (int u = 0; u < RS_SG; ++u) {
        const int i = i0 + u * RS_NT + tid;
        dst[u] = -1;
        if (i >= nr * seg_all) continue;
        const int rr = i / seg_all;
        int g = i - rr * seg_all, k = 0, off = rr * p.row_bytes;
        if (g >= p.seg16[0]) g -= p.seg16[0], off += 16 * p.seg16[0], k = 1;
        if (k == 1 && g >= p.seg16[1]) g -= p.seg16[1], off += 16 * p.seg16[1], k = 2;
        // plane fields by selection, not by a dynamic index (which would put the argument block in scratch)
        const int bpp = k == 0 ? p.bpp[0] : k == 1 ? p.bpp[1] : p.bpp[2];
        const uint8_t* base = k == 0 ? p.plane[0] : k == 1 ? p.plane[1] : p.plane[2];
        const long long nb = k == 0 ? p.plane_bytes[0] : k == 1 ? p.plane_bytes[1] : p.plane_bytes[2];
        const long long row = ((long long)b * p.Hi + r0 + rr) * p.Wi * bpp;
        const long long a = ((row + (long long)X0 * bpp) & ~15ll) + 16ll * g;
        if (a >= row + (long long)X1 * bpp) continue;  // past the window: never read
        if (a + 16 <= nb) {
          v[u] = *reinterpret_cast<const uint4*>(base + a);
        } else {
          unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
          for (int q = 0; q < 16; ++q)
            if (a + q < nb) w[q >> 2] |= (unsigned)base[a + q] << (8 * (q & 3));
          v[u] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        dst[u] = off + 16 * g;
      }
#pragma unroll
      for (int u = 0; u < RS_SG; ++u)
        if (dst[u] >= 0) *reinterpret_cast<uint4*>(raw + dst[u]) = v[u];
    }
    __syncthreads();
    // 2. width pass: [5][nr][TW] fp32
    for (int i = tid; i < nr * TW; i += RS_NT) {
      const int rr = i / TW, tx = i - rr * TW;
      if (tx >= nx) continue;
      const uint8_t* rowp[3];
      int off = rr * p.row_bytes;
      long long rbase[3];
      for (int k = 0; k < 3; ++k) {
        const long long row = ((long long)b * p.Hi + r0 + rr) * p.Wi * p.bpp[k];
        rbase[k] = row - ((row + (long long)X0 * p.bpp[k]) & ~15ll);  // LDS offset of the row's column 0
        rowp[k] = raw + off;
        off += 16 * p.seg16[k];
      }
      const float* w = wx + tx * p.ax.K;
      float h0 = 0.f, h1 = 0.f, h2 = 0.f, hm = 0.f, hd = 0.f;
      for (int j = 0, x = xmin[tx]; j < xsz[tx]; ++j, ++x) {
        const uint8_t* pi = rowp[0] + rbase[0] + 3 * x;
        const float wj = w[j];
        h0 = fmaf(u8f[pi[0]], wj, h0);
        h1 = fmaf(u8f[pi[1]], wj, h1);
        h2 = fmaf(u8f[pi[2]], wj, h2);
        hm = fmaf(u8f[rowp[1][rbase[1] + x]], wj, hm);
        const uint8_t* pd = rowp[2] + rbase[2] + (long long)p.bpp[2] * x;
        const float dv = p.bpp[2] == 2 ? (float)*reinterpret_cast<const uint16_t*>(pd)
                                       : (float)*reinterpret_cast<const int32_t*>(pd);
        hd = fmaf(dv, wj, hd);
      }
      const int o = rr * TW + tx, cs = R * TW;
      hb[o] = h0;
      hb[o + cs] = h1;
      hb[o + 2 * cs] = h2;
      hb[o + 3 * cs] = hm;
      hb[o + 4 * cs] = hd;
    }
    __syncthreads();
    // 3. height pass over the taps that fall in this chunk, in tap order
#pragma unroll
    for (int s = 0; s < RS_SLOTS; ++s) {
      const int q = tid + s * RS_NT, ty = q / TW, tx = q - ty * TW;
      if (ty >= ny || tx >= nx) continue;
      const int j0 = r0 - ymin[ty] > 0 ? r0 - ymin[ty] : 0;
      const int j1 = imin(ysz[ty], r0 + nr - ymin[ty]);
      const float* w = wy + ty * p.ay.K;
      for (int j = j0; j < j1; ++j) {
        const int o = (ymin[ty] + j - r0) * TW + tx, cs = R * TW;
        const float wj = w[j];
#pragma unroll
        for (int c = 0; c < 5; ++c) acc[s][c] = fmaf(hb[o + c * cs], wj, acc[s][c]);
      }
    }
    __syncthreads();  // the next chunk overwrites raw and hb
  }

  // 4. outputs
  unsigned dmax = 0u;
#pragma unroll
  for (int s = 0; s < RS_SLOTS; ++s) {
    const int q = tid + s * RS_NT, ty = q / TW, tx = q - ty * TW;
    if (ty >= ny || tx >= nx) continue;
    const long long pix = ((long long)b * p.Ho + oy0 + ty) * p.Wo + ox0 + tx;
    f32x4 v = {acc[s][0], acc[s][1], acc[s][2], 0.f};
    *reinterpret_cast<f32x4*>(p.img_out + 4 * pix) = v;
    p.mask_out[pix] = (long long)rintf(acc[s][3] * 255.0f);
    const float d = rintf(acc[s][4]) / 10000.0f;  // counts -> metres (nyuv2.py:126-127)
    p.depth_out[pix] = d;
    const unsigned bits = __float_as_uint(d);  // d >= 0: the bit patterns order like the values
    dmax = bits > dmax ? bits : dmax;
  }
  atomicMax(&tile_max, dmax);
  __syncthreads();
  if (tid == 0) p.part[((long long)b * p.tiles_y + tyi) * p.tiles_x + txi] = __uint_as_float(tile_max);
}

// depth /= max_depth on the samples whose resized maximum exceeds 1 (common_ds.py:47-50)
__global__ __launch_bounds__(RS_NT) void nyuv2_depth_scale_kernel(float* __restrict__ depth, const float* __restrict__ part,
                                                                   int ntiles, long long HW, float max_depth) {
  __shared__ unsigned smax;
  const int b = blockIdx.y;
  if (threadIdx.x == 0) smax = 0u;
  __syncthreads();
  unsigned m = 0u;
  for (int i = threadIdx.x; i < ntiles; i += RS_NT) {
    const unsigned v = __float_as_uint(part[(long long)b * ntiles + i]);
    m = v > m ? v : m;
  }
  atomicMax(&smax, m);
  __syncthreads();
  if (!(__uint_as_float(smax) > 1.0f)) return;
  float* d = depth + (long long)b * HW;
  for (long long i = (long long)blockIdx.x * RS_NT + threadIdx.x; i < HW; i += (long long)gridDim.x * RS_NT)
    d[i] = d[i] / max_depth;
}

static int depth_bpp(int depth_dtype) {
  return depth_dtype == VMTL_DEPTH_U16 ? 2 : depth_dtype == VMTL_DEPTH_I32 ? 4 : 0;
}

static bool sizes_ok(int B, int Hi, int Wi, int Ho, int Wo) {
  return B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && B <= 65535;
}

}  // namespace

extern "C" int vmtl_nyuv2_resize_parts(int B, int Hi, int Wi, int Ho, int Wo, int depth_dtype) {
  const int dbpp = depth_bpp(depth_dtype);
  if (!sizes_ok(B, Hi, Wi, Ho, Wo) || !dbpp) return VMTL_ERR_ARG;
  const int bpp[3] = {3, 1, dbpp};
  Plan pl;
  if (!make_plan(axis_aa(Wi, Wo), axis_aa(Hi, Ho), Ho, Wo, bpp, pl)) return VMTL_ERR_UNSUPPORTED;
  return B * cdiv(Ho, RS_TH) * cdiv(Wo, pl.TW);
}

extern "C" int vmtl_nyuv2_resize(const void* img, const void* mask, const void* depth, int depth_dtype, float* img_out,
                                 long long* mask_out, float* depth_out, float* part, int B, int Hi, int Wi, int Ho,
                                 int Wo, float max_depth, void* stream) {
  const int dbpp = depth_bpp(depth_dtype);
  if (!img || !mask || !depth || !img_out || !mask_out || !depth_out || !part || !dbpp || !sizes_ok(B, Hi, Wi, Ho, Wo) ||
      !(max_depth > 0.f))
    return VMTL_ERR_ARG;
  if (((uintptr_t)img | (uintptr_t)mask | (uintptr_t)depth | (uintptr_t)img_out) & 15) return VMTL_ERR_ARG;
  ResizeP p;
  p.bpp[0] = 3;
  p.bpp[1] = 1;
  p.bpp[2] = dbpp;
  p.ax = axis_aa(Wi, Wo);
  p.ay = axis_aa(Hi, Ho);
  Plan pl;
  if (!make_plan(p.ax, p.ay, Ho, Wo, p.bpp, pl)) return VMTL_ERR_UNSUPPORTED;
  VMTL_ENTER();
  p.plane[0] = (const uint8_t*)img;
  p.plane[1] = (const uint8_t*)mask;
  p.plane[2] = (const uint8_t*)depth;
  for (int k = 0; k < 3; ++k) p.plane_bytes[k] = (long long)B * Hi * Wi * p.bpp[k];
  p.img_out = img_out;
  p.mask_out = mask_out;
  p.depth_out = depth_out;
  p.part = part;
  p.B = B, p.Hi = Hi, p.Wi = Wi, p.Ho = Ho, p.Wo = Wo;
  p.TW = pl.TW, p.R = pl.R;
  p.tiles_x = cdiv(Wo, pl.TW), p.tiles_y = cdiv(Ho, RS_TH);
  for (int k = 0; k < 3; ++k) p.seg16[k] = pl.seg16[k];
  p.row_bytes = pl.row_bytes;
  p.off_wy = pl.off_wy, p.off_idx = pl.off_idx, p.off_raw = pl.off_raw, p.off_h = pl.off_h;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nyuv2_resize_kernel, dim3(p.tiles_x * p.tiles_y, B), dim3(RS_NT), pl.lds, st, p);
  if (vmtl_check_launch() != VMTL_OK) return VMTL_ERR_LAUNCH;
  const long long HW = (long long)Ho * Wo;
  const int gx = (int)(cdivll(HW, 4ll * RS_NT) < 1024 ? cdivll(HW, 4ll * RS_NT) : 1024);
  hipLaunchKernelGGL(nyuv2_depth_scale_kernel, dim3(gx, B), dim3(RS_NT), 0, st, depth_out, part,
                     p.tiles_x * p.tiles_y, HW, max_depth);
  return vmtl_check_launch();
}
