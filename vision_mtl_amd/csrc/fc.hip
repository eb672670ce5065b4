// Per-image fully connected layers (batch-sized GEMMs, M = B <= 64 rows) and the per-image spatial
// reductions around them: the squeeze-excite gate of the MobileNetV3 encoder (timm SqueezeExcite, the
// `basic` model's encoder: reference vision_mtl/models/basic_model.py:17-28 via smp/timm).
//
// A 32 x 960 x 240 product has two 64x144 tiles: run through the implicit-GEMM conv kernel it occupies two
// CUs for 30 dependent K steps.  Here a workgroup owns 16 output columns and ALL rows; its four waves split
// K, load both MFMA operands straight from global memory (no LDS staging: nothing is shared between waves)
// and combine through LDS once at the end.  N/16 workgroups, ~K/64 loads deep.
//
// The A operand can be handed over as `a_parts` partial sums ([parts][M][lda], summed and scaled on load):
// that is how the spatial mean / the gate gradient reach the GEMM without a finalize launch.  With `a_z`
// the A operand is multiplied by act'(a_z) on load (activation backward fused into the data gradient).
#include "common.h"

struct FcP {
  const float* a;     // [a_parts][M][lda]
  const float* a_z;   // nullable [M][lda]: pre-activations whose act_grad masks the A operand
  const float* w;     // [N][ldw], K contiguous
  const float* bias;  // nullable [N]
  float* a_out;       // nullable [M][lda]: the finished A operand (parts summed and scaled, before the a_z mask)
  float* z;           // nullable [M][ldy] pre-activation output
  float* y;           // [M][ldy] = act(z); pad columns zero
  long long a_part_stride;
  float a_scale;
  int a_parts, a_act;
  int M, K, N, lda, ldw, ldy, act;
};

#define FC_WAVES 8   // waves per workgroup, all splitting K
#define FC_UNROLL 4  // K chunks whose loads are issued together (the loop is load-latency bound)

template <int MT>
__global__ __launch_bounds__(FC_WAVES * 64) void fc_kernel(FcP p) {
  __shared__ f32x4 red[FC_WAVES][MT][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int n = n0 + l15;
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nchunks = (p.K + 15) >> 4;
  const bool wvec = (p.ldw & 3) == 0;
  for (int c0 = wv; c0 < nchunks; c0 += FC_WAVES * FC_UNROLL) {
    f32x4 fb[FC_UNROLL], fa[FC_UNROLL][MT];
#pragma unroll
    for (int u = 0; u < FC_UNROLL; ++u) {
      const int c = c0 + u * FC_WAVES;
      const int k4 = c * 16 + lq * 4;
      fb[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (c < nchunks && n < p.N && k4 < p.K) {
        const float* wp = p.w + (size_t)n * p.ldw + k4;
        if (wvec && k4 + 3 < p.K) {
          fb[u] = *reinterpret_cast<const f32x4*>(wp);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (k4 + e < p.K) fb[u][e] = wp[e];
        }
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int m = t * 16 + l15;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c < nchunks && m < p.M && k4 < p.lda) {
          const float* ap = p.a + (size_t)m * p.lda + k4;
          v = *reinterpret_cast<const f32x4*>(ap);
          for (int s = 1; s < p.a_parts; ++s) v += *reinterpret_cast<const f32x4*>(ap + s * p.a_part_stride);
          v *= p.a_scale;
          // every workgroup computes the same finished operand: workgroup (c mod grid) keeps chunk c
          if (p.a_out != nullptr && (c % (int)gridDim.x) == (int)blockIdx.x)
            *reinterpret_cast<f32x4*>(p.a_out + (size_t)m * p.lda + k4) = v;
          if (p.a_z != nullptr) {
            const f32x4 zv = *reinterpret_cast<const f32x4*>(p.a_z + (size_t)m * p.lda + k4);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= act_grad(zv[e], p.a_act);
          }
        }
        fa[u][t] = v;
      }
    }
#pragma unroll
    for (int u = 0; u < FC_UNROLL; ++u)
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[u][t][e], fb[u][e], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) red[wv][t][lane] = acc[t];
  __syncthreads();
  // C layout of 16x16x4: col = lane & 15, row = 4 * (lane >> 4) + reg.  Thread (ln, rg) finishes element rg of
  // lane ln's accumulator, tiles rt, rt + 2, ... (8 waves -> 2 tiles in flight)
  if (tid >= 512) return;
  const int ln = tid & 63, rg = (tid >> 6) & 3, rt = tid >> 8;
  const int col = ln & 15, row = 4 * (ln >> 4) + rg;
  const int nn = n0 + col;
  if (nn >= p.ldy) return;
  const float bv = (p.bias != nullptr && nn < p.N) ? p.bias[nn] : 0.f;
  for (int t = rt; t < MT; t += 2) {
    const int m = t * 16 + row;
    if (m >= p.M) continue;
    const float* r0 = reinterpret_cast<const float*>(&red[0][t][ln]) + rg;
    constexpr int WS = MT * 64 * 4;  // floats between the per-wave copies
    float v = bv;
#pragma unroll
    for (int w = 0; w < FC_WAVES; ++w) v += r0[w * WS];
    if (nn >= p.N) v = 0.f;
    if (p.z != nullptr) p.z[(size_t)m * p.ldy + nn] = v;
    p.y[(size_t)m * p.ldy + nn] = nn < p.N ? act_fwd(v, p.act) : 0.f;
  }
}

extern "C" int vmtl_fc_max_rows() { return 64; }

extern "C" int vmtl_fc_fwd(const float* a, int a_parts, long long a_part_stride, float a_scale, const float* a_z,
                           int a_act, float* a_out, const float* w, const float* bias, float* z, float* y, int M,
                           int K, int N, int lda, int ldw, int ldy, int act, void* stream) {
  VMTL_ENTER();
  if (!a || !w || !y || M <= 0 || M > 64 || K <= 0 || N <= 0 || (lda & 3) || lda < K || ldw < K || ldy < N ||
      a_parts < 1 || (a_parts > 1 && (a_part_stride & 3)))
    return VMTL_ERR_ARG;
  FcP p{a, a_z, w, bias, a_out, z, y, a_part_stride, a_scale, a_parts, a_act, M, K, N, lda, ldw, ldy, act};
  const dim3 grid(cdiv(ldy, 16));
  hipStream_t st = (hipStream_t)stream;
  switch (cdiv(M, 16)) {
    case 1: hipLaunchKernelGGL(fc_kernel<1>, grid, dim3(FC_WAVES * 64), 0, st, p); break;
    case 2: hipLaunchKernelGGL(fc_kernel<2>, grid, dim3(FC_WAVES * 64), 0, st, p); break;
    case 3: hipLaunchKernelGGL(fc_kernel<3>, grid, dim3(FC_WAVES * 64), 0, st, p); break;
    default: hipLaunchKernelGGL(fc_kernel<4>, grid, dim3(FC_WAVES * 64), 0, st, p); break;
  }
  return vmtl_check_launch();
}

// dw[n][k] = sum_m dz[m][n] * x[m][k],  db[n] = sum_m dz[m][n],  dz = dyo * act'(zo).  Written in the torch
// parameter layout ((N, K, 1, 1) contiguous): no unpack pass.  8 weight rows per workgroup.
struct FcWgP {
  const float* x;  // [x_parts][M][lda]
  const float* dyo;  // [dy_parts][M][ldn]
  const float* zo;   // nullable [M][ldn]
  float* dw;
  float* db;  // nullable
  long long x_part_stride, dy_part_stride;
  float x_scale;
  int x_parts, dy_parts, M, K, N, lda, ldn, act;
};

// one workgroup's 8 weight rows (bx: its index along N); shared by fc_wgrad_kernel and se_wgrad_kernel
__device__ __forceinline__ void fc_wgrad_block(const FcWgP& p, int bx) {
  __shared__ float dz[64][8];
  const int tid = threadIdx.x;
  const int n0 = bx * 8;
  for (int idx = tid; idx < p.M * 8; idx += 256) {
    const int m = idx >> 3, i = idx & 7, n = n0 + i;
    float v = 0.f;
    if (n < p.N) {
      const size_t off = (size_t)m * p.ldn + n;
      v = p.dyo[off];
      for (int s = 1; s < p.dy_parts; ++s) v += p.dyo[off + s * p.dy_part_stride];
      if (p.zo != nullptr) v *= act_grad(p.zo[off], p.act);
    }
    dz[m][i] = v;
  }
  __syncthreads();
  for (int k = tid; k < p.K; k += 256) {
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int mb = 0; mb < p.M; mb += 8) {  // 8 independent loads in flight per thread
      float xv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        xv[u] = 0.f;
        if (mb + u < p.M) {
          const size_t off = (size_t)(mb + u) * p.lda + k;
          xv[u] = p.x[off];
          for (int s = 1; s < p.x_parts; ++s) xv[u] += p.x[off + s * p.x_part_stride];
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (mb + u < p.M) {
          const float x1 = xv[u] * p.x_scale;
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] += dz[mb + u][i] * x1;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (n0 + i < p.N) p.dw[(size_t)(n0 + i) * p.K + k] = acc[i];
  }
  if (p.db != nullptr && tid < 8 && n0 + tid < p.N) {
    float s = 0.f;
    for (int m = 0; m < p.M; ++m) s += dz[m][tid];
    p.db[n0 + tid] = s;
  }
}

__global__ __launch_bounds__(256) void fc_wgrad_kernel(FcWgP p) { fc_wgrad_block(p, blockIdx.x); }

extern "C" int vmtl_fc_wgrad(const float* x, int x_parts, long long x_part_stride, float x_scale, const float* dyo,
                             int dy_parts, long long dy_part_stride, const float* zo, float* dw, float* db, int M,
                             int K, int N, int lda, int ldn, int act, void* stream) {
  VMTL_ENTER();
  if (!x || !dyo || !dw || M <= 0 || M > 64 || K <= 0 || N <= 0 || lda < K || ldn < N || x_parts < 1 || dy_parts < 1)
    return VMTL_ERR_ARG;
  FcWgP p{x, dyo, zo, dw, db, x_part_stride, dy_part_stride, x_scale, x_parts, dy_parts, M, K, N, lda, ldn, act};
  hipLaunchKernelGGL(fc_wgrad_kernel, dim3(cdiv(N, 8)), dim3(256), 0, (hipStream_t)stream, p);
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ per-image spatial reductions
// part[s][b][c] = sum over the s-th slice of HW of x[b][hw][c] (* y[b][hw][c] when y is given).
// Threads keep a fixed float4 channel group; 256 / CQ row lanes walk the slice in parallel.
__global__ __launch_bounds__(256) void hw_reduce_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        float* __restrict__ part, int B, int HW, int Cs, int rows_per) {
  __shared__ f32x4 red[256];
  const int CQ = Cs >> 2;
  const int cq = min(CQ, 256);         // channel groups handled by this workgroup column
  const int RP = 256 / cq;             // row lanes
  const int tid = threadIdx.x;
  const int ql = tid % cq, rg = tid / cq;
  const int q = blockIdx.x * 256 + ql;
  const int b = blockIdx.y, s = blockIdx.z;
  const int r_begin = s * rows_per, r_end = min(HW, r_begin + rows_per);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (rg < RP && q < CQ) {
    const float* xb = x + (size_t)b * HW * Cs + (size_t)q * 4;
    const float* yb = y != nullptr ? y + (size_t)b * HW * Cs + (size_t)q * 4 : nullptr;
    // 4 rows per trip: the loads are independent, the chain of adds is what serialises a plain loop
    f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1, a3 = a1;
    int r = r_begin + rg;
    for (; r + 3 * RP < r_end; r += 4 * RP) {
      f32x4 v0 = *reinterpret_cast<const f32x4*>(xb + (size_t)r * Cs);
      f32x4 v1 = *reinterpret_cast<const f32x4*>(xb + (size_t)(r + RP) * Cs);
      f32x4 v2 = *reinterpret_cast<const f32x4*>(xb + (size_t)(r + 2 * RP) * Cs);
      f32x4 v3 = *reinterpret_cast<const f32x4*>(xb + (size_t)(r + 3 * RP) * Cs);
      if (yb != nullptr) {
        v0 *= *reinterpret_cast<const f32x4*>(yb + (size_t)r * Cs);
        v1 *= *reinterpret_cast<const f32x4*>(yb + (size_t)(r + RP) * Cs);
        v2 *= *reinterpret_cast<const f32x4*>(yb + (size_t)(r + 2 * RP) * Cs);
        v3 *= *reinterpret_cast<const f32x4*>(yb + (size_t)(r + 3 * RP) * Cs);
      }
      acc += v0;
      a1 += v1;
      a2 += v2;
      a3 += v3;
    }
    for (; r < r_end; r += RP) {
      f32x4 v = *reinterpret_cast<const f32x4*>(xb + (size_t)r * Cs);
      if (yb != nullptr) v *= *reinterpret_cast<const f32x4*>(yb + (size_t)r * Cs);
      acc += v;
    }
    acc += a1 + (a2 + a3);
  }
  red[tid] = acc;
  __syncthreads();
  if (rg == 0 && q < CQ) {
    f32x4 t = red[ql];
    for (int g = 1; g < RP; ++g) t += red[g * cq + ql];  // fixed order: deterministic
    *reinterpret_cast<f32x4*>(part + ((size_t)s * B + b) * Cs + (size_t)q * 4) = t;
  }
}

// number of HW slices (= leading dimension of the partial buffer)
extern "C" int vmtl_hw_reduce_parts(int B, int HW, int Cs) {
  if (B <= 0 || HW <= 0 || Cs <= 0) return 0;
  const int cols = cdiv(Cs >> 2, 256);
  // ~128 workgroups; every extra slice is an extra operand read in the GEMMs that consume the partials
  int want = cdiv(128, B * cols);
  int cap = cdiv(HW, 32);                 // at least 32 rows per slice
  int S = want < cap ? want : cap;
  if (S < 1) S = 1;
  if (S > 32) S = 32;
  return cdiv(HW, cdiv(HW, S));           // drop empty slices
}

extern "C" int vmtl_hw_reduce(const float* x, const float* y, float* part, int B, int HW, int Cs, void* stream) {
  VMTL_ENTER();
  if (!x || !part || (Cs & 3) || B <= 0 || HW <= 0) return VMTL_ERR_ARG;
  const int S = vmtl_hw_reduce_parts(B, HW, Cs);
  const int rows_per = cdiv(HW, S);
  hipLaunchKernelGGL(hw_reduce_kernel, dim3(cdiv(Cs >> 2, 256), B, S), dim3(256), 0, (hipStream_t)stream, x, y, part, B,
                     HW, Cs, rows_per);
  return vmtl_check_launch();
}

// y[b][hw][c] = x[b][hw][c] * s[b][c] + t[b][c] * t_scale     (t nullable)
__global__ __launch_bounds__(256) void channel_scale_add_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                                const float* __restrict__ t, float t_scale,
                                                                float* __restrict__ y, int HW, int Cs, long long total4) {
  const int CQ = Cs >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
    const int q = (int)(i % CQ);
    const int b = (int)(i / ((long long)CQ * HW));
    f32x4 v = reinterpret_cast<const f32x4*>(x)[i] * *reinterpret_cast<const f32x4*>(s + (size_t)b * Cs + (size_t)q * 4);
    if (t != nullptr) v += *reinterpret_cast<const f32x4*>(t + (size_t)b * Cs + (size_t)q * 4) * t_scale;
    reinterpret_cast<f32x4*>(y)[i] = v;
  }
}

extern "C" int vmtl_channel_scale_add(const float* x, const float* s, const float* t, float t_scale, float* y, int B,
                                      int HW, int Cs, void* stream) {
  VMTL_ENTER();
  if (!x || !s || !y || (Cs & 3) || B <= 0 || HW <= 0) return VMTL_ERR_ARG;
  const long long total4 = (long long)B * HW * (Cs >> 2);
  hipLaunchKernelGGL(channel_scale_add_kernel, dim3(grid_1d(total4, 256, 4096)), dim3(256), 0, (hipStream_t)stream, x, s,
                     t, t_scale, y, HW, Cs, total4);
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ squeeze-excite gate: one launch per direction
// The gate of one image is two GEMVs behind a spatial reduction - a dependent chain that three launches (hw_reduce,
// fc, fc) spent mostly on launch latency and cold first loads.  Here ONE workgroup owns an image: it reduces the map,
// keeps the [C] / [R] vectors in LDS and walks both weight matrices in the torch layout, forward as row dot products
// (K contiguous), backward as weighted column sums (the other index order of the same matrices: no packed transposes).
// Every sum has a fixed order: no atomics, bit-identical from run to run.
#define SE_THREADS 1024
#define SE_MAX_VEC 8192  // floats of LDS for the [Cs] + [Rs] vectors

template <int V>
__device__ __forceinline__ void se_ld(const float* p, float* o) {
  if constexpr (V == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3];
  } else {
    o[0] = p[0];
  }
}
template <int V>
__device__ __forceinline__ void se_st(float* p, const float* o) {
  if constexpr (V == 4) {
    *reinterpret_cast<f32x4*>(p) = (f32x4){o[0], o[1], o[2], o[3]};
  } else {
    p[0] = o[0];
  }
}

// out[c] = sum_{r < rows} a[r][c] * f,  c < cols, a row-major with leading dimension ld (a multiple of V, like cols);
// MODE 0: f = 1, MODE 1: f = b[r][c], MODE 2: f = wv[r] (an LDS vector).  Threads keep a fixed group of V columns; the
// SE_THREADS / groups row lanes walk the rows in parallel and are summed through LDS in two fixed-order stages.
// Ends with a barrier: `out` (LDS) is visible to the whole workgroup on return.
template <int V, int MODE>
__device__ __forceinline__ void se_colsum(const float* __restrict__ a, const float* __restrict__ b, const float* wv, int rows,
                                          int cols, int ld, float* red, float* red2, float* out) {
  const int tid = threadIdx.x;
  const int ncg = cols / V;
  for (int q0 = 0; q0 < ncg; q0 += SE_THREADS) {
    const int cg = min(ncg - q0, SE_THREADS);
    const int RP = SE_THREADS / cg;
    const int ql = tid % cg, rg = tid / cg;
    float acc[4][V];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < V; ++e) acc[u][e] = 0.f;
    if (rg < RP) {
      const size_t col = (size_t)(q0 + ql) * V;
      int r = rg;
      for (; r + 3 * RP < rows; r += 4 * RP) {  // 4 independent rows in flight
        float v[4][V];
#pragma unroll
        for (int u = 0; u < 4; ++u) se_ld<V>(a + (size_t)(r + u * RP) * ld + col, v[u]);
        if constexpr (MODE == 1) {
          float w[4][V];
#pragma unroll
          for (int u = 0; u < 4; ++u) se_ld<V>(b + (size_t)(r + u * RP) * ld + col, w[u]);
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < V; ++e) v[u][e] *= w[u][e];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float f = MODE == 2 ? wv[r + u * RP] : 1.f;
#pragma unroll
          for (int e = 0; e < V; ++e) acc[u][e] += MODE == 2 ? v[u][e] * f : v[u][e];
        }
      }
      for (; r < rows; r += RP) {
        float v[V];
        se_ld<V>(a + (size_t)r * ld + col, v);
        if constexpr (MODE == 1) {
          float w[V];
          se_ld<V>(b + (size_t)r * ld + col, w);
#pragma unroll
          for (int e = 0; e < V; ++e) v[e] *= w[e];
        }
        const float f = MODE == 2 ? wv[r] : 1.f;
#pragma unroll
        for (int e = 0; e < V; ++e) acc[0][e] += MODE == 2 ? v[e] * f : v[e];
      }
#pragma unroll
      for (int e = 0; e < V; ++e) acc[0][e] += acc[1][e] + (acc[2][e] + acc[3][e]);
    }
    se_st<V>(red + (size_t)tid * V, acc[0]);
    __syncthreads();
    const int G = min(RP, 8);
    if (rg < G) {  // stage 1: G lanes per column group, each over every G-th row lane
      float t[V];
      se_ld<V>(red + (size_t)(rg * cg + ql) * V, t);
      for (int g = rg + G; g < RP; g += G) {
        float v[V];
        se_ld<V>(red + (size_t)(g * cg + ql) * V, v);
#pragma unroll
        for (int e = 0; e < V; ++e) t[e] += v[e];
      }
      se_st<V>(red2 + (size_t)(rg * cg + ql) * V, t);
    }
    __syncthreads();
    if (rg == 0) {
      float t[V];
      se_ld<V>(red2 + (size_t)ql * V, t);
      for (int g = 1; g < G; ++g) {
        float v[V];
        se_ld<V>(red2 + (size_t)(g * cg + ql) * V, v);
#pragma unroll
        for (int e = 0; e < V; ++e) t[e] += v[e];
      }
      se_st<V>(out + (size_t)(q0 + ql) * V, t);
    }
    __syncthreads();
  }
}

// fin(n, sum_k w[n][k] * v[k]) for n < rows; w is [rows][K] with K contiguous (a multiple of V), v an LDS vector.
// 1 .. 16 lanes share a row (four loads in flight each) and are summed by a fixed butterfly.
template <int V, class F>
__device__ __forceinline__ void se_rowdot(const float* __restrict__ w, int rows, int K, const float* v, F fin) {
  const int tid = threadIdx.x;
  const int KG = K / V;
  int LPR = 1;
  while (LPR < KG && LPR < 16) LPR <<= 1;
  const int l = tid & (LPR - 1), rl = tid / LPR, RIF = SE_THREADS / LPR;
  for (int n0 = 0; n0 < rows; n0 += RIF) {
    const int n = n0 + rl;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < rows) {
      const float* wp = w + (size_t)n * K;
      for (int k = l; k < KG; k += 4 * LPR) {
        float wv[4][V];
#pragma unroll
        for (int u = 0; u < 4; ++u) se_ld<V>(wp + (size_t)min(k + u * LPR, KG - 1) * V, wv[u]);  // clamped: in bounds
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int kk = k + u * LPR;
          if (kk < KG) {
#pragma unroll
            for (int e = 0; e < V; ++e) acc[u] += wv[u][e] * v[kk * V + e];
          }
        }
      }
    }
    float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    for (int o = LPR >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (l == 0 && n < rows) fin(n, s);
  }
}

struct SeFwdP {
  const float *x, *wr, *br, *we, *be;
  float *pooled, *z1, *h, *z2, *g;
  int HW, C, R, Cs, Rs, act1, act2, vec_r, vec_e;  // vec_*: 16-byte loads along that weight's rows are legal
};

__global__ __launch_bounds__(SE_THREADS) void se_gate_fwd_kernel(SeFwdP p) {
  extern __shared__ float se_vec[];  // [Cs] + [Rs]
  __shared__ f32x4 red4[SE_THREADS], red24[SE_THREADS];
  float* red = reinterpret_cast<float*>(red4);
  float* red2 = reinterpret_cast<float*>(red24);
  float* vc = se_vec;
  float* vr = se_vec + p.Cs;
  const int tid = threadIdx.x, b = blockIdx.x;
  se_colsum<4, 0>(p.x + (size_t)b * p.HW * p.Cs, nullptr, nullptr, p.HW, p.Cs, p.Cs, red, red2, vc);
  const float inv = 1.f / (float)p.HW;
  for (int c = tid; c < p.Cs; c += SE_THREADS) {  // pad channels of x are zero: so is their mean
    const float m = vc[c] * inv;
    vc[c] = m;
    p.pooled[(size_t)b * p.Cs + c] = m;
  }
  for (int r = p.R + tid; r < p.Rs; r += SE_THREADS) {
    vr[r] = 0.f;
    p.z1[(size_t)b * p.Rs + r] = 0.f;
    p.h[(size_t)b * p.Rs + r] = 0.f;
  }
  for (int c = p.C + tid; c < p.Cs; c += SE_THREADS) {
    p.z2[(size_t)b * p.Cs + c] = 0.f;
    p.g[(size_t)b * p.Cs + c] = 0.f;
  }
  __syncthreads();
  auto fin1 = [&](int n, float s) {
    const float z = s + p.br[n];
    const float hv = act_fwd(z, p.act1);
    p.z1[(size_t)b * p.Rs + n] = z;
    p.h[(size_t)b * p.Rs + n] = hv;
    vr[n] = hv;
  };
  if (p.vec_r) se_rowdot<4>(p.wr, p.R, p.C, vc, fin1);
  else se_rowdot<1>(p.wr, p.R, p.C, vc, fin1);
  __syncthreads();
  auto fin2 = [&](int n, float s) {
    const float z = s + p.be[n];
    p.z2[(size_t)b * p.Cs + n] = z;
    p.g[(size_t)b * p.Cs + n] = act_fwd(z, p.act2);
  };
  if (p.vec_e) se_rowdot<4>(p.we, p.C, p.R, vr, fin2);
  else se_rowdot<1>(p.we, p.C, p.R, vr, fin2);
}

struct SeBwdP {
  const float *dy, *x, *z1, *z2, *wr, *we;
  float *dg, *dh, *dmean;  // dmean nullable: the input needs no gradient
  int HW, C, R, Cs, Rs, act1, act2, vec_r, vec_e;
};

__global__ __launch_bounds__(SE_THREADS) void se_gate_bwd_kernel(SeBwdP p) {
  extern __shared__ float se_vec[];
  __shared__ f32x4 red4[SE_THREADS], red24[SE_THREADS];
  float* red = reinterpret_cast<float*>(red4);
  float* red2 = reinterpret_cast<float*>(red24);
  float* vc = se_vec;
  float* vr = se_vec + p.Cs;
  const int tid = threadIdx.x, b = blockIdx.x;
  const size_t img = (size_t)b * p.HW * p.Cs;
  se_colsum<4, 1>(p.dy + img, p.x + img, nullptr, p.HW, p.Cs, p.Cs, red, red2, vc);  // dg = sum_hw dy * x
  for (int c = tid; c < p.Cs; c += SE_THREADS) {
    const float d = vc[c];
    p.dg[(size_t)b * p.Cs + c] = d;
    vc[c] = c < p.C ? d * act_grad(p.z2[(size_t)b * p.Cs + c], p.act2) : 0.f;
  }
  __syncthreads();
  // dh[r] = sum_c dz2[c] * W_e[c][r]
  if (p.vec_e) se_colsum<4, 2>(p.we, nullptr, vc, p.C, p.R, p.R, red, red2, vr);
  else se_colsum<1, 2>(p.we, nullptr, vc, p.C, p.R, p.R, red, red2, vr);
  for (int r = tid; r < p.Rs; r += SE_THREADS) {
    const float d = r < p.R ? vr[r] : 0.f;
    p.dh[(size_t)b * p.Rs + r] = d;
    vr[r] = r < p.R ? d * act_grad(p.z1[(size_t)b * p.Rs + r], p.act1) : 0.f;
  }
  if (p.dmean == nullptr) return;
  __syncthreads();
  // dmean[c] = sum_r dz1[r] * W_r[r][c]
  if (p.vec_r) se_colsum<4, 2>(p.wr, nullptr, vr, p.R, p.C, p.C, red, red2, vc);
  else se_colsum<1, 2>(p.wr, nullptr, vr, p.R, p.C, p.C, red, red2, vc);
  for (int c = tid; c < p.Cs; c += SE_THREADS) p.dmean[(size_t)b * p.Cs + c] = c < p.C ? vc[c] : 0.f;
}

// both weight gradients of one gate: workgroups [0, nbe) take 8 rows of dW_e each, the rest 8 rows of dW_r
__global__ __launch_bounds__(256) void se_wgrad_kernel(FcWgP pe, FcWgP pr, int nbe) {
  if ((int)blockIdx.x < nbe) fc_wgrad_block(pe, blockIdx.x);
  else fc_wgrad_block(pr, blockIdx.x - nbe);
}

static inline int ceil4i(int c) { return (c + 3) & ~3; }
static inline bool se_vec_ok(const float* w, int ld) { return (ld & 3) == 0 && ((uintptr_t)w & 15) == 0; }
static inline bool se_shape_ok(int B, int HW, int C, int R) {
  return B > 0 && B <= 64 && HW > 0 && C > 0 && R > 0 && ceil4i(C) + ceil4i(R) <= SE_MAX_VEC;
}

// Which launches ops.squeeze_excite takes for a shape: bit 0 - vmtl_se_gate_bwd + vmtl_se_wgrad, bit 1 - vmtl_se_gate_fwd.
// One workgroup per image reads both weight matrices itself (B reads of each in all, ~16 dependent rounds of loads
// per 240 KB on one CU), where the batch-sized GEMM reads them once over N / 16 workgroups.  Measured in the step at
// bs 32 (profiles/r06_se_gate): the backward launch wins on every production shape (its reduction reads two maps and
// the GEMM it replaces sums up to 32 partial slices per workgroup), the forward launch wins at C x R = 72 x 24 and
// 120 x 32 (8-9 us against 17-19) and loses from 480 x 120 up (28 against 26 us, 58 against 26 at 960 x 240).  Its
// time grows with C x R, the sequence's hardly: the interpolated break-even is near 5e4 weights, the limit sits a
// factor of three below it.  VMTL_SE_FUSED: 0 - the four-launch sequence, 2 - both fused launches wherever supported.
#define SE_FWD_MAX_WEIGHTS 16384
extern "C" int vmtl_se_gate_supported(int B, int C, int R) {
  static EnvInt e{"VMTL_SE_FUSED", 1};
  const int mode = env_int(e);
  if (mode == 0 || !se_shape_ok(B, 1, C, R)) return 0;
  return 1 | ((mode >= 2 || (long long)C * R <= SE_FWD_MAX_WEIGHTS) ? 2 : 0);
}

extern "C" int vmtl_se_gate_fwd(const float* x, const float* wr, const float* br, const float* we, const float* be,
                                float* pooled, float* z1, float* h, float* z2, float* g, int B, int HW, int C, int R,
                                int act1, int act2, void* stream) {
  VMTL_ENTER();
  if (!x || !wr || !br || !we || !be || !pooled || !z1 || !h || !z2 || !g || !se_shape_ok(B, HW, C, R)) return VMTL_ERR_ARG;
  const int Cs = ceil4i(C), Rs = ceil4i(R);
  SeFwdP p{x, wr, br, we, be, pooled, z1, h, z2, g, HW, C, R, Cs, Rs, act1, act2, se_vec_ok(wr, C), se_vec_ok(we, R)};
  hipLaunchKernelGGL(se_gate_fwd_kernel, dim3(B), dim3(SE_THREADS), (Cs + Rs) * sizeof(float), (hipStream_t)stream, p);
  return vmtl_check_launch();
}

extern "C" int vmtl_se_gate_bwd(const float* dy, const float* x, const float* z1, const float* z2, const float* wr,
                                const float* we, float* dg, float* dh, float* dmean, int B, int HW, int C, int R, int act1,
                                int act2, void* stream) {
  VMTL_ENTER();
  if (!dy || !x || !z1 || !z2 || !wr || !we || !dg || !dh || !se_shape_ok(B, HW, C, R)) return VMTL_ERR_ARG;
  const int Cs = ceil4i(C), Rs = ceil4i(R);
  SeBwdP p{dy, x, z1, z2, wr, we, dg, dh, dmean, HW, C, R, Cs, Rs, act1, act2, se_vec_ok(wr, C), se_vec_ok(we, R)};
  hipLaunchKernelGGL(se_gate_bwd_kernel, dim3(B), dim3(SE_THREADS), (Cs + Rs) * sizeof(float), (hipStream_t)stream, p);
  return vmtl_check_launch();
}

extern "C" int vmtl_se_wgrad(const float* pooled, const float* h, const float* dg, const float* dh, const float* z1,
                             const float* z2, float* dwr, float* dbr, float* dwe, float* dbe, int B, int C, int R,
                             int act1, int act2, void* stream) {
  VMTL_ENTER();
  if (!pooled || !h || !dg || !dh || !z1 || !z2 || !dwr || !dwe || B <= 0 || B > 64 || C <= 0 || R <= 0)
    return VMTL_ERR_ARG;
  const int Cs = ceil4i(C), Rs = ceil4i(R);
  FcWgP pe{h, dg, z2, dwe, dbe, 0, 0, 1.f, 1, 1, B, R, C, Rs, Cs, act2};
  FcWgP pr{pooled, dh, z1, dwr, dbr, 0, 0, 1.f, 1, 1, B, C, R, Cs, Rs, act1};
  const int nbe = cdiv(C, 8);
  hipLaunchKernelGGL(se_wgrad_kernel, dim3(nbe + cdiv(R, 8)), dim3(256), 0, (hipStream_t)stream, pe, pr, nbe);
  return vmtl_check_launch();
}
