// Dataset-level evaluation metrics accumulated on the device.
//
// The per-step metrics of metrics.hip are computed per batch and averaged by the host; the numbers a Cityscapes / NYUv2
// table reports are functions of the WHOLE evaluation set.  Here the caller owns two small state arrays that every
// (captured) evaluation step adds its batch to without a host sync, and that are read once per epoch:
//   cm   int64   [C][C]  confusion matrix (target row, prediction column)
//   acc  float64 [16]    depth sums and counts, layout in vmtl.h
//
// Reproducibility: cm and the four counts are integers (LDS / global integer atomics in the pixel pass, integer sums in
// the fold: exact and order independent; a count enters acc as ONE exact fp64 addition of an integer).  The seven
// floating sums are fp64 per-thread sums, reduced per workgroup by a fixed shuffle tree into the workspace, and folded
// into acc by a single workgroup in a fixed order: no floating-point atomics anywhere, so the state after a given
// sequence of batches is bit-identical from run to run.
#include "common.h"

#define EA_MAX_C 64
#define EA_BLOCKS_MAX 1024  // the grid cap of confusion_kernel and the SILog pass
#define EA_WS 12            // 8-byte words per workgroup in the workspace: 7 fp64 sums, 4 uint64 counts, 1 pad;
                            // word k of workgroup b is at [k * nblk + b], so the fold's loads are coalesced
#define EA_NSUM 7

struct EaTerms {
  double s[EA_NSUM];
  unsigned n, d1, d2, d3;
};

// one valid pixel; every term in fp64 from the fp32 inputs, the prediction clamped below at min_depth first.
// g = ln p - ln t is taken as ln(p / t): the quotient is correctly rounded and the delta ratios need it anyway, so g
// costs ONE fp64 log and keeps its relative accuracy when p is close to t (the difference of two logs cancels there);
// |log10 p - log10 t| = |g| / ln 10.  The pass is bound by this arithmetic, not by its 8 bytes per pixel.
__device__ __forceinline__ void ea_pixel(float pf, float tf, float min_depth, EaTerms& a) {
  const double p = (double)fmaxf(pf, min_depth), t = (double)tf;
  const double d = p - t, ad = fabs(d);
  const double q = p / t;
  const double g = log(q);
  a.s[0] += ad;
  a.s[1] += ad / t;
  a.s[2] += d * d / t;
  a.s[3] += d * d;
  a.s[4] += g * g;
  a.s[5] += g;
  a.s[6] += fabs(g) * 0.43429448190325182765;  // 1 / ln 10
  const double r = fmax(q, t / p);
  a.n += 1u;
  a.d1 += r < 1.25 ? 1u : 0u;
  a.d2 += r < 1.5625 ? 1u : 0u;
  a.d3 += r < 1.953125 ? 1u : 0u;
}

// Segmentation part (P > 0): the LDS histogram of metrics.hip's confusion_kernel<true>, flushed into the int64 matrix.
// Depth part (Pd > 0): the first nblk_d workgroups sweep the pixels and leave one row of partials each.
// VEC: dpred / dtgt are 16-byte aligned (valid 4-byte aligned): float4 loads over Pd / 4 quads, scalar tail.
template <bool VEC, bool MASK>
__global__ __launch_bounds__(256) void ea_accum_kernel(const long long* __restrict__ pred,
                                                       const long long* __restrict__ tgt,
                                                       unsigned long long* __restrict__ cm, long long P, int C,
                                                       long long ignore, const float* __restrict__ dpred,
                                                       const float* __restrict__ dtgt,
                                                       const unsigned char* __restrict__ valid, float min_depth,
                                                       long long Pd, int nblk_d, double* __restrict__ partial) {
  extern __shared__ unsigned hist[];
  __shared__ double red[4][EA_NSUM];
  __shared__ unsigned long long cnt[4];
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0ull;  // ordered before the adds below by barrier A
  if (P > 0) {
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) hist[i] = 0u;
    __syncthreads();
    VMTL_GRID_STRIDE(i, P) {
      const long long t = tgt[i], p = pred[i];
      if (t != ignore && t >= 0 && t < C && p >= 0 && p < C) atomicAdd(&hist[(int)t * C + (int)p], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += blockDim.x)
      if (hist[i]) atomicAdd(&cm[i], (unsigned long long)hist[i]);  // integer atomics: exact and order independent
  }
  if (Pd <= 0 || (int)blockIdx.x >= nblk_d) return;  // uniform per workgroup
  EaTerms a;
#pragma unroll
  for (int k = 0; k < EA_NSUM; ++k) a.s[k] = 0.0;
  a.n = a.d1 = a.d2 = a.d3 = 0u;
  const long long stride = (long long)nblk_d * blockDim.x;
  if (VEC) {
    const long long nq = Pd >> 2;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += stride) {
      const f32x4 p = reinterpret_cast<const f32x4*>(dpred)[q];
      const f32x4 t = reinterpret_cast<const f32x4*>(dtgt)[q];
      uchar4 m = make_uchar4(0, 0, 0, 0);
      if (MASK) m = reinterpret_cast<const uchar4*>(valid)[q];
      if (MASK ? m.x != 0 : t.x > min_depth) ea_pixel(p.x, t.x, min_depth, a);
      if (MASK ? m.y != 0 : t.y > min_depth) ea_pixel(p.y, t.y, min_depth, a);
      if (MASK ? m.z != 0 : t.z > min_depth) ea_pixel(p.z, t.z, min_depth, a);
      if (MASK ? m.w != 0 : t.w > min_depth) ea_pixel(p.w, t.w, min_depth, a);
    }
    const long long i = (nq << 2) + threadIdx.x;  // the Pd % 4 pixels after the last quad
    if (blockIdx.x == 0 && threadIdx.x < 3 && i < Pd) {
      const float t = dtgt[i];
      if (MASK ? valid[i] != 0 : t > min_depth) ea_pixel(dpred[i], t, min_depth, a);
    }
  } else {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < Pd; i += stride) {
      const float t = dtgt[i];
      if (MASK ? valid[i] != 0 : t > min_depth) ea_pixel(dpred[i], t, min_depth, a);
    }
  }
  // wavefront sums by a fixed shuffle tree, then the four wavefronts in order: one row of partials per workgroup
#pragma unroll
  for (int k = 0; k < EA_NSUM; ++k) a.s[k] = wave_sum(a.s[k]);
  const unsigned c0 = wave_sum(a.n), c1 = wave_sum(a.d1), c2 = wave_sum(a.d2), c3 = wave_sum(a.d3);
  __syncthreads();  // A
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < EA_NSUM; ++k) red[threadIdx.x >> 6][k] = a.s[k];
    atomicAdd(&cnt[0], (unsigned long long)c0);
    atomicAdd(&cnt[1], (unsigned long long)c1);
    atomicAdd(&cnt[2], (unsigned long long)c2);
    atomicAdd(&cnt[3], (unsigned long long)c3);
  }
  __syncthreads();
  const int k = threadIdx.x;
  double* slot = partial + (size_t)k * nblk_d + blockIdx.x;  // k < EA_WS below
  if (k < EA_NSUM) *slot = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  else if (k < EA_NSUM + 4) *reinterpret_cast<unsigned long long*>(slot) = cnt[k - EA_NSUM];
}

// One workgroup: the workspace rows into acc in a fixed order, and / or a ready int32 step matrix into cm.
// Thread t takes rows t, t + 256, t + 512, t + 768 (nblk <= EA_BLOCKS_MAX = 4 * 256) with every load issued before the
// first addition: a loop over the rows pays the memory latency once per trip, and this launch is nothing but latency.
#define EA_FOLD_ROWS (EA_BLOCKS_MAX / 256)
__global__ __launch_bounds__(256) void ea_fold_kernel(const double* __restrict__ partial, int nblk,
                                                      double* __restrict__ acc, const int* __restrict__ step_cm,
                                                      long long* __restrict__ cm, int CC) {
  __shared__ double red[4][EA_NSUM];
  __shared__ unsigned long long cred[4][4];
  if (step_cm)
    for (int i = threadIdx.x; i < CC; i += blockDim.x) cm[i] += (long long)step_cm[i];
  if (nblk <= 0) return;
  const unsigned long long* ip = reinterpret_cast<const unsigned long long*>(partial);
  double v[EA_FOLD_ROWS][EA_NSUM];
  unsigned long long u[EA_FOLD_ROWS][4];
#pragma unroll
  for (int r = 0; r < EA_FOLD_ROWS; ++r) {
    const int b = threadIdx.x + r * 256;
    const bool in = b < nblk;
#pragma unroll
    for (int k = 0; k < EA_NSUM; ++k) v[r][k] = in ? partial[(size_t)k * nblk + b] : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) u[r][k] = in ? ip[(size_t)(EA_NSUM + k) * nblk + b] : 0ull;
  }
  double s[EA_NSUM];
  unsigned long long c[4];
#pragma unroll
  for (int k = 0; k < EA_NSUM; ++k) {
    s[k] = v[0][k];
#pragma unroll
    for (int r = 1; r < EA_FOLD_ROWS; ++r) s[k] += v[r][k];
    s[k] = wave_sum(s[k]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c[k] = u[0][k];
#pragma unroll
    for (int r = 1; r < EA_FOLD_ROWS; ++r) c[k] += u[r][k];
    c[k] = wave_sum(c[k]);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < EA_NSUM; ++k) red[threadIdx.x >> 6][k] = s[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) cred[threadIdx.x >> 6][k] = c[k];
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < EA_NSUM) {
    acc[1 + k] += ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];  // the wavefronts in order
  } else if (k < EA_NSUM + 4) {
    const int j = k - EA_NSUM;  // integer sums below 2^53: the fp64 addition is exact
    acc[j == 0 ? 0 : k] += (double)(cred[0][j] + cred[1][j] + cred[2][j] + cred[3][j]);  // acc[0], acc[8..10]
  }
}

// out[16] (layout in vmtl.h) and iou[C] from the state; one workgroup of 64 threads, thread c sums class c's
// row and column in int64, thread 0 folds the classes in order.
__global__ __launch_bounds__(64) void ea_finalize_kernel(const long long* __restrict__ cm,
                                                         const double* __restrict__ acc, int C, double beta, int ign,
                                                         double* __restrict__ out, double* __restrict__ iou) {
  __shared__ double tp_s[EA_MAX_C], row_s[EA_MAX_C], col_s[EA_MAX_C];
  const int c = threadIdx.x;
  if (c < C) {
    long long row = 0, col = 0;
    for (int k = 0; k < C; ++k) {
      row += cm[c * C + k];  // targets of class c
      col += cm[k * C + c];  // predictions of class c
    }
    tp_s[c] = (double)cm[c * C + c];
    row_s[c] = (double)row;
    col_s[c] = (double)col;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double nan = __builtin_nan("");
  const double b2 = beta * beta;
  double total = 0.0, correct = 0.0, fb = 0.0, acc_sum = 0.0, iou_sum = 0.0;
  int n_acc = 0, n_iou = 0;
  for (int k = 0; k < C; ++k) {
    const double tp = tp_s[k], row = row_s[k], fn = row - tp, fp = col_s[k] - tp;
    total += row;
    correct += tp;
    const double den = (1.0 + b2) * tp + b2 * fn + fp;
    fb += row * (den > 0.0 ? (1.0 + b2) * tp / den : 0.0);
    const double uni = tp + fp + fn;
    double v = nan;
    if (k != ign) {
      if (row > 0.0) {
        acc_sum += tp / row;
        ++n_acc;
      }
      if (uni > 0.0) {
        v = tp / uni;
        iou_sum += v;
        ++n_iou;
      }
    }
    iou[k] = v;
  }
  out[0] = total > 0.0 ? correct / total : nan;
  out[1] = total > 0.0 && n_acc > 0 ? acc_sum / n_acc : nan;
  out[2] = total > 0.0 && n_iou > 0 ? iou_sum / n_iou : nan;
  out[3] = total > 0.0 ? fb / total : nan;
  const double n = acc[0];
  if (n > 0.0) {
    const double eg2 = acc[5] / n, eg = acc[6] / n;
    out[4] = acc[1] / n;
    out[5] = acc[2] / n;
    out[6] = acc[3] / n;
    out[7] = sqrt(acc[4] / n);
    out[8] = sqrt(eg2);
    out[9] = acc[7] / n;
    out[10] = sqrt(fmax(eg2 - eg * eg, 0.0));
    out[11] = acc[8] / n;
    out[12] = acc[9] / n;
    out[13] = acc[10] / n;
  } else {
    for (int k = 4; k <= 13; ++k) out[k] = nan;
  }
  out[14] = n;
  out[15] = total;
}

static inline int ea_depth_blocks(long long Pd) {
  return grid_1d(Pd, 1024, EA_BLOCKS_MAX);
}

extern "C" long long vmtl_eval_accum_workspace_bytes(long long P) {
  return (long long)ea_depth_blocks(P) * EA_WS * sizeof(double);
}

extern "C" int vmtl_eval_accumulate(const long long* pred, const long long* target, const int* step_cm, long long P,
                                    int C, long long ignore_index, const float* dpred, const float* dtarget,
                                    const unsigned char* valid, float min_depth, long long Pd, long long* cm,
                                    double* acc, void* workspace, void* stream) {
  VMTL_ENTER();
  const bool pixels = pred || target;
  const bool depth = dpred || dtarget;
  if (pixels && (!pred || !target || step_cm || P <= 0 || P > (1LL << 40))) return VMTL_ERR_ARG;
  if ((pixels || step_cm) && (!cm || C <= 0 || C > EA_MAX_C)) return VMTL_ERR_ARG;
  if (depth && (!dpred || !dtarget || Pd <= 0 || !acc || !workspace || !(min_depth >= 0.f))) return VMTL_ERR_ARG;
  if (!pixels && !step_cm && !depth) return VMTL_ERR_ARG;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)acc & 7) || ((uintptr_t)cm & 7)) return VMTL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int nblk_d = depth ? ea_depth_blocks(Pd) : 0;
  if (pixels || depth) {
    long long nb = pixels ? cdivll(P, 256 * 8) : 1;
    if (nb > EA_BLOCKS_MAX) nb = EA_BLOCKS_MAX;
    if (nb < nblk_d) nb = nblk_d;
    const size_t lds = pixels ? (size_t)C * C * sizeof(unsigned) : 0;
    const bool vec = depth && (((uintptr_t)dpred | (uintptr_t)dtarget) & 15) == 0 && ((uintptr_t)valid & 3) == 0;
#define EA_LAUNCH(V, M)                                                                                              \
  hipLaunchKernelGGL((ea_accum_kernel<V, M>), dim3((int)nb), dim3(256), lds, st, pixels ? pred : nullptr,            \
                     pixels ? target : nullptr, (unsigned long long*)cm, pixels ? P : 0, C, ignore_index, dpred,     \
                     dtarget, valid, min_depth, depth ? Pd : 0, nblk_d, (double*)workspace)
    if (vec && valid) EA_LAUNCH(true, true);
    else if (vec) EA_LAUNCH(true, false);
    else if (valid) EA_LAUNCH(false, true);
    else EA_LAUNCH(false, false);
#undef EA_LAUNCH
  }
  if (depth || step_cm)
    hipLaunchKernelGGL(ea_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, nblk_d, acc, step_cm, cm,
                       step_cm ? C * C : 0);
  return vmtl_check_launch();
}

extern "C" int vmtl_eval_finalize(const long long* cm, const double* acc, int C, float beta, long long ignore_index,
                                  double* out, double* iou, void* stream) {
  VMTL_ENTER();
  if (!cm || !acc || !out || !iou || C <= 0 || C > EA_MAX_C || !(beta > 0.f)) return VMTL_ERR_ARG;
  const int ign = ignore_index >= 0 && ignore_index < C ? (int)ignore_index : -1;
  hipLaunchKernelGGL(ea_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, cm, acc, C, (double)beta, ign, out,
                     iou);
  return vmtl_check_launch();
}
