// Two-task gradient surgery (PCGrad, MGDA, IMTL-G) on a pair of per-task gradients: ops.dual_head hands it the two
// per-task gradients of the shared decoder map, whatever the caller wants otherwise.
//
//   vmtl_surgery_gram      per-workgroup fp64 partial sums of a*a, a*b, b*b (the 2x2 Gram matrix of the pair)
//   vmtl_surgery_control   partials -> state block: Gram matrix, the coefficients (alpha, beta) of the method, cosine,
//                          exact step / conflict counters (one workgroup)
//   vmtl_surgery_combine   out = alpha * a + beta * b, coefficients read from the state block
//
// Operands are `rows` rows of `width` floats with a leading dimension each, so one pair of kernels serves the
// interleaved [M][2*Cs] map of the step (b = a + Cs, lda = ldb = 2*Cs), two separate maps and two flat buffers.
// Conventions are optim.hip's: 4-byte-aligned pointers, a grid that is a function of rows * width alone, grid-stride
// loops, no atomics, sums in a fixed order (block_sum_n of reduce.h), so the same inputs at the same alignment give the
// same bits.  Dense rows (every leading dimension == width) are walked as ONE row.  The float4 body runs
//   one row:    when all pointers share their offset inside a 16-byte line; head and tail are peeled by workgroup 0
//   many rows:  when all pointers are 16-byte aligned and width and every leading dimension are multiples of 4
// and everything else takes the scalar fall-back on the same grid.
//
// State block: VMTL_SURGERY_STATE_FLOATS 4-byte words, 8-byte aligned, zeroed once by the caller
//   [0] n_a = <a,a>  [1] d = <a,b>  [2] n_b = <b,b>  [3] alpha  [4] beta  [5] cosine  [6..7] unused
//   [8..9] steps seen (one 64-bit integer)  [10..11] steps with d < 0 (one 64-bit integer)
// The coefficients are derived in fp64 from the fp32 Gram values the block holds and rounded once, so whoever reads
// the block can re-derive them from what it reads.
#include "optim.h"
#include "reduce.h"

#define VMTL_SURGERY_STATE_FLOATS 12
#define VMTL_SURGERY_SUM 0
#define VMTL_SURGERY_PCGRAD 1
#define VMTL_SURGERY_MGDA 2
#define VMTL_SURGERY_IMTL_G 3

// one grid for the float4 body and the scalar fall-back: vmtl_surgery_control has to know how many partials
// vmtl_surgery_gram wrote without knowing which of the two ran
static inline int surgery_blocks(long long n) { return opt_blocks(n); }

// How the host resolved (pointers, rows, width, leading dimensions) for the kernels.
struct SurgPlan {
  long long rows, width, lda, ldb, ldo;
  int head;  // floats in front of the first 16-byte boundary; 0 unless rows == 1
  bool vec;
};

static SurgPlan surgery_plan(const void* a, long long lda, const void* b, long long ldb, const void* o, long long ldo,
                             long long rows, long long width) {
  SurgPlan p;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, z = o ? (uintptr_t)o : x;
  if (!o) ldo = lda;
  if (rows > 1 && lda == width && ldb == width && ldo == width) {
    width *= rows;
    rows = 1;
  }
  p.rows = rows;
  p.width = width;
  p.lda = lda;
  p.ldb = ldb;
  p.ldo = ldo;
  if (rows == 1) {
    p.vec = (((x ^ y) | (x ^ z)) & 15) == 0;
    p.head = p.vec ? opt_head(a, width) : 0;
  } else {
    p.vec = ((x | y | z) & 15) == 0 && ((width | lda | ldb | ldo) & 3) == 0;
    p.head = 0;
  }
  return p;
}

static bool surgery_args(const void* a, long long lda, const void* b, long long ldb, long long rows, long long width) {
  if (!a || !b || rows <= 0 || width <= 0 || lda < width || ldb < width) return false;
  if (((uintptr_t)a | (uintptr_t)b) & 3) return false;
  return rows <= (1LL << 62) / width;  // rows * width fits
}

// A thread's walk over `total` items laid out as rows of W items: item i sits at (row i / W, column i % W).  The
// grid-stride step is taken on (row, column) directly: two divisions per thread, none per item.
struct SurgWalk {
  long long i, r, c, S, dr, dc, W;
  __device__ __forceinline__ SurgWalk(long long W_) : W(W_ > 0 ? W_ : 1) {
    i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x;
    S = (long long)gridDim.x * OPT_THREADS;
    r = i / W;
    c = i - r * W;
    dr = S / W;
    dc = S - dr * W;
  }
  __device__ __forceinline__ void step() {
    i += S;
    r += dr;
    c += dc;
    if (c >= W) {
      c -= W;
      ++r;
    }
  }
};

// workgroup 0 peels the floats around the float4 body of a single row: thread t < head takes float t, thread 64 + k
// (k < tail) takes float head + 4 * nvec + k; -1 for every other thread
__device__ __forceinline__ long long surgery_peel(int head, long long nvec, int tail) {
  if (blockIdx.x != 0) return -1;
  const int t = threadIdx.x;
  if (t < head) return t;
  if (t >= 64 && t - 64 < tail) return head + (nvec << 2) + (t - 64);
  return -1;
}

// ------------------------------------------------------------------ Gram matrix
// a product of two fp32 values is exact in fp64; each sum takes one rounding per element
__device__ __forceinline__ void gram_acc(double (&s)[3], float x, float y) {
  const double dx = (double)x, dy = (double)y;
  s[0] = fma(dx, dx, s[0]);
  s[1] = fma(dx, dy, s[1]);
  s[2] = fma(dy, dy, s[2]);
}

__device__ __forceinline__ void gram_acc4(double (&s)[3], const f32x4 x, const f32x4 y) {
  gram_acc(s, x.x, y.x);
  gram_acc(s, x.y, y.y);
  gram_acc(s, x.z, y.z);
  gram_acc(s, x.w, y.w);
}

template <bool VEC>
__global__ __launch_bounds__(OPT_THREADS) void surgery_gram_kernel(const float* __restrict__ a, long long lda,
                                                                   const float* __restrict__ b, long long ldb,
                                                                   long long rows, long long width, int head,
                                                                   double* __restrict__ partial) {
  __shared__ double sh[4][3];
  double s[3] = {0.0, 0.0, 0.0};
  if (VEC) {
    const long long W = (width - head) >> 2;  // float4 per row
    const int tail = (int)(width - head - (W << 2));
    const long long total = rows * W;
    SurgWalk w(W);
    // two float4 pairs per trip: four 16-byte loads in flight per thread before the first fp64 product
    while (w.i + w.S < total) {
      const float* a0 = a + w.r * lda + head + (w.c << 2);
      const float* b0 = b + w.r * ldb + head + (w.c << 2);
      w.step();
      const float* a1 = a + w.r * lda + head + (w.c << 2);
      const float* b1 = b + w.r * ldb + head + (w.c << 2);
      w.step();
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(a0), y0 = *reinterpret_cast<const f32x4*>(b0);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(a1), y1 = *reinterpret_cast<const f32x4*>(b1);
      gram_acc4(s, x0, y0);
      gram_acc4(s, x1, y1);
    }
    if (w.i < total) {
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(a + w.r * lda + head + (w.c << 2));
      const f32x4 y0 = *reinterpret_cast<const f32x4*>(b + w.r * ldb + head + (w.c << 2));
      gram_acc4(s, x0, y0);
    }
    const long long j = surgery_peel(head, W, tail);  // head / tail are 0 unless rows == 1
    if (j >= 0) gram_acc(s, a[j], b[j]);
  } else {
    const long long total = rows * width;
    for (SurgWalk w(width); w.i < total; w.step()) gram_acc(s, a[w.r * lda + w.c], b[w.r * ldb + w.c]);
  }
  block_sum_n<3>(s, sh);
  if (threadIdx.x == 0) {
    partial[(size_t)blockIdx.x * 3 + 0] = s[0];
    partial[(size_t)blockIdx.x * 3 + 1] = s[1];
    partial[(size_t)blockIdx.x * 3 + 2] = s[2];
  }
}

extern "C" long long vmtl_surgery_workspace_bytes(long long rows, long long width) {
  if (rows <= 0 || width <= 0 || rows > (1LL << 62) / width) return 0;
  return (long long)surgery_blocks(rows * width) * 3 * (long long)sizeof(double);
}

extern "C" int vmtl_surgery_gram(const float* a, long long lda, const float* b, long long ldb, long long rows,
                                 long long width, void* workspace, void* stream) {
  VMTL_ENTER();
  if (!surgery_args(a, lda, b, ldb, rows, width) || !workspace || ((uintptr_t)workspace & 7)) return VMTL_ERR_ARG;
  const SurgPlan p = surgery_plan(a, lda, b, ldb, nullptr, 0, rows, width);
  const dim3 grid(surgery_blocks(rows * width));
  if (p.vec)
    hipLaunchKernelGGL(surgery_gram_kernel<true>, grid, dim3(OPT_THREADS), 0, (hipStream_t)stream, a, p.lda, b, p.ldb,
                       p.rows, p.width, p.head, (double*)workspace);
  else
    hipLaunchKernelGGL(surgery_gram_kernel<false>, grid, dim3(OPT_THREADS), 0, (hipStream_t)stream, a, p.lda, b, p.ldb,
                       p.rows, p.width, p.head, (double*)workspace);
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ control step
__device__ __forceinline__ bool surgery_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN

__global__ __launch_bounds__(RED_THREADS) void surgery_control_kernel(const double* __restrict__ partial, int nblk,
                                                                      int method, float* __restrict__ state) {
  __shared__ double sh[4][3];
  double s[3] = {0.0, 0.0, 0.0};
  for (int blk = threadIdx.x; blk < nblk; blk += RED_THREADS) {
    s[0] += partial[(size_t)blk * 3 + 0];
    s[1] += partial[(size_t)blk * 3 + 1];
    s[2] += partial[(size_t)blk * 3 + 2];
  }
  block_sum_n<3>(s, sh);
  if (threadIdx.x != 0) return;
  const float fa = (float)s[0], fd = (float)s[1], fb = (float)s[2];
  const double na = (double)fa, d = (double)fd, nb = (double)fb;  // the values the block holds, see the head of the file
  // a zero norm (fp32 underflow included) or a Gram entry that is not finite: the sum passes through untouched
  const bool ok = surgery_finite(na) && surgery_finite(d) && surgery_finite(nb) && na > 0.0 && nb > 0.0;
  double alpha = 1.0, beta = 1.0, cosine = 0.0;
  if (ok) {
    cosine = d / sqrt(na * nb);
    if (method == VMTL_SURGERY_PCGRAD) {
      if (d < 0.0) {  // each gradient loses its component along the other: (a - d/n_b b) + (b - d/n_a a)
        alpha = 1.0 - d / na;
        beta = 1.0 - d / nb;
      }
    } else if (method == VMTL_SURGERY_MGDA) {  // min over gamma in [0, 1] of |gamma a + (1 - gamma) b|^2
      const double den = na - 2.0 * d + nb;    // |a - b|^2; rounding of the Gram values can leave it at or below 0
      const double gamma = den > 0.0 ? fmin(fmax((nb - d) / den, 0.0), 1.0) : 0.5;
      alpha = gamma;
      beta = 1.0 - gamma;
    } else if (method == VMTL_SURGERY_IMTL_G) {  // equal projections onto a / |a| and b / |b|, alpha + beta = 1
      const double ra = sqrt(na), rb = sqrt(nb);
      alpha = rb / (ra + rb);
      beta = 1.0 - alpha;
    }
    if (!surgery_finite(alpha) || !surgery_finite(beta)) alpha = beta = 1.0;
  }
  state[0] = fa;
  state[1] = fd;
  state[2] = fb;
  state[3] = (float)alpha;
  state[4] = (float)beta;
  state[5] = (float)cosine;
  long long* __restrict__ count = reinterpret_cast<long long*>(state + 8);
  count[0] += 1;
  if (ok && d < 0.0) count[1] += 1;
}

extern "C" int vmtl_surgery_control(const void* workspace, long long rows, long long width, int method, float* state,
                                    void* stream) {
  VMTL_ENTER();
  if (method < VMTL_SURGERY_SUM || method > VMTL_SURGERY_IMTL_G) return VMTL_ERR_UNSUPPORTED;
  if (!workspace || ((uintptr_t)workspace & 7) || !state || ((uintptr_t)state & 7)) return VMTL_ERR_ARG;
  if (rows <= 0 || width <= 0 || rows > (1LL << 62) / width) return VMTL_ERR_ARG;
  hipLaunchKernelGGL(surgery_control_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream,
                     (const double*)workspace, surgery_blocks(rows * width), method, state);
  return vmtl_check_launch();
}

// ------------------------------------------------------------------ combine
// alpha * a + beta * b evaluated in fp64 - both products are exact there, the sum takes one fp64 rounding - and rounded to
// fp32 once, in every path.  (The fp32 form fma(alpha, a, beta * b) rounds beta * b first: where one gradient dominates
// the map that is a second rounding as large as the last one, and the trunk's backward pass amplifies it; the kernel
// is bound by memory, so the wider arithmetic is free.)
__device__ __forceinline__ float surgery_elem(float x, float y, float alpha, float beta) {
  return (float)fma((double)alpha, (double)x, (double)beta * (double)y);
}

__device__ __forceinline__ f32x4 surgery_elem4(const f32x4 x, const f32x4 y, float alpha, float beta) {
  return (f32x4){surgery_elem(x.x, y.x, alpha, beta), surgery_elem(x.y, y.y, alpha, beta),
                 surgery_elem(x.z, y.z, alpha, beta), surgery_elem(x.w, y.w, alpha, beta)};
}

// out may be a: every element is read and then written by the one thread that owns it (no __restrict__ on the three)
template <bool VEC>
__global__ __launch_bounds__(OPT_THREADS) void surgery_combine_kernel(const float* a, long long lda, const float* b,
                                                                      long long ldb, const float* __restrict__ state,
                                                                      float* out, long long ldo, long long rows,
                                                                      long long width, int head) {
  const float alpha = state[3], beta = state[4];
  if (VEC) {
    const long long W = (width - head) >> 2;
    const int tail = (int)(width - head - (W << 2));
    const long long total = rows * W;
    SurgWalk w(W);
    while (w.i + w.S < total) {
      const long long r0 = w.r, c0 = head + (w.c << 2);
      w.step();
      const long long r1 = w.r, c1 = head + (w.c << 2);
      w.step();
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(a + r0 * lda + c0);
      const f32x4 y0 = *reinterpret_cast<const f32x4*>(b + r0 * ldb + c0);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(a + r1 * lda + c1);
      const f32x4 y1 = *reinterpret_cast<const f32x4*>(b + r1 * ldb + c1);
      *reinterpret_cast<f32x4*>(out + r0 * ldo + c0) = surgery_elem4(x0, y0, alpha, beta);
      *reinterpret_cast<f32x4*>(out + r1 * ldo + c1) = surgery_elem4(x1, y1, alpha, beta);
    }
    if (w.i < total) {
      const long long c0 = head + (w.c << 2);
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(a + w.r * lda + c0);
      const f32x4 y0 = *reinterpret_cast<const f32x4*>(b + w.r * ldb + c0);
      *reinterpret_cast<f32x4*>(out + w.r * ldo + c0) = surgery_elem4(x0, y0, alpha, beta);
    }
    const long long j = surgery_peel(head, W, tail);
    if (j >= 0) out[j] = surgery_elem(a[j], b[j], alpha, beta);
  } else {
    const long long total = rows * width;
    for (SurgWalk w(width); w.i < total; w.step())
      out[w.r * ldo + w.c] = surgery_elem(a[w.r * lda + w.c], b[w.r * ldb + w.c], alpha, beta);
  }
}

// Do the elements of p and q (rows rows of width floats, leading dimensions ldp / ldq) share no float?  Disjoint byte
// ranges, or - the interleaved layout - one leading dimension and lanes that never meet: q's lanes start r floats into
// p's rows (modulo the leading dimension) with width <= r <= ld - width.
static bool surgery_disjoint(const float* p, long long ldp, const float* q, long long ldq, long long rows,
                             long long width) {
  const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
  const uintptr_t nx = (uintptr_t)((rows - 1) * ldp + width) * 4, ny = (uintptr_t)((rows - 1) * ldq + width) * 4;
  if (x + nx <= y || y + ny <= x) return true;
  if (rows == 1 || ldp != ldq) return false;
  const long long delta = (long long)(((intptr_t)y - (intptr_t)x) / 4);
  const long long r = ((delta % ldp) + ldp) % ldp;
  return r >= width && r + width <= ldp;
}

extern "C" int vmtl_surgery_combine(const float* a, long long lda, const float* b, long long ldb, const float* state,
                                    float* out, long long ldo, long long rows, long long width, void* stream) {
  VMTL_ENTER();
  if (!surgery_args(a, lda, b, ldb, rows, width) || !out || ((uintptr_t)out & 3) || ldo < width) return VMTL_ERR_ARG;
  if (!state || ((uintptr_t)state & 7)) return VMTL_ERR_ARG;
  // out may BE a (same pointer, same leading dimension: every element is read and written by one thread); any other
  // overlap of out with an operand would race between threads and is refused, as vmtl_swap_ refuses its own
  if (!(out == a && ldo == lda) && !surgery_disjoint(out, ldo, a, lda, rows, width)) return VMTL_ERR_ARG;
  if (!surgery_disjoint(out, ldo, b, ldb, rows, width)) return VMTL_ERR_ARG;
  const SurgPlan p = surgery_plan(a, lda, b, ldb, out, ldo, rows, width);
  const dim3 grid(surgery_blocks(rows * width));
  if (p.vec)
    hipLaunchKernelGGL(surgery_combine_kernel<true>, grid, dim3(OPT_THREADS), 0, (hipStream_t)stream, a, p.lda, b, p.ldb,
                       state, out, p.ldo, p.rows, p.width, p.head);
  else
    hipLaunchKernelGGL(surgery_combine_kernel<false>, grid, dim3(OPT_THREADS), 0, (hipStream_t)stream, a, p.lda, b,
                       p.ldb, state, out, p.ldo, p.rows, p.width, p.head);
  return vmtl_check_launch();
}
