// Shared device/host helpers for the vmtl HIP kernels (gfx950 / CDNA4 only).
//
// Activation layout everywhere in this library: NHWC fp32, shape [B][H][W][Cs]
// where Cs ("storage channels") = round_up(C, 4) and channels c in [C, Cs) are
// always ZERO.  Every kernel that writes an activation keeps that invariant, so
// 16-byte loads along the channel axis are always aligned and K-padding in the
// implicit GEMMs contributes exact zeros.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#define VMTL_OK 0
#define VMTL_ERR_ARG (-1)
#define VMTL_ERR_LAUNCH (-2)
#define VMTL_ERR_UNSUPPORTED (-3)

// activation codes shared by the C-ABI and the kernels
#define VMTL_ACT_NONE 0
#define VMTL_ACT_RELU 1
#define VMTL_ACT_HSWISH 2
#define VMTL_ACT_HSIGMOID 3
#define VMTL_ACT_SIGMOID 4

// operand precision of the implicit-GEMM convolutions (the *_p entry points)
#define VMTL_PREC_FP32 0
#define VMTL_PREC_BF16 1
static inline bool valid_prec(int prec) { return prec == VMTL_PREC_FP32 || prec == VMTL_PREC_BF16; }

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Every launching entry point starts with VMTL_ENTER(): hipGetLastError() is per-thread state shared with
// every other HIP user in the process (e.g. an ignored status inside the framework that hosts us), and
// the status returned by vmtl_check_launch() must describe OUR launch only.
#define VMTL_ENTER() ((void)hipGetLastError())

extern thread_local int vmtl_last_hip_error;  // version.hip; read back with vmtl_last_error_string()

static inline int vmtl_check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) vmtl_last_hip_error = (int)e;
  return e == hipSuccess ? VMTL_OK : VMTL_ERR_LAUNCH;
}

// Tuning overrides (VMTL_FORCE_TILE, VMTL_BF16X3, ...) are read from the environment ONCE, on first use - never per
// launch (getenv walks the whole environment block: host cost on the eager path).  vmtl_reload_env() bumps the epoch so
// that the next use re-reads them (the parity tests toggle them between cases).
extern int vmtl_env_epoch;  // version.hip
struct EnvInt {
  const char* name;
  int dflt;
  int value = 0;
  int epoch = 0;
};
static inline int env_int(EnvInt& e) {
  if (e.epoch != vmtl_env_epoch) {
    const char* s = getenv(e.name);
    e.value = s ? atoi(s) : e.dflt;
    e.epoch = vmtl_env_epoch;
  }
  return e.value;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline long long cdivll(long long a, long long b) { return (a + b - 1) / b; }

// Blocks of a 1-D grid whose kernel strides over n items (VMTL_GRID_STRIDE): one block per `per_block` items, at least
// 1 and at most `cap`.  per_block and cap are each launch site's own (several were tuned).
static inline int grid_1d(long long n, int per_block, int cap) {
  const long long nb = cdivll(n, per_block);
  return nb < 1 ? 1 : (nb > cap ? cap : (int)nb);
}

// Compute units of the current device, queried once per process (version.hip); 256 when the query fails.
int vmtl_num_cus();

// Opts `kernel` into `bytes` of dynamic LDS (a launch that asks for more than 64 KB fails without it).  Set on every
// launch: a function attribute is per device, and a cached flag would be neither thread-safe nor right for a second
// GPU of the process (the call is a cheap driver-side table update).
static inline int allow_dynamic_lds(const void* kernel, size_t bytes) {
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) vmtl_last_hip_error = (int)e;
  return e == hipSuccess ? VMTL_OK : VMTL_ERR_LAUNCH;
}

__device__ __forceinline__ float act_fwd(float v, int act) {
  switch (act) {
    case VMTL_ACT_RELU: return v > 0.f ? v : 0.f;
    case VMTL_ACT_HSWISH: {
      float r = fminf(fmaxf(v + 3.f, 0.f), 6.f);
      return v * r * (1.f / 6.f);
    }
    case VMTL_ACT_HSIGMOID: return fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f);
    case VMTL_ACT_SIGMOID: return 1.f / (1.f + __expf(-v));
    default: return v;
  }
}

// the sigmoid of the depth head's post-processing (vmtl_eltwise mode 1; csrc/tta.hip applies it per tap): libm's expf,
// not the fast exponential of VMTL_ACT_SIGMOID above, and one definition so that both give the same bits
__device__ __forceinline__ float sigmoid_exact(float v) { return 1.f / (1.f + expf(-v)); }

// derivative of act at pre-activation v (torch conventions: relu'(0)=0,
// hardswish' = 0 for v<-3, 1 for v>3, (2v+3)/6 between (the torch releases this was written
// against use < and >: the boundary points take the middle formula; torch 2.10 returns 0 at -3
// and 1 at 3 - tests/test_bn_kernels_gpu.py pins the values here and prints torch's),
// hardsigmoid' = 1/6 on (-3,3)).
__device__ __forceinline__ float act_grad(float v, int act) {
  switch (act) {
    case VMTL_ACT_RELU: return v > 0.f ? 1.f : 0.f;
    case VMTL_ACT_HSWISH:
      return v < -3.f ? 0.f : (v > 3.f ? 1.f : (2.f * v + 3.f) * (1.f / 6.f));
    case VMTL_ACT_HSIGMOID: return (v > -3.f && v < 3.f) ? (1.f / 6.f) : 0.f;
    case VMTL_ACT_SIGMOID: {
      float s = 1.f / (1.f + __expf(-v));
      return s * (1.f - s);
    }
    default: return 1.f;
  }
}

// 64-lane wavefront sum by the xor-shuffle tree 32, 16, .., 1 (float, double, unsigned, unsigned long long); every lane
// gets the total.  The tree's order is part of the run-to-run reproducibility contract: reduce.h lists what is built on it.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The one grid-stride loop: element i of n for a 1-D grid of any size, 64-bit index.
#define VMTL_GRID_STRIDE(i, n)                                                      \
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n);     \
       i += (long long)gridDim.x * blockDim.x)

// fp32 -> bf16 operand rounding of the VMTL_PREC_BF16 contract: a plain cast, which is round-to-nearest-even with NaN
// staying NaN, and compiles to v_cvt_pk_bf16_f32 (two values per instruction).  The results are the packed bf16 bits.
__device__ __forceinline__ unsigned round_bf16x2(float lo, float hi) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){lo, hi}, bf16x2));
}
__device__ __forceinline__ u32x2 round_bf16x4(f32x4 v) {
  return __builtin_bit_cast(u32x2, __builtin_convertvector(v, bf16x4));
}
// a lane's eight k values of one v_mfma_f32_16x16x32_bf16 operand: two fp32 quads, rounded
__device__ __forceinline__ bf16x8 round_bf16x8(f32x4 lo, f32x4 hi) {
  const u32x2 l = round_bf16x4(lo), h = round_bf16x4(hi);
  return __builtin_bit_cast(bf16x8, (u32x4){l[0], l[1], h[0], h[1]});
}

// Buffer-resource access: 32-bit byte offsets against a descriptor (base, stride 0, num_records = bytes, flag word).
// 0x00020000 is word 3 of the descriptor with only DATA_FORMAT = 32-bit set (bits 15..18 = 4): a raw, unswizzled,
// untyped buffer without stride or thread-id addressing.  With stride 0 the hardware checks every access's byte offset
// against num_records: a load at an offset outside [0, bytes) returns zeros and a store there is dropped, so the
// kernels pass 0xFFFFFFFF for "no element here" (and a zero-length descriptor for "no tensor") instead of branching.
// Build descriptors from wave-uniform values only.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 buf_load16(__amdgpu_buffer_rsrc_t r, unsigned byte_offset) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_offset, 0, 0));
}

// LDS-only workgroup barrier: waits for this wave's LDS traffic, not for its global loads in flight (__syncthreads()
// would also drain a prefetch)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Sum over the four lane quarters (lanes l, l+16, l+32, l+48 of a wave; every lane gets the total).
// (Round 3 tried gfx950's v_permlane16_swap / v_permlane32_swap here - two VALU instructions instead of two ds_bpermute
// round trips.  Every kernel test passed, but MTAN's end-to-end gradients came out up to 18 % wrong in builds where the
// surrounding epilogue code was scheduled differently (tests/test_tight_grads_gpu.py; each of two unrelated source changes
// alone hid it): the swaps sit right in front of an EXEC-mask change, a hazard the compiler does not pad.  ds_bpermute it is.)
__device__ __forceinline__ float quarter_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// every lane gets the value its column's lane of quarter 0 holds (lane & 15)
__device__ __forceinline__ float quarter0_bcast(float v) { return __shfl(v, threadIdx.x & 15, 64); }

// XCD-aware bijective remap of a linear workgroup id: workgroups that end up
// with consecutive remapped ids share an XCD (and therefore an L2).  Speed
// only; any placement is correct.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}
