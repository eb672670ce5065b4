// Nearest-x2 upsample + concat + 3x3 conv for the NARROW decoder entries (vmtl_conv2d_up2_halo): the same result as
// vmtl_conv2d_up2_fwd, y = conv3x3(cat[nearest_x2(xl), skip]) evaluated as four 2x2 phase convs on the low-res map,
// from the same packed operand ([4][Cout][4*C0s + 9*C1s], vmtl_pack_up2_fwd).
//
// Why a second UP2 kernel: with 36 / 68 output columns the implicit GEMM (conv_igemm.hip, UP2) stages its 128-row A
// tile through LDS once per (phase, tap): every low-res input pixel is fetched 16 times to feed a few MFMA columns, and
// the launch is bound by its A-operand path (53-75 TF executed).  Here a workgroup owns an output
// tile of 2*TM x 32 full-resolution pixels = TM x 16 low-res pixels per phase:
//   * the (TM+2) x 18 low-res halo of xl and the (2TM+2) x 34 full-res halo of skip are staged into LDS ONCE; every
//     (phase, tap) view is a shifted LDS read of them (the skip taps read every second halo pixel);
//   * wave w computes phase (a, b) = (w >> 1, w & 1): TM MFMA row tiles (one per low-res row of the tile, 16 pixels)
//     x TN column tiles + NT VALU tail columns (33 = 32 + 1, 67 = 64 + 3: the NT convention of conv_small.h);
//   * the weights are NOT staged: the whole 4-phase operand does not fit in LDS next to the halo (block 3: 737 KB), and
//     a wave reads only its own phase's rows, so each B fragment is one buffer load from L2 straight into registers,
//     issued two k-groups ahead of its MFMAs.  Per k-group of 16 a wave issues TN + NT weight loads for 4 * TM * TN
//     MFMAs (TM = 4 for the 33-column layer, so 3 loads per 32 MFMAs);
//   * the K loop has no barrier; afterwards the halo region holds the output tile, which leaves as coalesced float4
//     rows, and (optionally) the tile's per-channel (mean, M2) BatchNorm partials: one statistics row per tile.
//
// LDS (float4 units, slot-major as conv_small.h: halo[channel quad][pixel]; the pixel extents are odd so that the
// staging ds_write_b128 of consecutive channel quads land on distinct banks; one zero quad feeds dead lanes):
//   67 -> 33 (C0s 68, TM 4):      xl halo 17 x 109 = 29.6 KB; output tile 256 px x 36 = 36.9 KB (reuses the halo)
//                                 + 4.6 KB reduction scratch = 41.5 KB -> 3 workgroups (12 waves) per CU
//   135+16 -> 67 (C0s 136 + 16, TM 2): xl halo 34 x 73 = 39.7 KB + skip halo 4 x 205 = 13.1 KB; output tile
//                                 128 px x 68 = 34.8 KB (reuses the halo) + 4.6 KB = 57.4 KB -> 2 workgroups per CU
// The register budget is capped for two waves per SIMD (amdgpu_waves_per_eu(2)).
//
// K order (the packed operand's, so the same weights meet the same inputs): per low-res tap the C0s/4 channel quads are
// consumed four at a time (one per lane quarter); the C0s/4 % 4 left-over quads of the four taps are gathered into
// shared k-groups (68 channels: 16 + 1 groups instead of 20); then the nine skip taps, C1s/4 quads each.
#include "common.h"

#define UH_TW 16  // low-res pixels per tile row (one MFMA row tile)

struct Up2HaloP {
  const float* xl;    // [B][H2][W2][C0S]
  const float* skip;  // [B][2H2][2W2][C1S] or null (C1S == 0)
  const float* wp;    // [4][Nw][KQ * 4] packed phase matrices
  float* y;           // [B][2H2][2W2][ldy]
  float* stats;       // [ntiles][2][ldy] per-tile (mean, M2) or null
  int B, H2, W2, Nw;
  int tiles_x, tiles_y;
  int xl_bytes, skip_bytes, wp_bytes;
};

template <int C0S, int C1S, int TM, int TN, int NT>
struct UhCfg {
  static constexpr int SP0 = C0S / 4, SP1 = C1S / 4;
  static constexpr int FG0 = SP0 / 4, RS0 = SP0 % 4, NGF0 = 4 * FG0, NR0 = 4 * RS0, NGR0 = (NR0 + 3) / 4;
  static constexpr int FG1 = SP1 / 4, NGF1 = 9 * FG1;
  static constexpr int NG = NGF0 + NGR0 + NGF1;  // k-groups of 16
  static constexpr int KQ = 4 * SP0 + 9 * SP1;   // k quads per weight row
  static constexpr int HX0 = UH_TW + 2, HX1 = 2 * UH_TW + 2;
  static constexpr int NP0 = ((TM + 2) * HX0) | 1;
  static constexpr int NP1 = SP1 > 0 ? ((2 * TM + 2) * HX1) | 1 : 0;
  static constexpr int NST0 = (TM + 2) * HX0 * SP0, NST1 = (2 * TM + 2) * HX1 * SP1;
  static constexpr int IT0 = (NST0 + 255) / 256, IT1 = (NST1 + 255) / 256;
  static constexpr int NROWS = 16 * TN;
  static constexpr int OS = NROWS + 4;  // floats per output pixel in LDS = ldy; 36 / 68 = 4 (mod 8)
  static constexpr int SQ = OS / 4;     // channel quads per output pixel
  static constexpr int NPX = 2 * TM * 2 * UH_TW;  // output pixels of a tile
  static constexpr int ZQ = SP0 * NP0 + SP1 * NP1;  // the zero quad
  static constexpr int HALO4 = ZQ + 1;
  static constexpr int OT4 = NPX * SQ;
  static constexpr int MAIN4 = HALO4 > OT4 ? HALO4 : OT4;
  static constexpr int RED4 = 256 + 32;  // [256] lane partials + [32] tile means
  static constexpr int LDS_BYTES = (MAIN4 + RED4) * 16;
  static_assert(C1S % 16 == 0, "skip channels: whole k-groups per tap");
  static_assert(NT >= 1 && NT <= 4, "tail columns");
  static_assert(256 / SQ * SQ <= 256, "statistics lanes");
};

template <int C0S, int C1S, int TM, int TN, int NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void conv_up2_halo_kernel(Up2HaloP p) {
  using C = UhCfg<C0S, C1S, TM, TN, NT>;
  constexpr int SP0 = C::SP0, SP1 = C::SP1, FG0 = C::FG0, RS0 = C::RS0, NGF0 = C::NGF0, NR0 = C::NR0, NGR0 = C::NGR0;
  constexpr int FG1 = C::FG1, NG = C::NG, KQ = C::KQ, HX0 = C::HX0, HX1 = C::HX1, NP0 = C::NP0, NP1 = C::NP1;
  constexpr int NROWS = C::NROWS, OS = C::OS, SQ = C::SQ, NPX = C::NPX, ZQ = C::ZQ;
  constexpr int NB = TN + NT;  // weight loads per k-group
  constexpr unsigned OOB = 0xFFFFFFFFu;

  extern __shared__ __attribute__((aligned(16))) f32x4 smem4[];
  f32x4* halo = smem4;                       // [SP0][NP0] xl, then [SP1][NP1] skip, then the zero quad
  float* otile = reinterpret_cast<float*>(smem4);  // after the K loop: [NPX][OS]
  f32x4* red = smem4 + C::MAIN4;              // [256 + 32]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int pa = wv >> 1, pb = wv & 1;  // this wave's output phase (row parity, column parity)

  int t = blockIdx.x;
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y, b = t / p.tiles_y;
  const int hl0 = ty * TM, wl0 = tx * UH_TW;  // low-res origin of the tile
  const int H = 2 * p.H2, W = 2 * p.W2;

  const __amdgpu_buffer_rsrc_t rs_x = buf_rsrc(p.xl, p.xl_bytes);
  const __amdgpu_buffer_rsrc_t rs_s =
      buf_rsrc(C1S > 0 ? p.skip : p.xl, C1S > 0 ? p.skip_bytes : 0);
  const __amdgpu_buffer_rsrc_t rs_w = buf_rsrc(p.wp, p.wp_bytes);

  // ---- weight rows of this wave's phase: byte offset of (row, k quad 0); rows >= Nw read zeros (out of range)
  unsigned wrow[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int n = j < TN ? 16 * j + l15 : NROWS + (j - TN);
    wrow[j] = n < p.Nw ? (unsigned)((wv * p.Nw + n) * KQ) * 16u : 0x80000000u;
  }
  // left-over k-groups of segment 0: per-lane halo index and k-quad byte offset (dead lanes: zero quad, no weight)
  int arem[NGR0 > 0 ? NGR0 : 1];
  unsigned krem[NGR0 > 0 ? NGR0 : 1];
#pragma unroll
  for (int h = 0; h < NGR0; ++h) {
    const int r = 4 * h + lq;
    if (r < NR0) {
      const int tap = r / (RS0 > 0 ? RS0 : 1), s = FG0 * 4 + r % (RS0 > 0 ? RS0 : 1);
      arem[h] = s * NP0 + (pa + (tap >> 1)) * HX0 + pb + (tap & 1) + l15;
      krem[h] = (unsigned)(tap * SP0 + s) * 16u;
    } else {
      arem[h] = -1;
      krem[h] = 0x40000000u;  // host: wp_bytes < 2^30
    }
  }
  const int a0 = lq * NP0 + pa * HX0 + pb + l15;                  // + cb * NP0 + tap offsets + i * HX0
  const int a1 = SP0 * NP0 + lq * NP1 + pa * HX1 + pb + 2 * l15;  // + cb * NP1 + tap offsets + i * 2 * HX1

  // ---- stage the two halos (out-of-image pixels read zeros: conv zero padding)
  {
    f32x4 r0[C::IT0], r1[C::IT1 > 0 ? C::IT1 : 1];
#pragma unroll
    for (int it = 0; it < C::IT0; ++it) {
      const int f = tid + 256 * it;
      const int pp = f / SP0, s = f - pp * SP0;
      const int hy = pp / HX0, hx = pp - hy * HX0;
      const int gh = hl0 - 1 + hy, gw = wl0 - 1 + hx;
      const bool ok = f < C::NST0 && (unsigned)gh < (unsigned)p.H2 && (unsigned)gw < (unsigned)p.W2;
      r0[it] = buf_load16(rs_x, ok ? (unsigned)((b * p.H2 + gh) * p.W2 + gw) * (unsigned)(C0S * 4) + 16u * s : OOB);
    }
#pragma unroll
    for (int it = 0; it < C::IT1; ++it) {
      const int f = tid + 256 * it;
      const int pp = f / (SP1 > 0 ? SP1 : 1), s = f - pp * SP1;
      const int hy = pp / HX1, hx = pp - hy * HX1;
      const int gh = 2 * hl0 - 1 + hy, gw = 2 * wl0 - 1 + hx;
      const bool ok = f < C::NST1 && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W;
      r1[it] = buf_load16(rs_s, ok ? (unsigned)((b * H + gh) * W + gw) * (unsigned)(C1S * 4) + 16u * s : OOB);
    }
#pragma unroll
    for (int it = 0; it < C::IT0; ++it) {
      const int f = tid + 256 * it;
      const int pp = f / SP0, s = f - pp * SP0;
      if (f < C::NST0) halo[s * NP0 + pp] = r0[it];
    }
#pragma unroll
    for (int it = 0; it < C::IT1; ++it) {
      const int f = tid + 256 * it;
      const int pp = f / (SP1 > 0 ? SP1 : 1), s = f - pp * SP1;
      if (f < C::NST1) halo[SP0 * NP0 + s * NP1 + pp] = r1[it];
    }
    if (tid == 0) halo[ZQ] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();

  // ---- K loop
  f32x4 acc[TM][TN];
  f32x2 tacc[TM][NT];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) tacc[i][tt] = (f32x2){0.f, 0.f};
  }
  // k-group g -> this lane's k-quad byte offset in a weight row, and its halo index for row tile 0 (-1: zero quad)
  auto group = [&](int g, unsigned& koff, int& ai, int& istep) {
    if (g < NGF0) {
      const int tap = g / FG0, cb = (g % FG0) * 4;
      koff = (unsigned)(tap * SP0 + cb + lq) * 16u;
      ai = a0 + cb * NP0 + (tap >> 1) * HX0 + (tap & 1);
      istep = HX0;
    } else if (g < NGF0 + NGR0) {
      koff = krem[g - NGF0];
      ai = arem[g - NGF0];
      istep = HX0;
    } else {
      const int g1 = g - NGF0 - NGR0;
      const int tap = g1 / (FG1 > 0 ? FG1 : 1), cb = (g1 % (FG1 > 0 ? FG1 : 1)) * 4;
      koff = (unsigned)(4 * SP0 + tap * SP1 + cb + lq) * 16u;
      ai = a1 + cb * NP1 + (tap / 3) * HX1 + tap % 3;
      istep = 2 * HX1;
    }
  };
  auto load_b = [&](int g, f32x4 (&bq)[NB]) {
    unsigned koff;
    int ai, istep;
    group(g, koff, ai, istep);
#pragma unroll
    for (int j = 0; j < NB; ++j) bq[j] = buf_load16(rs_w, wrow[j] + koff);
  };
  auto load_a = [&](int g, f32x4 (&aq)[TM]) {
    unsigned koff;
    int ai, istep;
    group(g, koff, ai, istep);
#pragma unroll
    for (int i = 0; i < TM; ++i) aq[i] = halo[ai < 0 ? ZQ : ai + i * istep];
  };
  auto mma = [&](const f32x4 (&aq)[TM], const f32x4 (&bq)[NB]) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[i][e], bq[j][e], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
      const f32x4 w = bq[TN + tt];
      const f32x2 lo = __builtin_shufflevector(w, w, 0, 1), hi = __builtin_shufflevector(w, w, 2, 3);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        tacc[i][tt] += __builtin_shufflevector(aq[i], aq[i], 0, 1) * lo;
        tacc[i][tt] += __builtin_shufflevector(aq[i], aq[i], 2, 3) * hi;
        asm volatile("" : "+v"(tacc[i][tt]));  // keep the tail FMAs next to their MFMAs (see conv_small.h)
      }
    }
  };
  // software pipeline: weights (L2) two k-groups ahead, halo fragments (LDS) one k-group ahead
  f32x4 bq[3][NB], aq[2][TM];
  load_b(0, bq[0]);
  if (NG > 1) load_b(1, bq[1]);
  load_a(0, aq[0]);
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    if (g + 2 < NG) load_b(g + 2, bq[(g + 2) % 3]);
    if (g + 1 < NG) load_a(g + 1, aq[(g + 1) & 1]);
    mma(aq[g & 1], bq[g % 3]);
    if (g + 2 < NG) __builtin_amdgcn_sched_group_barrier(0x020, NB, 0);  // weight loads of g+2
    if (g + 1 < NG) __builtin_amdgcn_sched_group_barrier(0x100, TM, 0);  // LDS reads of g+1
    __builtin_amdgcn_sched_group_barrier(0x008, 4 * TM * TN, 0);        // MFMAs of g
    __builtin_amdgcn_sched_group_barrier(0x002, 4 * TM * NT + 8, 0);    // tail FMAs (+ address VALU)
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- epilogue: C layout (column = lane & 15, pixel = 4 * (lane >> 4) + reg of row tile i) -> LDS output tile
  float tv[TM][NT];
#pragma unroll
  for (int tt = 0; tt < NT; ++tt)
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      float v = tacc[i][tt][0] + tacc[i][tt][1];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      tv[i][tt] = v;  // low-res pixel l15 of row tile i, column NROWS + tt
    }
  __syncthreads();  // every wave is out of the halo
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int prow = (2 * i + pa) * (2 * UH_TW) + pb;  // + 2 * low-res column
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) otile[(prow + 2 * (4 * lq + r)) * OS + 16 * j + l15] = acc[i][j][r];
    if (lq == 0) {
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) otile[(prow + 2 * l15) * OS + NROWS + tt] = tt < NT ? tv[i][tt < NT ? tt : 0] : 0.f;
    }
  }
  __syncthreads();

  // ---- coalesced float4 stores of the tile's full-resolution rows
  const f32x4* ot4 = reinterpret_cast<const f32x4*>(otile);
  constexpr int SIT = (NPX * SQ + 255) / 256;
#pragma unroll
  for (int it = 0; it < SIT; ++it) {
    const int f = tid + 256 * it;
    if (f < NPX * SQ) {
      const int px = f / SQ, q = f - px * SQ;
      const int gy = 2 * hl0 + px / (2 * UH_TW), gx = 2 * wl0 + px % (2 * UH_TW);
      if (gy < H && gx < W)
        *reinterpret_cast<f32x4*>(p.y + ((unsigned)((b * H + gy) * W + gx) * (unsigned)OS + 4u * q)) = ot4[f];
    }
  }

  // ---- per-tile BatchNorm partials (host: only for full tiles): mean first, M2 around it
  if (p.stats != nullptr) {
    constexpr int G = 256 / SQ;  // lanes per channel quad
    const int q = tid % SQ, gi = tid / SQ;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (gi < G)
      for (int px = gi; px < NPX; px += G) s += ot4[px * SQ + q];
    red[tid] = s;
    __syncthreads();
    if (tid < SQ) {
      f32x4 m = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < G; ++k) m += red[k * SQ + tid];
      red[256 + tid] = m * (1.f / (float)NPX);
    }
    __syncthreads();
    const f32x4 m = red[256 + q];
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    if (gi < G)
      for (int px = gi; px < NPX; px += G) {
        const f32x4 d = ot4[px * SQ + q] - m;
        c += d * d;
      }
    red[tid] = c;
    __syncthreads();
    if (tid < SQ) {
      f32x4 m2 = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < G; ++k) m2 += red[k * SQ + tid];
      *reinterpret_cast<f32x4*>(p.stats + ((size_t)blockIdx.x * 2 + 0) * OS + 4 * tid) = m;
      *reinterpret_cast<f32x4*>(p.stats + ((size_t)blockIdx.x * 2 + 1) * OS + 4 * tid) = m2;
    }
  }
}

template <int C0S, int C1S, int TM, int TN, int NT>
static int launch_up2_halo(Up2HaloP& p, hipStream_t st) {
  using C = UhCfg<C0S, C1S, TM, TN, NT>;
  static_assert(C::LDS_BYTES <= 64 * 1024, "at least two workgroups per CU");
  const int rc = allow_dynamic_lds(reinterpret_cast<const void*>(&conv_up2_halo_kernel<C0S, C1S, TM, TN, NT>), C::LDS_BYTES);
  if (rc) return rc;
  p.tiles_x = cdiv(p.W2, UH_TW);
  p.tiles_y = cdiv(p.H2, TM);
  hipLaunchKernelGGL((conv_up2_halo_kernel<C0S, C1S, TM, TN, NT>), dim3(p.B * p.tiles_x * p.tiles_y), dim3(256),
                     C::LDS_BYTES, st, p);
  return vmtl_check_launch();
}

// ---------------------------------------------------------------------------------------------- host side
// The instantiated shapes (the narrow decoder entries of the U-Net decoders): C0s + C1s -> Cout, low-res rows per tile.
//   68 + 0 -> 33:   TM 4, 2 MFMA column tiles + 1 tail column
//   136 + 16 -> 67: TM 2, 4 MFMA column tiles + 3 tail columns
static int up2_halo_tm(int C0s, int C1s, int ldy, int Cout) {
  if (C0s == 68 && C1s == 0 && Cout == 33 && ldy == 36) return 4;
  if (C0s == 136 && C1s == 16 && Cout == 67 && ldy == 68) return 2;
  return 0;
}

// 32-bit byte offsets in the kernel (buffer loads, output stores): every tensor under 2 GiB
static bool up2_halo_fits(int B, int H2, int W2, int C0s, int C1s, int ldy) {
  const long long px = (long long)B * H2 * W2;
  return px * C0s * 4 <= 0x7fffffffLL && 4 * px * C1s * 4 <= 0x7fffffffLL && 4 * px * ldy * 4 <= 0x7fffffffLL;
}

extern "C" int vmtl_conv2d_up2_halo_supported(int B, int H2, int W2, int C0s, int C1s, int ldy, int Cout) {
  return B > 0 && H2 > 0 && W2 > 0 && up2_halo_tm(C0s, C1s, ldy, Cout) > 0 && up2_halo_fits(B, H2, W2, C0s, C1s, ldy);
}

// statistics geometry: one row per tile of 2*TM x 32 full-resolution pixels; rows = 0 when the tiles do not cover the
// image exactly (statistics need equal rows) or the shape is not supported
extern "C" int vmtl_conv2d_up2_halo_stat_block(int C0s, int C1s, int ldy, int Cout) {
  return 4 * UH_TW * up2_halo_tm(C0s, C1s, ldy, Cout);
}

extern "C" int vmtl_conv2d_up2_halo_stat_rows(int B, int H2, int W2, int C0s, int C1s, int ldy, int Cout) {
  const int tm = up2_halo_tm(C0s, C1s, ldy, Cout);
  if (tm == 0 || B <= 0 || H2 <= 0 || W2 <= 0 || H2 % tm || W2 % UH_TW) return 0;
  return B * (H2 / tm) * (W2 / UH_TW);
}

extern "C" int vmtl_conv2d_up2_halo(const float* xl, const float* skip, const float* wp_eff, float* y, float* stats,
                                    int B, int H2, int W2, int C0s, int C1s, int ldy, int Cout, void* stream) {
  VMTL_ENTER();
  if (!xl || !wp_eff || !y || B <= 0 || H2 <= 0 || W2 <= 0 || C0s <= 0 || C1s < 0 || Cout <= 0 || Cout > ldy)
    return VMTL_ERR_ARG;
  if ((skip == nullptr) != (C1s == 0)) return VMTL_ERR_ARG;
  const int tm = up2_halo_tm(C0s, C1s, ldy, Cout);
  if (tm == 0) return VMTL_ERR_UNSUPPORTED;
  if (stats != nullptr && vmtl_conv2d_up2_halo_stat_rows(B, H2, W2, C0s, C1s, ldy, Cout) == 0) return VMTL_ERR_ARG;
  if (!up2_halo_fits(B, H2, W2, C0s, C1s, ldy)) return VMTL_ERR_UNSUPPORTED;
  const long long px = (long long)B * H2 * W2;
  Up2HaloP p;
  p.xl = xl; p.skip = skip; p.wp = wp_eff; p.y = y; p.stats = stats;
  p.B = B; p.H2 = H2; p.W2 = W2; p.Nw = Cout;
  p.xl_bytes = (int)(px * C0s * 4);
  p.skip_bytes = (int)(4 * px * C1s * 4);
  p.wp_bytes = 4 * Cout * (4 * C0s + 9 * C1s) * 4;  // < 2^30 for the instantiated shapes (dead lanes rely on it)
  hipStream_t st = (hipStream_t)stream;
  if (tm == 4) return launch_up2_halo<68, 0, 4, 2, 1>(p, st);
  return launch_up2_halo<136, 16, 2, 4, 3>(p, st);
}
