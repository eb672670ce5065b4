// 3x3 / stride 1 / pad 1 convolution for the MID-WIDTH layers (vmtl_conv3x3_halo): 64 or 68 input storage channels,
// 16 / 32 / 64 / 68 output storage channels - `basic` decoder block 3 conv2 and its data gradients, MTAN's 64-channel convs and
// csnet's 64-channel convs at full batch.  The same result as vmtl_conv2d_fwd / vmtl_conv2d_bnbwd on the same packed
// operand ([Nw][9 * CS], k = tap * CS + c: packs "fwd" / "dgrad").
//
// Why a third 3x3 kernel: the implicit GEMM (conv_igemm.hip) re-stages every input pixel once per tap, and pays four
// VALU tail columns next to the MFMAs of a 67-column layer (64-78 TF executed).  Here a workgroup
// owns a TM x 32 pixel output tile (TM = 4):
//   * the (TM+2) x 34 input halo is staged into LDS ONCE (transformed by the optional prologue); every tap is a
//     shifted LDS read of it;
//   * the waves split the OUTPUT COLUMNS: with 4 MFMA column tiles, wave w owns column tile w across all 2 * TM row
//     tiles of 16 pixels, so per k-group of 16 it issues ONE weight load for 8 x 4 MFMAs (a row split would make all
//     four waves load the same fragments).  With 1 / 2 column tiles the waves split the rows as well;
//   * the weights (166 KB for 68 -> 67) do not fit next to the halo: each B fragment is one buffer load from L2
//     straight into registers, issued two k-groups ahead of its MFMAs (as conv_up2_halo.hip);
//   * the 65th..68th columns are VALU tail columns (conv_small.h's convention: only the remainder off the matrix
//     pipe).  Wave w computes tail column 64 + w over the whole tile: one more weight load per k-group and 2 * 2 * TM
//     packed FMAs next to its 32 MFMAs; rows >= Nw read zeros;
//   * the K loop has no barrier; afterwards the halo region holds the output tile, which leaves as coalesced float4
//     rows through the epilogue (bias; per-tile BatchNorm (mean, M2); or the fused BatchNorm + activation backward of
//     the producer: dz = acc * act'(z) and per-tile (sum dz, sum dz * xhat), as conv_small.h's ep_mode 2).
//
// LDS (float4 units, slot-major as conv_small.h: halo[channel quad][pixel], odd pixel extent 205 so that the staging
// ds_write_b128 of consecutive channel quads land on distinct banks; one zero quad feeds the dead lanes of the shared
// left-over k-groups):
//   CS 68: halo 17 x 205 + 1 = 55.8 KB; output tile 128 px x 68 = 34.8 KB + 8 KB reduction scratch (both reuse the
//          halo) + 1.9 KB per-channel parameters = 57.7 KB -> 2 workgroups (8 waves) per CU
//   CS 64: 16 x 205 + 1 = 52.5 KB + 1.9 KB = 54.4 KB
// The register budget is capped for two waves per SIMD (amdgpu_waves_per_eu(2)).
//
// K order: per tap the CS/4 channel quads are consumed four at a time (one per lane quarter); the CS/4 % 4 left-over
// quads of the nine taps share k-groups (68 channels: 36 + 3 groups of 16 instead of 45), as conv_small.h.
#include "common.h"

#define CH_TM 4                         // output rows per tile
#define CH_TW 32                        // output pixels per tile row
#define CH_HX (CH_TW + 2)               // halo row extent
#define CH_NHALO ((CH_TM + 2) * CH_HX)  // 204 halo pixels
#define CH_NP (CH_NHALO | 1)            // slot-major pixel extent (odd)
#define CH_NPX (CH_TM * CH_TW)          // 128 output pixels per tile

struct HaloP {
  const float* x;     // [B][H][W][CS]
  const float* pa;    // [CS] prologue coefficients (null: identity prologue)
  const float* pc;
  float* a_out;       // optional: transformed input, same shape as x
  const float* wp;    // [Nw][9 * CS] packed
  const float* bias;  // [Cout] or null
  float* y;           // [B][H][W][ldy]
  float* stats;       // [ntiles][2][ldy] (ep_mode 1, 2)
  const float* ez_x;  // ep_mode 2: pre-BatchNorm activation of the producer of y's tensor, [B][H][W][ldy]
  const float* ez_mean;
  const float* ez_invstd;
  const float* ez_gamma;
  const float* ez_beta;
  int act_in, ep_mode, ez_act;
  int B, H, W, ldy, Nw, Cout;
  int tiles_x, tiles_y;
  unsigned x_bytes, wp_bytes;
};

template <int CS, int TN, bool TAIL>
struct HaloCfg {
  static constexpr int SP = CS / 4, FG = SP / 4, RS = SP % 4;
  static constexpr int KQ = 9 * SP;                  // k quads per weight row
  static constexpr int NGF = 9 * FG, NR = 9 * RS, NGR = (NR + 3) / 4;
  static constexpr int NG = NGF + NGR;               // k-groups of 16
  static constexpr int NROWS = 16 * TN;              // MFMA columns
  static constexpr int OS = NROWS + 4;               // floats per output pixel in LDS: 4 (mod 8)
  static constexpr int SQ = TAIL ? OS / 4 : TN * 4;  // quads per stored pixel: ldy = round_up(Nw, 4) / 4
  static constexpr int NRT = 2 * CH_TM;              // row tiles of 16 pixels
  static constexpr int WM = 4 / TN;                  // waves along the rows
  static constexpr int RT = NRT / WM;                // row tiles per wave
  static constexpr int NST = CH_NHALO * SP;          // float4 elements of the halo
  static constexpr int IT = (NST + 255) / 256;
  static constexpr int ZQ = SP * CH_NP;              // the zero quad
  static constexpr int HALO4 = ZQ + 1;
  static constexpr int OT4 = CH_NPX * OS / 4;
  static constexpr int RED4 = 2 * 256;               // [2][256] lane partials
  static constexpr int MAIN4 = HALO4 > OT4 + RED4 ? HALO4 : OT4 + RED4;
  static constexpr int PQ = (OS + 3) / 4;            // parameter quads per channel set (>= ldy / 4)
  static constexpr int PAR4 = 2 * SP + 5 * PQ;       // prologue (pa, pc) + epilogue (bias, mean, invstd, gamma, beta)
  static constexpr int LDS_BYTES = (MAIN4 + PAR4) * 16;
  static_assert(TN == 1 || TN == 2 || TN == 4, "column tiles");
  static_assert(!TAIL || TN == 4, "tail columns only next to 4 MFMA column tiles (one per wave)");
  static_assert(CS % 4 == 0 && FG >= 1, "channel quads");
};

template <int CS, int TN, bool TAIL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void conv3x3_halo_kernel(HaloP p) {
  using C = HaloCfg<CS, TN, TAIL>;
  constexpr int SP = C::SP, FG = C::FG, RS = C::RS, KQ = C::KQ, NGF = C::NGF, NR = C::NR, NGR = C::NGR, NG = C::NG;
  constexpr int NROWS = C::NROWS, OS = C::OS, RT = C::RT, IT = C::IT, ZQ = C::ZQ, PQ = C::PQ;
  constexpr int NB = TAIL ? 2 : 1;  // weight loads per k-group: the wave's column tile (+ its tail column)
  constexpr unsigned OOB = 0xFFFFFFFFu;

  extern __shared__ __attribute__((aligned(16))) f32x4 smem4[];
  f32x4* halo = smem4;                             // [SP][NP] + the zero quad
  float* otile = reinterpret_cast<float*>(smem4);  // after the K loop: [NPX][OS]
  f32x4* red = smem4 + C::OT4;                     // after the K loop: [2][256]
  f32x4* par = smem4 + C::MAIN4;                   // [SP] pa, [SP] pc, then [5][PQ] epilogue parameters
  f32x4* epar = par + 2 * SP;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int jw = wv % TN, rw = wv / TN;  // this wave's column tile and row-tile group

  int t = blockIdx.x;
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y, b = t / p.tiles_y;
  const int h0 = ty * CH_TM, w0 = tx * CH_TW;

  const __amdgpu_buffer_rsrc_t rs_x = buf_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t rs_w = buf_rsrc(p.wp, p.wp_bytes);

  // ---- per-channel parameters into LDS (vectors of logical length: element-wise, zeros past the end)
  const bool has_pro = p.pa != nullptr;
  if (tid < 2 * SP) {
    const float* src = tid < SP ? p.pa : p.pc;
    const int s = tid < SP ? tid : tid - SP;
    par[tid] = has_pro ? *reinterpret_cast<const f32x4*>(src + 4 * s) : (f32x4){0.f, 0.f, 0.f, 0.f};  // [CS] each
  }
  if (tid < 5 * PQ) {
    const int which = tid / PQ, q = tid - which * PQ;
    const float* src = which == 0 ? p.bias : (which == 1 ? p.ez_mean : (which == 2 ? p.ez_invstd : (which == 3 ? p.ez_gamma : p.ez_beta)));
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (src != nullptr && (which == 0 || p.ep_mode == 2)) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < p.Cout) v[e] = src[4 * q + e];
    }
    epar[tid] = v;
  }

  // ---- weight rows of this wave: byte offset of (row, k quad 0); rows >= Nw read zeros (out of range)
  unsigned wrow[NB];
  {
    const int n = 16 * jw + l15;
    wrow[0] = n < p.Nw ? (unsigned)(n * KQ) * 16u : 0x80000000u;
    if (TAIL) {
      const int nt = NROWS + wv;  // tail column of this wave (wave-uniform row)
      wrow[NB - 1] = nt < p.Nw ? (unsigned)(nt * KQ) * 16u : 0x80000000u;
    }
  }
  // left-over k-groups: per-lane halo index and k-quad byte offset (dead lanes: zero quad, no weight)
  int arem[NGR > 0 ? NGR : 1];
  unsigned krem[NGR > 0 ? NGR : 1];
#pragma unroll
  for (int h = 0; h < NGR; ++h) {
    const int r = 4 * h + lq;
    if (r < NR) {
      const int tap = r / (RS > 0 ? RS : 1), s = FG * 4 + r % (RS > 0 ? RS : 1);
      arem[h] = s * CH_NP + (tap / 3) * CH_HX + tap % 3 + l15;
      krem[h] = (unsigned)(tap * SP + s) * 16u;
    } else {
      arem[h] = -1;
      krem[h] = 0x40000000u;  // host: wp_bytes < 2^30
    }
  }
  const int a0 = lq * CH_NP + l15;  // + cb * NP + tap offset + row-tile offset
  // halo offset of row tile i (output row i >> 1, pixels 16 * (i & 1) ..)
  auto rtoff = [](int i) { return (i >> 1) * CH_HX + 16 * (i & 1); };

  // ---- stage the halo (out-of-image pixels are zeros AFTER the prologue: conv zero padding)
  {
    f32x4 r0[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int f = tid + 256 * it;
      const int pp = f / SP, s = f - pp * SP;
      const int hy = pp / CH_HX, hx = pp - hy * CH_HX;
      const int gh = h0 - 1 + hy, gw = w0 - 1 + hx;
      const bool ok = f < C::NST && (unsigned)gh < (unsigned)p.H && (unsigned)gw < (unsigned)p.W;
      r0[it] = buf_load16(rs_x, ok ? (unsigned)((b * p.H + gh) * p.W + gw) * (unsigned)(CS * 4) + 16u * s : OOB);
    }
    if (has_pro) __syncthreads();  // the prologue coefficients are in LDS
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int f = tid + 256 * it;
      if (f >= C::NST) continue;
      const int pp = f / SP, s = f - pp * SP;
      f32x4 v = r0[it];
      if (has_pro) {
        const int hy = pp / CH_HX, hx = pp - hy * CH_HX;
        const int gh = h0 - 1 + hy, gw = w0 - 1 + hx;
        const bool ok = (unsigned)gh < (unsigned)p.H && (unsigned)gw < (unsigned)p.W;
        v = v * par[s] + par[SP + s];
        if (p.act_in == VMTL_ACT_RELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        if (!ok) v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (p.a_out != nullptr && ok && hy >= 1 && hy <= CH_TM && hx >= 1 && hx <= CH_TW)
          *reinterpret_cast<f32x4*>(p.a_out + (size_t)((b * p.H + gh) * p.W + gw) * CS + 4 * s) = v;
      }
      halo[s * CH_NP + pp] = v;
    }
    if (tid == 0) halo[ZQ] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  // ---- epilogue geometry: thread <-> (channel quad q, pixel group gi): coalesced float4 rows, fixed quad per thread
  constexpr int SQ = C::SQ, G = 256 / SQ;  // quads stored per pixel, pixel groups
  constexpr int EIT = (CH_NPX + G - 1) / G;  // passes over the tile's pixels
  const int eq = tid % SQ, gi = tid / SQ;
  const bool elane = gi < G;
  // mode 2: the producer's pre-BatchNorm activation of this thread's pixels, fetched under the K loop
  f32x4 rz[EIT];
  if (p.ep_mode == 2) {
#pragma unroll
    for (int it = 0; it < EIT; ++it) {
      const int px = gi + it * G;
      const int gy = h0 + px / CH_TW, gx = w0 + px % CH_TW;
      rz[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (elane && px < CH_NPX && gy < p.H && gx < p.W)
        rz[it] = *reinterpret_cast<const f32x4*>(p.ez_x + (size_t)((b * p.H + gy) * p.W + gx) * p.ldy + 4 * eq);
    }
  }
  __syncthreads();

  // ---- K loop
  f32x4 acc[RT];
  f32x2 tacc[TAIL ? C::NRT : 1];
#pragma unroll
  for (int i = 0; i < RT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < (TAIL ? C::NRT : 1); ++i) tacc[i] = (f32x2){0.f, 0.f};
  const int rbase = rw * RT;  // first row tile of this wave
  // k-group g -> this lane's k-quad byte offset in a weight row, and its halo index for row tile 0 (-1: zero quad)
  auto group = [&](int g, unsigned& koff, int& ai) {
    if (g < NGF) {
      const int tap = g / FG, cb = (g % FG) * 4;
      koff = (unsigned)(tap * SP + cb + lq) * 16u;
      ai = a0 + cb * CH_NP + (tap / 3) * CH_HX + tap % 3;
    } else {
      koff = krem[g - NGF];
      ai = arem[g - NGF];
    }
  };
  auto load_b = [&](int g, f32x4 (&bq)[NB]) {
    unsigned koff;
    int ai;
    group(g, koff, ai);
#pragma unroll
    for (int j = 0; j < NB; ++j) bq[j] = buf_load16(rs_w, wrow[j] + koff);
  };
  auto load_a = [&](int g, f32x4 (&aq)[RT]) {
    unsigned koff;
    int ai;
    group(g, koff, ai);
#pragma unroll
    for (int i = 0; i < RT; ++i) aq[i] = halo[ai < 0 ? ZQ : ai + rtoff(rbase + i)];
  };
  auto mma = [&](const f32x4 (&aq)[RT], const f32x4 (&bq)[NB]) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < RT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[i][e], bq[0][e], acc[i], 0, 0, 0);
    if (TAIL) {  // TN == 4: every wave holds all row tiles
      const f32x4 w = bq[NB - 1];
      const f32x2 lo = __builtin_shufflevector(w, w, 0, 1), hi = __builtin_shufflevector(w, w, 2, 3);
#pragma unroll
      for (int i = 0; i < (TAIL ? C::NRT : 1); ++i) {
        tacc[i] += __builtin_shufflevector(aq[i], aq[i], 0, 1) * lo;
        tacc[i] += __builtin_shufflevector(aq[i], aq[i], 2, 3) * hi;
        asm volatile("" : "+v"(tacc[i]));  // keep the tail FMAs next to their MFMAs (see conv_small.h)
      }
    }
  };
  // software pipeline: weights (L2) two k-groups ahead, halo fragments (LDS) one k-group ahead
  f32x4 bq[3][NB], aq[2][RT];
  load_b(0, bq[0]);
  if (NG > 1) load_b(1, bq[1]);
  load_a(0, aq[0]);
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    if (g + 2 < NG) load_b(g + 2, bq[(g + 2) % 3]);
    if (g + 1 < NG) load_a(g + 1, aq[(g + 1) & 1]);
    mma(aq[g & 1], bq[g % 3]);
    if (g + 2 < NG) __builtin_amdgcn_sched_group_barrier(0x020, NB, 0);       // weight loads of g+2
    if (g + 1 < NG) __builtin_amdgcn_sched_group_barrier(0x100, RT, 0);       // LDS reads of g+1
    __builtin_amdgcn_sched_group_barrier(0x008, 4 * RT, 0);                  // MFMAs of g
    if (TAIL) __builtin_amdgcn_sched_group_barrier(0x002, 4 * C::NRT + 8, 0);  // tail FMAs (+ address VALU)
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- C layout (column = lane & 15, pixel = 4 * (lane >> 4) + reg of row tile i) -> LDS output tile
  float tv[TAIL ? C::NRT : 1];
  if (TAIL) {
#pragma unroll
    for (int i = 0; i < (TAIL ? C::NRT : 1); ++i) tv[i] = quarter_sum(tacc[i][0] + tacc[i][1]);  // pixel 16 i + l15
  }
  __syncthreads();  // every wave is out of the halo
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    const int px0 = 16 * (rbase + i) + 4 * lq;  // row tile i covers pixels 16 i .. 16 i + 15 of the tile
#pragma unroll
    for (int r = 0; r < 4; ++r) otile[(px0 + r) * OS + 16 * jw + l15] = acc[i][r];
  }
  if (TAIL && lq == 0) {
#pragma unroll
    for (int i = 0; i < (TAIL ? C::NRT : 1); ++i) otile[(16 * i + l15) * OS + NROWS + wv] = tv[i];
  }
  __syncthreads();

  // ---- epilogue: bias / act' + coalesced float4 stores; per-thread sums of its channel quad
  const f32x4* ot4 = reinterpret_cast<const f32x4*>(otile);
  constexpr int SQS = OS / 4;  // quads per pixel of the LDS tile
  f32x4 val[EIT];
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
#pragma unroll
  for (int it = 0; it < EIT; ++it) {
    const int px = gi + it * G;
    val[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (elane && px < CH_NPX) {
      f32x4 v = ot4[px * SQS + eq];
      const int gy = h0 + px / CH_TW, gx = w0 + px % CH_TW;
      const bool ok = gy < p.H && gx < p.W;
      if (p.ep_mode == 2) {
        const f32x4 xh = (rz[it] - epar[PQ + eq]) * epar[2 * PQ + eq];
        const f32x4 z = epar[3 * PQ + eq] * xh + epar[4 * PQ + eq];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= act_grad(z[e], p.ez_act);
        if (!ok) v = (f32x4){0.f, 0.f, 0.f, 0.f};
        s1 += v;
        s2 += v * xh;
      } else {
        v += epar[eq];
        if (ok) s1 += v;
      }
      val[it] = v;
      if (ok) *reinterpret_cast<f32x4*>(p.y + (size_t)((b * p.H + gy) * p.W + gx) * p.ldy + 4 * eq) = v;
    }
  }

  // ---- per-tile statistics rows (host: only for full tiles)
  if (p.ep_mode != 0) {
    red[tid] = s1;
    red[256 + tid] = s2;
    __syncthreads();
    f32x4* srow = reinterpret_cast<f32x4*>(p.stats + (size_t)blockIdx.x * 2 * p.ldy);
    if (p.ep_mode == 1) {
      // (mean, M2): the tile mean first, M2 around it
      f32x4 m = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < G; ++k) m += red[k * SQ + eq];
      m *= 1.f / (float)CH_NPX;
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int it = 0; it < EIT; ++it)
        if (elane && gi + it * G < CH_NPX) c += (val[it] - m) * (val[it] - m);
      red[256 + tid] = c;  // mode 1 reads only the first half above
      __syncthreads();
      if (tid < SQ) {
        f32x4 m2 = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < G; ++k) m2 += red[256 + k * SQ + tid];
        srow[tid] = m;
        srow[SQ + tid] = m2;
      }
    } else if (tid < SQ) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
      for (int k = 0; k < G; ++k) {
        a += red[k * SQ + tid];
        c += red[256 + k * SQ + tid];
      }
      srow[tid] = a;
      srow[SQ + tid] = c;
    }
  }
}

template <int CS, int TN, bool TAIL>
static int launch_halo(HaloP& p, hipStream_t st) {
  using C = HaloCfg<CS, TN, TAIL>;
  static_assert(C::LDS_BYTES * 2 <= 160 * 1024, "two workgroups per CU");
  const int rc = allow_dynamic_lds(reinterpret_cast<const void*>(&conv3x3_halo_kernel<CS, TN, TAIL>), C::LDS_BYTES);
  if (rc) return rc;
  p.tiles_x = cdiv(p.W, CH_TW);
  p.tiles_y = cdiv(p.H, CH_TM);
  hipLaunchKernelGGL((conv3x3_halo_kernel<CS, TN, TAIL>), dim3(p.B * p.tiles_x * p.tiles_y), dim3(256), C::LDS_BYTES, st, p);
  return vmtl_check_launch();
}

// ---------------------------------------------------------------------------------------------- host side
// output storage channels -> MFMA column tiles: 16 -> 1, 32 -> 2, 64 -> 4, 68 -> 4 + VALU tail columns.  The weight rows
// Nw may be up to 3 fewer (ldy = round_up(Nw, 4)): rows >= Nw read zeros, so the route depends on the shape of y alone.
static int halo_tn(int ldy) {
  return ldy == 16 ? 1 : (ldy == 32 ? 2 : (ldy == 64 || ldy == 68 ? 4 : 0));
}

// 32-bit byte offsets in the buffer loads: x under 2 GiB; the weight operand under 2^30 bytes (dead lanes rely on it)
extern "C" int vmtl_conv3x3_halo_supported(int B, int H, int W, int Cs, int ldy, int Nw) {
  if (B <= 0 || H <= 0 || W <= 0 || (Cs != 64 && Cs != 68) || halo_tn(ldy) == 0 || Nw < 1 || ((Nw + 3) & ~3) != ldy)
    return 0;
  return (long long)B * H * W * Cs * 4 <= 0x7fffffffLL;
}

// statistics rows (one per TM x 32 tile); 0 when the tiles do not cover the image exactly (statistics need equal rows)
extern "C" int vmtl_conv3x3_halo_stat_rows(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || H % CH_TM || W % CH_TW) return 0;
  return B * (H / CH_TM) * (W / CH_TW);
}

extern "C" int vmtl_conv3x3_halo_stat_block(int B, int H, int W) {
  return vmtl_conv3x3_halo_stat_rows(B, H, W) > 0 ? CH_NPX : 0;
}

extern "C" int vmtl_conv3x3_halo(const float* x, const float* pa, const float* pc, int act_in, float* a_out,
                                 const float* wp, const float* bias, float* y, float* stats, int ep_mode,
                                 const float* ez_x, const float* ez_mean, const float* ez_invstd, const float* ez_gamma,
                                 const float* ez_beta, int ez_act, int B, int H, int W, int Cs, int ldy, int Nw,
                                 int Cout, void* stream) {
  VMTL_ENTER();
  if (!x || !wp || !y || B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cout > Nw) return VMTL_ERR_ARG;
  if ((pa == nullptr) != (pc == nullptr) || (a_out != nullptr && pa == nullptr)) return VMTL_ERR_ARG;
  if (act_in != VMTL_ACT_NONE && act_in != VMTL_ACT_RELU) return VMTL_ERR_ARG;
  if (ep_mode < 0 || ep_mode > 2 || (ep_mode != 0 && !stats) || (ep_mode == 0 && stats)) return VMTL_ERR_ARG;
  if (ep_mode != 0 && vmtl_conv3x3_halo_stat_rows(B, H, W) == 0) return VMTL_ERR_ARG;  // partial tiles
  if (ep_mode == 2 && (!ez_x || !ez_mean || !ez_invstd || !ez_gamma || !ez_beta || bias)) return VMTL_ERR_ARG;
  if (!vmtl_conv3x3_halo_supported(B, H, W, Cs, ldy, Nw)) return VMTL_ERR_UNSUPPORTED;
  HaloP p;
  p.x = x; p.pa = pa; p.pc = pc; p.a_out = a_out; p.wp = wp; p.bias = bias; p.y = y; p.stats = stats;
  p.ez_x = ez_x; p.ez_mean = ez_mean; p.ez_invstd = ez_invstd; p.ez_gamma = ez_gamma; p.ez_beta = ez_beta;
  p.act_in = act_in; p.ep_mode = ep_mode; p.ez_act = ez_act;
  p.B = B; p.H = H; p.W = W; p.ldy = ldy; p.Nw = Nw; p.Cout = Cout;
  p.x_bytes = (unsigned)((long long)B * H * W * Cs * 4);
  p.wp_bytes = (unsigned)(Nw * 9 * Cs * 4);
  hipStream_t st = (hipStream_t)stream;
  const int tn = halo_tn(ldy);
  if (Cs == 68) {
    if (tn == 1) return launch_halo<68, 1, false>(p, st);
    if (tn == 2) return launch_halo<68, 2, false>(p, st);
    return ldy == 64 ? launch_halo<68, 4, false>(p, st) : launch_halo<68, 4, true>(p, st);
  }
  if (tn == 1) return launch_halo<64, 1, false>(p, st);
  if (tn == 2) return launch_halo<64, 2, false>(p, st);
  return ldy == 64 ? launch_halo<64, 4, false>(p, st) : launch_halo<64, 4, true>(p, st);
}
