// Weight gradient of the NARROW full-resolution 3x3 convs (<= 68 storage channels on both sides, stride 1, pad 1, width a
// multiple of 32): the layers where conv_wgrad_kernel is furthest from any roofline (csnet's 32 -> 16 / 16 -> 16 layers at 1 M
// pixels: 407 / 272 us at 47 / 36 TF; MTAN's 32 -> 32: 246 us; basic's 33 -> 33 / 33 -> 20: 277 / 197 us).  That kernel gathers
// im2col(x) per tap: every input pixel is fetched nine times (by up to three column-tile workgroups), 60 KB of loads per 32
// pixels for 16-36 useful channels.
//
// Here a workgroup walks DOWN a strip of 32 output columns.  Per step (one output row of the strip) it loads ONE new input row
// segment (34 pixels with the halo) and one dY row segment; the three input rows a 3x3 window needs sit in a ring of four LDS
// row slots, so x is read from memory once (+ 2 halo rows per strip segment and 2 halo columns per row).  The nine taps are
// shifted LDS views:  slab[co][tap*Cs + ci] = sum_pixels dY[p][co] * X[p + tap][ci]  with the MFMA's k = 4 consecutive pixels
// of the row (lane quarter q = pixel 4s+q), A = dY (rows co), B = X at the tap's shift (columns kk = tap*Cs + ci); the 16-wide
// kk tiles are dealt round-robin to the waves (a tile that straddles two taps just has per-lane offsets).  LDS pixels are
// [channel] rows of 48 floats, 80 on a side with more than 36 channels (both == 16 mod 32: the four quarters of a fragment read
// start 16 banks apart); the floats past Cs / ldy are zeroed once and never written again - lanes of a kk (co) tile beyond Ktot
// (ldy) read them.
// Output rows past the last whole 16-row MFMA tile (the 33rd, the 17-20th, the 65-68th channel) are NTR "tail" rows on the
// vector ALU, as in conv_wgrad_kernel: a third co tile for one row is half as many MFMAs again.
// One slab per workgroup, summed by vmtl_unpack_weights like the slabs of conv_wgrad_kernel (same [Nw][9*Cs] layout).
#include "common.h"

#define WS_SW 32       // strip width = pixels per step
#define WS_NARROW 36   // channels an LDS pixel of 48 floats holds (+ zero pad)
#define WS_MAXC 68     // ... and one of 80 floats

struct WsP {
  const float* x;   // [B][H][W][Cs]
  const float* dy;  // [B][H][W][ldy]
  float* slabs;     // [segments][Nw][9*Cs]
  int B, H, W, Cs, ldy, Nw, Ktot;
  int R;            // output rows per strip segment
  int bands, strips;
};

// NI 16-row MFMA tiles (+ NTR tail rows) of dY, JW kk tiles per wave, NW waves; LDX / LDY: LDS floats per pixel of x / dY
template <int NI, int JW, int NTR, int NW, int LDX, int LDY>
__global__ __launch_bounds__(NW * 64) void wgrad_small_kernel(WsP p) {
  constexpr int NT = NW * 64;
  constexpr int XROW = (WS_SW + 2) * LDX;  // one input row slot (with the halo columns)
  constexpr int YROW = WS_SW * LDY;
  // float4 loads per thread and row: the widest side the pixel stride holds
  constexpr int XIT = ((WS_SW + 2) * ((LDX == 48 ? WS_NARROW : WS_MAXC) / 4) + NT - 1) / NT;
  constexpr int YIT = (WS_SW * ((LDY == 48 ? WS_NARROW : WS_MAXC) / 4) + NT - 1) / NT;
  static_assert(LDX % 32 == 16 && LDY % 32 == 16, "the four quarters of a fragment read start 16 banks apart");
  static_assert((LDX == 48 ? WS_NARROW : WS_MAXC) < LDX, "a dead lane reads the zero pad float at channel Cs");
  static_assert(NI * 16 + NTR <= LDY, "every co tile (and the tail quad) lies inside a dY pixel");
  static_assert(NTR >= 0 && NTR <= 4, "the tail is one 16-byte LDS word");
  __shared__ __attribute__((aligned(16))) float Xs[4 * XROW];
  __shared__ __attribute__((aligned(16))) float Ys[2 * YROW];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wn = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;

  const int seg = blockIdx.x;
  const int band = seg % p.bands;
  const int t0 = seg / p.bands;
  const int strip = t0 % p.strips, b = t0 / p.strips;
  const int c0 = strip * WS_SW;
  const int r0 = band * p.R, r1 = min(p.H, r0 + p.R);

  // zero the whole LDS image once: the floats past Cs / ldy of every pixel stay zero (the loaders never touch them)
  for (int i = tid; i < (4 * XROW) / 4; i += NT) reinterpret_cast<f32x4*>(Xs)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < (2 * YROW) / 4; i += NT) reinterpret_cast<f32x4*>(Ys)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- loaders: per-thread constants (pixel of the segment, channel quad), the row is a scalar ----
  const int CQ = p.Cs >> 2, YQ = p.ldy >> 2;
  constexpr unsigned OOB = 0xFFFFFFFFu;
  int xoff[XIT], xlds[XIT];  // byte offset inside an image row of x (or -1), LDS float offset inside a row slot
#pragma unroll
  for (int it = 0; it < XIT; ++it) {
    const int idx = tid + it * NT;
    const int px = idx / CQ, q = idx - px * CQ;
    const int c = c0 - 1 + px;
    const bool ok = idx < (WS_SW + 2) * CQ && c >= 0 && c < p.W;
    xoff[it] = ok ? (c * p.Cs + q * 4) * 4 : -1;
    xlds[it] = idx < (WS_SW + 2) * CQ ? px * LDX + q * 4 : -1;
  }
  int yoff[YIT], ylds[YIT];
#pragma unroll
  for (int it = 0; it < YIT; ++it) {
    const int idx = tid + it * NT;
    const int px = idx / YQ, q = idx - px * YQ;
    const bool ok = idx < WS_SW * YQ;
    yoff[it] = ok ? ((c0 + px) * p.ldy + q * 4) * 4 : -1;
    ylds[it] = ok ? px * LDY + q * 4 : -1;
  }
  const __amdgpu_buffer_rsrc_t rs_x =
      buf_rsrc(p.x, (int)((unsigned)p.B * p.H * p.W * p.Cs * 4u));
  const __amdgpu_buffer_rsrc_t rs_dy =
      buf_rsrc(p.dy, (int)((unsigned)p.B * p.H * p.W * p.ldy * 4u));
  // input row rr of image b (zeros outside the image): scalar row base + thread constant
  auto load_x = [&](int rr, f32x4* rx) {
    const bool rok = rr >= 0 && rr < p.H;
    const unsigned base = (unsigned)(b * p.H + rr) * (unsigned)p.W * (unsigned)p.Cs * 4u;
#pragma unroll
    for (int it = 0; it < XIT; ++it) rx[it] = buf_load16(rs_x, (rok & (xoff[it] >= 0)) ? base + (unsigned)xoff[it] : OOB);
  };
  auto load_y = [&](int rr, f32x4* ry) {
    const bool rok = rr < r1;  // rows past the segment (or the image) contribute nothing
    const unsigned base = (unsigned)(b * p.H + rr) * (unsigned)p.W * (unsigned)p.ldy * 4u;
#pragma unroll
    for (int it = 0; it < YIT; ++it) ry[it] = buf_load16(rs_dy, (rok & (yoff[it] >= 0)) ? base + (unsigned)yoff[it] : OOB);
  };
  auto store_x = [&](int rr, const f32x4* rx) {  // row rr lives in slot (rr + 1) & 3
    float* xs = Xs + ((rr + 1) & 3) * XROW;
#pragma unroll
    for (int it = 0; it < XIT; ++it)
      if (xlds[it] >= 0) *reinterpret_cast<f32x4*>(xs + xlds[it]) = rx[it];
  };
  auto store_y = [&](int buf, const f32x4* ry) {
    float* ys = Ys + buf * YROW;
#pragma unroll
    for (int it = 0; it < YIT; ++it)
      if (ylds[it] >= 0) *reinterpret_cast<f32x4*>(ys + ylds[it]) = ry[it];
  };

  // ---- this wave's kk tiles: j = wn + NW*jw; per lane the tap shift and channel of column kk = 16*j + l15 ----
  int bdh[JW];   // tap row offset -1..1 (0 for a dead lane)
  int bcol[JW];  // float offset inside a row slot of pixel (lq + 1 + dw), channel ci - or of a zero pad for a dead lane
#pragma unroll
  for (int jw = 0; jw < JW; ++jw) {
    const int kk = (wn + NW * jw) * 16 + l15;
    if (kk < p.Ktot) {
      const int tap = kk / p.Cs, ci = kk - tap * p.Cs;
      const int th = tap / 3;
      bdh[jw] = th - 1;
      bcol[jw] = (lq + tap - 3 * th) * LDX + ci;  // 1 + dw = tap % 3
    } else {
      bdh[jw] = 0;
      bcol[jw] = lq * LDX + p.Cs;  // Cs < LDX: a zero pad float of every pixel this lane would touch
    }
  }
  const int acol = lq * LDY + l15;  // dY: pixel lq, channel l15 (+ 16 i)

  f32x4 acc[NI][JW];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int jw = 0; jw < JW; ++jw) acc[i][jw] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float tacc[NTR > 0 ? NTR : 1][JW];  // tail rows: this lane quarter's pixels only
#pragma unroll
  for (int t = 0; t < (NTR > 0 ? NTR : 1); ++t)
#pragma unroll
    for (int jw = 0; jw < JW; ++jw) tacc[t][jw] = 0.f;

  f32x4 rx[XIT], ry[YIT];
  __syncthreads();  // the zero fill is complete before the first row lands
  // prologue: rows r0-1, r0, r0+1 of x and row r0 of dY
  load_x(r0 - 1, rx);
  store_x(r0 - 1, rx);
  load_x(r0, rx);
  store_x(r0, rx);
  load_x(r0 + 1, rx);
  store_x(r0 + 1, rx);
  load_y(r0, ry);
  store_y(0, ry);
  __syncthreads();

  for (int r = r0; r < r1; ++r) {
    const int buf = (r - r0) & 1;
    const bool more = r + 1 < r1;
    if (more) {  // the next step's operands travel under this step's MFMAs
      load_x(r + 2, rx);
      load_y(r + 1, ry);
    }
    const float* ys = Ys + buf * YROW + acol;
    const float* xb[JW];
#pragma unroll
    for (int jw = 0; jw < JW; ++jw) xb[jw] = Xs + ((r + bdh[jw] + 1) & 3) * XROW + bcol[jw];
#pragma unroll
    for (int s = 0; s < WS_SW / 4; ++s) {  // pixels 4s .. 4s+3 of the row, lane quarter q = pixel 4s+q
      float fa[NI], fb[JW];
#pragma unroll
      for (int i = 0; i < NI; ++i) fa[i] = ys[4 * s * LDY + i * 16];
#pragma unroll
      for (int jw = 0; jw < JW; ++jw) fb[jw] = xb[jw][4 * s * LDX];
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int jw = 0; jw < JW; ++jw)
          acc[i][jw] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[jw], acc[i][jw], 0, 0, 0);
      if (NTR > 0) {  // dY[pixel 4s+lq][NI*16 .. +3]: one LDS read (16 bytes, 4 for a single row), broadcast within the quarter
        const float* yt = Ys + buf * YROW + (4 * s + lq) * LDY + NI * 16;
        f32x4 ty;
        if constexpr (NTR == 1) ty[0] = yt[0];
        else ty = *reinterpret_cast<const f32x4*>(yt);
#pragma unroll
        for (int t = 0; t < NTR; ++t)  // all NTR rows, branch-free: a row past Nw (a pad lane of dY) is computed and not stored
#pragma unroll
          for (int jw = 0; jw < JW; ++jw) tacc[t][jw] += ty[t] * fb[jw];
      }
    }
    if (more) {
      store_x(r + 2, rx);  // slot (r + 3) & 3 held row r - 2: dead since the previous step's barrier
      store_y(buf ^ 1, ry);
    }
    __syncthreads();
  }

  // D layout of 16x16x4: column (kk) = lane & 15, row (co) = 4 * (lane >> 4) + register
  float* slab = p.slabs + (size_t)seg * p.Nw * p.Ktot;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int jw = 0; jw < JW; ++jw) {
      const int kk = (wn + NW * jw) * 16 + l15;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = i * 16 + 4 * lq + e;
        if (co < p.Nw && kk < p.Ktot) slab[(size_t)co * p.Ktot + kk] = acc[i][jw][e];
      }
    }
  if (NTR > 0) {
#pragma unroll
    for (int t = 0; t < NTR; ++t)
#pragma unroll
      for (int jw = 0; jw < JW; ++jw) {
        const float v = quarter_sum(tacc[t][jw]);
        const int co = NI * 16 + t;
        const int kk = (wn + NW * jw) * 16 + l15;
        if (lq == 0 && co < p.Nw && kk < p.Ktot) slab[(size_t)co * p.Ktot + kk] = v;
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
static EnvInt ws_e_wide{"VMTL_WGRAD_SMALL_WIDE", 1};  // A/B aid: 0 = the routes and tiles from before the tail rows / 80-float pixels

// the layers the kernel took before its tail rows / 80-float pixels.  33..36 channels on BOTH sides (basic's last decoder conv:
// 3 co tiles for 33 rows, 24 kk tile slots for 20.25 tiles) lost to conv_wgrad_kernel and its VALU tail row without them: 274
// us there against 284-290 here
static bool ws_before_tails(int Cs, int ldy) { return Cs <= WS_NARROW && ldy <= WS_NARROW && !(Cs > 32 && ldy > 32); }

static void ws_geometry(int B, int H, int W, int Cs, int ldy, int* R, int* bands, int* strips) {
  // ~1024 workgroups (four per CU; 38 KB of LDS each; 512 / 768 / 2048 measured 1-5 % slower), at least 8 rows per segment (two
  // halo rows are loaded on top).  A side of 40-68 channels: slabs of up to 164 KB that vmtl_unpack_weights reads again, and up
  // to 62.5 KB of LDS - fewer, longer segments.  Kernel + slab sum at 256 / 512 / 768 / 1024 segments (bs 32, 64x128):
  // 67 -> 67 195 / 214 / 236 / 254 us, 16 -> 67 93 / 83 / 86 / 96 us (profiles/wgrad_strip/segments_sweep.jsonl)
  static EnvInt e_target{"VMTL_WS_TARGET", 0};  // tuning aid
  const int st = W / WS_SW;
  const int target = env_int(e_target) > 0 ? env_int(e_target) : Cs > WS_NARROW ? 256 : ldy > WS_NARROW ? 512 : 1024;
  long long nb = cdivll((long long)target, (long long)B * st);
  if (nb < 1) nb = 1;
  int rows = cdiv(H, (int)nb);
  if (rows < 8) rows = H < 8 ? H : 8;
  *R = rows;
  *bands = cdiv(H, rows);
  *strips = st;
}

// Can the kernel run this (fp32) layer: what the entry point checks.
extern "C" int vmtl_conv3x3_wgrad_small_supported(int Cs, int ldy, int W) {
  static EnvInt e{"VMTL_WGRAD_SMALL", 1};  // tuning aid: 0 = conv_wgrad_kernel everywhere
  if (env_int(e) == 0 || Cs < 4 || (Cs & 3) || ldy < 4 || (ldy & 3) || W < WS_SW || W % WS_SW) return 0;
  if (ws_before_tails(Cs, ldy)) return 1;
  return env_int(ws_e_wide) != 0 && Cs <= WS_MAXC && ldy <= WS_MAXC;
}

// Should a training step's launch of `pixels` = B*H*W output pixels come here rather than to conv_wgrad_kernel at `precision`
// (VMTL_PREC_*)?  The layers the kernel took before its tail rows / 80-float pixels: always (bf16 on conv_wgrad_kernel measured
// slower there).  The classes those added were measured against fp32 conv_wgrad_kernel only, at 262,144 pixels and more: a
// bf16 launch of them stays there (its bf16 weight gradient is 1.4-2.7x its fp32 one, this kernel 8-15 % better than that),
// and so does a launch below 65,536 pixels - 256 segments of 8 rows by 32 columns, the first size at which the wide geometry
// has a workgroup per CU (VMTL_WS_WIDE_MIN_PIXELS: tuning aid, the tests run the new classes at a few thousand pixels).
extern "C" int vmtl_conv3x3_wgrad_small_supported_p(int Cs, int ldy, int W, long long pixels, int precision) {
  static EnvInt e_min{"VMTL_WS_WIDE_MIN_PIXELS", 65536};
  if (!vmtl_conv3x3_wgrad_small_supported(Cs, ldy, W)) return 0;
  if (ws_before_tails(Cs, ldy)) return 1;
  return precision == VMTL_PREC_FP32 && pixels >= env_int(e_min);
}

// slabs the caller provides: vmtl_conv3x3_wgrad_small_slabs_for(B, H, W, Cs, ldy, Nw) * Nw * 9 * Cs floats
extern "C" int vmtl_conv3x3_wgrad_small_slabs_for(int B, int H, int W, int Cs, int ldy, int Nw) {
  if (B <= 0 || H <= 0 || W < WS_SW || W % WS_SW || Cs <= 0 || ldy <= 0 || Nw <= 0) return 0;
  int R, bands, strips;
  ws_geometry(B, H, W, Cs, ldy, &R, &bands, &strips);
  return B * strips * bands;
}

// ... of a layer with Cs, ldy <= 36
extern "C" int vmtl_conv3x3_wgrad_small_slabs(int B, int H, int W) {
  return vmtl_conv3x3_wgrad_small_slabs_for(B, H, W, WS_NARROW, WS_NARROW, WS_NARROW);
}

template <int NI, int NTR, int NW, int LDX, int LDY>
static int ws_launch(const WsP& p, int jwn, int grid, hipStream_t st) {
#define WS_CASE(J)                                                                                                       \
  case J: hipLaunchKernelGGL((wgrad_small_kernel<NI, J, NTR, NW, LDX, LDY>), dim3(grid), dim3(NW * 64), 0, st, p); break;
  if constexpr (LDX == 48) {  // Ktot <= 324: at most 21 kk tiles on four waves
    switch (jwn) {
      WS_CASE(1) WS_CASE(2) WS_CASE(3) WS_CASE(4) WS_CASE(5) WS_CASE(6)
      default: return VMTL_ERR_UNSUPPORTED;
    }
  } else {  // Ktot = 360 .. 612: 23 .. 39 kk tiles on eight waves
    switch (jwn) {
      WS_CASE(3) WS_CASE(4) WS_CASE(5)
      default: return VMTL_ERR_UNSUPPORTED;
    }
  }
#undef WS_CASE
  return vmtl_check_launch();
}

// the co tiling of Nw rows: whole 16-row MFMA tiles, and the 1-4 rows past them on the vector ALU
template <int NW, int LDX, int LDY>
static int ws_launch_rows(const WsP& p, bool tail, int jwn, int grid, hipStream_t st) {
  const int full = p.Nw >> 4, rest = p.Nw & 15;
  if constexpr (LDY == 48) {
    if (tail && rest == 1 && full == 1) return ws_launch<1, 1, NW, LDX, LDY>(p, jwn, grid, st);
    if (tail && rest == 1 && full == 2) return ws_launch<2, 1, NW, LDX, LDY>(p, jwn, grid, st);  // 18 accumulators fewer than NTR = 4
    if (tail && rest >= 2 && rest <= 4 && full == 1) return ws_launch<1, 4, NW, LDX, LDY>(p, jwn, grid, st);
    if (tail && rest >= 2 && rest <= 4 && full == 2) return ws_launch<2, 4, NW, LDX, LDY>(p, jwn, grid, st);
    switch (cdiv(p.Nw, 16)) {
      case 1: return ws_launch<1, 0, NW, LDX, LDY>(p, jwn, grid, st);
      case 2: return ws_launch<2, 0, NW, LDX, LDY>(p, jwn, grid, st);
      case 3: return ws_launch<3, 0, NW, LDX, LDY>(p, jwn, grid, st);
      default: return VMTL_ERR_UNSUPPORTED;
    }
  } else {  // ldy = 40 .. 68
    if (p.Nw > 64) return ws_launch<4, 4, NW, LDX, LDY>(p, jwn, grid, st);
    if (p.Nw > 48) return ws_launch<4, 0, NW, LDX, LDY>(p, jwn, grid, st);
    return ws_launch<3, 0, NW, LDX, LDY>(p, jwn, grid, st);
  }
}

// x [B][H][W][Cs], dy [B][H][W][ldy] (3x3, stride 1, pad 1: same extent), slabs [nslabs][Nw][9*Cs] with
// nslabs = vmtl_conv3x3_wgrad_small_slabs_for(B, H, W, Cs, ldy, Nw); vmtl_unpack_weights(..., nslabs) sums them
extern "C" int vmtl_conv3x3_wgrad_small(const float* x, const float* dy, float* slabs, int nslabs, int B, int H, int W, int Cs,
                                        int ldy, int Nw, void* stream) {
  VMTL_ENTER();
  if (!x || !dy || !slabs || B <= 0 || H <= 0 || Nw <= 0 || Nw > ldy) return VMTL_ERR_ARG;
  if (!vmtl_conv3x3_wgrad_small_supported(Cs, ldy, W)) return VMTL_ERR_UNSUPPORTED;
  if ((long long)B * H * W * Cs * 4 >= (1ll << 32) || (long long)B * H * W * ldy * 4 >= (1ll << 32)) return VMTL_ERR_UNSUPPORTED;
  WsP p;
  p.x = x; p.dy = dy; p.slabs = slabs; p.B = B; p.H = H; p.W = W; p.Cs = Cs; p.ldy = ldy; p.Nw = Nw; p.Ktot = 9 * Cs;
  ws_geometry(B, H, W, Cs, ldy, &p.R, &p.bands, &p.strips);
  const int grid = B * p.strips * p.bands;
  if (nslabs != grid) return VMTL_ERR_ARG;
  const bool tail = env_int(ws_e_wide) != 0;
  const int nj = cdiv(p.Ktot, 16);
  hipStream_t st = (hipStream_t)stream;
  if (Cs <= WS_NARROW)
    return ldy <= WS_NARROW ? ws_launch_rows<4, 48, 48>(p, tail, cdiv(nj, 4), grid, st)
                            : ws_launch_rows<4, 48, 80>(p, tail, cdiv(nj, 4), grid, st);
  return ldy <= WS_NARROW ? ws_launch_rows<8, 80, 48>(p, tail, cdiv(nj, 8), grid, st)
                          : ws_launch_rows<8, 80, 80>(p, tail, cdiv(nj, 8), grid, st);
}
