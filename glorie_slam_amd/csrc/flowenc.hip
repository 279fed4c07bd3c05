// First convolution of the flow encoder (scope row A4): 7x7, zero padding 3, 4 -> 128 channels,
// + bias + ReLU  (/root/reference/src/modules/droid_net/droid_net.py:79-83).
//
// With only 4 input channels a GEMM library sees K = 196 and pads / transposes its way to 90 us
// for 10 GFLOP.  Here a kernel ROW of the stencil is one MFMA K-slice: 7 taps x 4 channels = 28
// values, padded to 8 taps = 32 -- and in a channels-last fp32 motion map [pixel][4] those 32
// values are 128 contiguous bytes.  A lane builds its v_mfma_f32_16x16x32_f16 pixel fragment with
// two 16-byte loads (2 taps x 4 channels) and a conversion; the weights are the MFMA "A" operand,
// so a lane ends up with 4 consecutive output channels of one pixel (8-byte stores).  A workgroup
// walks 16-pixel tiles; its 4 waves split the 128 output channels and keep their 32 x 224 slice of
// the weight panel in registers (a first version staged the panel in LDS and re-read it per tile:
// 56 exposed LDS round trips per tile, 60 us; this one: see profiles).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "common.hiph"

namespace glorie {

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int kFlowK = 224;       // 7 rows x (8 taps x 4 channels)

// 4 waves per workgroup; wave w owns output channels 32w .. 32w+31 of EVERY pixel tile of the
// workgroup and keeps its slice of the weight panel (2 blocks x 7 K slices = 14 fragments, 56 VGPRs)
// in registers for the whole kernel: no LDS, no barrier, occupancy limited by registers only.
__global__ __launch_bounds__(256) void flow_conv7_kernel(const float* __restrict__ flow,
                                                         const _Float16* __restrict__ wp,
                                                         const float* __restrict__ bias,
                                                         _Float16* __restrict__ out, int os, long P, int H,
                                                         int W) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int col = lane & 15, kg = lane >> 4;
  f16x8 wf[2][7];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ky = 0; ky < 7; ++ky)
      wf[mi][ky] = *reinterpret_cast<const f16x8*>(wp + (size_t)(wv * 32 + mi * 16 + col) * kFlowK + ky * 32 + kg * 8);
  float4 b[2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) b[mi] = *reinterpret_cast<const float4*>(bias + wv * 32 + mi * 16 + kg * 4);

  const int ntiles = (int)((P + 15) / 16);       // P < 2^31 (checked by the host)
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * 16 + col;
    const bool pv = p < (int)P;
    const int rowi = p / W;
    const int x = p - rowi * W, y = rowi % H;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const int x0 = x - 3 + 2 * kg;                 // this lane's two taps of every stencil row
    const bool c0 = (unsigned)x0 < (unsigned)W, c1 = (unsigned)(x0 + 1) < (unsigned)W;
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
      const int yy = y + ky - 3;
      const bool rv = pv && (unsigned)yy < (unsigned)H;
      const float* src = flow + ((long)p + (ky - 3) * W - 3 + 2 * kg) * 4;
      // unconditional loads from a clamped address + select: the loads of all 7 stencil rows can be
      // in flight together
      const bool v0 = rv && c0, v1 = rv && c1;
      const float4 f0 = *reinterpret_cast<const float4*>(v0 ? src : flow);
      const float4 f1 = *reinterpret_cast<const float4*>(v1 ? src + 4 : flow);
      // (component-wise selects: a float4 ternary is lowered to a select through scratch memory)
      const f16x8 xf = {(_Float16)(v0 ? f0.x : 0.f), (_Float16)(v0 ? f0.y : 0.f), (_Float16)(v0 ? f0.z : 0.f),
                        (_Float16)(v0 ? f0.w : 0.f), (_Float16)(v1 ? f1.x : 0.f), (_Float16)(v1 ? f1.y : 0.f),
                        (_Float16)(v1 ? f1.z : 0.f), (_Float16)(v1 ? f1.w : 0.f)};
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) acc[mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[mi][ky], xf, acc[mi], 0, 0, 0);
    }
    if (pv) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        f16x4 o;
        o[0] = (_Float16)fmaxf(acc[mi][0] + b[mi].x, 0.0f);
        o[1] = (_Float16)fmaxf(acc[mi][1] + b[mi].y, 0.0f);
        o[2] = (_Float16)fmaxf(acc[mi][2] + b[mi].z, 0.0f);
        o[3] = (_Float16)fmaxf(acc[mi][3] + b[mi].w, 0.0f);
        *reinterpret_cast<f16x4*>(out + (long)p * os + wv * 32 + mi * 16 + kg * 4) = o;
      }
    }
  }
}

// Second form (the one launched): the motion map as ZERO-PADDED fp16, [N][H+6][W+8][4] halfs (3 zero rows above and below
// every map, 3 zero pixels left and 5 right; written by glorie_motion_padded or glorie_flow_pad).  The first form is bound
// by its vector ALU and load-path work, not by the 14 MFMAs of a tile: address arithmetic, zero-padding selects and
// fp32 -> fp16 conversions of the pixel fragment, repeated by all four channel-slice waves, and 14 KB of 16-byte loads per
// wave and tile through the texture path (stand-alone ablation at 36x60x80: 15 us of ALU + MFMA, +12 loads, +20 stores).  Here
//  * a lane's two taps x 4 channels of a stencil row are 16 contiguous bytes of fp16 that ARE its MFMA B fragment: one
//    load per stencil row, no conversion, no select - the padding supplies the zeros;
//  * a wave owns 64 output channels (4 blocks x 7 K slices = 28 weight fragments, 112 VGPRs) and the wave PAIRS of a
//    workgroup walk different pixel tiles: half the redundant loads;
//  * the pixel position advances incrementally from tile to tile (no division in the loop), the loads of tiles t+1 and
//    t+2 are in flight during the MFMAs of tile t;
//  * the MFMA rows are assigned to channels so that a lane ends up with two runs of 8 consecutive channels (row i of block
//    mi is channel 32*(mi/2) + 8*(i/4) + 4*(mi%2) + i%4 of the wave's 64): two 16-byte stores per lane, the four lanes of
//    a pixel cover 64 contiguous bytes with each; the stores are unconditional buffer stores (pixels past the end are
//    dropped by the range check) so that the compiler can count them instead of waiting for vmcnt(0).
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_;
constexpr int kFlowPadY = 3, kFlowPadL = 3, kFlowPadW = 8;     // rows above/below, pixels left, extra pixels per row

__global__ __launch_bounds__(256, 2) void flow_conv7_padded_kernel(const _Float16* __restrict__ fp,
                                                                   const _Float16* __restrict__ wp,
                                                                   const float* __restrict__ bias,
                                                                   _Float16* __restrict__ out, int os, long P, int H,
                                                                   int W) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int col = lane & 15, kg = lane >> 4;
  const int ch0 = (wv & 1) * 64;
  f16x8 wf[4][7];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int ch = ch0 + (mi >> 1) * 32 + (col >> 2) * 8 + (mi & 1) * 4 + (col & 3);       // MFMA row `col` of block mi
#pragma unroll
    for (int ky = 0; ky < 7; ++ky)
      wf[mi][ky] = *reinterpret_cast<const f16x8*>(wp + (size_t)ch * kFlowK + ky * 32 + kg * 8);
  }
  float4 b[4];                                       // the lane's channels ch0 + 32*(mi/2) + 8*kg + 4*(mi%2) .. +3
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
    b[mi] = *reinterpret_cast<const float4*>(bias + ch0 + (mi >> 1) * 32 + kg * 8 + (mi & 1) * 4);

  const __amdgpu_buffer_rsrc_t rF = __builtin_amdgcn_make_buffer_rsrc((void*)fp, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, 0x7fffffff, 0x00020000);
  const int ntiles = (int)((P + 15) / 16);
  const int stride = gridDim.x * 2;
  const int WP = W + kFlowPadW, HP = H + 2 * kFlowPadY;
  // tile -> tile + stride moves the pixel by stride*16 = (dn*H + dy)*W + dx
  const int step = stride * 16;
  const int drow = step / W, dx = step - drow * W, dn = drow / H, dy = drow - dn * H;

  int tile = blockIdx.x * 2 + (wv >> 1);
  if (tile >= ntiles) return;
  int p = tile * 16 + col;
  int x, y, n;
  {
    const int pc = min(p, (int)P - 1);               // lanes past the end read (and drop) the last pixel
    const int rowi = pc / W;
    x = pc - rowi * W; n = rowi / H; y = rowi - n * H;
  }
  // byte offset of the lane's taps (x - 3 + 2kg, x - 2 + 2kg) of stencil row 0 (= map row y - 3): padded row y, pixel x + 2kg
  auto offset = [&]() { return (unsigned)((((n * HP + y) * WP) + x + 2 * kg) * 8); };
  auto issue = [&](u32x4_ (&r)[7]) {
    const unsigned off = offset();
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) r[ky] = __builtin_amdgcn_raw_buffer_load_b128(rF, off, ky * WP * 8, 0);
  };
  auto advance = [&]() {
    p += step;
    x += dx; y += dy; n += dn;
    if (x >= W) { x -= W; y += 1; }
    if (y >= H) { y -= H; n += 1; }
    if (p >= (int)P) { x = 0; y = 0; n = 0; }        // past the end: any valid address
  };
  auto finish = [&](int pp, const u32x4_ (&r)[7]) {
    f32x4 acc[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) acc[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
      const f16x8 xf = __builtin_bit_cast(f16x8, r[ky]);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) acc[mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[mi][ky], xf, acc[mi], 0, 0, 0);
    }
    f16x8 o[2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      o[mi >> 1][(mi & 1) * 4 + 0] = (_Float16)fmaxf(acc[mi][0] + b[mi].x, 0.0f);
      o[mi >> 1][(mi & 1) * 4 + 1] = (_Float16)fmaxf(acc[mi][1] + b[mi].y, 0.0f);
      o[mi >> 1][(mi & 1) * 4 + 2] = (_Float16)fmaxf(acc[mi][2] + b[mi].z, 0.0f);
      o[mi >> 1][(mi & 1) * 4 + 3] = (_Float16)fmaxf(acc[mi][3] + b[mi].w, 0.0f);
    }
    const unsigned so = pp < (int)P ? (unsigned)(((long)pp * os + ch0 + kg * 8) * 2) : 0x80000000u;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_, o[0]), rO, so, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_, o[1]), rO, so, 64, 0);
  };

  // three register sets in a ring: the taps of the next TWO tiles are in flight while this one runs its MFMAs (one tile
  // of MFMAs is ~0.25 us, a load round trip ~1 us; two waves per SIMD).  The loads past the last tile are issued too
  // (valid address, result unused): no branch, no register copies around it.
  u32x4_ r[3][7];
  int pq[3];
  pq[0] = p; issue(r[0]); advance();
  pq[1] = p; issue(r[1]); advance();
  while (true) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      constexpr int nx[3] = {2, 0, 1};
      pq[nx[k]] = p; issue(r[nx[k]]); advance();
      finish(pq[k], r[k]);
      tile += stride;
      if (tile >= ntiles) return;
    }
  }
#endif
}

// fp32 channels-last motion map [N][H][W][4] -> the zero-padded fp16 form (interior only: the borders of `padded` must be
// zero, they are never written)
__global__ __launch_bounds__(256) void flow_pad_kernel(const float4* __restrict__ flow, _Float16* __restrict__ padded,
                                                       long P, int H, int W) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const long rowi = i / W;
  const int x = (int)(i - rowi * W);
  const long n = rowi / H;
  const int y = (int)(rowi - n * H);
  const float4 f = flow[i];
  const f16x4 h = {(_Float16)f.x, (_Float16)f.y, (_Float16)f.z, (_Float16)f.w};
  *reinterpret_cast<f16x4*>(padded + (((n * (H + 2 * kFlowPadY) + y + kFlowPadY) * (W + kFlowPadW)) + x + kFlowPadL) * 4) = h;
}

// ------------------------------------------------------------------------------------------------------------------
// The whole flow encoder as one launch: relu(conv3x3(relu(conv7x7(motion) + b7)) + b3), 4 -> 128 -> 64 channels.
//
// A workgroup owns an 8 x 16 pixel tile of one map.
// Stage 1 evaluates the 7x7 layer for the tile plus a one-pixel halo (10 x 18 = 180 hidden pixels, 12 MFMA pixel blocks of
// which the last holds 4) with the arithmetic of flow_conv7_padded_kernel - same weight and pixel fragments, the seven K
// slices in the same order, same bias / ReLU / fp16 rounding - and writes the 128 channels of every hidden pixel into LDS
// instead of HBM (46 KB, [pixel][128] halfs, the 16-byte slot of a row XORed with the row's low four bits).  The 16 x 25
// pixels of the padded motion map that the tile's stencils touch are staged in LDS once (3.3 KB); a wave owns 32 hidden
// channels (14 weight fragments, loaded once per workgroup) and walks all 12 pixel blocks.  A hidden pixel OUTSIDE the map is
// the 3x3 layer's zero padding, not a value of the 7x7 layer: it is written as zeros.
// Stage 2 is the 3x3 layer of conv_igemm_kernel<EPI_BIAS_ACT, 4, 2> on that tile: a wave owns 32 output channels
// (two 16-row blocks of the paired weight layout) x 4 tile rows of 16 pixels; K runs 64-channel chunk outermost, the nine
// taps inside, the two 32-wide slices of a chunk in order, so every accumulator sees the MFMA sequence of the two-launch
// path and the output is bit-identical.  The pixel fragments are ds_read_b128 at the tap's row / column offset in the hidden
// tile.  The weights of a K step (64 rows x 64 channels, 8 KB, the same for every workgroup: L2 resident) are loaded
// ROW-contiguous - 8 lanes per 128-byte row segment, a quarter of the step per wave; a load in fragment order has every
// lane on a cache line of its own and the kernel is bound by the tag look-ups: 74 us - kFeAhead K steps ahead into
// registers, and pass through a double-buffered LDS tile that turns them into MFMA fragments: one barrier per K step.
// (Each wave staging its own 32 rows in a private buffer needs no barrier but fetches every row twice: 52.6 us against
// 49.1.)
// What it saves against the two launches: the 44 MB hidden map written to and read back from HBM, the per-tap staging of the
// pixel operand, one launch.  What it pays: the 7x7 layer is evaluated for 192 pixel slots per 128 outputs.
constexpr int kFeTH = 8, kFeTW = 16;                                  // output tile
constexpr int kFeHW = kFeTW + 2, kFeHH = kFeTH + 2;                   // hidden tile
constexpr int kFeHP = kFeHW * kFeHH;                                  // 180 hidden pixels
[[maybe_unused]] constexpr int kFeBlocks = (kFeHP + 15) / 16;                          // 12 MFMA pixel blocks
constexpr int kFeC = 128, kFeNpad = 128, kFeNout = 64;                // hidden channels, packed rows per tap, outputs
constexpr int kFePR = kFeHH + 6, kFePC = 26;                          // motion patch: 16 rows x 25 (+ 1) pixels of 4 halfs
static_assert(kFePC >= kFeHW + 7 && kFePC % 2 == 0 && kFePR * (kFePC / 2) <= 256, "one 16-byte unit of the patch per thread");
[[maybe_unused]] constexpr int kFePB = kFePR * kFePC * 8 + 128;                        // second copy: 32 banks away from the first
[[maybe_unused]] constexpr int kFeAhead = 8;                          // K steps of stage-2 weights in flight (8 VGPRs each)
[[maybe_unused]] constexpr int kFeSteps = 18;                         // 2 chunks of 64 channels x 9 taps

__global__ __launch_bounds__(256, 2) void flow_encoder_kernel(const _Float16* __restrict__ fp, unsigned fp_bytes,
                                                              const _Float16* __restrict__ w7,
                                                              const float* __restrict__ b7,
                                                              const _Float16* __restrict__ w3, unsigned w3_bytes,
                                                              const float* __restrict__ b3, _Float16* __restrict__ out,
                                                              unsigned out_bytes, int os, int H, int W, int tiles_x,
                                                              int tiles_y) {
#if defined(__HIP_DEVICE_COMPILE__)
  __shared__ __attribute__((aligned(16))) char hid[kFeHP * kFeC * 2];
  // kFePR x kFePC pixels of 8 bytes, twice: at 0 as pairs (2u, 2u + 1), at kFePB as pairs (2u + 1, 2u + 2), so that the two
  // pixels of any fragment are ONE aligned 16-byte unit (an 8-byte-aligned fragment is read as ds_read2_b64: 16 LDS cycles
  // instead of 4); + 16 bytes that the threads without a unit write
  __shared__ __attribute__((aligned(16))) char patch[kFePB + kFePR * kFePC * 8 + 128];
  __shared__ __attribute__((aligned(16))) char wbuf[2][64 * 128];        // two K steps of weights: 64 rows x 64 channels each
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int col = lane & 15, kg = lane >> 4;
  const int tx = blockIdx.x % tiles_x, trest = blockIdx.x / tiles_x;
  const int ty = trest % tiles_y, n = trest / tiles_y;
  const int y0 = ty * kFeTH, x0 = tx * kFeTW;
  const int wm = wv & 1, wn = wv >> 1;

  // the tile's patch of the padded motion map: patch row pr / pixel pc = padded row y0 - 1 + pr / pixel x0 - 1 + pc (the
  // stencil rows of hidden row hy are patch rows hy .. hy + 6, the taps of hidden column hx and lane group kg are patch
  // pixels hx + 2kg, hx + 2kg + 1).  One pass of 8-byte loads, issued ahead of the weight loads; a pixel outside the
  // padded map (only hidden pixels outside the map read those) is refused by the descriptor's range check: zeros.
  u32x2_ pv0, pv1, pv2;
  const int punit = tid < kFePR * (kFePC / 2) ? tid * 16 : kFePR * kFePC * 8;     // (the gap behind either copy)
  {
    const __amdgpu_buffer_rsrc_t rF = __builtin_amdgcn_make_buffer_rsrc((void*)fp, 0, fp_bytes, 0x00020000);
    const int WP = W + kFlowPadW, HP = H + 2 * kFlowPadY;
    const int ppr = tid / (kFePC / 2), ppu = tid - ppr * (kFePC / 2);
    const int prow = y0 - 1 + ppr, pcol = x0 - 1 + 2 * ppu;
    const bool rok = ppr < kFePR && (unsigned)prow < (unsigned)HP;
    const bool ok0 = rok && (unsigned)pcol < (unsigned)WP, ok1 = rok && (unsigned)(pcol + 1) < (unsigned)WP;
    const bool ok2 = rok && (unsigned)(pcol + 2) < (unsigned)WP;
    const int base = ((n * HP + prow) * WP + pcol) * 8;
    pv0 = __builtin_amdgcn_raw_buffer_load_b64(rF, ok0 ? (unsigned)base : 0x80000000u, 0, 0);
    pv1 = __builtin_amdgcn_raw_buffer_load_b64(rF, ok1 ? (unsigned)(base + 8) : 0x80000000u, 0, 0);
    pv2 = __builtin_amdgcn_raw_buffer_load_b64(rF, ok2 ? (unsigned)(base + 16) : 0x80000000u, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }

  // stage-1 weights: the wave's hidden channels 32 wv .. 32 wv + 31; MFMA row `col` of block mi is channel
  // 32 wv + 8 (col / 4) + 4 mi + col % 4, so that the lane ends up with the 8 consecutive channels 32 wv + 8 kg .. + 7
  f16x8 wf[2][7];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int ch = wv * 32 + (col >> 2) * 8 + mi * 4 + (col & 3);
#pragma unroll
    for (int ky = 0; ky < 7; ++ky)
      wf[mi][ky] = *reinterpret_cast<const f16x8*>(w7 + (size_t)ch * kFlowK + ky * 32 + kg * 8);
  }
  float4 b[2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) b[mi] = *reinterpret_cast<const float4*>(b7 + wv * 32 + kg * 8 + mi * 4);
  __builtin_amdgcn_sched_barrier(0);

  // stage-2 weights of K step t (chunk t / 9, tap t % 9), 64 rows x 128 bytes: the wave fetches rows 16 wv + 8 i + lane / 8
  // (i = 0, 1), 16-byte piece lane % 8.  The first kFeAhead steps are in flight during stage 1.
  const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)w3, 0, w3_bytes, 0x00020000);
  const unsigned wvoff = (unsigned)(((wv * 16 + (lane >> 3)) * kFeC) * 2 + (lane & 7) * 16);
  auto load_w = [&](int t, u32x4_ (&wr)[2]) {
    const int ch = t / 9, d = t - ch * 9;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      wr[i] = __builtin_amdgcn_raw_buffer_load_b128(rW, wvoff, ((d * kFeNpad + i * 8) * kFeC + ch * 64) * 2, 0);
  };
  constexpr int D = kFeAhead, R = kFeAhead + 1;
  u32x4_ wq[R][2];
#pragma unroll
  for (int t = 0; t < D; ++t) load_w(t, wq[t]);
  __builtin_amdgcn_sched_barrier(0);

  // ---- stage 1: the hidden tile ----
  {
    // (every thread stores - the threads past the patch write zeros behind it: no branch for the loads to sink into)
    *reinterpret_cast<u32x4_*>(patch + punit) = u32x4_{pv0[0], pv0[1], pv1[0], pv1[1]};
    *reinterpret_cast<u32x4_*>(patch + kFePB + punit) = u32x4_{pv1[0], pv1[1], pv2[0], pv2[1]};
    __syncthreads();
    // hidden pixel hp = 16 blk + col sits at map pixel (y0 - 1 + hp / 18, x0 - 1 + hp % 18)
    auto issue = [&](int blk, u32x4_ (&r)[7]) {
      const int hp = min(blk * 16 + col, kFeHP - 1), hy = hp / kFeHW, hx = hp - hy * kFeHW;
      const int q = hx + 2 * kg;                       // first of the lane's two patch pixels: copy q & 1, unit q / 2
      const u32x4_* src = reinterpret_cast<const u32x4_*>(patch) + (q & 1) * (kFePB / 16) + hy * (kFePC / 2) + (q >> 1);
#pragma unroll
      for (int ky = 0; ky < 7; ++ky) r[ky] = src[ky * (kFePC / 2)];
    };
    auto finish = [&](int blk, const u32x4_ (&r)[7]) {
      f32x4 acc[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) acc[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ky = 0; ky < 7; ++ky) {
        const f16x8 xf = __builtin_bit_cast(f16x8, r[ky]);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) acc[mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[mi][ky], xf, acc[mi], 0, 0, 0);
      }
      const int hp = blk * 16 + col, hy = hp / kFeHW, hx = hp - hy * kFeHW;
      const int y = y0 - 1 + hy, x = x0 - 1 + hx;
      const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
      f16x8 o;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        o[mi * 4 + 0] = in ? (_Float16)fmaxf(acc[mi][0] + b[mi].x, 0.0f) : (_Float16)0.0f;
        o[mi * 4 + 1] = in ? (_Float16)fmaxf(acc[mi][1] + b[mi].y, 0.0f) : (_Float16)0.0f;
        o[mi * 4 + 2] = in ? (_Float16)fmaxf(acc[mi][2] + b[mi].z, 0.0f) : (_Float16)0.0f;
        o[mi * 4 + 3] = in ? (_Float16)fmaxf(acc[mi][3] + b[mi].w, 0.0f) : (_Float16)0.0f;
      }
      if (hp < kFeHP)                                  // channels 32 wv + 8 kg .. + 7 of hidden pixel hp: slot 4 wv + kg
        *reinterpret_cast<f16x8*>(hid + hp * (kFeC * 2) + (((wv * 4 + kg) ^ (hp & 15)) << 4)) = o;
    };
    u32x4_ r[2][7];
    issue(0, r[0]);
#pragma unroll
    for (int i = 0; i < kFeBlocks; ++i) {
      if (i + 1 < kFeBlocks) issue(i + 1, r[(i + 1) & 1]);
      finish(i, r[i & 1]);
    }
  }

  // ---- stage 2: 3x3 over the hidden tile.  Wave = 32 output channels (wm) x tile rows 4 wn .. 4 wn + 3 ----
  // byte address of the lane's fragment (hidden row 4 wn + j, hidden column col + dx, logical slot kg); the slots of the
  // other K slices differ in bits 2-3 only: one XOR on the address
  unsigned abase[6][3];
#pragma unroll
  for (int j = 0; j < 6; ++j)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int row = (wn * 4 + j) * kFeHW + dx + col;
      abase[j][dx] = (unsigned)(row * (kFeC * 2) + ((kg ^ (row & 15)) << 4));
    }
  // a weight buffer: row r (of 64), 16-byte piece c (of 8) at r * 128 + ((c ^ (r & 7)) << 4) - the swizzle of
  // conv_igemm_kernel's 128-byte rows.  Written in load order (row 16 wv + 8 i + lane / 8, piece lane % 8), read as fragments
  // (row 32 wm + 16 mi + col, piece 4 kk + kg).
  const int wst = (wv * 16 + (lane >> 3)) * 128 + (((lane & 7) ^ (lane >> 3)) << 4);      // + i * 1024: the key is lane / 8
  int wfo[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) wfo[kk] = (wm * 32 + col) * 128 + (((kk * 4 + kg) ^ (col & 7)) << 4);   // + mi * 2048: key col & 7
  auto put_w = [&](int buf, const u32x4_ (&wr)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4_*>(wbuf[buf] + wst + i * 1024) = wr[i];
  };
  f32x4 acc[2][4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  put_w(0, wq[0]);
#pragma unroll
  for (int t = 0; t < kFeSteps; ++t) {
    const int ch = t / 9, d = t - ch * 9, dy = d / 3, dx = d - dy * 3;
    // one barrier per K step: buffer t & 1 (and, at t = 0, the hidden tile) is complete, and every wave has its fragments
    // of step t - 1, so buffer (t + 1) & 1 may be overwritten
    __syncthreads();
    f16x8 af[2][2], xf[2][4];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) af[kk][mi] = *reinterpret_cast<const f16x8*>(wbuf[t & 1] + wfo[kk] + mi * 2048);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        xf[kk][ni] = *reinterpret_cast<const f16x8*>(hid + (abase[ni + dy][dx] ^ (unsigned)((ch * 8 + kk * 4) << 4)));
    }
    if (t + 1 < kFeSteps) put_w((t + 1) & 1, wq[(t + 1) % R]);
    if (t + D < kFeSteps) load_w(t + D, wq[(t + D) % R]);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[kk][mi], xf[kk][ni], acc[mi][ni], 0, 0, 0);
  }

  // ---- epilogue (conv_epilogue_pair of conv.hip for one pair of blocks): rows 4kg .. 4kg+3 of blocks 0 and 1 are the 8
  // consecutive channels wm*32 + 8kg .. +7 of pixel (y0 + 4 wn + ni, x0 + col); pixels past the map edge are dropped ----
  const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, out_bytes, 0x00020000);
  const int nch = wm * 32 + 8 * kg;
  const float4 g0 = *reinterpret_cast<const float4*>(b3 + nch), g1 = *reinterpret_cast<const float4*>(b3 + nch + 4);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int y = y0 + wn * 4 + ni, x = x0 + col;
    f16x8 o;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
      const f32x4 v = acc[hb][ni];
      const float4 gg = hb ? g1 : g0;
      o[4 * hb + 0] = (_Float16)fmaxf(v[0] + gg.x, 0.0f);
      o[4 * hb + 1] = (_Float16)fmaxf(v[1] + gg.y, 0.0f);
      o[4 * hb + 2] = (_Float16)fmaxf(v[2] + gg.z, 0.0f);
      o[4 * hb + 3] = (_Float16)fmaxf(v[3] + gg.w, 0.0f);
    }
    const bool ok = y < H && x < W;
    const unsigned vo = ok ? (unsigned)(((long)((n * H + y) * W + x) * os + nch) * 2) : 0x80000000u;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_, o), rO, vo, 0, 0);
  }
#endif
}

}  // namespace glorie

using namespace glorie;

extern "C" int glorie_flow_conv7(const float* flow, const void* w_packed, const float* bias, void* out,
                                 int out_stride, int N, int H, int W, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || (out_stride & 3) || out_stride < 128) return GLORIE_EINVAL;
  if (N == 0) return GLORIE_OK;
  if (!flow || !w_packed || !bias || !out) return GLORIE_EINVAL;
  const long P = (long)N * H * W, ntiles = (P + 15) / 16;
  if (P >= 0x7fffffffL) return GLORIE_EUNSUPPORTED;
  const unsigned grid = (unsigned)(ntiles < 1024 ? ntiles : 1024);   // 4 workgroups per CU: ~10 tiles each amortise the weight load
  hipLaunchKernelGGL(flow_conv7_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, flow,
                     reinterpret_cast<const _Float16*>(w_packed), bias, reinterpret_cast<_Float16*>(out),
                     out_stride, P, H, W);
  return check_launch();
}

extern "C" int glorie_flow_pad(const float* flow, void* padded, int N, int H, int W, void* stream) {
  if (N < 0 || H <= 0 || W <= 0) return GLORIE_EINVAL;
  if (N == 0) return GLORIE_OK;
  if (!flow || !padded) return GLORIE_EINVAL;
  const long P = (long)N * H * W;
  hipLaunchKernelGGL(flow_pad_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(flow), reinterpret_cast<_Float16*>(padded), P, H, W);
  return check_launch();
}

extern "C" int glorie_flow_conv7_padded(const void* padded, const void* w_packed, const float* bias, void* out,
                                        int out_stride, int N, int H, int W, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || (out_stride & 7) || out_stride < 128) return GLORIE_EINVAL;
  if (N == 0) return GLORIE_OK;
  if (!padded || !w_packed || !bias || !out) return GLORIE_EINVAL;
  const long P = (long)N * H * W, ntiles = (P + 15) / 16;
  // 31-bit byte offsets into the padded map and the output
  if ((long)N * (H + 6) * (W + 8) * 8 >= 0x7fffffffL || P * (long)out_stride * 2 >= 0x7fffffffL) return GLORIE_EUNSUPPORTED;
  const long wgs = (ntiles + 1) / 2;
  const unsigned grid = (unsigned)(wgs < 512 ? wgs : 512);             // 2 workgroups per CU (register-limited)
  hipLaunchKernelGGL(flow_conv7_padded_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const _Float16*>(padded), reinterpret_cast<const _Float16*>(w_packed), bias,
                     reinterpret_cast<_Float16*>(out), out_stride, P, H, W);
  return check_launch();
}

extern "C" int glorie_flow_encoder(const void* padded, const void* w7_packed, const float* b7, const void* w3_packed,
                                   const float* b3, void* out, int out_stride, int N, int H, int W, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || out_stride < kFeNout) return GLORIE_EINVAL;
  if (N == 0) return GLORIE_OK;
  if (!padded || !w7_packed || !b7 || !w3_packed || !b3 || !out) return GLORIE_EINVAL;
  // 16-byte stores of 8 channels: the caller takes the two-launch path for anything else
  if ((out_stride & 7) || (reinterpret_cast<uintptr_t>(out) & 15) || (reinterpret_cast<uintptr_t>(padded) & 15) ||
      (reinterpret_cast<uintptr_t>(w3_packed) & 15) || (reinterpret_cast<uintptr_t>(w7_packed) & 15))
    return GLORIE_EUNSUPPORTED;
  const long P = (long)N * H * W;
  const long fp_bytes = (long)N * (H + 2 * kFlowPadY) * (W + kFlowPadW) * 8;
  const long out_bytes = ((P - 1) * (long)out_stride + kFeNout) * 2;
  const long tiles_x = (W + kFeTW - 1) / kFeTW, tiles_y = (H + kFeTH - 1) / kFeTH, wgs = tiles_x * tiles_y * N;
  // 31-bit byte offsets into the padded map and the output, a one-dimensional grid
  if (fp_bytes >= 0x7fffffffL || out_bytes >= 0x7fffffffL || wgs >= 0x7fffffffL) return GLORIE_EUNSUPPORTED;
  const unsigned w3_bytes = (9u * kFeNpad * kFeC + 64u) * 2u;        // pack_conv_igemm: [9][128][128] + 64 halfs
  hipLaunchKernelGGL(flow_encoder_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const _Float16*>(padded), (unsigned)fp_bytes,
                     reinterpret_cast<const _Float16*>(w7_packed), b7, reinterpret_cast<const _Float16*>(w3_packed),
                     w3_bytes, b3, reinterpret_cast<_Float16*>(out), (unsigned)out_bytes, out_stride, H, W, (int)tiles_x,
                     (int)tiles_y);
  return check_launch();
}
