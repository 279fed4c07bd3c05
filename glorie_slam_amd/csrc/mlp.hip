// Fused neural-point decoders on the matrix cores (scope row R3) for gfx950.
//
// Replaces the chains of small nn.Linear launches of
//   MLP_geometry.forward   (reference) src/modules/conv_onet/models/decoder.py:175-225
//   MLP_color.get_feature_at_pos (per-neighbour F_theta)              decoder.py:340-389, 228-243
//   MLP_color.forward                                                 decoder.py:391-433
// with three kernels that keep every activation in registers:
//   geo  : Fourier(93, sin) -> 5 x (Linear(32) ReLU + fc_c(c)) with the skip at layer 2 -> occ
//   nb   : per neighbour [sin,cos](rel B)(20) ++ col_feat(32) -> Linear(128) softplus -> IDW sum
//          -> Linear(32).  The second layer is linear, so it is applied ONCE to the weighted
//          sum:  sum_k w_k (W2 y_k + b2) = W2 (sum_k w_k y_k) + b2 sum_k w_k   (8x fewer MACs).
//   col  : [sin,cos](p B)(40) ++ [sin,cos](v B)(40) -> 5 x (Linear(128) softplus + fc_c(c)),
//          skip at layer 2 -> sigmoid rgb
//
// Each kernel exists twice around a different MFMA core: exact fp32 on v_mfma_f32_16x16x4_f32 (mlp_*_v3; the reference
// runs fp32, no xf32 on gfx950) and the 3-term fp16 split on v_mfma_f32_16x16x32_f16 (mlp_geo_v4 / mlp_nb_v4 / mlp_col_v5,
// the product path).  Everything around the core - gathers, embeddings, activations, output layers, staging - is shared.
// All GEMMs run in the transposed form  H'^T = W^T H^T : the 16 MFMA rows are output channels (A = weights from LDS), the 16
// columns are a wave's 16 samples (B = activations).  The accumulator fragment of one layer is then
// directly the B fragment of the next (see mlp_col_v3_kernel), so no activation ever touches LDS.  The skip connection is
// two GEMMs on the split weight (embedding rows / hidden rows) - the concatenated activation is never built.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include "common.hiph"

namespace glorie {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;

template <int NT>
__device__ __forceinline__ void zero(f32x4 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ f32x4 as_f32x4(const float4 v) { return f32x4{v.x, v.y, v.z, v.w}; }

// ---- packed parameters (device pointers into one buffer, see kPackFloats below and point_ops.pack_decoders) ----
// Only what a kernel reads through a pointer is here; the layer weights travel as the LDS images / fragments.
struct GeoParams {
  const float* B;          // [3][96]   Fourier matrix (93 cols, zero padded)
  const float* bias;       // [5][32]   pts_linears biases
  const float* fcb;        // [5][32]   fc_c biases
  const float* bout;       // [4]       output bias (element 0)
};

struct NbParams {
  const float* B;          // [3][10]
  const float* W1;         // [52][128]
  const float* b1;         // [128]
  const float* W2;         // [128][32]
  const float* b2;         // [32]
};

struct ColParams {
  const float* Bp;         // [3][20]
  const float* Bv;         // [3][20]
  const float* Wout;       // [128][16] (cols 0..2 real)
  const float* bias;       // [5][128]
  const float* fcb;        // [5][128]
  const float* bout;       // [4]       output bias (rgb)
};

// ====================================================================================
// 128 samples per workgroup.  The colour weights (442 KB) are streamed through LDS in 32-row
// chunks (double buffered, shared by the waves); the geometry and per-neighbour weights are resident.
// ====================================================================================
constexpr int kTM2 = 128;

// Lane (r, g) of wave wv: MFMA column r = a sample, k-slot / accumulator row group g.  qs is the lane's sample when the
// wave's 16-sample column blocks are numbered wv * nb + b from sample q0 on (all four k-slots of a column share it),
// q the same clamped into [0, Q) for the loads of a ragged last workgroup
struct Lane { int wv, lane, r, g, qs, q; };
__device__ __forceinline__ Lane lane_of(int q0, int Q, int nb = 1, int b = 0) {
  Lane L;
  L.wv = threadIdx.x >> 6; L.lane = threadIdx.x & 63;
  L.r = L.lane & 15; L.g = L.lane >> 4;
  L.qs = q0 + (L.wv * nb + b) * 16 + L.r;
  L.q = min(L.qs, Q - 1);
  return L;
}

// torch.nn.Softplus(beta=100, threshold=20) on the bare base-2 hardware transcendentals (v_exp_f32 /
// v_log_f32, 1 ulp each), in the overflow-free form
//   softplus(x) = max(x, 0) + (ln 2 / 100) log2(1 + 2^(-100 log2(e) |x|))
// which needs no threshold branch: for 100 x > 20 the second term is log2(1 + < 2^-28) = 0 in fp32, i.e.
// exactly x like torch's threshold.  On this chip VALU work does not hide behind fp32 MFMAs of the same
// SIMD (tools/probes/mfma_valu_overlap.hip: the two add up), and expf / logf cost 3.7x these two instructions.
__device__ __forceinline__ float softplus100_fast(float x) {
#ifdef EXP_MLP_NO_SOFTPLUS
  return fmaxf(x, 0.0f);                                    // ablation (tools/exp_mlp_ablate.sh): what do the transcendentals cost?
#endif
  const float e = __builtin_amdgcn_exp2f(-144.26950408889634f * __builtin_fabsf(x));
  return fmaf(0.006931471805599453f, __builtin_amdgcn_logf(1.0f + e), fmaxf(x, 0.0f));
}
// sin / cos of 2 pi rev on v_sin_f32 / v_cos_f32 (argument in revolutions, reduced with v_fract_f32)
__device__ __forceinline__ float sin_rev(float rev) { return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(rev)); }
__device__ __forceinline__ float cos_rev(float rev) { return __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(rev)); }

// ---- 3-term fp16 split ----------------------------------------------------------------------------------------------
// The fp32 MFMA (16x16x4, 64 flops per cycle and SIMD) is the slowest matrix path of the chip; the fp16 one (16x16x32) is
// 16x faster.  Every weight and activation is split as x = hi + lo (hi = fp16(x), lo = fp16(x - hi): 22 mantissa bits) and
// a product is accumulated as hi*hi + hi*lo + lo*hi in fp32 - the dropped lo*lo term is 2^-22 relative, the fp16 products
// are exact in the fp32 accumulator - so a 32-row chunk costs 3 x 8 MFMAs of 16 cycles instead of 64 of 32.  The
// transposed formulation carries over: the accumulator blocks (2t, 2t+1) of a layer, split and packed, are the eight
// k-slots of a lane's B operand for chunk t of the next layer (slot s <-> chunk row 16 (s >> 2) + 4 g + (s & 3), the same
// row order as the fp32 chunks); the weights are packed once per chunk as A fragments
// [hi|lo][out block][lane 64][8 halfs] (point_ops.pack_decoders) and copied to LDS as they are (linear copy,
// conflict-free ds_read_b128).  Activations, biases and the output layers stay fp32 as in the exact kernels.
//
// split two accumulator blocks (channels 4g + rr of block 0 -> slots 0..3, of block 1 -> slots 4..7) into hi / lo halfs
__device__ __forceinline__ void split2(const f32x4 a, const f32x4 b, h16x8& hi, h16x8& lo) {
  const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    hi[s] = (_Float16)v[s];
#ifdef EXP_MLP_NO_SPLIT
    lo[s] = (_Float16)0.0f;                                 // ablation: the cost of forming the low halves
#else
    lo[s] = (_Float16)(v[s] - (float)hi[s]);
#endif
  }
}
// acc += A B for one A fragment pair of a split chunk (the three kept terms, in this order everywhere)
__device__ __forceinline__ f32x4 mfma_h3(const h16x8 ahi, const h16x8 alo, const h16x8 bhi, const h16x8 blo, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bhi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, blo, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bhi, acc, 0, 0, 0);
}
// Range guard of the split kernels.  The split holds |x| <= 65504 (fp16 max).  A larger operand becomes hi = inf,
// lo = x - inf = -inf, and its products a.hi * inf + a.hi * (-inf) are NaN in EVERY output channel it feeds; softplus, the
// (NaN-keeping) ReLU below, the biases, the next split and the fp32 output layers all pass a NaN on, so an overflow anywhere
// in a network surfaces as a non-finite value at its output.  The kernels therefore test only what they are about to store
// (a handful of values per lane - tracking max |x| at every split costs ~100 registers' worth of spills in the colour
// kernel) and raise the caller's flag; the host then repeats the call on the exact-fp32 MFMA kernels.  (Small magnitudes are
// safe: below 2^-3 the low half falls into fp16 subnormals and the split's error becomes ABSOLUTE, 2^-25 per operand.)
// The shared output helpers return the test's result; the exact kernels drop it.
__device__ __forceinline__ bool not_finite(float x) { return !(__builtin_fabsf(x) <= 3.0e38f); }
__device__ __forceinline__ void report_range(bool bad, int* __restrict__ range_flag) {
  if (range_flag && __builtin_amdgcn_ballot_w64(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(range_flag, 1);
}

// ---- hidden-layer activation: acc = F(acc + bias) + fc_c bias, NT 16-channel blocks of NB column blocks ----------------
__device__ __forceinline__ float relu(float x) { return fmaxf(x, 0.0f); }
__device__ __forceinline__ float relu_keep_nan(float x) { return x < 0.0f ? 0.0f : x; }

template <float (*F)(float), int NT, int NB>
__device__ __forceinline__ void act_layer(f32x4 (*acc)[NT], const float* bias, const float* fcb, int li, int g) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float4 bb = *reinterpret_cast<const float4*>(bias + li * (16 * NT) + 16 * t + 4 * g);
    const float4 fb = *reinterpret_cast<const float4*>(fcb + li * (16 * NT) + 16 * t + 4 * g);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      acc[nb][t][0] = F(acc[nb][t][0] + bb.x) + fb.x;
      acc[nb][t][1] = F(acc[nb][t][1] + bb.y) + fb.y;
      acc[nb][t][2] = F(acc[nb][t][2] + bb.z) + fb.z;
      acc[nb][t][3] = F(acc[nb][t][3] + bb.w) + fb.w;
    }
  }
}

// ====================================================================================
// geometry decoder
// ====================================================================================
// Exact kernel: all weights of the network (480 K-rows of 32 outputs, 61 KB, + the 32 x 16 output layer) are staged once
// per workgroup as the LDS image built by point_ops.pack_decoders: row k holds output 16 to + r at 2 r + to, so
// one ds_read_b64 per lane fetches the A operands of the two 16-channel output blocks.  Embedding (96, sin),
// feature c (32) and hidden state (32) live in registers as B fragments; no barrier after the staging.
// Split kernel: the 480 K-rows are 15 chunks of 32, packed as A fragments [chunk][hi|lo][out block 2][lane 64][8 halfs]
// (1024 floats per chunk), staged once per workgroup and followed by the same fp32 output layer.
constexpr int kGeoRows = 480;
constexpr int kGeoOut = 32 * 16;                     // the 32 -> 1 output layer, 16 padded columns, natural order
constexpr int kGeoImage = kGeoRows * 32 + kGeoOut;   // floats
constexpr int kGeoFrag = 15 * 1024;                  // floats

// one 16-feature block t of the embedding as a B fragment: sin of the phases of channels 16t + 4g + rr.  Columns 93..95 of
// B are zero padding (sin 0 = 0) and so are the matching weight rows
__device__ __forceinline__ f32x4 geo_embed_block(float x, float y, float z, const float* __restrict__ B, int t, int g) {
  const float4 b0 = *reinterpret_cast<const float4*>(B + 16 * t + 4 * g);
  const float4 b1 = *reinterpret_cast<const float4*>(B + 96 + 16 * t + 4 * g);
  const float4 b2 = *reinterpret_cast<const float4*>(B + 192 + 16 * t + 4 * g);
  f32x4 e;
  e[0] = sin_rev(fmaf(z, b2.x, fmaf(y, b1.x, x * b0.x)));
  e[1] = sin_rev(fmaf(z, b2.y, fmaf(y, b1.y, x * b0.y)));
  e[2] = sin_rev(fmaf(z, b2.z, fmaf(y, b1.z, x * b0.z)));
  e[3] = sin_rev(fmaf(z, b2.w, fmaf(y, b1.w, x * b0.w)));
  return e;
}

#ifndef GLORIE_GEO_NB
#define GLORIE_GEO_NB 2
#endif
// The geometry feature c of sample q as two B fragments (channels 16t + 4g + rr): read from c_geo, or - geo_feats given -
// the IDW interpolation of the neighbours' features right here (decoder.py:130-173; same summation order as
// idw_gather_kernel), so that the loads travel with the weights and c_geo never exists in HBM.  NBR_ID(k) / NBR_W(k) yield
// neighbour k's row (clamped to >= 0) and weight - loaded at this point or long before, the kernel's choice; PREFETCH is
// placed behind the first gathers, where the split kernel requests its next block's ids.
// The rows of GEO_NB neighbours are requested together and unconditionally (zero-weight rows dropped by a select - the same
// bits): a load under `if (wk != 0)` is one exposed L2 round trip per neighbour at the head of every workgroup.
// A macro, because mlp_geo_v3_kernel lives at 124 of the 128 registers that four waves per SIMD have: with this text in a
// forced-inline function (ids and weights by pointer or by lambda alike) the compiler orders the same operations into 30
// spilled registers, and pinning the embedding in front of the call instead (106 registers, no spill) takes its loads out of
// the gather's shadow: 0.241 against 0.200 ms per 614,400 samples.
#define GLORIE_IDW_FEATURE(c, c_geo, geo_feats, q, g, on, NBR_ID, NBR_W, PREFETCH)                                      \
  if (geo_feats) {                                                                                                      \
    zero<2>(c);                                                                                                         \
    constexpr int GEO_NB = GLORIE_GEO_NB;                                                                               \
    _Pragma("unroll") for (int k0 = 0; k0 < 8; k0 += GEO_NB) {                                                          \
      float wk[GEO_NB];                                                                                                 \
      float4 v[GEO_NB][2];                                                                                              \
      _Pragma("unroll") for (int k = 0; k < GEO_NB; ++k) {                                                              \
        wk[k] = NBR_W(k0 + k);                                                                                          \
        const auto ik = NBR_ID(k0 + k);                                                                                 \
        _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                                   \
          v[k][t] = *reinterpret_cast<const float4*>(geo_feats + (size_t)ik * 32 + 16 * t + 4 * g);                     \
      }                                                                                                                 \
      if (k0 == 0) { PREFETCH; }                                                                                        \
      _Pragma("unroll") for (int k = 0; k < GEO_NB; ++k) {                                                              \
        const bool use = on && wk[k] != 0.0f;                                                                           \
        _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                                                 \
          c[t][0] = use ? c[t][0] + wk[k] * v[k][t].x : c[t][0];                                                        \
          c[t][1] = use ? c[t][1] + wk[k] * v[k][t].y : c[t][1];                                                        \
          c[t][2] = use ? c[t][2] + wk[k] * v[k][t].z : c[t][2];                                                        \
          c[t][3] = use ? c[t][3] + wk[k] * v[k][t].w : c[t][3];                                                        \
        }                                                                                                               \
      }                                                                                                                 \
    }                                                                                                                   \
  } else {                                                                                                              \
    PREFETCH;                                                                                                           \
    _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                                       \
      c[t] = as_f32x4(*reinterpret_cast<const float4*>(c_geo + (size_t)q * 32 + 16 * t + 4 * g));                       \
  }

// output layer 32 -> 1 in fp32 (Wout: [32][16] in LDS): lanes with g == 0 get channel 0 of their sample in o[0] and store
// the occupancy, -100 where the sample has no neighbour (Renderer.py:206-207).  Returns the range test of what was stored
__device__ __forceinline__ bool geo_output(const f32x4 (&acc)[2], const float* Wout, const float* __restrict__ bout,
                                           const Lane& L, int Q, bool on, float* __restrict__ raw) {
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* wp = Wout + (4 * L.g) * 16 + L.r;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[(16 * t + rr) * 16], acc[t][rr], o, 0, 0, 0);
  if (L.g != 0 || L.qs >= Q) return false;
  raw[(size_t)L.qs * 4 + 3] = on ? o[0] + bout[0] : -100.0f;
  return on && not_finite(o[0]);
}

template <int NT, int NB>
__device__ __forceinline__ void mma_geo(f32x4 (&acc)[2], const f32x4 (&b)[NB], const float* Wrows) {
  const int lane = threadIdx.x & 63;
  const float* wp = Wrows + (lane >> 4) * 4 * 32 + (lane & 15) * 2;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const float2 w = *reinterpret_cast<const float2*>(wp + (16 * t + rr) * 32);
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, b[t][rr], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, b[t][rr], acc[1], 0, 0, 0);
    }
}

__global__ __launch_bounds__(512, 4) void mlp_geo_v3_kernel(GeoParams P, const float* __restrict__ image,
                                                            const float* __restrict__ pts,
                                                            const float* __restrict__ c_geo,
                                                            const float* __restrict__ geo_feats,
                                                            const int64_t* __restrict__ I,
                                                            const float* __restrict__ wts,
                                                            const uint8_t* __restrict__ has, int Q,
                                                            float* __restrict__ raw) {
  extern __shared__ float smem[];
  const Lane L = lane_of(blockIdx.x * kTM2, Q);
  const int g = L.g;
  const size_t q = L.q;
  for (int idx = threadIdx.x; idx < kGeoImage / 4; idx += 512)
    reinterpret_cast<float4*>(smem)[idx] = reinterpret_cast<const float4*>(image)[idx];
  // B fragments: channel 16t + 4g + rr of sample r
  f32x4 e[6], c[2], h[2], acc[2];
  const float x = pts[q * 3 + 0], y = pts[q * 3 + 1], z = pts[q * 3 + 2];
#pragma unroll
  for (int t = 0; t < 6; ++t) e[t] = geo_embed_block(x, y, z, P.B, t, g);
  const bool on = has[q] != 0;
#define V3_NBR_ID(k) max(I[q * 8 + (k)], 0L)
#define V3_NBR_W(k) wts[q * 8 + (k)]
  GLORIE_IDW_FEATURE(c, c_geo, geo_feats, q, g, on, V3_NBR_ID, V3_NBR_W, )
#undef V3_NBR_W
#undef V3_NBR_ID
  __syncthreads();
  auto act = [&](int li) { act_layer<relu, 2, 1>(&acc, P.bias, P.fcb, li, g); };
  auto next_layer = [&]() {
#pragma unroll
    for (int t = 0; t < 2; ++t) { h[t] = acc[t]; acc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  };
  const float* W = smem;   // row offsets: W0 0 | Fc0 96 | W1 128 | Fc1 160 | W2 192 | Fc2 224 | W3e 256 | W3h 352
                           //              | Fc3 384 | W4 416 | Fc4 448 | Wout 480 (16 columns, natural order)
  zero<2>(acc);
  mma_geo<6, 6>(acc, e, W);               act(0); mma_geo<2, 2>(acc, c, W + 96 * 32);
  next_layer();
  mma_geo<2, 2>(acc, h, W + 128 * 32);    act(1); mma_geo<2, 2>(acc, c, W + 160 * 32);
  next_layer();
  mma_geo<2, 2>(acc, h, W + 192 * 32);    act(2); mma_geo<2, 2>(acc, c, W + 224 * 32);
  next_layer();
  mma_geo<6, 6>(acc, e, W + 256 * 32);
  mma_geo<2, 2>(acc, h, W + 352 * 32);    act(3); mma_geo<2, 2>(acc, c, W + 384 * 32);
  next_layer();
  mma_geo<2, 2>(acc, h, W + 416 * 32);    act(4); mma_geo<2, 2>(acc, c, W + 448 * 32);
  geo_output(acc, W + kGeoRows * 32, P.bout, L, Q, on, raw);
}

__device__ __forceinline__ void mma_g3(f32x4 (&acc)[2], const h16x8 bhi, const h16x8 blo, const float* chunk) {
  const h16x8* wp = reinterpret_cast<const h16x8*>(chunk) + (threadIdx.x & 63);
#pragma unroll
  for (int to = 0; to < 2; ++to) acc[to] = mfma_h3(wp[to * 64], wp[(2 + to) * 64], bhi, blo, acc[to]);
  __builtin_amdgcn_sched_barrier(0);
}

// The 96-channel embedding is evaluated where it is consumed (layer 0 and again at the skip layer) instead of being kept:
// 24 v_sin per sample against 24 registers that the 128-register budget of four waves per SIMD does not have.
// GO (gather only): the measurement instantiation behind stage_flags bit 2 of glorie_render_mlp - the kernel's R2 phase
// alone (ids, weights, the 8 feature rows and their interpolation) with the decoder removed, so that bench.py can time the
// feature pull AS THE PRODUCT PERFORMS IT (inside this kernel, not in a stand-alone gather launch) in its own process.
template <bool GO>
__global__ __launch_bounds__(512, 4) void mlp_geo_v4_kernel(GeoParams P, const float* __restrict__ frags,
                                                            const float* __restrict__ wout,
                                                            const float* __restrict__ pts,
                                                            const float* __restrict__ c_geo,
                                                            const float* __restrict__ geo_feats,
                                                            const int64_t* __restrict__ I,
                                                            const float* __restrict__ wts,
                                                            const uint8_t* __restrict__ has, int Q,
                                                            float* __restrict__ raw, int* __restrict__ range_flag) {
  bool bad = false;
  extern __shared__ float smem[];              // [15][1024] fragments | [32][16] output layer
  const int tid = threadIdx.x;
  if constexpr (!GO) {                        // (the weights are no part of the feature pull)
#pragma unroll 2
    for (int idx = tid; idx < kGeoFrag / 4; idx += 512)
      reinterpret_cast<float4*>(smem)[idx] = reinterpret_cast<const float4*>(frags)[idx];
    if (tid < kGeoOut / 4) reinterpret_cast<float4*>(smem + kGeoFrag)[tid] = reinterpret_cast<const float4*>(wout)[tid];
  }
  __syncthreads();
  // persistent over the sample blocks: the 61 KB of fragments are staged once per workgroup (a launch used to stage them
  // for every 128 samples, 4800 times per 614k-sample batch, with the first MFMA of a workgroup waiting behind it)
  const int nblk = (Q + kTM2 - 1) / kTM2;
  // per-sample inputs of a block: position, neighbour ids, IDW weights.  They are requested one block AHEAD, so a block's
  // feature gather (which needs the ids) starts at once instead of behind a second dependent memory round trip
  struct Meta { float x, y, z; int id[8]; float wk[8]; bool on; };
  auto load_meta = [&](int blk, Meta& m) {
    const size_t qq = lane_of(blk * kTM2, Q).q;
    m.x = pts[qq * 3 + 0]; m.y = pts[qq * 3 + 1]; m.z = pts[qq * 3 + 2];
    m.on = has[qq] != 0;
    if (geo_feats) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        m.id[k] = (int)max(I[qq * 8 + k], 0L);
        m.wk[k] = wts[qq * 8 + k];
      }
    }
  };
  Meta cur;
  if ((int)blockIdx.x < nblk) load_meta(blockIdx.x, cur);
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const Lane L = lane_of(blk * kTM2, Q);
    const int g = L.g;
    h16x8 chi, clo, hhi, hlo;
    f32x4 acc[2];
    const float x = cur.x, y = cur.y, z = cur.z;
    const bool on = cur.on;
    Meta nxt = cur;
    {
      f32x4 c[2];
#define V4_NBR_ID(k) cur.id[k]
#define V4_NBR_W(k) cur.wk[k]
      GLORIE_IDW_FEATURE(c, c_geo, geo_feats, L.q, g, on, V4_NBR_ID, V4_NBR_W,
                         if (blk + (int)gridDim.x < nblk) load_meta(blk + gridDim.x, nxt))
#undef V4_NBR_W
#undef V4_NBR_ID
      split2(c[0], c[1], chi, clo);
      if constexpr (GO) {
        // the interpolated feature's sum stands in for the occupancy
        if (g == 0 && L.qs < Q) raw[(size_t)L.qs * 4 + 3] = (c[0][0] + c[0][1]) + (c[1][2] + c[1][3]);
        cur = nxt;
        continue;
      }
    }
    auto act = [&](int li) { act_layer<relu_keep_nan, 2, 1>(&acc, P.bias, P.fcb, li, g); };
    auto next_layer = [&]() {
      split2(acc[0], acc[1], hhi, hlo);
      zero<2>(acc);
    };
    auto ch = [&](int c) { return smem + c * 1024; };
    // embedding blocks (2cc, 2cc + 1) -> chunk `chunk`: evaluated, split, multiplied, forgotten
    auto embed = [&](int cc, int chunk) {
      h16x8 ehi, elo;
      split2(geo_embed_block(x, y, z, P.B, 2 * cc, g), geo_embed_block(x, y, z, P.B, 2 * cc + 1, g), ehi, elo);
      mma_g3(acc, ehi, elo, ch(chunk));
    };
    // chunks: W0 0-2 | Fc0 3 | W1 4 | Fc1 5 | W2 6 | Fc2 7 | W3e 8-10 | W3h 11 | Fc3 12 | W4 13 | Fc4 14
    zero<2>(acc);
    embed(0, 0); embed(1, 1); embed(2, 2);
    act(0); mma_g3(acc, chi, clo, ch(3));
    next_layer();
    mma_g3(acc, hhi, hlo, ch(4));  act(1); mma_g3(acc, chi, clo, ch(5));
    next_layer();
    mma_g3(acc, hhi, hlo, ch(6));  act(2); mma_g3(acc, chi, clo, ch(7));
    next_layer();
    embed(0, 8); embed(1, 9); embed(2, 10);
    mma_g3(acc, hhi, hlo, ch(11)); act(3); mma_g3(acc, chi, clo, ch(12));
    next_layer();
    mma_g3(acc, hhi, hlo, ch(13)); act(4); mma_g3(acc, chi, clo, ch(14));
    bad = bad | geo_output(acc, smem + kGeoFrag, P.bout, L, Q, on, raw);
    cur = nxt;
  }
  report_range(bad, range_flag);
}

// ====================================================================================
// colour decoder
// ====================================================================================
// Every layer is evaluated as  H'^T = W^T . H^T : the MFMA's 16 "rows" are output channels (A = weights
// from the LDS chunk), its 16 "columns" are the wave's 16 samples (B = activations).  The D fragment
// of lane (r = lane & 15, g = lane >> 4) then holds channels 16t + 4g + rr (t = 0..7, rr = 0..3) of
// sample r - and the B operand of the next layer wants, for k-slot g, *some* channel of sample r.  The
// order in which the reduction runs over channels is free, so k-step (t, rr) simply takes channel
// 16t + 4g + rr from slot g: the accumulator registers of one layer are the B operands of the next,
// no transposition through LDS, no activation buffer at all.  The embedding and the colour feature
// use the same channel -> (step, slot) assignment.  LDS only holds the double-buffered weight chunk
// (33 KB), so two workgroups share a CU and one's barriers hide behind the other's MFMAs.

// The 80-feature embedding [sin p | cos p | sin v | cos v] x 20 of sample q (view direction normalised) as the five B
// fragments of channels 16t + 4g + rr.  Phases in revolutions: the 2 pi of the reference's embedding is the period of
// v_sin / v_cos.  (Bp / Bv as pointers: read through a reference to ColParams, the matrix loads of a wave's two sample
// blocks are not merged - 112 loads against 76 in mlp_col_v5_kernel, and a measurable 1 %)
__device__ __forceinline__ void col_embed(f32x4 (&e)[5], const float* Bp, const float* Bv, const float* __restrict__ pts,
                                          const float* __restrict__ views, size_t q, int g) {
  const float px = pts[q * 3 + 0], py = pts[q * 3 + 1], pz = pts[q * 3 + 2];
  float vx = views[q * 3 + 0], vy = views[q * 3 + 1], vz = views[q * 3 + 2];
  const float nrm = fmaxf(sqrtf(vx * vx + vy * vy + vz * vz), 1e-12f);
  vx = vx / nrm; vy = vy / nrm; vz = vz / nrm;
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int f = 16 * t + 4 * g + rr;   // feature index 0..79
      const int blk = f / 20, ff = f - blk * 20;
      const float* Bm = blk < 2 ? Bp : Bv;
      const float x = blk < 2 ? px : vx, y = blk < 2 ? py : vy, z = blk < 2 ? pz : vz;
      const float a = fmaf(z, Bm[40 + ff], fmaf(y, Bm[20 + ff], x * Bm[ff]));
      e[t][rr] = (blk & 1) ? cos_rev(a) : sin_rev(a);
    }
}

// output layer 128 -> 3 in fp32 (A straight from global: Wout is [128][16], 3 real columns) and the sigmoid; lanes with
// g == 0 end up with channels 0..3 of their sample.  Returns the range test of the layer's outputs
__device__ __forceinline__ bool col_output(const f32x4 (&acc)[8], const ColParams& P, const Lane& L, int Q,
                                           float* __restrict__ raw) {
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* wp = P.Wout + (4 * L.g) * 16 + L.r;
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[(16 * t + rr) * 16], acc[t][rr], o, 0, 0, 0);
  bool bad = false;
  if (L.g == 0 && L.qs < Q) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      bad = bad | not_finite(o[ch]);
      raw[(size_t)L.qs * 4 + ch] = 1.0f / (1.0f + __expf(-(o[ch] + P.bout[ch])));
    }
  }
  return bad;
}

// The colour weights as the kernels stream them: 27 chunks of 32 K-rows,
//   W0 (80 -> 96 rows) Fc0 | W1 Fc1 | W2 Fc2 | W3e (80 -> 96) W3h Fc3 | W4 Fc4.
// CHUNK(i, operand, b): chunk i multiplies block b of the embedding (E), the hidden state (H) or the colour feature (C);
// ACT(l): the activation of layer l, due once its pts_linears chunks are in; NEXT: the accumulators become the hidden state.
// Layer 3 is the skip: W3e on the embedding, W3h on the hidden state.
constexpr int kColChunks = 27;
#define GLORIE_COL_SCHEDULE(CHUNK, ACT, NEXT)                                                                   \
  CHUNK(0, E, 0) CHUNK(1, E, 1) CHUNK(2, E, 2) ACT(0) CHUNK(3, C, 0) NEXT                                       \
  CHUNK(4, H, 0) CHUNK(5, H, 1) CHUNK(6, H, 2) CHUNK(7, H, 3) ACT(1) CHUNK(8, C, 0) NEXT                        \
  CHUNK(9, H, 0) CHUNK(10, H, 1) CHUNK(11, H, 2) CHUNK(12, H, 3) ACT(2) CHUNK(13, C, 0) NEXT                    \
  CHUNK(14, E, 0) CHUNK(15, E, 1) CHUNK(16, E, 2)                                                               \
  CHUNK(17, H, 0) CHUNK(18, H, 1) CHUNK(19, H, 2) CHUNK(20, H, 3) ACT(3) CHUNK(21, C, 0) NEXT                   \
  CHUNK(22, H, 0) CHUNK(23, H, 1) CHUNK(24, H, 2) CHUNK(25, H, 3) ACT(4) CHUNK(26, C, 0)

// one step of the double-buffered stream: chunk cidx + 1 travels L2 -> registers while chunk cidx is multiplied out of LDS
// buffer cidx & 1, and lands in the other buffer before the barrier.  (A macro, not a function taking three lambdas: the
// registers that carry the next chunk stay in memory when they are captured.)
#define GLORIE_COL_CHUNK_STEP(cidx, LOAD_NEXT, MMA, STORE_NEXT) \
  {                                                             \
    if ((cidx) + 1 < kColChunks) { LOAD_NEXT; }                 \
    MMA;                                                        \
    if ((cidx) + 1 < kColChunks) { STORE_NEXT; }                \
    __syncthreads();                                            \
  }

// ---- exact fp32: chunks of [32][128] floats, LDS rows padded to 132 ------------------------------------------------
constexpr int kLdw3 = 132;                  // chunk row stride in LDS (floats)
constexpr int kChunkFloats3 = 32 * kLdw3;

struct ChunkRegs { float4 a, b; };
// thread t of 512 moves 8 floats: row = t >> 4 (0..31), cols (t & 15) * 8 .. + 7
__device__ __forceinline__ ChunkRegs chunk_load(const float* __restrict__ Wall, int chunk) {
  const int t = threadIdx.x;
  const float4* src = reinterpret_cast<const float4*>(Wall + ((size_t)chunk * 32 + (t >> 4)) * 128 + (t & 15) * 8);
  ChunkRegs r;
  r.a = src[0];
  r.b = src[1];
  return r;
}
__device__ __forceinline__ void chunk_store3(float* Wb, const ChunkRegs& r) {
  const int t = threadIdx.x;
  float4* dst = reinterpret_cast<float4*>(Wb + (t >> 4) * kLdw3 + (t & 15) * 8);
  dst[0] = r.a;
  dst[1] = r.b;
}

// one k-step of the 128-output fp32 layers: the eight A operands are two 16-byte reads (w0, w1) of a permuted row
__device__ __forceinline__ void mfma_step8(f32x4 (&acc)[8], const float4 w0, const float4 w1, float bv) {
  acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.x, bv, acc[0], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.y, bv, acc[1], 0, 0, 0);
  acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.z, bv, acc[2], 0, 0, 0);
  acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.w, bv, acc[3], 0, 0, 0);
  acc[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.x, bv, acc[4], 0, 0, 0);
  acc[5] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.y, bv, acc[5], 0, 0, 0);
  acc[6] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.z, bv, acc[6], 0, 0, 0);
  acc[7] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.w, bv, acc[7], 0, 0, 0);
}

// acc[to] += W[16 tt + 4g + rr][16 to + r] * b[T0 + tt][rr]  for tt < NT, rr < 4 (rows relative to the chunk).
// The columns of a chunk row are stored permuted - column 16 to + r at (to >> 2) * 64 + 4 r + (to & 3) - so
// the eight A operands of a k-step are two ds_read_b128 (16 lanes read 256 contiguous bytes).
template <int T0, int NT, int NB>
__device__ __forceinline__ void mma_t(f32x4 (&acc)[8], const f32x4 (&b)[NB], const float* Wb) {
  const int lane = threadIdx.x & 63;
  const float* wp = Wb + (lane >> 4) * 4 * kLdw3 + (lane & 15) * 4;
#pragma unroll
  for (int tt = 0; tt < NT; ++tt)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      mfma_step8(acc, *reinterpret_cast<const float4*>(wp + (16 * tt + rr) * kLdw3),
                 *reinterpret_cast<const float4*>(wp + (16 * tt + rr) * kLdw3 + 64), b[T0 + tt][rr]);
}

__global__ __launch_bounds__(512, 4) void mlp_col_v3_kernel(ColParams P, const float* __restrict__ Wall,
                                                            const float* __restrict__ pts,
                                                            const float* __restrict__ views,
                                                            const float* __restrict__ c_col, int Q,
                                                            float* __restrict__ raw) {
  extern __shared__ float smem[];
  float* Wbuf = smem;                         // [2][32][132]
  const Lane L = lane_of(blockIdx.x * kTM2, Q);
  const int g = L.g;

  // ---- B fragments: the embedding e (80 channels) stays in registers; the colour feature c (32
  // channels) is re-read from L2 before each of its five uses (8 registers short of 4 waves / SIMD)
  f32x4 e[5], c[2];
  auto load_c = [&]() {
    int q = L.q;
    asm volatile("" : "+v"(q));   // a READ each time: the compiler may not keep the eight values (or the row address) instead
#pragma unroll
    for (int t = 0; t < 2; ++t) c[t] = as_f32x4(*reinterpret_cast<const float4*>(c_col + (size_t)q * 32 + 16 * t + 4 * g));
  };
  col_embed(e, P.Bp, P.Bv, pts, views, L.q, g);
  // evaluated HERE, before the first chunk is requested: four waves per SIMD have 128 registers, and an embedding that the
  // compiler interleaves with the chunk copy (60 values of Bp / Bv in flight) spills 6-10 of them (114 with both asm lines)
#pragma unroll
  for (int t = 0; t < 5; ++t) asm volatile("" : "+v"(e[t]));

  f32x4 acc[8], h[8];
  ChunkRegs nxt = chunk_load(Wall, 0);
  chunk_store3(Wbuf, nxt);
  __syncthreads();

  // E / H blocks b are k-step blocks 2b, 2b + 1 (the 80-channel embedding ends with block 4)
#define V3_MMA_E(b, Wb) mma_t<2 * (b), (b) == 2 ? 1 : 2, 5>(acc, e, Wb)
#define V3_MMA_H(b, Wb) mma_t<2 * (b), 2, 8>(acc, h, Wb)
#define V3_MMA_C(b, Wb) mma_t<0, 2, 2>(acc, c, Wb)
#define V3_CHUNK(cidx, OP, b)                                                                                   \
  GLORIE_COL_CHUNK_STEP(cidx, nxt = chunk_load(Wall, (cidx) + 1), V3_MMA_##OP(b, Wbuf + ((cidx) & 1) * kChunkFloats3), \
                        chunk_store3(Wbuf + (((cidx) + 1) & 1) * kChunkFloats3, nxt))
#define V3_ACT(li) load_c(); act_layer<softplus100_fast, 8, 1>(&acc, P.bias, P.fcb, li, g);
#define V3_NEXT                                                                                       \
  _Pragma("unroll") for (int t = 0; t < 8; ++t) { h[t] = acc[t]; acc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  zero<8>(acc);
  GLORIE_COL_SCHEDULE(V3_CHUNK, V3_ACT, V3_NEXT)
#undef V3_NEXT
#undef V3_ACT
#undef V3_CHUNK
#undef V3_MMA_C
#undef V3_MMA_H
#undef V3_MMA_E
  col_output(acc, P, L, Q, raw);
}

// ---- 3-term split: chunks of 4096 floats = [hi|lo][out block 8][lane 64][8 halfs], NB column blocks per wave ----------
// Round 2's colour kernel (removed in round 4) gave a wave 16 samples: every A fragment (weights) read from LDS feeds 3
// MFMAs, and the 442 KB weight stream is re-staged for every 128 samples - LDS reads (1 KB per 3 x 16 MFMA cycles and wave:
// 1024 LDS cycles against 768 matrix cycles per chunk and CU) and the L2 -> LDS stream (2.1 GB per 614k-sample batch) bound
// it, not the matrix pipe (MfmaUtil 41 %).  Here a wave owns NB = 2 blocks of 16 samples: an A fragment feeds 6 MFMAs, a
// workgroup of WAVES waves covers 32 WAVES samples per staged chunk, and the second block's vector work (softplus, splits)
// overlaps the first one's MFMAs inside the same wave.  Same packed weights, same arithmetic per sample (bit-identical
// results to that kernel).  Launched as <2, 4>: measured per 614k-sample batch against 16 samples per wave and against
// 8-wave workgroups, 427 vs 495 / 485 us (the other two forms were removed in round 4).
//
// Round 6, measured and not kept: three waves per SIMD instead of two (236 -> 168 registers: the embedding formed where it is
// consumed, the colour feature re-read before each use, the weight chunk L2 -> LDS by DMA instead of through 16 VGPRs, layer 3
// with its hidden chunks first) - 0.858-0.860 ms for the three decoder kernels against 0.838-0.853 ms, frame 5.49 / 5.63 against
// 5.47 / 5.61 ms in interleaved runs (tools/time_mlp.py): like every occupancy change tried on these kernels, no gain.  (The
// first build also failed the fixture test - a wrong chunk order in the re-ordered layer - and was not debugged further.)
constexpr int kChunkFloats16 = 4096;          // 2 x 8 x 64 x 8 halfs

template <int THREADS>
__device__ __forceinline__ void chunk_copy16(const float* __restrict__ W16, int chunk, float4 (&regs)[4096 / 4 / THREADS]) {
  const float4* src = reinterpret_cast<const float4*>(W16 + (size_t)chunk * kChunkFloats16);
#pragma unroll
  for (int i = 0; i < 4096 / 4 / THREADS; ++i) regs[i] = src[threadIdx.x + i * THREADS];
}
template <int THREADS>
__device__ __forceinline__ void chunk_put16(float* Wb, const float4 (&regs)[4096 / 4 / THREADS]) {
  float4* dst = reinterpret_cast<float4*>(Wb);
#pragma unroll
  for (int i = 0; i < 4096 / 4 / THREADS; ++i) dst[threadIdx.x + i * THREADS] = regs[i];
}

template <int NB>
__device__ __forceinline__ void mma_h3n(f32x4 (&acc)[NB][8], const h16x8 (&bhi)[NB], const h16x8 (&blo)[NB], const float* Wb) {
  const int lane = threadIdx.x & 63;
  const h16x8* wp = reinterpret_cast<const h16x8*>(Wb) + lane;
#pragma unroll
  for (int to = 0; to < 8; ++to) {
    const h16x8 ahi = wp[to * 64], alo = wp[(8 + to) * 64];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb][to] = mfma_h3(ahi, alo, bhi[nb], blo[nb], acc[nb][to]);
  }
}

template <int NB, int WAVES>
__global__ __launch_bounds__(WAVES * 64, NB == 1 ? 4 : 2)
void mlp_col_v5_kernel(ColParams P, const float* __restrict__ W16, const float* __restrict__ pts,
                       const float* __restrict__ views, const float* __restrict__ c_col, int Q, float* __restrict__ raw,
                       int* __restrict__ range_flag) {
  bool bad = false;
  constexpr int THREADS = WAVES * 64;
  extern __shared__ float smem[];
  float* Wbuf = smem;                         // [2][4096]
  Lane L[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) L[nb] = lane_of(blockIdx.x * (WAVES * 16 * NB), Q, NB, nb);
  const int g = L[0].g;
  h16x8 ehi[3][NB], elo[3][NB], chi[NB], clo[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const size_t qq = (size_t)L[nb].q;
    f32x4 e[5];
    col_embed(e, P.Bp, P.Bv, pts, views, qq, g);
    // (the sixth block of the third chunk is zero: 80 channels)
    split2(e[0], e[1], ehi[0][nb], elo[0][nb]);
    split2(e[2], e[3], ehi[1][nb], elo[1][nb]);
    split2(e[4], f32x4{0.f, 0.f, 0.f, 0.f}, ehi[2][nb], elo[2][nb]);
    const float4 v0 = *reinterpret_cast<const float4*>(c_col + qq * 32 + 4 * g);
    const float4 v1 = *reinterpret_cast<const float4*>(c_col + qq * 32 + 16 + 4 * g);
    split2(as_f32x4(v0), as_f32x4(v1), chi[nb], clo[nb]);
  }

  f32x4 acc[NB][8];
  h16x8 hhi[4][NB], hlo[4][NB];
  float4 nxt[4096 / 4 / THREADS];
  chunk_copy16<THREADS>(W16, 0, nxt);
  chunk_put16<THREADS>(Wbuf, nxt);
  __syncthreads();

#define V5_B_E(b) ehi[b], elo[b]
#define V5_B_H(b) hhi[b], hlo[b]
#define V5_B_C(b) chi, clo
#define V5_CHUNK(cidx, OP, b)                                                                                   \
  GLORIE_COL_CHUNK_STEP(cidx, chunk_copy16<THREADS>(W16, (cidx) + 1, nxt),                                      \
                        mma_h3n<NB>(acc, V5_B_##OP(b), Wbuf + ((cidx) & 1) * kChunkFloats16),                   \
                        chunk_put16<THREADS>(Wbuf + (((cidx) + 1) & 1) * kChunkFloats16, nxt))
#define V5_ACT(li) act_layer<softplus100_fast, 8, NB>(acc, P.bias, P.fcb, li, g);
#define V5_NEXT                                                                                       \
  _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) {                                                 \
    _Pragma("unroll") for (int c = 0; c < 4; ++c) split2(acc[nb][2 * c], acc[nb][2 * c + 1], hhi[c][nb], hlo[c][nb]); \
    zero<8>(acc[nb]);                                                                                 \
  }
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) zero<8>(acc[nb]);
  GLORIE_COL_SCHEDULE(V5_CHUNK, V5_ACT, V5_NEXT)
#undef V5_NEXT
#undef V5_ACT
#undef V5_CHUNK
#undef V5_B_C
#undef V5_B_H
#undef V5_B_E
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) bad = bad | col_output(acc[nb], P, L[nb], Q, raw);
  report_range(bad, range_flag);
}

// ====================================================================================
// per-neighbour F_theta
// ====================================================================================
// Transposed formulation (see mlp_col_v3_kernel): W1 (52 x 128) resident in LDS, the 52 input channels of neighbour k
// built directly as B fragments - lane (r, g) owns sample r and supplies, for k-slot g, colour-feature channels
// 16t + 4g + rr (two 16-byte loads of the neighbour's feature row) and embedding features 4s + g (s = 0..4; sin for
// feature < 10, cos otherwise).  No staging buffer and no barrier inside the neighbour loop; the weighted sum of the eight
// softplus outputs stays in the accumulator layout, which is again the B layout of the second layer.

// LDS of a workgroup: the kernel's form of W1 (WFLOATS floats), then what both kernels share
struct NbLds {
  float* b1s;     // [128]
  float* wbuf;    // [128][8] IDW weights (0 for an absent neighbour)
  int* ibuf;      // [128][8] neighbour ids (0 for an absent one)
  float* bs;      // [20][4] B[:, f mod 10] (revolutions per metre): 15 registers short otherwise
};
constexpr size_t nb_lds_bytes(int wfloats) {
  return sizeof(float) * (wfloats + 128 + kTM2 * 8 + 80) + sizeof(int) * kTM2 * 8;
}
__device__ __forceinline__ NbLds nb_lds(float* smem, int wfloats) {
  NbLds s;
  s.b1s = smem + wfloats;
  s.wbuf = s.b1s + 128;
  s.ibuf = reinterpret_cast<int*>(s.wbuf + kTM2 * 8);
  s.bs = reinterpret_cast<float*>(s.ibuf + kTM2 * 8);
  return s;
}
constexpr int kNbW1Lds = 52 * kLdw3;          // exact kernel: [52][132], columns permuted like the colour chunks
constexpr int kNbFrag = 8192;                 // split kernel: [2 chunks][hi|lo][8][64] fragments of 8 halfs = 32 KB

// frequency vectors, IDW weights and neighbour ids of the workgroup's 128 samples (from sample q0) into LDS
__device__ __forceinline__ void nb_stage_meta(const NbLds& s, const float* __restrict__ B, const int64_t* __restrict__ I,
                                              const float* __restrict__ wts, int q0, int Q) {
  const int tid = threadIdx.x;
  if (tid < 80) {
    const int f = tid >> 2, d = tid & 3;
    s.bs[tid] = d < 3 ? B[d * 10 + (f < 10 ? f : f - 10)] : 0.0f;
  }
  for (int idx = tid; idx < kTM2 * 8; idx += 512) {
    const int row = idx >> 3;
    const int q = min(q0 + row, Q - 1);
    const int ii = (int)I[(size_t)q * 8 + (idx & 7)];
    s.wbuf[idx] = (q0 + row < Q && ii >= 0) ? wts[(size_t)q * 8 + (idx & 7)] : 0.0f;
    s.ibuf[idx] = ii < 0 ? 0 : ii;
  }
}

// neighbour k of the lane's sample: IDW weight, the two 16-byte pieces of its colour-feature row this lane supplies, and its
// position relative to the sample at (qx, qy, qz)
struct NbRow { float w; float4 c0, c1; float rx, ry, rz; };
__device__ __forceinline__ NbRow nb_row(const NbLds& s, int srow, int k, const float* __restrict__ cloud,
                                        const float* __restrict__ col_feats, int g, float qx, float qy, float qz, int qs) {
#ifdef EXP_NB_NO_GATHER
  const int pt = qs & 0xffff;                               // ablation: consecutive rows instead of the neighbours'
#else
  const int pt = s.ibuf[srow * 8 + k];
#endif
  NbRow n;
  n.w = s.wbuf[srow * 8 + k];
  n.c0 = *reinterpret_cast<const float4*>(col_feats + (size_t)pt * 32 + 4 * g);
  n.c1 = *reinterpret_cast<const float4*>(col_feats + (size_t)pt * 32 + 16 + 4 * g);
  n.rx = cloud[(size_t)pt * 3 + 0] - qx; n.ry = cloud[(size_t)pt * 3 + 1] - qy; n.rz = cloud[(size_t)pt * 3 + 2] - qz;
  return n;
}
// embedding feature 4 sidx + g of the relative position: frequency column (f mod 10), sin for f < 10; phases in revolutions
__device__ __forceinline__ float nb_embed(const NbRow& n, const float* bsl, int sidx, int g) {
  const float4 bf = *reinterpret_cast<const float4*>(bsl + 16 * sidx);
  const float a = fmaf(n.rz, bf.z, fmaf(n.ry, bf.y, n.rx * bf.x));
#ifdef EXP_NB_NO_SINCOS
  return a;
#else
  return (4 * sidx + g >= 10) ? cos_rev(a) : sin_rev(a);
#endif
}

// ysum += w softplus(acc + b1): one neighbour's first-layer output into the IDW sum
__device__ __forceinline__ void nb_accumulate(f32x4 (&ysum)[8], const f32x4 (&acc)[8], float w, const float* b1s, int g) {
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const float4 bb = *reinterpret_cast<const float4*>(b1s + 16 * t + 4 * g);
    ysum[t][0] += w * softplus100_fast(acc[t][0] + bb.x);
    ysum[t][1] += w * softplus100_fast(acc[t][1] + bb.y);
    ysum[t][2] += w * softplus100_fast(acc[t][2] + bb.z);
    ysum[t][3] += w * softplus100_fast(acc[t][3] + bb.w);
  }
}

// second layer 128 -> 32 in fp32 on the IDW sum (A = W2 straight from global / L2, 16 KB shared by everybody), + b2 sw, and
// the store of the sample's colour feature (0 without neighbours).  Returns the range test of what was stored
__device__ __forceinline__ bool nb_finish(const f32x4 (&ysum)[8], float sw, const NbParams& P, const Lane& L, int Q,
                                          const uint8_t* __restrict__ has, float* __restrict__ c_col) {
  const int g = L.g;
  f32x4 o[2];
  zero<2>(o);
  const float* wp = P.W2 + (4 * g) * 32 + L.r;
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      o[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[(16 * t + rr) * 32], ysum[t][rr], o[0], 0, 0, 0);
      o[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[(16 * t + rr) * 32 + 16], ysum[t][rr], o[1], 0, 0, 0);
    }
  bool bad = false;
  if (L.qs < Q) {
    const bool h = has[L.qs] != 0;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float4 b2 = *reinterpret_cast<const float4*>(P.b2 + 16 * t + 4 * g);
      float4 v;
      v.x = h ? o[t][0] + b2.x * sw : 0.0f;
      v.y = h ? o[t][1] + b2.y * sw : 0.0f;
      v.z = h ? o[t][2] + b2.z * sw : 0.0f;
      v.w = h ? o[t][3] + b2.w * sw : 0.0f;
      bad = bad | not_finite(v.x + v.y + v.z + v.w);
      *reinterpret_cast<float4*>(c_col + (size_t)L.qs * 32 + 16 * t + 4 * g) = v;
    }
  }
  return bad;
}

__global__ __launch_bounds__(512, 4) void mlp_nb_v3_kernel(NbParams P, const float* __restrict__ pts,
                                                           const float* __restrict__ cloud,
                                                           const float* __restrict__ col_feats,
                                                           const int64_t* __restrict__ I,
                                                           const float* __restrict__ wts,
                                                           const uint8_t* __restrict__ has, int Q,
                                                           float* __restrict__ c_col) {
  extern __shared__ float smem[];
  float* W1s = smem;
  const NbLds s = nb_lds(smem, kNbW1Lds);
  const int tid = threadIdx.x;
  const int q0 = blockIdx.x * kTM2;
  for (int idx = tid; idx < 52 * 128; idx += 512) {
    const int col = idx & 127, to = col >> 4, rc = col & 15;
    W1s[(idx >> 7) * kLdw3 + (to >> 2) * 64 + rc * 4 + (to & 3)] = P.W1[idx];
  }
  if (tid < 128) s.b1s[tid] = P.b1[tid];
  nb_stage_meta(s, P.B, I, wts, q0, Q);
  __syncthreads();
  const Lane L = lane_of(q0, Q);
  const int r = L.r, g = L.g;
  const int srow = L.wv * 16 + r;             // this lane's sample row inside the workgroup
  const float qx = pts[(size_t)L.q * 3 + 0], qy = pts[(size_t)L.q * 3 + 1], qz = pts[(size_t)L.q * 3 + 2];
  const float* bsl = s.bs + 4 * g;
  f32x4 ysum[8];
  zero<8>(ysum);
  float sw = 0.0f;
  const float* wpe = W1s + g * kLdw3 + r * 4;               // embedding rows 4s + g
  const float* wpc = W1s + (20 + 4 * g) * kLdw3 + r * 4;    // colour-feature rows 20 + 16t + 4g + rr
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    const NbRow n = nb_row(s, srow, k, cloud, col_feats, g, qx, qy, qz, L.qs);
    f32x4 acc[8];
    zero<8>(acc);
    // 13 k-steps, software pipelined by hand: the two 16-byte weight reads of step i + 1 are issued before
    // the eight MFMAs of step i; the scheduling barrier keeps the compiler from hoisting all 26 reads
    // (104 registers) to the top.  Embedding steps first: they only need the neighbour position, the
    // colour-feature loads (a full L2 round trip behind the index) complete meanwhile.
#define NB_LOAD(WP) w0n = *reinterpret_cast<const float4*>(WP); w1n = *reinterpret_cast<const float4*>((WP) + 64);
#define NB_STEP(BV, NEXT)                                                                \
    {                                                                                    \
      const float4 w0 = w0n, w1 = w1n;                                                   \
      const float bv = (BV);                                                             \
      NEXT                                                                               \
      mfma_step8(acc, w0, w1, bv);                                                       \
      __builtin_amdgcn_sched_barrier(0);                                                 \
    }
    float4 w0n, w1n;
    NB_LOAD(wpe)
#pragma unroll
    for (int sidx = 0; sidx < 5; ++sidx) {
      const float ev = nb_embed(n, bsl, sidx, g);
      if (sidx < 4) NB_STEP(ev, NB_LOAD(wpe + 4 * (sidx + 1) * kLdw3))
      else NB_STEP(ev, NB_LOAD(wpc))
    }
    NB_STEP(n.c0.x, NB_LOAD(wpc + 1 * kLdw3))
    NB_STEP(n.c0.y, NB_LOAD(wpc + 2 * kLdw3))
    NB_STEP(n.c0.z, NB_LOAD(wpc + 3 * kLdw3))
    NB_STEP(n.c0.w, NB_LOAD(wpc + 16 * kLdw3))
    NB_STEP(n.c1.x, NB_LOAD(wpc + 17 * kLdw3))
    NB_STEP(n.c1.y, NB_LOAD(wpc + 18 * kLdw3))
    NB_STEP(n.c1.z, NB_LOAD(wpc + 19 * kLdw3))
    NB_STEP(n.c1.w, )
#undef NB_STEP
#undef NB_LOAD
    sw += n.w;
    nb_accumulate(ysum, acc, n.w, s.b1s, g);
  }
  nb_finish(ysum, sw, P, L, Q, has, c_col);
}

// one 32-slot chunk of the split kernel's first layer: fragments FRAG0 .. FRAG0 + 15 of W1 ([hi 8 | lo 8] output blocks)
template <int FRAG0>
__device__ __forceinline__ void nb_chunk_h3(f32x4 (&acc)[8], const h16x8 bhi, const h16x8 blo, const h16x8* wl) {
#pragma unroll
  for (int to = 0; to < 8; ++to) {
#ifdef EXP_NB_NO_LDSW
    const h16x8 ahi = bhi, alo = blo;                     // ablation: no fragment reads
#else
    const h16x8 ahi = wl[(FRAG0 + to) * 64], alo = wl[(FRAG0 + 8 + to) * 64];
#endif
#ifdef EXP_NB_NO_MFMA
    acc[to][FRAG0 / 16] += (float)ahi[0] * (float)bhi[to & 7] + (float)alo[1] * (float)blo[to & 7];      // ablation: no matrix work
#else
    acc[to] = mfma_h3(ahi, alo, bhi, blo, acc[to]);
#endif
    __builtin_amdgcn_sched_barrier(0);     // keeps the compiler from hoisting all 32 fragment reads (128 registers)
  }
}

// The 52 input channels of a neighbour are two 32-slot chunks: chunk 0 = the 20 embedding features (lane slot s < 5 <->
// feature 4s + g, slots 5..7 zero), chunk 1 = the 32 colour-feature channels (slot s <-> channel 16 (s >> 2) + 4 g + (s & 3),
// the two 16-byte loads of the feature row).  W1 is packed split, as A fragments [chunk][hi|lo][out block][lane][8]
// (point_ops.pack_decoders), and copied to LDS once per workgroup.  GO: see mlp_geo_v4_kernel.
//
// Round 3, measured and not kept (614,400 samples, this kernel = 394 us): two column blocks per wave in
// lockstep 415-463 us; two accumulator sets with the MFMAs of neighbour k+1 issued between the softplus instructions of
// neighbour k (software pipeline inside the wave) 495 us at 2 waves per SIMD, 624 us at 3 (spills) - four resident waves per
// SIMD alternating their phases already overlap the matrix pipe with the vector ALU better than one wave can by itself;
// the kernel sits on its vector floor (8 x 128 softplus per sample, two quarter-rate transcendentals each: ~340 us).  A
// degree-6 polynomial for log2(1 + e) on packed fp32 FMAs instead of v_log_f32 was slower too (405 us: v_pk_fma_f32 beside
// MFMAs is no faster than two v_fma_f32, MI355X_MICROARCH.md), as was the colour kernel with it (450 vs 427 us).
//
// Round 4: what the kernel's 397 us are made of (tools/exp_mlp_ablate.sh, builds with -DEXP_NB_* / -DEXP_MLP_*; every line is
// the kernel with ONE thing removed): fragment reads from LDS 268 (-129), MFMAs 303 (-94), softplus 304 (-91), neighbour
// gather made sequential 366 (-31), low halves of the split 375 (-20), sin / cos 394; without MFMAs, fragment reads and
// softplus 170.  The transcendentals are NOT the floor the round-3 note took them for (v_exp_f32 / v_log_f32 issue at
// ~5/3 of a plain VALU slot on this part, MI355X_MICROARCH.md; a packed-fp16 polynomial for the correction term needs
// degree 8 on [0, 8] and its monomial coefficients ~8^k / k! cancel catastrophically in fp16) - the A operand is: the same
// 32 KB of W1 fragments are read from LDS in front of every MFMA, 1 KB per read, 1024 clocks of the CU's one LDS pipe per
// 816 clocks of MFMA on its four SIMDs.  Keeping the 16 high fragments in 64 VGPRs (a third of the reads, 198 VGPRs, 2
// waves per SIMD, a wave walking 16-sample blocks with the next neighbour's row prefetched; bit-identical) measured 432 us:
// what the reads save, the lost occupancy costs (4 -> 2 waves per SIMD hide the gather and interleave MFMA with VALU
// worse).  Not kept.  The untried middle followed at the end of the round: two 16-sample blocks per wave with the 128 output
// features walked in two halves (2 x 4 accumulator tiles + 2 x 8 sum tiles: 162 VGPRs, no spill, 3 waves per SIMD, 4-wave
// workgroups; every fragment read feeds six MFMAs; bit-identical) - and a 640x480 frame takes 5.42-5.51 ms with it against
// 5.42-5.56 ms without, the single-batch 1/8 share 0.894-0.902 against 0.891-0.918 ms (interleaved builds, same box): halving
// the fragment reads buys exactly what the fourth wave per SIMD was worth.  Not kept either.
template <bool GO>
__global__ __launch_bounds__(512, 4) void mlp_nb_v4_kernel(NbParams P, const float* __restrict__ W1frag,
                                                           const float* __restrict__ pts,
                                                           const float* __restrict__ cloud,
                                                           const float* __restrict__ col_feats,
                                                           const int64_t* __restrict__ I,
                                                           const float* __restrict__ wts,
                                                           const uint8_t* __restrict__ has, int Q,
                                                           float* __restrict__ c_col, int* __restrict__ range_flag) {
  extern __shared__ float smem[];
  const NbLds s = nb_lds(smem, kNbFrag);
  const int tid = threadIdx.x;
  const int q0 = blockIdx.x * kTM2;
  if constexpr (!GO) {                                        // (the weights are no part of the feature pull)
    for (int idx = tid; idx < kNbFrag / 4; idx += 512)        // the split fragments as packed
      reinterpret_cast<float4*>(smem)[idx] = reinterpret_cast<const float4*>(W1frag)[idx];
    if (tid < 128) s.b1s[tid] = P.b1[tid];
  }
  nb_stage_meta(s, P.B, I, wts, q0, Q);
  __syncthreads();
  const Lane L = lane_of(q0, Q);
  const int g = L.g;
  const int srow = L.wv * 16 + L.r;           // this lane's sample row inside the workgroup
  const float qx = pts[(size_t)L.q * 3 + 0], qy = pts[(size_t)L.q * 3 + 1], qz = pts[(size_t)L.q * 3 + 2];
  const float* bsl = s.bs + 4 * g;
  f32x4 ysum[8];
  zero<8>(ysum);
  float sw = 0.0f;
  const h16x8* wl = reinterpret_cast<const h16x8*>(smem) + L.lane;
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    const NbRow n = nb_row(s, srow, k, cloud, col_feats, g, qx, qy, qz, L.qs);
    if constexpr (GO) {
      // measurement instantiation: the neighbour's feature row and position, weighted - no embedding, no layers
      ysum[0][0] += n.w * (n.c0.x + n.c1.x + n.rx); ysum[0][1] += n.w * (n.c0.y + n.c1.y + n.ry);
      ysum[0][2] += n.w * (n.c0.z + n.c1.z + n.rz); ysum[0][3] += n.w * (n.c0.w + n.c1.w);
      sw += n.w;
      continue;
    }
    f32x4 acc[8];
    zero<8>(acc);
    h16x8 bhi, blo;
    // chunk 0: the embedding features
    split2(f32x4{nb_embed(n, bsl, 0, g), nb_embed(n, bsl, 1, g), nb_embed(n, bsl, 2, g), nb_embed(n, bsl, 3, g)},
           f32x4{nb_embed(n, bsl, 4, g), 0.0f, 0.0f, 0.0f}, bhi, blo);
    nb_chunk_h3<0>(acc, bhi, blo, wl);
    // chunk 1: the neighbour's colour feature (a full L2 round trip behind the index: issued above, used here)
    split2(as_f32x4(n.c0), as_f32x4(n.c1), bhi, blo);
    nb_chunk_h3<16>(acc, bhi, blo, wl);
    sw += n.w;
    nb_accumulate(ysum, acc, n.w, s.b1s, g);
  }
  report_range(nb_finish(ysum, sw, P, L, Q, has, c_col), range_flag);
}
}  // namespace glorie

using namespace glorie;

// ---- the packed parameter buffer: its sections in order, sizes in floats.  point_ops.pack_decoders writes them in this
// order; the size the library reports and every pointer handed to a kernel come from this one list ----
namespace {
enum PackSection {
  kSecGeoB, kSecGeoBias, kSecGeoFcb, kSecGeoBout,                              // GeoParams
  kSecNbB, kSecNbW1, kSecNbB1, kSecNbW2, kSecNbB2,                             // NbParams
  kSecColBp, kSecColBv, kSecColWout, kSecColBias, kSecColFcb, kSecColBout,     // ColParams
  kSecColChunks,  // colour K-rows, 27 chunks of [32][128], columns permuted (mlp_col_v3_kernel)
  kSecGeoImage,   // geometry K-rows as the LDS image of mlp_geo_v3_kernel; its trailing output layer serves mlp_geo_v4 too
  kSecColFrags,   // colour chunks as split A fragments (mlp_col_v5_kernel)
  kSecNbFrags,    // W1 as split A fragments (mlp_nb_v4_kernel)
  kSecGeoFrags,   // geometry K-rows as split A fragments (mlp_geo_v4_kernel)
  kPackSections
};
constexpr size_t kPackFloats[kPackSections] = {
    3 * 96, 5 * 32, 5 * 32, 4,
    3 * 10 + 2 /* pad to 16 bytes */, 52 * 128, 128, 128 * 32, 32,
    3 * 20, 3 * 20, 128 * 16, 5 * 128, 5 * 128, 4,
    (size_t)kColChunks * 32 * 128, kGeoImage, (size_t)kColChunks * kChunkFloats16, kNbFrag, kGeoFrag};
constexpr size_t pack_offset(int section) {
  size_t o = 0;
  for (int i = 0; i < section; ++i) o += kPackFloats[i];
  return o;
}
}  // namespace

extern "C" size_t glorie_decoder_pack_floats(void) { return pack_offset(kPackSections); }

extern "C" int glorie_render_mlp(const float* packed, const float* pts, const float* views,
                                 const float* cloud_pos, const float* col_feats,
                                 const float* c_geo, const float* geo_feats, const int64_t* I,
                                 const float* weights, const uint8_t* has, int Q, float* c_col_scratch,
                                 float* raw, int stage_flags, int* range_flag, void* stream) {
  const int stage_color = stage_flags & 1;
  const bool force_f32 = (stage_flags & 2) != 0;
  const bool gather_only = (stage_flags & 4) != 0;        // measurement: the R2 phases of the geometry / per-neighbour kernels alone
  if (Q < 0) return GLORIE_EINVAL;
  if (Q == 0) return GLORIE_OK;
  if (!packed || !pts || !has || !raw) return GLORIE_EINVAL;
  if (!c_geo && !(geo_feats && I && weights)) return GLORIE_EINVAL;   // interpolated feature, or what it takes
  if (stage_color && (!views || !cloud_pos || !col_feats || !I || !weights || !c_col_scratch))
    return GLORIE_EINVAL;
  if (gather_only && (force_f32 || !(geo_feats && I && weights))) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  auto at = [&](PackSection s) { return packed + pack_offset(s); };
  const GeoParams g{at(kSecGeoB), at(kSecGeoBias), at(kSecGeoFcb), at(kSecGeoBout)};
  const NbParams n{at(kSecNbB), at(kSecNbW1), at(kSecNbB1), at(kSecNbW2), at(kSecNbB2)};
  const ColParams k{at(kSecColBp), at(kSecColBv), at(kSecColWout), at(kSecColBias), at(kSecColFcb), at(kSecColBout)};
  const float* geo_image = at(kSecGeoImage);
  // fp16 matrix cores with the 3-term split (fp32 accuracy) unless the caller or GLORIE_MLP_F32=1 asks for the fp32 MFMA
  // kernels; read at every call (bench.py toggles it between launches)
  const char* f32env = getenv("GLORIE_MLP_F32");
  const bool precise = force_f32 || (f32env && f32env[0] == '1');
  const dim3 blocks((Q + kTM2 - 1) / kTM2), threads(512);
  const dim3 geo4_blocks(blocks.x < 512 ? blocks.x : 512);            // persistent over the sample blocks
  constexpr size_t geo_lds = sizeof(float) * kGeoImage, geo4_lds = sizeof(float) * (kGeoFrag + kGeoOut);
  constexpr size_t nb_lds3 = nb_lds_bytes(kNbW1Lds), nb_lds4 = nb_lds_bytes(kNbFrag);
  constexpr size_t col_lds = sizeof(float) * 2 * kChunkFloats3, col16_lds = sizeof(float) * 2 * kChunkFloats16;
  // a feature source the kernels ignore is not passed on: c_geo wins over geo_feats (except in the gather measurement)
  const float* feats = (c_geo && !gather_only) ? nullptr : geo_feats;
  if (gather_only) {
    GLORIE_TRY(launch_lds<mlp_geo_v4_kernel<true>>(geo4_blocks, threads, geo4_lds, st, g, at(kSecGeoFrags), geo_image + kGeoRows * 32,
                                                   pts, c_geo, feats, I, weights, has, Q, raw, range_flag));
    if (stage_color)
      GLORIE_TRY(launch_lds<mlp_nb_v4_kernel<true>>(blocks, threads, nb_lds4, st, n, at(kSecNbFrags), pts, cloud_pos, col_feats, I,
                                                    weights, has, Q, c_col_scratch, range_flag));
    return check_launch();
  }
  if (precise)
    GLORIE_TRY(launch_lds<mlp_geo_v3_kernel>(blocks, threads, geo_lds, st, g, geo_image, pts, c_geo, feats, I, weights, has, Q,
                                             raw));
  else
    GLORIE_TRY(launch_lds<mlp_geo_v4_kernel<false>>(geo4_blocks, threads, geo4_lds, st, g, at(kSecGeoFrags),
                                                    geo_image + kGeoRows * 32, pts, c_geo, feats, I, weights, has, Q, raw,
                                                    range_flag));
  if (stage_color && precise) {
    GLORIE_TRY(launch_lds<mlp_nb_v3_kernel>(blocks, threads, nb_lds3, st, n, pts, cloud_pos, col_feats, I, weights, has, Q,
                                            c_col_scratch));
    GLORIE_TRY(launch_lds<mlp_col_v3_kernel>(blocks, threads, col_lds, st, k, at(kSecColChunks), pts, views, c_col_scratch, Q, raw));
  } else if (stage_color) {
    GLORIE_TRY(launch_lds<mlp_nb_v4_kernel<false>>(blocks, threads, nb_lds4, st, n, at(kSecNbFrags), pts, cloud_pos, col_feats, I,
                                                   weights, has, Q, c_col_scratch, range_flag));
    // 32 samples per wave, 4 waves per workgroup
    GLORIE_TRY((launch_lds<mlp_col_v5_kernel<2, 4>>(dim3((Q + 127) / 128), dim3(256), col16_lds, st, k, at(kSecColFrags), pts, views,
                                                    c_col_scratch, Q, raw, range_flag)));
  }
  return check_launch();
}
