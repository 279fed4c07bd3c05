// LPIPS (torchmetrics' _LPIPS, version 0.1, AlexNet, eval mode) of two images, for the re-render evaluation (reference:
// src/utils/eval_render.py:27-28, :64-65, :85-86): five convolutions, two max-pools and a score, all f32 features.
//
// Convolutions (lpips_conv_kernel, one launch per layer, both images as blockIdx.z): implicit GEMM on the exact-f32 MFMA
//   (v_mfma_f32_16x16x4_f32).  A workgroup of 256 threads owns 64 output pixels of one image x 64 output channels; each of
//   its four waves owns 32 x 32 of that as 2 x 2 MFMA tiles.  conv3 to conv5 have few output pixels (2 x 29 x 39 at
//   480x640) and take 32 pixels per workgroup - 16 x 32 per wave - for twice the workgroups (measured: DESIGN 4.4n).  K runs over (ky, kx, c) with c innermost - the features are
//   stored [2, h, w, C] - in chunks of 32: the weights [32][64] (A operand, rows = output channels) and the gathered
//   inputs [64 or 32][32] (B operand, columns = pixels) are staged in LDS through registers, so the global loads of the next
//   chunk are in flight while the MFMAs of this one run.  Every run of 16 k starts from a zero accumulator - a k-ordered
//   f32 fmaf chain of four MFMAs - and is then added to an fp64 running total, so the only f32 roundings of a feature
//   are those inside the short chains and the final store: with K up to 3456 the rounding of an f32 running total would
//   otherwise dominate the error of the small late taps.  An output value depends only on its own operands in a fixed
//   order, so two identical images give bit-identical features.  Bias (added in fp64) and ReLU in the epilogue, 16-byte
//   stores.
//   Staging modes: kImage (conv1) gathers from the caller's image in either layout and applies clamp, 2x - 1 and the
//   shift / scale; a padded tap is 0 in the scaled domain.  kPlain reads a feature map, kPool the 3x3 / stride-2 maximum
//   of one (the pool folded into the staging; flag GLORIE_LPIPS_FOLD_POOLS).  Without the flag the pools are launches
//   of their own (lpips_pool_kernel).  Both give the same bits: a maximum does not round.
// Score (lpips_score_kernel, one launch for the five taps; lpips_finish_kernel): a wave per pixel forms both channel
//   norms, the normalised difference and the lin-weighted sum in fp64; per-workgroup partials are added in a fixed order
//   (ordered_sum).  No atomics, no host synchronisation, no allocation: everything records into a hipGraph.
#include "compact.hiph"

using namespace glorie;

namespace {

constexpr int kLayers = 5;
constexpr int kBM = 64;                       // output pixels of one workgroup, conv1 and conv2
constexpr int kBMLate = 32;                   // ... conv3 to conv5: few output pixels, twice the workgroups
constexpr int kBN = 64;                       // output channels of one workgroup
constexpr int kBK = 32;                       // K of one staged chunk
constexpr int kRun = 16;                      // K of one f32 MFMA chain; the chains are added in fp64
constexpr int kThreads = 256;
constexpr int kLdW = 80;                      // floats per k-row of the weight chunk: the four k-rows of a read hit 64 banks
constexpr int kLdX = 36;                      // floats per pixel row of the input chunk: 16 pixels x 4 k hit 64 banks
constexpr int kMinSide = 31, kMaxSide = 16384;
constexpr int kMaxScoreBlocks = 256;
constexpr int kConv1Taps = 363;               // 11 * 11 * 3, padded to 364 in the packed weights
// torchmetrics' form of the channel normalisation: f / sqrt(eps + sum f^2) with eps = 1e-8 inside the root (the original
// lpips package divides by sqrt(sum) + 1e-10)
constexpr double kNormEps = 1e-8;

struct LayerDef {
  int ci, co, ks, stride, pad, kpad;
};
constexpr LayerDef kNet[kLayers] = {{3, 64, 11, 4, 2, 364},
                                    {64, 192, 5, 1, 2, 1600},
                                    {192, 384, 3, 1, 1, 1728},
                                    {384, 256, 3, 1, 1, 3456},
                                    {256, 256, 3, 1, 1, 2304}};
static_assert(kNet[0].co % kBN == 0 && kNet[1].co % kBN == 0 && kNet[2].co % kBN == 0 && kNet[3].co % kBN == 0 &&
              kNet[4].co % kBN == 0, "every layer's output channels tile by kBN");
static_assert(kNet[1].ci % kBK == 0 && kNet[2].ci % kBK == 0 && kNet[3].ci % kBK == 0 && kNet[4].ci % kBK == 0,
              "a K chunk of the feature layers stays inside one tap");
static_assert(kThreads == 256 && kBK == 32 && kBN == 64 && kBM % 32 == 0 && kBMLate % 32 == 0,
              "staging maps: 8 threads x 16 bytes per pixel row, 32 pixel rows per pass; 16 threads per k-row");

enum Mode { kImage = 0, kPlain = 1, kPool = 2 };

struct ConvArgs {
  const float* in0;      // kImage: x; else the source feature map [2, sh, sw, ci]
  const float* in1;      // kImage: y
  const float* w;        // [kpad][co]
  const float* bias;     // [co]
  float* out;            // [2, oh, ow, co]
  int ih, iw;            // the convolution's input size (after the pool for kPool)
  int sh, sw;            // the source map's size (before the pool for kPool; = ih, iw otherwise)
  int ci, co, ks, stride, pad, kpad, oh, ow;
  int chw;               // kImage: the images are [3,H,W]
};

struct Net {
  int h[kLayers], w[kLayers];   // of the five taps
  int ph[2], pw[2];             // of the two pooled maps
  int score_blocks;
};

using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float4 max4(float4 a, float4 b) {
  return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

// one scaled input value of conv1: clamp, 2x - 1, (v - shift) / scale
__device__ __forceinline__ float scaled_pixel(const float* __restrict__ img, int chw, int H, int W, int y, int x, int c) {
  const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
  const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
  float v = chw ? img[((size_t)c * H + y) * W + x] : img[((size_t)y * W + x) * 3 + c];
  v = fminf(fmaxf(v, 0.f), 1.f);
  v = 2.f * v - 1.f;
  return (v - shift) / scale;
}

// the 4 consecutive k of chunk row `k` (a multiple of 4) for output pixel (oy, ox) of image `img`; 0 where the tap is padding
template <int MODE>
__device__ __forceinline__ float4 gather(const ConvArgs& a, int img, bool valid, int oy, int ox, int k) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!valid) return v;
  if (MODE == kImage) {
    const float* src = img ? a.in1 : a.in0;
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kk = k + j;
      const int ky = kk / 33, r = kk - ky * 33, kx = r / 3, c = r - kx * 3;
      const int iy = oy * 4 - 2 + ky, ix = ox * 4 - 2 + kx;
      const bool in = kk < kConv1Taps && iy >= 0 && iy < a.ih && ix >= 0 && ix < a.iw;
      e[j] = in ? scaled_pixel(src, a.chw, a.ih, a.iw, iy, ix, c) : 0.f;
    }
    return make_float4(e[0], e[1], e[2], e[3]);
  }
  const int tap = k / a.ci, c = k - tap * a.ci;
  const int ky = tap / a.ks, kx = tap - ky * a.ks;
  const int iy = oy * a.stride - a.pad + ky, ix = ox * a.stride - a.pad + kx;
  if (tap >= a.ks * a.ks || iy < 0 || iy >= a.ih || ix < 0 || ix >= a.iw) return v;
  if (MODE == kPlain) {
    return *reinterpret_cast<const float4*>(a.in0 + (((size_t)img * a.sh + iy) * a.sw + ix) * a.ci + c);
  }
  // kPool: rows 2 iy .. 2 iy + 2 and columns 2 ix .. 2 ix + 2 of the source are inside it (floor mode, no padding)
  const float* p = a.in0 + (((size_t)img * a.sh + 2 * iy) * a.sw + 2 * ix) * a.ci + c;
  v = *reinterpret_cast<const float4*>(p);
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
      if (dy || dx) v = max4(v, *reinterpret_cast<const float4*>(p + ((size_t)dy * a.sw + dx) * a.ci));
  return v;
}

template <int MODE, int BM>
__global__ void __launch_bounds__(kThreads) lpips_conv_kernel(ConvArgs a) {
  constexpr int NP = BM / 32;                 // staging passes over the pixel rows = 16-pixel MFMA tiles of one wave
  __shared__ __attribute__((aligned(16))) float Ws[kBK * kLdW];
  __shared__ __attribute__((aligned(16))) float Xs[BM * kLdX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.z, n0 = blockIdx.y * kBN, p0 = blockIdx.x * BM;
  const int npx = a.oh * a.ow;
  // staging: thread -> 4 k of pixel rows (tid >> 3) (+ 32 with BM = 64); 4 channels of k-rows (tid >> 4) and (tid >> 4) + 16
  const int xk = (tid & 7) * 4, xp = tid >> 3;
  const int wk = tid >> 4, wc = (tid & 15) * 4;
  int oy[NP], ox[NP];
  bool pv[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int p = p0 + xp + 32 * i;
    pv[i] = p < npx;
    oy[i] = pv[i] ? p / a.ow : 0;
    ox[i] = pv[i] ? p - oy[i] * a.ow : 0;
  }
  float4 rx[NP], rw[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NP; ++i) rx[i] = gather<MODE>(a, img, pv[i], oy[i], ox[i], k0 + xk);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = k0 + wk + 16 * i;
      rw[i] = row < a.kpad ? *reinterpret_cast<const float4*>(a.w + (size_t)row * a.co + n0 + wc)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  // compute: wave -> pixels 16 NP wm .., channels 32 wn ..; lane -> k = g, pixel / channel r inside a 16 x 16 tile
  const int g = lane >> 4, r = lane & 15;
  const int wm = wave & 1, wn = wave >> 1;
  double total[2][NP][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < NP; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) total[t][u][q] = 0.0;
  fetch(0);
  for (int k0 = 0; k0 < a.kpad; k0 += kBK) {
    __syncthreads();                          // the previous chunk has been read
#pragma unroll
    for (int i = 0; i < NP; ++i) *reinterpret_cast<float4*>(&Xs[(xp + 32 * i) * kLdX + xk]) = rx[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(&Ws[(wk + 16 * i) * kLdW + wc]) = rw[i];
    __syncthreads();
    if (k0 + kBK < a.kpad) fetch(k0 + kBK);
#pragma unroll
    for (int half = 0; half < kBK / kRun; ++half) {
      f32x4 acc[2][NP];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < NP; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = half * (kRun / 4); s < (half + 1) * (kRun / 4); ++s) {
        float wa[2], xb[NP];
#pragma unroll
        for (int t = 0; t < 2; ++t) wa[t] = Ws[(4 * s + g) * kLdW + 32 * wn + 16 * t + r];
#pragma unroll
        for (int u = 0; u < NP; ++u) xb[u] = Xs[(16 * NP * wm + 16 * u + r) * kLdX + 4 * s + g];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int u = 0; u < NP; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t], xb[u], acc[t][u], 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < NP; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) total[t][u][q] += (double)acc[t][u][q];
    }
  }
  // accumulator element q of lane (g, r): channel 4 g + q of the tile, pixel r
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const int p = p0 + 16 * NP * wm + 16 * u + r;
    if (p >= npx) continue;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int ch = n0 + 32 * wn + 16 * t + 4 * g;
      const float4 b = *reinterpret_cast<const float4*>(a.bias + ch);
      const double* v = total[t][u];
      *reinterpret_cast<float4*>(a.out + ((size_t)img * npx + p) * a.co + ch) =
          make_float4(fmaxf((float)(v[0] + (double)b.x), 0.f), fmaxf((float)(v[1] + (double)b.y), 0.f),
                      fmaxf((float)(v[2] + (double)b.z), 0.f), fmaxf((float)(v[3] + (double)b.w), 0.f));
    }
  }
}

// max_pool2d(3, stride 2), no padding, floor mode: in [n, sh, sw, C] -> out [n, ph, pw, C], 4 channels per thread
__global__ void __launch_bounds__(kThreads)
lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int sh, int sw, int ph, int pw, int c4,
                  long long total) {
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
    const int c = (int)(e % c4);
    long long q = e / c4;
    const int x = (int)(q % pw);
    q /= pw;
    const int y = (int)(q % ph), n = (int)(q / ph);
    const float4* p = reinterpret_cast<const float4*>(in) + (((size_t)n * sh + 2 * y) * sw + 2 * x) * c4 + c;
    float4 v = p[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx)
        if (dy || dx) v = max4(v, p[((size_t)dy * sw + dx) * c4]);
    reinterpret_cast<float4*>(out)[e] = v;
  }
}

struct ScoreArgs {
  const float* f[kLayers];      // [2, npx, c]
  const float* lin[kLayers];    // [c]
  int npx[kLayers], c[kLayers];
};

// partial[tap][block] = sum over the block's pixels of sum_c lin[c] (f_x / |f_x| - f_y / |f_y|)^2; a wave per pixel
__global__ void __launch_bounds__(kThreads) lpips_score_kernel(ScoreArgs a, double* __restrict__ partial) {
  const int tap = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int npx = a.npx[tap], C = a.c[tap];
  const float* __restrict__ fx = a.f[tap];
  const float* __restrict__ fy = fx + (size_t)npx * C;
  const float* __restrict__ lin = a.lin[tap];
  double sum = 0.0;
  for (int p = blockIdx.x * (kThreads / 64) + wave; p < npx; p += gridDim.x * (kThreads / 64)) {
    const float* px = fx + (size_t)p * C;
    const float* py = fy + (size_t)p * C;
    double sx = 0.0, sy = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double vx = (double)px[c], vy = (double)py[c];
      sx += vx * vx;
      sy += vy * vy;
    }
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    const double ix = 1.0 / sqrt(kNormEps + sx), iy = 1.0 / sqrt(kNormEps + sy);
    double s = 0.0;
    for (int c = lane; c < C; c += 64) {
      // both products are rounded before the subtraction (no fma): identical features give exactly 0, and swapping the
      // images only changes the sign of d
#pragma clang fp contract(off)
      const double d = (double)px[c] * ix - (double)py[c] * iy;
      s += (double)lin[c] * (d * d);
    }
    sum += wave_sum(s);
  }
  // every lane of a wave holds the wave's sum already: lane 0's goes into the workgroup sum.  The butterfly then only adds
  // zeros (same bits; 8 more VGPRs, occupancy unchanged): the price of one reduction helper instead of a store-only variant
  const double t = block_sum<kThreads / 64>(lane == 0 ? sum : 0.0);
  if (threadIdx.x == 0) partial[(size_t)tap * gridDim.x + blockIdx.x] = t;
}

// out[1 + l] = mean over the pixels of tap l; out[0] = their sum
__global__ void __launch_bounds__(64 * kLayers)
lpips_finish_kernel(const double* __restrict__ partial, int n_blocks, ScoreArgs a, float* __restrict__ out) {
  __shared__ double mean[kLayers];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double t = ordered_sum(partial + (size_t)wave * n_blocks, n_blocks, 1);
  if (lane == 0) mean[wave] = t / (double)a.npx[wave];
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int l = 0; l < kLayers; ++l) {
      total += mean[l];
      out[1 + l] = (float)mean[l];
    }
    out[0] = (float)total;
  }
}

bool make_net(int H, int W, Net* net) {
  if (H < kMinSide || W < kMinSide || H > kMaxSide || W > kMaxSide) return false;
  auto conv = [](int n, const LayerDef& d) { return (n + 2 * d.pad - d.ks) / d.stride + 1; };
  auto pool = [](int n) { return (n - 3) / 2 + 1; };
  net->h[0] = conv(H, kNet[0]);
  net->w[0] = conv(W, kNet[0]);
  net->ph[0] = pool(net->h[0]);
  net->pw[0] = pool(net->w[0]);
  net->h[1] = conv(net->ph[0], kNet[1]);
  net->w[1] = conv(net->pw[0], kNet[1]);
  net->ph[1] = pool(net->h[1]);
  net->pw[1] = pool(net->w[1]);
  for (int l = 2; l < kLayers; ++l) {
    net->h[l] = conv(l == 2 ? net->ph[1] : net->h[l - 1], kNet[l]);
    net->w[l] = conv(l == 2 ? net->pw[1] : net->w[l - 1], kNet[l]);
  }
  const long long waves = ((long long)net->h[0] * net->w[0] + kThreads / 64 - 1) / (kThreads / 64);
  net->score_blocks = (int)(waves < kMaxScoreBlocks ? waves : kMaxScoreBlocks);
  return true;
}

// doubles of the score partials, rounded up to an even count (the float maps behind them stay 16-byte aligned)
inline size_t partial_doubles(const Net& n) { return ((size_t)kLayers * n.score_blocks + 1) & ~(size_t)1; }
inline size_t map_floats(const Net& n, int l) { return 2 * (size_t)n.h[l] * n.w[l] * kNet[l].co; }
inline size_t pooled_floats(const Net& n, int i) { return 2 * (size_t)n.ph[i] * n.pw[i] * kNet[i].co; }
inline size_t own_floats(const Net& n) {
  size_t f = 0;
  for (int l = 0; l < kLayers; ++l) f += map_floats(n, l);
  return f;
}

// workspace: partials double [5][score_blocks] | the five feature maps | the two pooled maps.  Every piece is a multiple of
// 16 bytes (an even count of doubles, channel counts that are multiples of 4), which the float4 accesses of the maps need
struct LpipsWs {
  Carver c;
  Net net;
  double* partial = c.take<double>(partial_doubles(net));
  float* own = c.take<float>(own_floats(net));
  float* pooled[2] = {c.take<float>(pooled_floats(net, 0)), c.take<float>(pooled_floats(net, 1))};
};

template <int MODE, int BM>
int launch_conv(const ConvArgs& a, hipStream_t st) {
  const dim3 grid((a.oh * a.ow + BM - 1) / BM, a.co / kBN, 2);
  hipLaunchKernelGGL((lpips_conv_kernel<MODE, BM>), grid, dim3(kThreads), 0, st, a);
  return check_launch();
}

}  // namespace

// packed weights: per layer W [kpad][co] (k = (ky * ks + kx) * ci + c; rows past ks ks ci are 0), then the five biases,
// then the five lin weights
extern "C" size_t glorie_lpips_weight_floats(void) {
  size_t n = 0;
  for (int l = 0; l < kLayers; ++l) n += (size_t)kNet[l].kpad * kNet[l].co + 2 * (size_t)kNet[l].co;
  return n;
}

extern "C" int glorie_lpips_shapes(int H, int W, int* hw) {
  Net net;
  if (!hw || !make_net(H, W, &net)) return GLORIE_EINVAL;
  for (int l = 0; l < kLayers; ++l) {
    hw[2 * l] = net.h[l];
    hw[2 * l + 1] = net.w[l];
  }
  return GLORIE_OK;
}

extern "C" size_t glorie_lpips_workspace(int H, int W) {
  Net net;
  return make_net(H, W, &net) ? carved_bytes<LpipsWs>(net) : 0;
}

extern "C" int glorie_lpips(const float* x, const float* y, int H, int W, int channels_first, const float* weights,
                            void* workspace, float* out, float* features, int flags, void* stream) {
  Net net;
  if (!x || !y || !weights || !workspace || !out) return GLORIE_EINVAL;
  if ((flags & ~GLORIE_LPIPS_FOLD_POOLS) != 0) return GLORIE_EINVAL;
  if (((uintptr_t)weights | (uintptr_t)workspace | (uintptr_t)features) & 15) return GLORIE_EINVAL;   // 16-byte loads
  if (!make_net(H, W, &net)) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const bool fold = (flags & GLORIE_LPIPS_FOLD_POOLS) != 0;
  const LpipsWs ws{Carver(workspace), net};
  double* partial = ws.partial;
  float* const* pooled = ws.pooled;
  float* maps[kLayers];
  float* base = features ? features : ws.own;
  for (int l = 0; l < kLayers; ++l) {
    maps[l] = base;
    base += map_floats(net, l);
  }
  const float* wl[kLayers];
  const float* bias[kLayers];
  const float* lin[kLayers];
  const float* wp = weights;
  for (int l = 0; l < kLayers; ++l) {
    wl[l] = wp;
    wp += (size_t)kNet[l].kpad * kNet[l].co;
  }
  for (int l = 0; l < kLayers; ++l) {
    bias[l] = wp;
    wp += kNet[l].co;
  }
  for (int l = 0; l < kLayers; ++l) {
    lin[l] = wp;
    wp += kNet[l].co;
  }
  for (int l = 0; l < kLayers; ++l) {
    const LayerDef& d = kNet[l];
    ConvArgs a;
    a.w = wl[l];
    a.bias = bias[l];
    a.out = maps[l];
    a.ci = d.ci, a.co = d.co, a.ks = d.ks, a.stride = d.stride, a.pad = d.pad, a.kpad = d.kpad;
    a.oh = net.h[l], a.ow = net.w[l];
    a.chw = channels_first ? 1 : 0;
    a.in1 = nullptr;
    if (l == 0) {
      a.in0 = x, a.in1 = y;
      a.ih = a.sh = H, a.iw = a.sw = W;
      GLORIE_TRY((launch_conv<kImage, kBM>(a, st)));
    } else if (l <= 2) {
      const int i = l - 1;                    // the pool in front of conv2 and conv3
      a.ih = net.ph[i], a.iw = net.pw[i];
      if (fold) {
        a.in0 = maps[i];
        a.sh = net.h[i], a.sw = net.w[i];
        GLORIE_TRY(l == 1 ? (launch_conv<kPool, kBM>(a, st)) : (launch_conv<kPool, kBMLate>(a, st)));
      } else {
        const long long total = (long long)pooled_floats(net, i) / 4;
        const int blocks = (int)((total + kThreads - 1) / kThreads < 4096 ? (total + kThreads - 1) / kThreads : 4096);
        hipLaunchKernelGGL(lpips_pool_kernel, dim3(blocks), dim3(kThreads), 0, st, maps[i], pooled[i], net.h[i], net.w[i],
                           net.ph[i], net.pw[i], kNet[i].co / 4, total);
        GLORIE_TRY(check_launch());
        a.in0 = pooled[i];
        a.sh = a.ih, a.sw = a.iw;
        GLORIE_TRY(l == 1 ? (launch_conv<kPlain, kBM>(a, st)) : (launch_conv<kPlain, kBMLate>(a, st)));
      }
    } else {
      a.in0 = maps[l - 1];
      a.ih = a.sh = net.h[l - 1], a.iw = a.sw = net.w[l - 1];
      GLORIE_TRY((launch_conv<kPlain, kBMLate>(a, st)));
    }
  }
  ScoreArgs s;
  for (int l = 0; l < kLayers; ++l) {
    s.f[l] = maps[l];
    s.lin[l] = lin[l];
    s.npx[l] = net.h[l] * net.w[l];
    s.c[l] = kNet[l].co;
  }
  hipLaunchKernelGGL(lpips_score_kernel, dim3(net.score_blocks, kLayers), dim3(kThreads), 0, st, s, partial);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(lpips_finish_kernel, dim3(1), dim3(64 * kLayers), 0, st, partial, net.score_blocks, s, out);
  return check_launch();
}
