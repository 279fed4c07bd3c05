// Image-quality metrics of the re-render evaluation (reference: src/utils/eval_render.py:59-89): MS-SSIM with the
// defaults of pytorch_msssim, the PSNR / depth-L1 sums of one frame, and the masking of the saved maps.
//
// MS-SSIM, `levels` + 1 launches (ms_ssim_level_kernel per level, ms_ssim_finish_kernel):
//   a workgroup of 256 threads owns a 32 x 16 tile of one channel's valid-convolution output.  It stages the 42 x 26
//   haloed tile of X and Y in LDS once (fp32, zero outside the image), forms the five moment planes G*X, G*Y, G*(X.X),
//   G*(Y.Y), G*(X.Y) with a horizontal 11-tap pass (fp64, into LDS) and a vertical one (fp64, in registers), evaluates
//   cs and ssim per pixel and reduces the valid ones to one (ssim, cs) pair per workgroup.  Workgroups with
//   blockIdx.z >= 3 of the same launch write the next level instead: avg_pool2d(2, 2, padding = size % 2,
//   count_include_pad) of both images into the planar fp32 pyramid.  The finishing workgroup sums the partials of every
//   (level, channel) in a fixed order in fp64, applies relu, powers, product and channel mean.
// Frame sums, 2 launches (frame_reduce_kernel, frame_finish_kernel): squared colour difference over the frame and over
//   the mask, the mask count, |depth - gt_depth| over the mask; fp32 differences accumulated in fp64.
// No floating-point atomics anywhere: every sum is a per-workgroup partial added in a fixed order (ordered_sum), so
// repeated calls are bitwise equal.  No host synchronisation, no allocation: everything records into a hipGraph.
#include "compact.hiph"

using namespace glorie;

namespace {

constexpr int kWin = 11;                      // taps of the gaussian window
constexpr int kTW = 32, kTH = 16;             // output tile of one workgroup
constexpr int kInW = kTW + kWin - 1;          // 42
constexpr int kInH = kTH + kWin - 1;          // 26
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kHSeg = 4;                      // outputs per thread along a row, horizontal pass
constexpr int kVSeg = 2;                      // outputs per thread along a column, vertical pass
constexpr int kMaxLevels = 5;
constexpr double kC1 = 1e-4, kC2 = 9e-4;      // (0.01 * data_range)^2, (0.03 * data_range)^2 with data_range 1

static_assert(kTW * (kTH / kVSeg) == kThreads, "vertical pass: one thread per column and row pair");
static_assert(kTW % kHSeg == 0 && kTH % kVSeg == 0, "segments tile the output");

struct Window {
  double g[kWin];
};

struct Pyramid {
  int levels;
  int h[kMaxLevels], w[kMaxLevels];
  int blocks[kMaxLevels];                     // workgroups (tiles) per channel of the level
  long long offset[kMaxLevels];               // of the level's partials, in doubles
  double weight[kMaxLevels];
};

__device__ __forceinline__ size_t pixel_index(int hwc, int c, int y, int x, int h, int w) {
  return hwc ? ((size_t)y * w + x) * 3 + c : ((size_t)c * h + y) * w + x;
}

// 2x2 average pooling of one channel of x and y into the planar next level; input index 2o - pad, 2o - pad + 1
__device__ __forceinline__ float pool_at(const float* __restrict__ img, int hwc, int c, int h, int w, int oy, int ox) {
  const int y0 = 2 * oy - (h & 1), x0 = 2 * ox - (w & 1);
  double s = 0.0;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int y = y0 + dy, x = x0 + dx;
      if (y >= 0 && y < h && x >= 0 && x < w) s += (double)img[pixel_index(hwc, c, y, x, h, w)];
    }
  return (float)(0.25 * s);
}

__global__ void __launch_bounds__(kThreads)
ms_ssim_level_kernel(const float* __restrict__ x, const float* __restrict__ y, int h, int w, int hwc, Window win,
                     double* __restrict__ partial, float* __restrict__ next_x, float* __restrict__ next_y) {
  __shared__ float sx[kInH][kInW + 1], sy[kInH][kInW + 1];
  __shared__ double hp[5][kInH][kTW + 1];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  if (blockIdx.z >= 3) {
    // the next level: this workgroup's 32 x 16 pixels of it (the grid covers it: (w - 10) >= ceil(w / 2) for w >= 21)
    const int c = blockIdx.z - 3;
    const int oh = (h + 1) / 2, ow = (w + 1) / 2;
    for (int e = tid; e < kTW * kTH; e += kThreads) {
      const int oy = y0 + e / kTW, ox = x0 + e % kTW;
      if (oy < oh && ox < ow) {
        const size_t o = ((size_t)c * oh + oy) * ow + ox;
        next_x[o] = pool_at(x, hwc, c, h, w, oy, ox);
        next_y[o] = pool_at(y, hwc, c, h, w, oy, ox);
      }
    }
    return;
  }
  const int c = blockIdx.z;
  for (int e = tid; e < kInH * kInW; e += kThreads) {
    const int ly = e / kInW, lx = e - ly * kInW;
    const int gy = y0 + ly, gx = x0 + lx;
    const bool in = gy < h && gx < w;
    const size_t p = in ? pixel_index(hwc, c, gy, gx, h, w) : 0;
    sx[ly][lx] = in ? x[p] : 0.f;
    sy[ly][lx] = in ? y[p] : 0.f;
  }
  __syncthreads();
  // horizontal pass: a thread owns kHSeg neighbouring outputs of one row; consecutive threads take consecutive rows
  for (int item = tid; item < kInH * (kTW / kHSeg); item += kThreads) {
    const int r = item % kInH, s0 = (item / kInH) * kHSeg;
    double acc[kHSeg][5];
#pragma unroll
    for (int o = 0; o < kHSeg; ++o)
#pragma unroll
      for (int q = 0; q < 5; ++q) acc[o][q] = 0.0;
#pragma unroll
    for (int i = 0; i < kHSeg + kWin - 1; ++i) {
      const double a = (double)sx[r][s0 + i], b = (double)sy[r][s0 + i];
      const double aa = a * a, bb = b * b, ab = a * b;
#pragma unroll
      for (int o = 0; o < kHSeg; ++o) {
        const int k = i - o;
        if (k >= 0 && k < kWin) {
          const double g = win.g[k];
          acc[o][0] += g * a;
          acc[o][1] += g * b;
          acc[o][2] += g * aa;
          acc[o][3] += g * bb;
          acc[o][4] += g * ab;
        }
      }
    }
#pragma unroll
    for (int o = 0; o < kHSeg; ++o)
#pragma unroll
      for (int q = 0; q < 5; ++q) hp[q][r][s0 + o] = acc[o][q];
  }
  __syncthreads();
  // vertical pass: a thread owns kVSeg outputs of one column
  const int col = tid % kTW, r0 = (tid / kTW) * kVSeg;
  double m[kVSeg][5];
#pragma unroll
  for (int o = 0; o < kVSeg; ++o)
#pragma unroll
    for (int q = 0; q < 5; ++q) m[o][q] = 0.0;
#pragma unroll
  for (int q = 0; q < 5; ++q)
#pragma unroll
    for (int j = 0; j < kVSeg + kWin - 1; ++j) {
      const double v = hp[q][r0 + j][col];
#pragma unroll
      for (int o = 0; o < kVSeg; ++o) {
        const int k = j - o;
        if (k >= 0 && k < kWin) m[o][q] += win.g[k] * v;
      }
    }
  double sum_ssim = 0.0, sum_cs = 0.0;
#pragma unroll
  for (int o = 0; o < kVSeg; ++o) {
    const double mu1 = m[o][0], mu2 = m[o][1];
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const double s1 = m[o][2] - mu1_sq, s2 = m[o][3] - mu2_sq, s12 = m[o][4] - mu12;
    const double cs = (2.0 * s12 + kC2) / (s1 + s2 + kC2);
    const double ssim = ((2.0 * mu12 + kC1) / (mu1_sq + mu2_sq + kC1)) * cs;
    const bool valid = (y0 + r0 + o) < h - (kWin - 1) && (x0 + col) < w - (kWin - 1);
    sum_ssim += valid ? ssim : 0.0;
    sum_cs += valid ? cs : 0.0;
  }
  const double sums[2] = {sum_ssim, sum_cs};
  const double s = block_sum<kWaves>(sums);
  if (tid < 2) {
    const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const size_t n_blk = (size_t)gridDim.x * gridDim.y;
    partial[((size_t)c * n_blk + blk) * 2 + tid] = s;
  }
}

// out[0] = ms-ssim; out[1 + 2 l], out[2 + 2 l] = channel means of ssim and cs of level l
__global__ void __launch_bounds__(kThreads)
ms_ssim_finish_kernel(const double* __restrict__ partial, Pyramid pyr, float* __restrict__ out) {
  __shared__ double mean[kMaxLevels][3][2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_series = pyr.levels * 6;
  for (int s0 = 0; s0 < n_series; s0 += kWaves) {
    const int s = s0 + wave;
    if (s < n_series) {
      const int l = s / 6, c = (s / 2) % 3, q = s & 1;
      const int n = pyr.blocks[l];
      const double t = ordered_sum(partial + pyr.offset[l] + (size_t)c * n * 2 + q, n, 2);
      if (lane == 0) mean[l][c][q] = t / ((double)(pyr.h[l] - (kWin - 1)) * (double)(pyr.w[l] - (kWin - 1)));
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int c = 0; c < 3; ++c) {
      double prod = 1.0;
      for (int l = 0; l < pyr.levels; ++l) {
        const double v = fmax(mean[l][c][l == pyr.levels - 1 ? 0 : 1], 0.0);
        prod *= pow(v, pyr.weight[l]);
      }
      total += prod;
    }
    out[0] = (float)(total / 3.0);
    for (int l = 0; l < pyr.levels; ++l) {
      out[1 + 2 * l] = (float)((mean[l][0][0] + mean[l][1][0] + mean[l][2][0]) / 3.0);
      out[2 + 2 * l] = (float)((mean[l][0][1] + mean[l][1][1] + mean[l][2][1]) / 3.0);
    }
  }
}

// partial [blocks][4]: squared colour difference over the frame, over the mask, mask count, |depth - gt_depth| over it
__global__ void __launch_bounds__(kThreads)
frame_reduce_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n_pix,
                    const unsigned char* __restrict__ mask, const float* __restrict__ depth,
                    const float* __restrict__ gt_depth, double* __restrict__ partial) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < n_pix; p += (long long)gridDim.x * kThreads) {
    double e = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = a[3 * p + c] - b[3 * p + c];
      e += (double)d * (double)d;
    }
    s[0] += e;
    if (mask && mask[p]) {
      s[1] += e;
      s[2] += 1.0;
      if (depth && gt_depth) s[3] += (double)fabsf(depth[p] - gt_depth[p]);
    }
  }
  const double t = block_sum<kWaves>(s);
  if (threadIdx.x < 4) partial[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
}

// out = {psnr, masked_psnr, depth_l1}; count = pixels of the mask
__global__ void __launch_bounds__(kThreads)
frame_finish_kernel(const double* __restrict__ partial, int n_blocks, long long n_pix, float* __restrict__ out,
                    int* __restrict__ count) {
  __shared__ double total[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double t = ordered_sum(partial + wave, n_blocks, 4);
  if (lane == 0) total[wave] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double mse = total[0] / (3.0 * (double)n_pix);
    const double masked_mse = total[1] / (3.0 * total[2]);          // 0 / 0 on an empty mask: NaN, as mse_loss
    out[0] = (float)(-10.0 * log10(mse));
    out[1] = (float)(-10.0 * log10(masked_mse));
    out[2] = (float)(total[3] / total[2]);
    if (count) count[0] = (int)total[2];
  }
}

__global__ void __launch_bounds__(kThreads)
mask_apply_kernel(const unsigned char* __restrict__ mask, long long n_pix, const float* __restrict__ depth,
                  const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ depth_out,
                  float* __restrict__ a_out, float* __restrict__ b_out) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < n_pix; p += (long long)gridDim.x * kThreads) {
    const bool keep = mask[p] != 0;
    if (depth_out) depth_out[p] = keep ? depth[p] : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (a_out) a_out[3 * p + c] = keep ? a[3 * p + c] : 0.f;
      if (b_out) b_out[3 * p + c] = keep ? b[3 * p + c] : 0.f;
    }
  }
}

inline int tiles_of(int h, int w) { return ((w - (kWin - 1) + kTW - 1) / kTW) * ((h - (kWin - 1) + kTH - 1) / kTH); }

// the sizes of the pyramid; false when a level is smaller than the window
bool make_pyramid(int H, int W, int levels, Pyramid* pyr) {
  static const double weights[kMaxLevels] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  if (levels < 1 || levels > kMaxLevels || H <= 0 || W <= 0) return false;
  pyr->levels = levels;
  long long off = 0;
  int h = H, w = W;
  for (int l = 0; l < levels; ++l) {
    if (h < kWin || w < kWin) return false;
    pyr->h[l] = h;
    pyr->w[l] = w;
    pyr->blocks[l] = tiles_of(h, w);
    pyr->offset[l] = off;
    pyr->weight[l] = weights[l];
    off += 6LL * pyr->blocks[l];
    h = (h + 1) / 2;
    w = (w + 1) / 2;
  }
  return true;
}

// floats of one image of level l, rounded up to an even count (the next image stays 8-byte aligned)
inline size_t level_floats(const Pyramid& p, int l) { return (3 * (size_t)p.h[l] * p.w[l] + 1) & ~(size_t)1; }

inline int reduce_blocks(long long n_pix) { return capped_blocks(n_pix, kThreads); }

// the pooled images of levels 1.. : x then y of a level, float [3, h_l, w_l] each
struct LevelImages {
  float *x[kMaxLevels], *y[kMaxLevels];
};
inline LevelImages take_images(Carver& c, const Pyramid& p) {
  LevelImages m = {};
  for (int l = 1; l < p.levels; ++l) {
    m.x[l] = c.take<float>(level_floats(p, l));
    m.y[l] = c.take<float>(level_floats(p, l));
  }
  return m;
}

// workspace: partials double [sum over levels of 3 * blocks * 2] (level l at pyr.offset[l]) | the images of levels 1..
struct SsimWs {
  Carver c;
  Pyramid pyr;
  double* partial = c.take<double>(pyr.offset[pyr.levels - 1] + 6 * (size_t)pyr.blocks[pyr.levels - 1]);
  LevelImages img = take_images(c, pyr);
};

}  // namespace

extern "C" size_t glorie_ms_ssim_workspace(int H, int W, int levels) {
  Pyramid pyr;
  return make_pyramid(H, W, levels, &pyr) ? carved_bytes<SsimWs>(pyr) : 0;
}

extern "C" int glorie_ms_ssim(const float* x, const float* y, int H, int W, int channels_first, int levels,
                              void* workspace, float* out, void* stream) {
  Pyramid pyr;
  if (!x || !y || !workspace || !out) return GLORIE_EINVAL;
  if (!make_pyramid(H, W, levels, &pyr)) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  Window win;
  double sum = 0.0;
  for (int i = 0; i < kWin; ++i) {
    const double d = (double)(i - kWin / 2);
    win.g[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += win.g[i];
  }
  for (int i = 0; i < kWin; ++i) win.g[i] /= sum;
  const SsimWs ws{Carver(workspace), pyr};
  double* partial = ws.partial;
  const float *cx = x, *cy = y;
  int hwc = channels_first ? 0 : 1;
  for (int l = 0; l < levels; ++l) {
    const bool last = l == levels - 1;
    float* nx = last ? nullptr : ws.img.x[l + 1];
    float* ny = last ? nullptr : ws.img.y[l + 1];
    const dim3 grid((pyr.w[l] - (kWin - 1) + kTW - 1) / kTW, (pyr.h[l] - (kWin - 1) + kTH - 1) / kTH, last ? 3 : 6);
    hipLaunchKernelGGL(ms_ssim_level_kernel, grid, dim3(kThreads), 0, st, cx, cy, pyr.h[l], pyr.w[l], hwc, win,
                       partial + pyr.offset[l], nx, ny);
    GLORIE_TRY(check_launch());
    if (!last) {
      cx = nx;
      cy = ny;
      hwc = 0;
    }
  }
  hipLaunchKernelGGL(ms_ssim_finish_kernel, dim3(1), dim3(kThreads), 0, st, partial, pyr, out);
  return check_launch();
}

extern "C" size_t glorie_frame_reduce_workspace(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  return 4 * (size_t)reduce_blocks((long long)H * W) * sizeof(double);
}

extern "C" int glorie_frame_reduce(const float* color_a, const float* color_b, int H, int W, const unsigned char* mask,
                                   const float* depth, const float* gt_depth, void* workspace, float* out, int* count,
                                   void* stream) {
  if (H <= 0 || W <= 0 || !color_a || !color_b || !workspace || !out) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long long n_pix = (long long)H * W;
  const int blocks = reduce_blocks(n_pix);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(frame_reduce_kernel, dim3(blocks), dim3(kThreads), 0, st, color_a, color_b, n_pix, mask, depth,
                     gt_depth, partial);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(frame_finish_kernel, dim3(1), dim3(kThreads), 0, st, partial, blocks, n_pix, out, count);
  return check_launch();
}

extern "C" int glorie_mask_apply(const unsigned char* mask, int H, int W, const float* depth, const float* color_a,
                                 const float* color_b, float* depth_out, float* color_a_out, float* color_b_out,
                                 void* stream) {
  if (H <= 0 || W <= 0 || !mask) return GLORIE_EINVAL;
  if ((depth_out && !depth) || (color_a_out && !color_a) || (color_b_out && !color_b)) return GLORIE_EINVAL;
  const long long n_pix = (long long)H * W;
  hipLaunchKernelGGL(mask_apply_kernel, dim3(reduce_blocks(n_pix)), dim3(kThreads), 0, (hipStream_t)stream, mask, n_pix,
                     depth, color_a, color_b, depth_out, color_a_out, color_b_out);
  return check_launch();
}
