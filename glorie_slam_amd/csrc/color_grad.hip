// Colour-gradient pieces of the mapper: the dynamic search radii and the gradient-ranked pixel draw
// (reference: src/mapper.py:767-784 Mapper.run's radius block, src/utils/common.py:96-186 get_sample_uv_with_grad).
//
// Gradient maps, one launch (color_grad_maps_kernel): a 16x16 tile per workgroup with a one-pixel halo of gray values in
// LDS (each halo pixel converted once).  Gray is rgb . [0.2125, 0.7154, 0.0721] in fp32 (skimage.color.rgb2gray, a
// fused multiply-add chain as numpy's float32 matmul has it); the
// Sobel responses are scipy.ndimage.convolve with [1,0,-1] x [1,2,1]/4, mode='reflect' (index -1 reads 0, index H reads
// H-1, border pixels not zeroed), the six products summed in double and rounded once to fp32 as scipy does; the magnitude
// is sqrt(gx^2 + gy^2) with every fp32 operation rounded on its own (no fused multiply-add), as numpy does.  The radii are
// interp1d([0, 0.01, thr], [rmax, rmax, rmin]) of the magnitude clipped to [0, float32(thr)], evaluated in double.
//
// Top-M selection, 12 launches whatever the data (records into a hipGraph), no host synchronisation:
//   topm_init_kernel         the bins cleared, the rank M-1 from the top
//   radix_hist_kernel x4     radix select of the M-th largest key over order-preserving uint keys, 8 bits per pass:
//                            LDS bins, then one global integer atomic per bin and workgroup (radix.hiph)
//   topm_pick_kernel x4      one wave: the bin holding the M-th largest key, the narrowed prefix, the histogram cleared
//   topm_count_kernel        per workgroup: keys above the threshold key, keys equal to it, keys >= 0 (wave ballots)
//   topm_scan_kernel         one workgroup: exclusive scans of the three counts, the valid count of the selection
//   topm_write_kernel        every key above the threshold and the lowest-index `M - above` keys equal to it, written in
//                            ascending index order
// The float keys and the count, scan and rank steps are those of compact.hiph, the select's passes those of radix.hiph.
// Every decision is an integer count: repeated calls are bitwise equal.
#include "radix.hiph"

using namespace glorie;

namespace {

constexpr int kTile = 16;                 // output tile edge
constexpr int kHalo = kTile + 2;
constexpr int kTopThreads = 256;
constexpr int kTopWaves = kTopThreads / 64;
constexpr int kHistItems = 8;             // keys per thread in a histogram pass

struct RadiusMap {
  double g_lo;                            // 0.01, the end of the flat segment
  double thr;                             // the last interpolation node
  float thr_f;                            // float32(thr): where numpy clips a float32 magnitude
  double y_hi, slope;                     // rmax, (rmin - rmax) / (thr - 0.01)
};

// interp1d's linear branch (searchsorted(x, x_new, 'left') clipped to [1, 2], slope * (x_new - x_lo) + y_lo)
__device__ __forceinline__ double radius_of(const RadiusMap& m, float g) {
  const double x = (double)fminf(fmaxf(g, 0.f), m.thr_f);
  if (x <= m.g_lo) return m.y_hi;                             // slope 0 on [0, 0.01]
  return __dadd_rn(__dmul_rn(m.slope, __dsub_rn(x, m.g_lo)), m.y_hi);
}

__device__ __forceinline__ float gray_at(const float* __restrict__ img, int H, int W, int chw, int y, int x) {
  // scipy 'reflect' for a one-pixel reach: -1 -> 0, H -> H-1
  y = y < 0 ? 0 : (y >= H ? H - 1 : y);
  x = x < 0 ? 0 : (x >= W ? W - 1 : x);
  const size_t p = (size_t)y * W + x;
  float r, g, b;
  if (chw) {
    const size_t hw = (size_t)H * W;
    r = img[p];
    g = img[hw + p];
    b = img[2 * hw + p];
  } else {
    r = img[3 * p];
    g = img[3 * p + 1];
    b = img[3 * p + 2];
  }
  // numpy's float32 `rgb @ coeffs` accumulates as a fused multiply-add chain
  return __fmaf_rn(b, 0.0721f, __fmaf_rn(g, 0.7154f, __fmul_rn(r, 0.2125f)));
}

__global__ void __launch_bounds__(kTile * kTile)
color_grad_maps_kernel(const float* __restrict__ img, int H, int W, int chw, const unsigned char* __restrict__ valid,
                       RadiusMap add, RadiusMap query, const float* __restrict__ depth_add,
                       const float* __restrict__ depth_query, float* __restrict__ grad, float* __restrict__ r_add,
                       float* __restrict__ r_query) {
  __shared__ float tile[kHalo][kHalo + 1];
  const int x0 = blockIdx.x * kTile - 1, y0 = blockIdx.y * kTile - 1;
  const int tid = threadIdx.y * kTile + threadIdx.x;
  for (int e = tid; e < kHalo * kHalo; e += kTile * kTile) {
    const int ly = e / kHalo, lx = e - ly * kHalo;
    tile[ly][lx] = gray_at(img, H, W, chw, y0 + ly, x0 + lx);
  }
  __syncthreads();
  const int x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
  if (x >= W || y >= H) return;
  const int tx = threadIdx.x + 1, ty = threadIdx.y + 1;
  // sobel_h (along rows) and sobel_v (along columns); scipy's convolve flips the kernel, which only changes the sign
  double gy = 0.0, gx = 0.0;
  gy += 0.25 * (double)tile[ty + 1][tx - 1];
  gy += 0.5 * (double)tile[ty + 1][tx];
  gy += 0.25 * (double)tile[ty + 1][tx + 1];
  gy -= 0.25 * (double)tile[ty - 1][tx - 1];
  gy -= 0.5 * (double)tile[ty - 1][tx];
  gy -= 0.25 * (double)tile[ty - 1][tx + 1];
  gx += 0.25 * (double)tile[ty - 1][tx + 1];
  gx += 0.5 * (double)tile[ty][tx + 1];
  gx += 0.25 * (double)tile[ty + 1][tx + 1];
  gx -= 0.25 * (double)tile[ty - 1][tx - 1];
  gx -= 0.5 * (double)tile[ty][tx - 1];
  gx -= 0.25 * (double)tile[ty + 1][tx - 1];
  const float fx = (float)gx, fy = (float)gy;
  const float g = __fsqrt_rn(__fadd_rn(__fmul_rn(fx, fx), __fmul_rn(fy, fy)));
  const size_t p = (size_t)y * W + x;
  if (grad) grad[p] = (valid && valid[p] == 0) ? -1.f : g;
  if (r_add) {
    const double r = radius_of(add, g);
    r_add[p] = (float)(depth_add ? __dmul_rn(__ddiv_rn(r, 3.0), (double)depth_add[p]) : r);
  }
  if (r_query) {
    const double r = radius_of(query, g);
    r_query[p] = (float)(depth_query ? __dmul_rn(__ddiv_rn(r, 3.0), (double)depth_query[p]) : r);
  }
}

// state: [0] prefix of the threshold key, [1] rank still to skip from the top inside the prefix, [2] need (ties taken),
// [3] -
__global__ void __launch_bounds__(256)
topm_init_kernel(unsigned int* __restrict__ hist, unsigned int* __restrict__ state, int M) {
  hist[threadIdx.x] = 0u;
  if (threadIdx.x < 4) state[threadIdx.x] = threadIdx.x == 1 ? (unsigned int)(M - 1) : 0u;
}

// one wave: find the bin holding the rank-th largest key counted from the top, narrow the prefix, clear the bins
__global__ void __launch_bounds__(64)
topm_pick_kernel(unsigned int* __restrict__ state, unsigned int* __restrict__ hist, int pass) {
  __shared__ unsigned int bins[256];
  const BinPick p = bin_pick_global(hist, bins, state[1], true);
  if (threadIdx.x == 0) {
    state[1] = p.rank;
    state[0] |= p.digit << (8 * pass);
  }
}

__global__ void __launch_bounds__(kTopThreads)
topm_count_kernel(const float* __restrict__ keys, int n, const unsigned int* __restrict__ state,
                  int* __restrict__ cnt_gt, int* __restrict__ cnt_eq, int* __restrict__ cnt_nonneg) {
  __shared__ int red[3][kTopWaves];
  const unsigned int t = state[0];
  const int i = blockIdx.x * kTopThreads + threadIdx.x;
  const float f = i < n ? keys[i] : -1.f;
  const unsigned int k = float_key(f);
  const bool in = i < n;
  wave_count(in && k > t, red[0]);
  wave_count(in && k == t, red[1]);
  wave_count(in && f >= 0.f, red[2]);
  __syncthreads();
  if (threadIdx.x < 3) {
    int* cnt = threadIdx.x == 0 ? cnt_gt : threadIdx.x == 1 ? cnt_eq : cnt_nonneg;
    cnt[blockIdx.x] = slot_sum(red[threadIdx.x], kTopWaves);
  }
}

// one workgroup: exclusive scans of cnt_gt and cnt_eq in place; state[2] = M - (keys above the threshold);
// valid[0] = min(M, keys >= 0)
__global__ void __launch_bounds__(kScanThreads)
topm_scan_kernel(int* cnt_gt, int* cnt_eq, const int* __restrict__ cnt_nonneg, int n_blocks, int M,
                 unsigned int* __restrict__ state, int* __restrict__ valid) {
  const int* const in[2] = {cnt_gt, cnt_eq};
  int* const out[2] = {cnt_gt, cnt_eq};
  int above_equal[2];
  block_exclusive_scan<2>(in, out, n_blocks, above_equal);
  int nn = 0;
  for (int b = threadIdx.x; b < n_blocks; b += kScanThreads) nn += cnt_nonneg[b];
  nn = block_sum<kScanThreads / 64>(nn);
  if (threadIdx.x == 0) {
    state[2] = (unsigned int)(M - above_equal[0]);
    valid[0] = min(M, nn);
  }
}

__global__ void __launch_bounds__(kTopThreads)
topm_write_kernel(const float* __restrict__ keys, int n, const unsigned int* __restrict__ state,
                  const int* __restrict__ off_gt, const int* __restrict__ off_eq, int M, int64_t* __restrict__ out) {
  __shared__ int wg[kTopWaves], we[kTopWaves];
  const unsigned int t = state[0];
  const int need = (int)state[2];
  const int i = blockIdx.x * kTopThreads + threadIdx.x;
  const unsigned int k = i < n ? float_key(keys[i]) : 0u;
  const bool gt = i < n && k > t, eq = i < n && k == t;
  const unsigned long long bg = wave_count(gt, wg), be = wave_count(eq, we);
  __syncthreads();
  const int g = off_gt[blockIdx.x] + block_rank(bg, wg), e = off_eq[blockIdx.x] + block_rank(be, we);
  // position = selected keys of lower index: every key above the threshold, the first `need` ties
  const int pos = g + min(e, need);
  if ((gt || (eq && e < need)) && pos >= 0 && pos < M) out[pos] = i;
}

inline int top_blocks(int n) { return (n + kTopThreads - 1) / kTopThreads; }

RadiusMap make_map(double rmax, double rmin, double thr) {
  RadiusMap m;
  m.g_lo = 0.01;
  m.thr = thr;
  m.thr_f = (float)thr;
  m.y_hi = rmax;
  m.slope = (rmin - rmax) / (thr - 0.01);
  return m;
}

// workspace: hist uint [256] | state uint [4] | cnt_gt, cnt_eq, cnt_nonneg int [B] each
struct TopmWs {
  Carver c;
  int n;
  unsigned int* hist = c.take<unsigned int>(256);
  unsigned int* state = c.take<unsigned int>(4);
  int* cnt_gt = c.take<int>(top_blocks(n));
  int* cnt_eq = c.take<int>(top_blocks(n));
  int* cnt_nn = c.take<int>(top_blocks(n));
};

}  // namespace

extern "C" int glorie_color_grad_maps(const float* image, int H, int W, int channels_first,
                                      const unsigned char* valid, double color_grad_threshold, double radius_add_max,
                                      double radius_add_min, double radius_query_ratio, const float* depth_add,
                                      const float* depth_query, float* grad, float* r_add, float* r_query,
                                      void* stream) {
  if (H <= 0 || W <= 0 || !image) return GLORIE_EINVAL;
  if (!(color_grad_threshold > 0.01)) return GLORIE_EINVAL;     // interp1d needs 0 < 0.01 < thr
  if (!grad && !r_add && !r_query) return GLORIE_OK;
  const RadiusMap add = make_map(radius_add_max, radius_add_min, color_grad_threshold);
  const RadiusMap query = make_map(radius_query_ratio * radius_add_max, radius_query_ratio * radius_add_min,
                                   color_grad_threshold);
  const dim3 grid((W + kTile - 1) / kTile, (H + kTile - 1) / kTile);
  hipLaunchKernelGGL(color_grad_maps_kernel, grid, dim3(kTile, kTile), 0, (hipStream_t)stream, image, H, W,
                     channels_first ? 1 : 0, valid, add, query, depth_add, depth_query, grad, r_add, r_query);
  return check_launch();
}

extern "C" size_t glorie_topm_workspace(int n) { return n < 0 ? 0 : carved_bytes<TopmWs>(n); }

extern "C" int glorie_topm(const float* keys, int n, int M, void* workspace, int64_t* indices, int* valid_count,
                           void* stream) {
  if (n < 0 || M < 0 || !valid_count) return GLORIE_EINVAL;
  if (M > n) return GLORIE_EINVAL;                              // np.argpartition(kth=-M) raises
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return check_hip(hipMemsetAsync(valid_count, 0, sizeof(int), st));
  if (!keys || !workspace || !indices) return GLORIE_EINVAL;
  const int B = top_blocks(n);
  const TopmWs w{Carver(workspace), n};
  // state = {prefix 0, rank M-1 from the top, -, -}, bins cleared
  hipLaunchKernelGGL(topm_init_kernel, dim3(1), dim3(256), 0, st, w.hist, w.state, M);
  GLORIE_TRY(check_launch());
  const int hb = (n + kHistThreads * kHistItems - 1) / (kHistThreads * kHistItems);
  for (int pass = 3; pass >= 0; --pass) {
    hipLaunchKernelGGL(radix_hist_kernel<FloatKeys>, dim3(hb), dim3(kHistThreads), 0, st, FloatKeys{keys}, n, pass,
                       w.state, 0, w.hist);
    GLORIE_TRY(check_launch());
    hipLaunchKernelGGL(topm_pick_kernel, dim3(1), dim3(64), 0, st, w.state, w.hist, pass);
    GLORIE_TRY(check_launch());
  }
  hipLaunchKernelGGL(topm_count_kernel, dim3(B), dim3(kTopThreads), 0, st, keys, n, w.state, w.cnt_gt, w.cnt_eq,
                     w.cnt_nn);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(topm_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, w.cnt_gt, w.cnt_eq, w.cnt_nn, B, M, w.state,
                     valid_count);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(topm_write_kernel, dim3(B), dim3(kTopThreads), 0, st, keys, n, w.state, w.cnt_gt, w.cnt_eq, M,
                     indices);
  return check_launch();
}
