// Adjoints of the correlation lookups for gfx950: what CorrSampler.backward and CorrLayer.backward call.
//
// Replaces droid_backends.corr_index_backward (src/lib/correlation_kernels.cu:73-124,157-185) and
// droid_backends.altcorr_backward (src/lib/altcorr_kernel.cu:153-286,321-356); the pyramid form
// is the adjoint of glorie_corr_lookup_pyramid (corr.hip).
//
// Index / pyramid backward.  Source pixel (n, y, x) OWNS its plane volume_grad[n][y][x][:][:]: one wave writes the whole
// plane, zeros included, in one pass of 16-byte stores (scalar stores only for the < 16-byte head and tail of a plane
// whose address is not 16-byte aligned).  No memset, no read-modify-write, no atomics: the launch is a pure write stream
// of N h1 w1 h2 w2 sizeof bytes and its result is bitwise repeatable.  The <= (2r+2)^2 non-zero elements of a plane are
// the window taps; tap (i, j) at (floor(x0) - r + i, floor(y0) - r + j) receives, in the reference's order,
//     g[i-1][j-1] dx dy + g[i-1][j] dx (1-dy) + g[i][j-1] (1-dx) dy + g[i][j] (1-dx)(1-dy)      (terms that exist),
// g[i][j] = corr_grad[n][i][j][y][x] (x-offset major, as the forward writes it).  A tap outside the plane has no element
// and so contributes nothing - the forward skipped it.
// Numerics: weights, products and the <= 4-term sum are fp32 for both dtypes; an fp16 result is rounded ONCE, at the
// store.  The reference evaluates every step in half; this kernel is therefore closer to the exact adjoint and is not
// bit-identical to the reference's half sequence.
// Coordinates are finite by contract; floor(x0) is clamped to +-2^30 before the integer conversion, so huge finite
// coordinates name a window far outside the plane and write zeros only.
//
// alt-corr backward (fp32 only, as the reference dispatches it; the adjoint of glorie_altcorr_fwd of altcorr.hip, channel
// (iy-1) + rd (ix-1)).  With t = g_tap(s, ix, iy) the same four-term sum as above (dx <-> ix, dy <-> iy):
//   fmap1_grad[b][h][w][:] = sum over s and in-bounds taps of t * fmap2[b][tap][:]   - owned by its source pixel: one wave,
//       register accumulation in a fixed order, one plain store; bitwise repeatable;
//   fmap2_grad[b][tap][:] += t * fmap1[b][h][w][:]                                   - a scatter: the caller zero-fills,
//       the kernel adds with float atomics.  A workgroup takes a 4 x 4 source tile and one s.  Over the bounding box of the
//       tile's 16 windows (neighbouring windows overlap almost entirely under smooth flow: 11 x 11 targets instead of 1024
//       taps) it writes the tap gradients into an LDS table [target][pixel], multiplies the table with the tile's 16 feature
//       rows held in registers - row[target][:] = sum_p table[target][p] fmap1[p][:], no LDS accumulation, no LDS atomics -
//       and issues ONE global atomic row add per touched target: C contiguous floats, 256 contiguous bytes per wave
//       instruction.  A tile whose box holds more than kMaxSlots targets (scattered coordinates) falls back to one atomic
//       row per tap.
//   Because of the float atomics fmap2_grad is NOT bitwise repeatable on general data: the order of the adds is free.  It is
//   where every partial sum is exact.  Coordinates get no gradient (the reference returns zeros).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/glorie_hip.h"
#include "common.hiph"

namespace glorie {

constexpr int kBwdLevels = 4;
constexpr int kBwdMaxRadius = 7;                                   // (2r+2)^2 <= 256 window taps
constexpr int kBwdMaxTaps = (2 * kBwdMaxRadius + 2) * (2 * kBwdMaxRadius + 2);
constexpr float kCoordClamp = 1073741824.0f;                       // 2^30

struct BwdLevels {
  void* grad[kBwdLevels];
  int h2[kBwdLevels];
  int w2[kBwdLevels];
};

// window origin floor(c) - r (clamped, see above) and the fraction c - floor(c)
__device__ __forceinline__ int window_origin(float c, int r, float& frac) {
  const float f = floorf(c);
  frac = c - f;
  return static_cast<int>(fminf(fmaxf(f, -kCoordClamp), kCoordClamp)) - r;
}

// the four-term sum of tap (i, j), i <-> x, from the (2r+1)^2 gradients g[i * rd + j] of one source pixel
__device__ __forceinline__ float tap_grad(const float* g, int i, int j, int rd, float dx, float dy) {
  float t = 0.0f;
  if (i > 0 && j > 0) t += g[(i - 1) * rd + (j - 1)] * (dx * dy);
  if (i > 0 && j < rd) t += g[(i - 1) * rd + j] * (dx * (1.0f - dy));
  if (i < rd && j > 0) t += g[i * rd + (j - 1)] * ((1.0f - dx) * dy);
  if (i < rd && j < rd) t += g[i * rd + j] * ((1.0f - dx) * (1.0f - dy));
  return t;
}

template <typename T> struct __attribute__((aligned(16))) Vec16 { T v[16 / sizeof(T)]; };

// element e of a plane of width w2: the tap gradient if (e / w2, e % w2) lies in the window, else zero
__device__ __forceinline__ float plane_value(const float* taps, int ty, int tx, int ix0, int iy0, int rd) {
  const unsigned i = (unsigned)tx - (unsigned)ix0, j = (unsigned)ty - (unsigned)iy0;
  return (i <= (unsigned)rd && j <= (unsigned)rd) ? taps[i * (rd + 1) + j] : 0.0f;
}

// 256 threads = 4 waves = 4 consecutive source pixels; grid (ceil(N h1 w1 / 4), levels)
template <typename T>
__global__ __launch_bounds__(256) void corr_index_bwd_kernel(BwdLevels lv, int scale_coords, const float* __restrict__ coords,
                                                             const T* __restrict__ grad, long long NP, int HW, int radius,
                                                             int grad_channels) {
  __shared__ float gbuf[4][(2 * kBwdMaxRadius + 1) * (2 * kBwdMaxRadius + 1)];
  __shared__ float taps[4][kBwdMaxTaps];
  constexpr int VEC = 16 / sizeof(T);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l = blockIdx.y;
  const long long pix = (long long)blockIdx.x * 4 + wv;           // n * HW + p
  const bool live = pix < NP;                                     // wave-uniform
  const int rd = 2 * radius + 1, rt = rd + 1;
  const int h2 = lv.h2[l], w2 = lv.w2[l];
  const int plane = h2 * w2;
  int ix0 = 0, iy0 = 0;
  float dx = 0.0f, dy = 0.0f;
  if (live) {
    const long long n = pix / HW;
    const int p = (int)(pix - n * HW);
    const float inv = scale_coords ? 1.0f / (float)(1 << l) : 1.0f;
    ix0 = window_origin(coords[((size_t)n * 2 + 0) * HW + p] * inv, radius, dx);
    iy0 = window_origin(coords[((size_t)n * 2 + 1) * HW + p] * inv, radius, dy);
    const T* gp = grad + ((size_t)n * grad_channels + (size_t)l * rd * rd) * HW + p;
    for (int c = lane; c < rd * rd; c += 64) gbuf[wv][c] = (float)gp[(size_t)c * HW];
  }
  __syncthreads();
  if (live)
    for (int t = lane; t < rt * rt; t += 64) taps[wv][t] = tap_grad(gbuf[wv], t / rt, t % rt, rd, dx, dy);
  __syncthreads();
  if (!live || plane == 0) return;

  T* pl = reinterpret_cast<T*>(lv.grad[l]) + (size_t)pix * (size_t)plane;
  const float* tp = taps[wv];
  // flat element range that holds the window rows: everything outside is zero without any index arithmetic
  const long long lo = (long long)iy0 * w2, hi = ((long long)iy0 + rt) * w2;
  const int head = min(plane, (int)(((16 - (reinterpret_cast<uintptr_t>(pl) & 15)) & 15) / sizeof(T)));
  const int nvec = (plane - head) / VEC;
  const int tail = head + nvec * VEC;
  if (lane < head) pl[lane] = (T)plane_value(tp, lane / w2, lane % w2, ix0, iy0, rd);
  for (int c = lane; c < nvec; c += 64) {
    const int e = head + c * VEC;
    Vec16<T> o;
    if (e + VEC <= lo || e >= hi) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) o.v[k] = (T)0.0f;
    } else {
      int ty = e / w2, tx = e - ty * w2;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        o.v[k] = (T)plane_value(tp, ty, tx, ix0, iy0, rd);
        if (++tx == w2) { tx = 0; ++ty; }
      }
    }
    *reinterpret_cast<Vec16<T>*>(pl + e) = o;
  }
  if (tail + lane < plane) {                                       // fewer than VEC <= 8 elements
    const int e = tail + lane;
    pl[e] = (T)plane_value(tp, e / w2, e % w2, ix0, iy0, rd);
  }
}

template <typename T>
static int launch_index_bwd(const BwdLevels& lv, int num_levels, int scale, const float* coords, const void* grad, int N,
                            int h1, int w1, int radius, hipStream_t st) {
  const long long NP = (long long)N * h1 * w1;
  const long long blocks = (NP + 3) / 4;
  if (blocks > 0x7fffffffLL) return GLORIE_EUNSUPPORTED;
  const int rd = 2 * radius + 1;
  hipLaunchKernelGGL(corr_index_bwd_kernel<T>, dim3((unsigned)blocks, num_levels), dim3(256), 0, st, lv, scale, coords,
                     reinterpret_cast<const T*>(grad), NP, h1 * w1, radius, num_levels * rd * rd);
  return check_launch();
}

static int index_bwd(const float* coords, const void* grad, void* const* volume_grads, int num_levels, int scale, int N,
                     int h1, int w1, int h2, int w2, int radius, int dtype, void* stream) {
  if (num_levels < 1 || num_levels > kBwdLevels || N < 0 || h1 < 0 || w1 < 0 || h2 < 0 || w2 < 0 || radius < 0)
    return GLORIE_EINVAL;
  if (dtype != GLORIE_F16 && dtype != GLORIE_F32) return GLORIE_EUNSUPPORTED;
  if (radius > kBwdMaxRadius) return GLORIE_EUNSUPPORTED;
  if (N == 0 || h1 * w1 == 0) return GLORIE_OK;
  if (!coords || !grad || !volume_grads) return GLORIE_EINVAL;
  const size_t esize = dtype == GLORIE_F16 ? 2 : 4;
  BwdLevels lv{};
  for (int l = 0; l < num_levels; ++l) {
    lv.h2[l] = h2 >> l;
    lv.w2[l] = w2 >> l;
    lv.grad[l] = volume_grads[l];
    if ((long long)lv.h2[l] * lv.w2[l] > 0x7fffffffLL) return GLORIE_EUNSUPPORTED;
    if (lv.h2[l] * lv.w2[l] > 0 && (!lv.grad[l] || (reinterpret_cast<uintptr_t>(lv.grad[l]) & (esize - 1)))) return GLORIE_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == GLORIE_F16) return launch_index_bwd<_Float16>(lv, num_levels, scale, coords, grad, N, h1, w1, radius, st);
  return launch_index_bwd<float>(lv, num_levels, scale, coords, grad, N, h1, w1, radius, st);
}

// ---- alt-corr backward -----------------------------------------------------------------------------------------------
constexpr int kAltTile = 4;                   // source tile 4 x 4
constexpr int kMaxSlots = 400;                // box targets of a tile: 11 x 11 under identity flow, up to 20 x 20 when stretched

__device__ __forceinline__ float lane_bcast(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}
__device__ __forceinline__ int lane_bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }

// gradients of the (2r+1)^2 outputs of (b, s, pixel p): corr_grad[b][s][c][p], c = iy + rd ix
struct AltTap { float t; int h2, w2; bool inb; };
// tap `k` = ix * (rd + 1) + iy of the window of a pixel at (x0, y0)
__device__ __forceinline__ AltTap alt_tap(const float* __restrict__ g, size_t HW, int k, int radius, float x0, float y0, int H2,
                                          int W2) {
  const int rd = 2 * radius + 1, rt = rd + 1;
  const int ix = k / rt, iy = k - ix * rt;
  float dx, dy;
  const int ox = window_origin(x0, radius, dx), oy = window_origin(y0, radius, dy);
  AltTap a;
  a.w2 = ox + ix;
  a.h2 = oy + iy;
  a.inb = a.h2 >= 0 && a.h2 < H2 && a.w2 >= 0 && a.w2 < W2;
  float t = 0.0f;
  if (a.inb) {       // channel = (row offset) + rd * (column offset), see altcorr_generic_kernel
    if (iy > 0 && ix > 0) t += g[(size_t)((iy - 1) + rd * (ix - 1)) * HW] * (dy * dx);
    if (iy > 0 && ix < rd) t += g[(size_t)((iy - 1) + rd * ix) * HW] * (dy * (1.0f - dx));
    if (iy < rd && ix > 0) t += g[(size_t)(iy + rd * (ix - 1)) * HW] * ((1.0f - dy) * dx);
    if (iy < rd && ix < rd) t += g[(size_t)(iy + rd * ix) * HW] * ((1.0f - dy) * (1.0f - dx));
  }
  a.t = t;
  return a;
}

// fmap1_grad: one wave per source pixel, 128 channels at a time (two per lane) over all s and taps in a fixed order.
// grid (ceil(HW / 4), B)
__global__ __launch_bounds__(256) void altcorr_bwd_f1_kernel(const float* __restrict__ fmap2, const float* __restrict__ coords,
                                                             const float* __restrict__ corr_grad, float* __restrict__ fmap1_grad,
                                                             int S, int H, int W, int H2, int W2, int C, int radius) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int HW = H * W;
  const int b = blockIdx.y;
  const int p = blockIdx.x * 4 + wv;
  if (p >= HW) return;                                             // wave-uniform, no barrier below
  const int rd = 2 * radius + 1, ntap = (rd + 1) * (rd + 1);
  for (int c0 = 0; c0 < C; c0 += 128) {
    const int ca = c0 + lane, cb = c0 + 64 + lane;
    float acc_a = 0.0f, acc_b = 0.0f;
    for (int s = 0; s < S; ++s) {
      const size_t e = ((size_t)b * S + s) * HW + p;
      const float x0 = coords[e * 2 + 0], y0 = coords[e * 2 + 1];
      const float* g = corr_grad + ((size_t)b * S + s) * rd * rd * HW + p;
      for (int k0 = 0; k0 < ntap; k0 += 64) {
        AltTap a{0.0f, 0, 0, false};
        if (k0 + lane < ntap) a = alt_tap(g, HW, k0 + lane, radius, x0, y0, H2, W2);
        const int row = a.inb ? a.h2 * W2 + a.w2 : -1;
        const int kn = min(64, ntap - k0);
        for (int k = 0; k < kn; ++k) {
          const int r = lane_bcast(row, k);
          if (r < 0) continue;                                     // wave-uniform
          const float t = lane_bcast(a.t, k);
          const float* f2 = fmap2 + ((size_t)b * H2 * W2 + r) * C;
          if (ca < C) acc_a = fmaf(t, f2[ca], acc_a);
          if (cb < C) acc_b = fmaf(t, f2[cb], acc_b);
        }
      }
    }
    float* o = fmap1_grad + ((size_t)b * HW + p) * C;
    if (ca < C) o[ca] = acc_a;
    if (cb < C) o[cb] = acc_b;
  }
}

// fmap2_grad: one workgroup per (4 x 4 source tile, s, b); wave w serves tile row w.  grid (tiles, S, B)
__global__ __launch_bounds__(256) void altcorr_bwd_f2_kernel(const float* __restrict__ fmap1, const float* __restrict__ coords,
                                                             const float* __restrict__ corr_grad, float* __restrict__ fmap2_grad,
                                                             int S, int H, int W, int H2, int W2, int C, int radius) {
  __shared__ __attribute__((aligned(16))) float taps[kMaxSlots][kAltTile * kAltTile];   // [box slot][tile pixel]: 25 KB
  __shared__ unsigned touched[(kMaxSlots + 31) / 32];
  __shared__ int org[2][kAltTile * kAltTile];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int HW = H * W;
  const int tiles_x = (W + kAltTile - 1) / kAltTile;
  const int ty0 = (blockIdx.x / tiles_x) * kAltTile, tx0 = (blockIdx.x % tiles_x) * kAltTile;
  const int s = blockIdx.y, b = blockIdx.z;
  const int rd = 2 * radius + 1, ntap = (rd + 1) * (rd + 1);
  const size_t e0 = ((size_t)b * S + s) * HW;

  // the box of the tile's window origins (pixels outside the map do not count)
  if (tid < kAltTile * kAltTile) {
    const int y = ty0 + tid / kAltTile, x = tx0 + tid % kAltTile;
    int ox = 0x7fffffff, oy = 0x7fffffff;                          // marks a pixel outside the map
    if (y < H && x < W) {
      float f;
      ox = window_origin(coords[(e0 + (size_t)y * W + x) * 2 + 0], radius, f);
      oy = window_origin(coords[(e0 + (size_t)y * W + x) * 2 + 1], radius, f);
    }
    org[0][tid] = ox;
    org[1][tid] = oy;
  }
  if (tid < (kMaxSlots + 31) / 32) touched[tid] = 0u;
  __syncthreads();
  int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = -0x7fffffff, by1 = -0x7fffffff;
  for (int q = 0; q < kAltTile * kAltTile; ++q) {
    const int ox = org[0][q], oy = org[1][q];
    if (ox == 0x7fffffff) continue;
    bx0 = min(bx0, ox); bx1 = max(bx1, ox);
    by0 = min(by0, oy); by1 = max(by1, oy);
  }
  const long long bw = (long long)bx1 - bx0 + rd + 1, bh = (long long)by1 - by0 + rd + 1;   // the tile has a live pixel
  const long long area = bw * bh;
  const bool boxed = area <= kMaxSlots;                            // workgroup-uniform
  constexpr int NP = kAltTile * kAltTile;
  if (boxed) {
    for (int i = tid; i < (int)area * NP; i += 256) (&taps[0][0])[i] = 0.0f;
    __syncthreads();
  }
  // pass 1, wave w = tile row w: the tap gradients of its pixels.  Boxed: into the table (a pixel has at most one tap per
  // target: plain stores).  Otherwise: one global atomic row per in-bounds tap.
  for (int q = 0; q < kAltTile; ++q) {
    const int y = ty0 + wv, x = tx0 + q;
    if (y >= H || x >= W) continue;                                // wave-uniform
    const int p = y * W + x;
    const float x0 = coords[(e0 + p) * 2 + 0], y0 = coords[(e0 + p) * 2 + 1];
    const float* g = corr_grad + ((size_t)b * S + s) * rd * rd * HW + p;
    const float* f1 = fmap1 + ((size_t)b * HW + p) * C;
    for (int k0 = 0; k0 < ntap; k0 += 64) {
      AltTap a{0.0f, 0, 0, false};
      if (k0 + lane < ntap) a = alt_tap(g, HW, k0 + lane, radius, x0, y0, H2, W2);
      if (boxed) {
        if (a.inb) {
          const int slot = (a.h2 - by0) * (int)bw + (a.w2 - bx0);
          taps[slot][wv * kAltTile + q] = a.t;
          atomicOr(&touched[slot >> 5], 1u << (slot & 31));
        }
        continue;
      }
      const int row = a.inb ? a.h2 * W2 + a.w2 : -1;
      const int kn = min(64, ntap - k0);
      for (int k = 0; k < kn; ++k) {
        const int r = lane_bcast(row, k);
        if (r < 0) continue;                                       // wave-uniform
        const float t = lane_bcast(a.t, k);
        float* o = fmap2_grad + ((size_t)b * H2 * W2 + r) * C;
        for (int c = lane; c < C; c += 64) atomicAdd(&o[c], t * f1[c]);
      }
    }
  }
  if (!boxed) return;
  __syncthreads();
  // pass 2: row[slot][:] = sum over the 16 pixels of taps[slot][pixel] * fmap1[pixel][:] - a [area x 16] x [16 x C] product with
  // the tile's features in registers (two channels per lane, 128 channels at a time) and the table row read as a broadcast -
  // and ONE atomic row per touched target: wave w takes slots w, w + 4, ...
  for (int c0 = 0; c0 < C; c0 += 128) {
    const int ca = c0 + lane, cb = c0 + 64 + lane;
    float fa[NP], fb[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int y = ty0 + q / kAltTile, x = tx0 + q % kAltTile;
      const bool in = y < H && x < W;                              // a pixel outside the map has a zero column
      const float* f1 = fmap1 + ((size_t)b * HW + (in ? y * W + x : 0)) * C;
      fa[q] = (in && ca < C) ? f1[ca] : 0.0f;
      fb[q] = (in && cb < C) ? f1[cb] : 0.0f;
    }
    for (int slot = wv; slot < (int)area; slot += 4) {
      if (!((touched[slot >> 5] >> (slot & 31)) & 1u)) continue;   // wave-uniform
      float sa = 0.0f, sb = 0.0f;
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const float t = taps[slot][q];
        sa = fmaf(t, fa[q], sa);
        sb = fmaf(t, fb[q], sb);
      }
      const int h2 = by0 + slot / (int)bw, w2 = bx0 + slot % (int)bw;   // in the map: only in-bounds taps set the bit
      float* o = fmap2_grad + (((size_t)b * H2 + h2) * W2 + w2) * C;
      if (ca < C) atomicAdd(&o[ca], sa);
      if (cb < C) atomicAdd(&o[cb], sb);
    }
  }
}

}  // namespace glorie

using namespace glorie;

extern "C" int glorie_corr_index_bwd(const float* coords, const void* corr_grad, void* volume_grad, int N, int h1, int w1,
                                     int h2, int w2, int radius, int dtype, void* stream) {
  void* levels[1] = {volume_grad};
  return index_bwd(coords, corr_grad, levels, 1, 0, N, h1, w1, h2, w2, radius, dtype, stream);
}

extern "C" int glorie_corr_lookup_pyramid_bwd(const float* coords, const void* grad, void* const* volume_grads,
                                              int num_levels, int N, int h1, int w1, int h2, int w2, int radius, int dtype,
                                              void* stream) {
  return index_bwd(coords, grad, volume_grads, num_levels, 1, N, h1, w1, h2, w2, radius, dtype, stream);
}

extern "C" int glorie_altcorr_bwd(const float* fmap1, const float* fmap2, const float* coords, const float* corr_grad,
                                  float* fmap1_grad, float* fmap2_grad, int B, int S, int H, int W, int H2, int W2, int C,
                                  int radius, void* stream) {
  if (B < 0 || S < 0 || H < 0 || W < 0 || H2 < 0 || W2 < 0 || C < 0 || radius < 0) return GLORIE_EINVAL;
  if (radius > kBwdMaxRadius) return GLORIE_EUNSUPPORTED;
  if (B == 0 || H * W == 0 || C == 0) return GLORIE_OK;
  if (!fmap1 || !fmap1_grad || (S > 0 && (!coords || !corr_grad))) return GLORIE_EINVAL;
  if (S > 0 && H2 * W2 > 0 && (!fmap2 || !fmap2_grad)) return GLORIE_EINVAL;
  if (S > 65535 || B > 65535) return GLORIE_EUNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int HW = H * W;
  // S == 0: the kernel still writes fmap1_grad (zeros)
  hipLaunchKernelGGL(altcorr_bwd_f1_kernel, dim3((HW + 3) / 4, B), dim3(256), 0, st, fmap2, coords, corr_grad, fmap1_grad, S,
                     H, W, H2, W2, C, radius);
  GLORIE_TRY(check_launch());
  if (S == 0 || H2 * W2 == 0) return GLORIE_OK;
  const int tiles = ((H + kAltTile - 1) / kAltTile) * ((W + kAltTile - 1) / kAltTile);
  hipLaunchKernelGGL(altcorr_bwd_f2_kernel, dim3(tiles, S, B), dim3(256), 0, st, fmap1, coords, corr_grad, fmap2_grad, S, H,
                     W, H2, W2, C, radius);
  return check_launch();
}
