// The mapper's per-keyframe visualisation (reference: src/utils/Visualizer.py:118-203, called from src/mapper.py:664-673):
// a 4 x 3 contact sheet of the keyframe's input, rendered and residual depth and colour, the tracker depth, the projected
// cloud and its mask, the valid sample counts, the sparse cloud and the mono prior.  The reference copies twelve maps to
// the host and draws a matplotlib figure; here the maps stay where they are and three launches turn them into the
// bytes of the picture.  The definition of every byte is in include/glorie_hip.h; tests/vis_ref.py restates it in numpy.
//
// Range pass (two launches).  The sheet has three data-dependent ranges: max(droid_depth) and the min / max of the depth
// residual.  vis_range_kernel walks the three maps once, float4 per lane where the pointers allow it, keeps the three
// extrema in registers (non-finite values skipped), reduces them over the wave with shuffles and over the workgroup
// through LDS and writes one partial triple per workgroup; vis_range_final_kernel reduces the partials in one workgroup
// and writes the ranges.  min and max do not depend on the order they are taken in, so the result is bit-exact; there
// are no atomics and nothing to zero between calls.
//
// Compose pass (one launch).  One lane owns kPix contiguous pixels of one sheet row, a wave a row segment of 64 kPix
// pixels, a workgroup four rows.  Every pixel finds its panel from its coordinates (everything outside a panel is
// white), reads the source pixel the decimation names and maps it; the 256 x 3 byte colour table is packed into 256
// dwords of LDS by the workgroup, one ds_read_b32 per lookup.  No residual map exists in memory: panels 2 and 5 are
// computed from their sources.  A lane's 12 bytes leave as three dword stores when the sheet's base and row pitch are
// dword-aligned (64 lanes cover 768 contiguous bytes) and as byte stores otherwise.  Neighbouring lanes read neighbouring
// source pixels (scale 1) or the same cache lines at a stride (scale > 1).
//
// Frame entry point: float colour -> uint8, saturate(rint(255 x)), four values per lane.
//
// No launch reads anything on the host: all of it can be recorded into a hipGraph.
#include <math.h>

#include "common.hiph"

using namespace glorie;

namespace {

constexpr int kPix = 4;                       // contiguous sheet pixels per lane
constexpr int kLanesX = 64, kRows = 4;        // workgroup: one wave per sheet row, four rows
constexpr int kRangeThreads = 256, kRangeMaxBlocks = 1024;
constexpr unsigned kWhite = 0x00ffffffu;      // r | g << 8 | b << 16

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-inf

// min(|render_depth - depth|, 0.2) with a NaN kept, 0 where the render depth is 0 (Visualizer.py:121-123)
__device__ __forceinline__ float depth_residual(float rd, float d) {
  if (rd == 0.0f) return 0.0f;
  const float r = fabsf(rd - d);
  return r > 0.2f ? 0.2f : r;
}

struct Extrema {
  float dmax, rmin, rmax;
  __device__ __forceinline__ void take(float rd, float d, float droid) {
    if (finite_f(droid)) dmax = fmaxf(dmax, droid);
    const float r = depth_residual(rd, d);
    if (finite_f(r)) {
      rmin = fminf(rmin, r);
      rmax = fmaxf(rmax, r);
    }
  }
  __device__ __forceinline__ void merge(float a, float b, float c) {
    dmax = fmaxf(dmax, a);
    rmin = fminf(rmin, b);
    rmax = fmaxf(rmax, c);
  }
};

// the extrema of the workgroup in thread 0 (every thread calls)
__device__ __forceinline__ Extrema block_extrema(Extrema e) {
  __shared__ float part[3][kRangeThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    e.merge(__shfl_xor(e.dmax, off, 64), __shfl_xor(e.rmin, off, 64), __shfl_xor(e.rmax, off, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    part[0][wave] = e.dmax;
    part[1][wave] = e.rmin;
    part[2][wave] = e.rmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kRangeThreads / 64; ++w) e.merge(part[0][w], part[1][w], part[2][w]);
  }
  return e;
}

// partials f32 [gridDim.x, 3]
template <bool kVec>
__global__ void __launch_bounds__(kRangeThreads)
vis_range_kernel(const float* __restrict__ render_depth, const float* __restrict__ depth,
                 const float* __restrict__ droid_depth, long long n, float* __restrict__ partials) {
  Extrema e = {-INFINITY, INFINITY, -INFINITY};
  const long long groups = (n + 3) / 4;
  for (long long g = (long long)blockIdx.x * kRangeThreads + threadIdx.x; g < groups;
       g += (long long)gridDim.x * kRangeThreads) {
    const long long i = 4 * g;
    if (kVec && i + 4 <= n) {
      const float4 a = *reinterpret_cast<const float4*>(render_depth + i);
      const float4 b = *reinterpret_cast<const float4*>(depth + i);
      const float4 c = *reinterpret_cast<const float4*>(droid_depth + i);
      e.take(a.x, b.x, c.x);
      e.take(a.y, b.y, c.y);
      e.take(a.z, b.z, c.z);
      e.take(a.w, b.w, c.w);
    } else {
      for (long long j = i; j < i + 4 && j < n; ++j) e.take(render_depth[j], depth[j], droid_depth[j]);
    }
  }
  e = block_extrema(e);
  if (threadIdx.x == 0) {
    float* __restrict__ p = partials + 3 * (size_t)blockIdx.x;
    p[0] = e.dmax;
    p[1] = e.rmin;
    p[2] = e.rmax;
  }
}

// an extremum nothing was merged into is still infinite: the range of nothing is [0, 0]; a zero is written as +0
__device__ __forceinline__ float range_value(float v) { return (!finite_f(v) || v == 0.0f) ? 0.0f : v; }

__global__ void __launch_bounds__(kRangeThreads)
vis_range_final_kernel(const float* __restrict__ partials, int n_partials, float* __restrict__ ranges) {
  Extrema e = {-INFINITY, INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < n_partials; b += kRangeThreads)
    e.merge(partials[3 * b], partials[3 * b + 1], partials[3 * b + 2]);
  e = block_extrema(e);
  if (threadIdx.x == 0) {
    ranges[0] = range_value(e.dmax);
    ranges[1] = range_value(e.rmin);
    ranges[2] = range_value(e.rmax);
    ranges[3] = 0.0f;
  }
}

// ---- compose --------------------------------------------------------------------------------------------------------
struct SheetMaps {
  const float* render_depth;
  const float* depth;
  const float* color;      // [H, W, 3]
  const float* gt_color;   // [H, W, 3]
  const float* droid_depth;
  const float* proj_depth;
  const float* valid_count;
  const float* sparse_depth;
  const float* mono_depth;
};

struct SheetGeom {
  int H, W, scale, gutter, title, ph, pw, SH, SW;
};

// the colour table entry of a scalar, packed; white for a non-finite value
__device__ __forceinline__ unsigned colormap(const unsigned* __restrict__ lut, float v, float vmin, float vmax) {
  if (!finite_f(v)) return kWhite;
  const float t = vmin == vmax ? 0.0f : __fdiv_rn(v - vmin, vmax - vmin);
  const float f = t * 256.0f;
  const int idx = f >= 255.0f ? 255 : (f > 0.0f ? (int)f : 0);       // a NaN (inf / inf) takes entry 0
  return lut[idx];
}

// trunc(clamp(x, 0, 1) * 255); a NaN gives 0
__device__ __forceinline__ unsigned level(float x) {
  const float c = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;
  return (unsigned)(int)(c * 255.0f);
}
__device__ __forceinline__ unsigned pack_rgb(float r, float g, float b) {
  return level(r) | (level(g) << 8) | (level(b) << 16);
}
// torch.round(color * 255) / 255 (Visualizer.py:119)
__device__ __forceinline__ float round_level(float x) { return __fdiv_rn(rintf(x * 255.0f), 255.0f); }

// sheet pixel (y, x), y < SH, x < SW -> r | g << 8 | b << 16
__device__ __forceinline__ unsigned sheet_pixel(const SheetMaps& m, const SheetGeom& g, const float* __restrict__ ranges,
                                                float count_max, const unsigned* __restrict__ lut, int py, int ly, int x) {
  // py, ly: panel row and the row inside it (negative: gutter or title strip), the same for the whole lane
  const int cell_w = g.pw + g.gutter;
  const int xr = x - g.gutter;
  if (ly < 0 || xr < 0) return kWhite;
  const int px = xr / cell_w, lx = xr - px * cell_w;
  if (px >= 3 || lx >= g.pw) return kWhite;
  const int sy = min(ly * g.scale + g.scale / 2, g.H - 1);
  const int sx = min(lx * g.scale + g.scale / 2, g.W - 1);
  const size_t s = (size_t)sy * g.W + sx;
  const float dmax = ranges[0];
  switch (py * 3 + px) {
    case 0: return colormap(lut, m.render_depth[s], 0.0f, dmax);
    case 1: return colormap(lut, m.depth[s], 0.0f, dmax);
    case 2: return colormap(lut, depth_residual(m.render_depth[s], m.depth[s]), ranges[1], ranges[2]);
    case 3: return pack_rgb(m.gt_color[3 * s], m.gt_color[3 * s + 1], m.gt_color[3 * s + 2]);
    case 4:
      return pack_rgb(round_level(m.color[3 * s]), round_level(m.color[3 * s + 1]), round_level(m.color[3 * s + 2]));
    case 5: {
      if (m.render_depth[s] == 0.0f) return 0u;
      return pack_rgb(fabsf(m.gt_color[3 * s] - round_level(m.color[3 * s])),
                      fabsf(m.gt_color[3 * s + 1] - round_level(m.color[3 * s + 1])),
                      fabsf(m.gt_color[3 * s + 2] - round_level(m.color[3 * s + 2])));
    }
    case 6: return colormap(lut, m.droid_depth[s], 0.0f, dmax);
    case 7: return colormap(lut, m.proj_depth[s], 0.0f, dmax);
    case 8: return colormap(lut, m.proj_depth[s] > 0.0f ? 1.0f : 0.0f, 0.0f, 1.0f);
    case 9: return colormap(lut, m.valid_count[s], 0.0f, count_max);
    case 10: return colormap(lut, m.sparse_depth[s], 0.0f, dmax);
    default: return colormap(lut, m.mono_depth[s], 0.0f, dmax);
  }
}

template <bool kAligned>
__global__ void __launch_bounds__(kLanesX* kRows)
vis_compose_kernel(SheetMaps m, SheetGeom g, const float* __restrict__ ranges, float count_max,
                   const uint8_t* __restrict__ table, uint8_t* __restrict__ sheet) {
  __shared__ unsigned lut[256];
  {
    const int t = threadIdx.y * kLanesX + threadIdx.x;                // 256 threads, one table entry each
    lut[t] = (unsigned)table[3 * t] | ((unsigned)table[3 * t + 1] << 8) | ((unsigned)table[3 * t + 2] << 16);
  }
  __syncthreads();
  const int y = blockIdx.y * kRows + threadIdx.y;
  const int x0 = (blockIdx.x * kLanesX + threadIdx.x) * kPix;
  if (y >= g.SH || x0 >= g.SW) return;

  // the panel row of this sheet row: a cell is title + ph + gutter rows, the panel starts after the title strip
  const int cell_h = g.title + g.ph + g.gutter;
  const int yr = y - g.gutter;
  int py = 0, ly = -1;
  if (yr >= 0) {
    py = yr / cell_h;
    ly = yr - py * cell_h - g.title;
    if (py >= 4 || ly >= g.ph) ly = -1;
  }

  unsigned p[kPix];
#pragma unroll
  for (int i = 0; i < kPix; ++i)
    p[i] = x0 + i < g.SW ? sheet_pixel(m, g, ranges, count_max, lut, py, ly, x0 + i) : kWhite;

  uint8_t* __restrict__ o = sheet + 3 * ((size_t)y * g.SW + x0);
  if (kAligned && x0 + kPix <= g.SW) {
    // 4 pixels = 12 bytes = 3 dwords: rgbr gbrg brgb
    uint32_t* __restrict__ o4 = reinterpret_cast<uint32_t*>(o);
    o4[0] = p[0] | (p[1] << 24);
    o4[1] = (p[1] >> 8) | (p[2] << 16);
    o4[2] = (p[2] >> 16) | (p[3] << 8);
  } else {
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      if (x0 + i >= g.SW) break;
      o[3 * i] = (uint8_t)(p[i] & 0xff);
      o[3 * i + 1] = (uint8_t)((p[i] >> 8) & 0xff);
      o[3 * i + 2] = (uint8_t)((p[i] >> 16) & 0xff);
    }
  }
}

// ---- float colour -> uint8 ------------------------------------------------------------------------------------------
// saturate(rint(255 x)), NaN -> 0 (cv2.imwrite of a float image: saturate_cast<uchar>, which rounds ties to even)
__device__ __forceinline__ unsigned rgb8_level(float x) {
  const float r = rintf(x * 255.0f);
  return r >= 255.0f ? 255u : (r > 0.0f ? (unsigned)(int)r : 0u);
}

template <bool kVec>
__global__ void __launch_bounds__(256)
vis_rgb8_kernel(const float* __restrict__ color, long long n, uint8_t* __restrict__ out) {
  const long long groups = (n + 3) / 4;
  for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (long long)gridDim.x * 256) {
    const long long i = 4 * gi;
    if (kVec && i + 4 <= n) {
      const float4 v = *reinterpret_cast<const float4*>(color + i);
      *reinterpret_cast<uint32_t*>(out + i) =
          rgb8_level(v.x) | (rgb8_level(v.y) << 8) | (rgb8_level(v.z) << 16) | (rgb8_level(v.w) << 24);
    } else {
      for (long long j = i; j < i + 4 && j < n; ++j) out[j] = (uint8_t)rgb8_level(color[j]);
    }
  }
}

bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int range_blocks(long long n) {
  const long long want = (n + 4LL * kRangeThreads - 1) / (4LL * kRangeThreads);
  return (int)(want < 1 ? 1 : (want > kRangeMaxBlocks ? kRangeMaxBlocks : want));
}

}  // namespace

extern "C" size_t glorie_vis_ranges_workspace(void) { return sizeof(float) * 3 * kRangeMaxBlocks; }

extern "C" int glorie_vis_ranges(const float* render_depth, const float* depth, const float* droid_depth, long long n,
                                 float* ranges, void* workspace, void* stream) {
  if (n < 0 || !ranges || !workspace || (n > 0 && (!render_depth || !depth || !droid_depth))) return GLORIE_EINVAL;
  if (!aligned_to(workspace, 4) || !aligned_to(ranges, 4)) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  float* partials = static_cast<float*>(workspace);
  const int blocks = range_blocks(n);
  if (aligned_to(render_depth, 16) && aligned_to(depth, 16) && aligned_to(droid_depth, 16))
    hipLaunchKernelGGL(vis_range_kernel<true>, dim3(blocks), dim3(kRangeThreads), 0, st, render_depth, depth, droid_depth,
                       n, partials);
  else
    hipLaunchKernelGGL(vis_range_kernel<false>, dim3(blocks), dim3(kRangeThreads), 0, st, render_depth, depth,
                       droid_depth, n, partials);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(vis_range_final_kernel, dim3(1), dim3(kRangeThreads), 0, st, partials, blocks, ranges);
  return check_launch();
}

extern "C" int glorie_vis_sheet_size(int H, int W, int scale, int gutter, int title, int* SH, int* SW) {
  if (H < 1 || W < 1 || scale < 1 || gutter < 0 || title < 0 || !SH || !SW) return GLORIE_EINVAL;
  const long long ph = ((long long)H + scale - 1) / scale, pw = ((long long)W + scale - 1) / scale;
  const long long sh = gutter + 4 * ((long long)title + ph + gutter), sw = gutter + 3 * (pw + gutter);
  if (sh * sw > 0x7fffffffLL / 3) return GLORIE_EUNSUPPORTED;
  *SH = (int)sh;
  *SW = (int)sw;
  return GLORIE_OK;
}

extern "C" int glorie_vis_compose(const float* render_depth, const float* depth, const float* color, const float* gt_color,
                                  const float* droid_depth, const float* proj_depth, const float* valid_count,
                                  const float* sparse_depth, const float* mono_depth, int H, int W, const float* ranges,
                                  float count_max, const uint8_t* table, int scale, int gutter, int title, uint8_t* sheet,
                                  void* stream) {
  SheetGeom g;
  GLORIE_TRY(glorie_vis_sheet_size(H, W, scale, gutter, title, &g.SH, &g.SW));
  if ((long long)H * W > 0x7fffffffLL / 3) return GLORIE_EUNSUPPORTED;
  if (!render_depth || !depth || !color || !gt_color || !droid_depth || !proj_depth || !valid_count || !sparse_depth ||
      !mono_depth || !ranges || !table || !sheet)
    return GLORIE_EINVAL;
  g.H = H, g.W = W, g.scale = scale, g.gutter = gutter, g.title = title;
  g.ph = (H + scale - 1) / scale, g.pw = (W + scale - 1) / scale;
  const SheetMaps m = {render_depth, depth, color, gt_color, droid_depth, proj_depth, valid_count, sparse_depth, mono_depth};
  const int span = kLanesX * kPix;
  const dim3 grid((unsigned)((g.SW + span - 1) / span), (unsigned)((g.SH + kRows - 1) / kRows)), block(kLanesX, kRows);
  if (grid.y > 65535u) return GLORIE_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  // dword stores need every 4-pixel group to start on a dword: the base and the row pitch 3 SW
  if (aligned_to(sheet, 4) && g.SW % 4 == 0)
    hipLaunchKernelGGL(vis_compose_kernel<true>, grid, block, 0, st, m, g, ranges, count_max, table, sheet);
  else
    hipLaunchKernelGGL(vis_compose_kernel<false>, grid, block, 0, st, m, g, ranges, count_max, table, sheet);
  return check_launch();
}

extern "C" int glorie_vis_rgb8(const float* color, long long n, uint8_t* out, void* stream) {
  if (n < 0 || (n > 0 && (!color || !out))) return GLORIE_EINVAL;
  if (n == 0) return GLORIE_OK;
  const long long want = (n + 4 * 256 - 1) / (4 * 256);
  const dim3 grid((unsigned)(want > 2048 ? 2048 : want)), block(256);
  if (aligned_to(color, 16) && aligned_to(out, 4))
    hipLaunchKernelGGL(vis_rgb8_kernel<true>, grid, block, 0, (hipStream_t)stream, color, n, out);
  else
    hipLaunchKernelGGL(vis_rgb8_kernel<false>, grid, block, 0, (hipStream_t)stream, color, n, out);
  return check_launch();
}
