// Frame ingest: a batch of raw camera frames -> the working-size float images of the tracker (reference:
// src/utils/datasets.py:60-83 get_color, :98-137 __getitem__, which run cv2.undistort + cv2.resize + a float conversion
// per frame on the host and upload float32).
//
// Colour.  The uint8 frame is uploaded as it is (a quarter of the float bytes) and one launch per batch does
//   undistort (optional) -> bilinear resize -> crop -> optional R/B swap -> level / 255
// in integer arithmetic; the definition is in include/glorie_hip.h.  Everything that depends only on the camera is a small
// device table built once on the host (glorie_slam_amd/ingest.py): the undistortion map in 1/32-pixel fixed point and,
// per output column and per output row, the two source indices and their 11-bit weights - already cropped, so the
// kernel never sees the edges.
//
// One thread per output pixel, all three channels.  Fused, the pixel needs the 2 x 2 block of undistorted pixels at
// (x0|x1, y0|y1) and each of those the 2 x 2 block of source pixels its map entry names: up to 16 source pixels, each
// rounded stage kept as the two-pass definition has it, so the result equals two whole-image passes bit for bit while
// the undistorted image never exists in memory.  It is a byte gather: pixels are 3 bytes and a row is 3 W bytes, so
// nothing is aligned at odd widths - every load is a single byte and none is combined across pixels or past a row's
// end.  Neighbouring lanes are neighbouring output columns: their source bytes share cache lines and the output stores
// are coalesced, one plane at a time.  The 256-entry level -> float table and the row / column tables are read by every
// workgroup and stay in cache.
//
// Depth.  Nearest resampling through two index tables, then float32(v) / float32(scale), correctly rounded.
//
// No atomics, no workspace, no host synchronisation: both entry points can be captured in a hipGraph.
#include "common.hiph"

using namespace glorie;

namespace {

constexpr int kTileX = 64, kTileY = 4;       // 256 threads: one wave per output row segment

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the three channels of the undistorted pixel (u, v) of one frame, as uint8 levels
template <bool kMap>
__device__ __forceinline__ void mid_pixel(const uint8_t* __restrict__ frame, const int2* __restrict__ map, int H, int W,
                                          int u, int v, int (&p)[3]) {
  if (!kMap) {
    const uint8_t* __restrict__ s = frame + 3 * ((size_t)v * W + u);
    p[0] = s[0];
    p[1] = s[1];
    p[2] = s[2];
    return;
  }
  const int2 m = map[(size_t)v * W + u];
  const int x0 = m.x >> 5, y0 = m.y >> 5, a = m.x & 31, b = m.y & 31;
  const int wx[2] = {32 - a, a}, wy[2] = {32 - b, b};
  int acc[3] = {512, 512, 512};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int y = y0 + j;
    if ((unsigned)y >= (unsigned)H) continue;                      // a tap outside the image contributes 0
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int x = x0 + i;
      if ((unsigned)x >= (unsigned)W) continue;
      const uint8_t* __restrict__ s = frame + 3 * ((size_t)y * W + x);
      const int w = wx[i] * wy[j];
      acc[0] += w * s[0];
      acc[1] += w * s[1];
      acc[2] += w * s[2];
    }
  }
  p[0] = acc[0] >> 10;
  p[1] = acc[1] >> 10;
  p[2] = acc[2] >> 10;
}

template <bool kMap>
__global__ void __launch_bounds__(kTileX* kTileY)
ingest_color_kernel(const uint8_t* __restrict__ frames, const int2* __restrict__ map, const int4* __restrict__ xtab,
                    const int4* __restrict__ ytab, const float* __restrict__ lut, int H, int W, int H_out, int W_out,
                    int swap_rb, float* __restrict__ out) {
  const int ox = blockIdx.x * kTileX + threadIdx.x;
  const int oy = blockIdx.y * kTileY + threadIdx.y;
  if (ox >= W_out || oy >= H_out) return;
  const int b = blockIdx.z;
  const uint8_t* __restrict__ frame = frames + (size_t)b * H * W * 3;

  // {s0, s1, a0, a1}: a table entry outside the frame cannot read outside it
  const int4 tx = xtab[ox], ty = ytab[oy];
  const int x0 = clampi(tx.x, 0, W - 1), x1 = clampi(tx.y, 0, W - 1);
  const int y0 = clampi(ty.x, 0, H - 1), y1 = clampi(ty.y, 0, H - 1);

  int p00[3], p01[3], p10[3], p11[3];
  mid_pixel<kMap>(frame, map, H, W, x0, y0, p00);
  mid_pixel<kMap>(frame, map, H, W, x1, y0, p01);
  mid_pixel<kMap>(frame, map, H, W, x0, y1, p10);
  mid_pixel<kMap>(frame, map, H, W, x1, y1, p11);

  const size_t plane = (size_t)H_out * W_out;
  float* __restrict__ o = out + (size_t)b * 3 * plane + (size_t)oy * W_out + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int row0 = p00[c] * tx.z + p01[c] * tx.w;
    const int row1 = p10[c] * tx.z + p11[c] * tx.w;
    const int level = (((ty.z * (row0 >> 4)) >> 16) + ((ty.w * (row1 >> 4)) >> 16) + 2) >> 2;
    const int dst = swap_rb ? 2 - c : c;
    o[dst * plane] = lut[clampi(level, 0, 255)];
  }
}

template <typename T>
__global__ void __launch_bounds__(kTileX* kTileY)
ingest_depth_kernel(const T* __restrict__ raw, const int* __restrict__ ysrc, const int* __restrict__ xsrc, float scale,
                    int H, int W, int H_out, int W_out, float* __restrict__ out) {
  const int ox = blockIdx.x * kTileX + threadIdx.x;
  const int oy = blockIdx.y * kTileY + threadIdx.y;
  if (ox >= W_out || oy >= H_out) return;
  const int b = blockIdx.z;
  const int x = clampi(xsrc[ox], 0, W - 1), y = clampi(ysrc[oy], 0, H - 1);
  const float v = (float)raw[((size_t)b * H + y) * W + x];
  out[((size_t)b * H_out + oy) * W_out + ox] = __fdiv_rn(v, scale);
}

bool bad_shape(int B, int H, int W, int H_out, int W_out) {
  return B < 0 || H < 1 || W < 1 || H_out < 1 || W_out < 1 || (long long)H * W > 0x7fffffffLL / 3 ||
         (long long)H_out * W_out > 0x7fffffffLL;
}

dim3 ingest_grid(int B, int H_out, int W_out) {
  return dim3((unsigned)((W_out + kTileX - 1) / kTileX), (unsigned)((H_out + kTileY - 1) / kTileY), (unsigned)B);
}

}  // namespace

extern "C" int glorie_ingest_color(const uint8_t* frames, int B, int H, int W, const int32_t* map, const int32_t* xtab,
                                   const int32_t* ytab, const float* lut, int H_out, int W_out, int swap_rb, float* out,
                                   void* stream) {
  if (bad_shape(B, H, W, H_out, W_out)) return GLORIE_EINVAL;
  if (B == 0) return GLORIE_OK;
  if (B > 65535 || (H_out + kTileY - 1) / kTileY > 65535) return GLORIE_EUNSUPPORTED;
  if (!frames || !xtab || !ytab || !lut || !out) return GLORIE_EINVAL;
  const dim3 grid = ingest_grid(B, H_out, W_out), block(kTileX, kTileY);
  const int2* m = reinterpret_cast<const int2*>(map);
  const int4* tx = reinterpret_cast<const int4*>(xtab);
  const int4* ty = reinterpret_cast<const int4*>(ytab);
  if (map)
    hipLaunchKernelGGL(ingest_color_kernel<true>, grid, block, 0, (hipStream_t)stream, frames, m, tx, ty, lut, H, W, H_out,
                       W_out, swap_rb ? 1 : 0, out);
  else
    hipLaunchKernelGGL(ingest_color_kernel<false>, grid, block, 0, (hipStream_t)stream, frames, m, tx, ty, lut, H, W,
                       H_out, W_out, swap_rb ? 1 : 0, out);
  return check_launch();
}

extern "C" int glorie_ingest_depth(const void* raw, int dtype, int B, int H, int W, const int32_t* ysrc,
                                   const int32_t* xsrc, float scale, int H_out, int W_out, float* out, void* stream) {
  if (bad_shape(B, H, W, H_out, W_out) || (dtype != GLORIE_INGEST_U16 && dtype != GLORIE_INGEST_F32)) return GLORIE_EINVAL;
  if (B == 0) return GLORIE_OK;
  if (B > 65535 || (H_out + kTileY - 1) / kTileY > 65535) return GLORIE_EUNSUPPORTED;
  if (!raw || !ysrc || !xsrc || !out) return GLORIE_EINVAL;
  const dim3 grid = ingest_grid(B, H_out, W_out), block(kTileX, kTileY);
  if (dtype == GLORIE_INGEST_U16)
    hipLaunchKernelGGL(ingest_depth_kernel<uint16_t>, grid, block, 0, (hipStream_t)stream,
                       static_cast<const uint16_t*>(raw), ysrc, xsrc, scale, H, W, H_out, W_out, out);
  else
    hipLaunchKernelGGL(ingest_depth_kernel<float>, grid, block, 0, (hipStream_t)stream, static_cast<const float*>(raw),
                       ysrc, xsrc, scale, H, W, H_out, W_out, out);
  return check_launch();
}
