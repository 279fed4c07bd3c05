// The rays of one training iteration over a whole window of keyframes (reference: src/mapper.py:437-466 gathers them
// frame by frame with get_samples; ray convention src/utils/common.py:39-54, get_rays_from_uv).
//
// Ray r of N = M * per belongs to window slot m = r / per and reads pixel (i, j) = (ii[r], jj[r]) of that slot's depth map,
// image and (optionally) radius map, each reached through a device table of M pointers.  It is a gather: about 40 B in
// and 44 B out per ray, and the only data with any reuse are the slot's three pointers and its matrix.
//
// One launch.  A workgroup is one wave and serves 64 consecutive rays of ONE slot (the grid is M x ceil(per / 64)
// workgroups, flattened), so the slot is a function of blockIdx alone: its pointers and the twelve matrix entries are
// wave-uniform and the compiler fetches them through the scalar cache, once per wave; the per-ray work is two index
// loads, five or six gathers and eleven stores.  No atomics, no host synchronisation, no output sized by the data.
//
// The direction is formed in the reference's order with every operation rounded to fp32 on its own (contraction is
// switched off inside gather_ray, window_rays.hiph, which map_sample.hip shares: the library is built with the compiler's
// default, and a fused multiply-add would round once where torch rounds twice).
#include "window_rays.hiph"

using namespace glorie;

namespace {

constexpr int kRayThreads = 64;      // one wave: the slot of a workgroup is uniform without any cross-lane step

__global__ void __launch_bounds__(kRayThreads)
window_rays_kernel(const float* const* __restrict__ depth_table, const float* const* __restrict__ image_table,
                   const float* const* __restrict__ radius_table, const float* __restrict__ c2ws, int per, int chunks,
                   int chw, int H, int W, float fx, float fy, float cx, float cy, const int64_t* __restrict__ ii,
                   const int64_t* __restrict__ jj, float const_radius, float* __restrict__ rays_o,
                   float* __restrict__ rays_d, float* __restrict__ depth, float* __restrict__ color,
                   float* __restrict__ radius) {
  const int m = blockIdx.x / chunks;                                  // window slot (uniform)
  const int k = (blockIdx.x - m * chunks) * kRayThreads + threadIdx.x;   // ray within the slot
  if (k >= per) return;
  const size_t r = (size_t)m * per + k;

  // a draw outside the image cannot read outside a map
  const long long iq = ii[r], jq = jj[r];
  const int i = (int)(iq < 0 ? 0 : (iq > W - 1 ? W - 1 : iq));
  const int j = (int)(jq < 0 ? 0 : (jq > H - 1 ? H - 1 : jq));
  gather_ray(c2ws + 16 * (size_t)m, depth_table[m], image_table[m], (radius && radius_table) ? radius_table[m] : nullptr,
             chw, H, W, fx, fy, cx, cy, i, j, r, const_radius, rays_o, rays_d, depth, color, radius);
}

}  // namespace

extern "C" int glorie_window_rays(const void* depth_table, const void* image_table, const void* radius_table,
                                  const float* c2ws, int M, int per, int chw, int H, int W, float fx, float fy, float cx,
                                  float cy, const int64_t* ii, const int64_t* jj, float const_radius, int want_radius,
                                  float* rays_o, float* rays_d, float* depth, float* color, float* radius, void* stream) {
  if (M < 0 || per < 0 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return GLORIE_EINVAL;
  if (M == 0 || per == 0) return GLORIE_OK;                           // N = 0: nothing is launched
  const long long chunks = ((long long)per + kRayThreads - 1) / kRayThreads;
  if ((long long)M * per > 0x7fffffffLL || (long long)M * chunks > 0x7fffffffLL) return GLORIE_EUNSUPPORTED;
  if (!depth_table || !image_table || !c2ws || !ii || !jj || !rays_o || !rays_d || !depth || !color) return GLORIE_EINVAL;
  if (want_radius && !radius) return GLORIE_EINVAL;
  hipLaunchKernelGGL(window_rays_kernel, dim3((unsigned)(M * chunks)), dim3(kRayThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const float* const*>(depth_table),
                     reinterpret_cast<const float* const*>(image_table),
                     reinterpret_cast<const float* const*>(radius_table), c2ws, per, (int)chunks, chw ? 1 : 0, H, W, fx,
                     fy, cx, cy, ii, jj, const_radius, rays_o, rays_d, depth, color, want_radius ? radius : nullptr);
  return check_launch();
}
