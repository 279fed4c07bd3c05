// Deformation of the neural point cloud after tracker updates, and the proxy depth of the mapper
// (reference: src/neural_point.py:378-438 NeuralPointCloud.update_points_pos, :446-506 proj_depth_map, :509-537
// update_points_pos(npc, video), :539-575 get_proxy_render_depth; src/depth_video.py:313-324 get_pose /
// get_depth_and_pose; src/utils/common.py:39-54 get_rays_from_uv).
//
// Deformation, one memset and three launches over the input points, driven by the keyframes' npc_dirty flags on the
// device (no host index list, no host read):
//   deform_range_kernel   per keyframe: the number of dirty input points with a valid depth d != 0 and the largest
//                         binary exponent of their terms prev * d and prev^2 (integer atomics: order-independent)
//   deform_scale_kernel   those terms, computed exactly in double, scaled by 2^e_v and rounded once to int64, summed per
//                         keyframe with int64 atomics (one per wave when the wave's points share a keyframe, which the
//                         contiguous insertion runs make the common case).  e_v = 61 - (max exponent) - (bit length of
//                         the count) bounds every term by 2^61 / count, so the sum cannot overflow whatever the depth
//                         range, and its resolution is 2^-60 of the largest term.  Integer sums are exact in any order:
//                         the scale is bitwise repeatable.
//   deform_apply_kernel   d == 0 -> s_v * prev, s_v = sum(prev d) / sum(prev^2); then the ray of the point's pixel from the
//                         keyframe's current c2w, and the input point plus its N_add cloud rows
// glorie_iproj_dirty: iproj of every dirty keyframe (the device code of glorie_iproj) and a copy of its valid-depth mask,
// then (optionally) a launch that clears the flags after everything else has read them.
// glorie_proxy_depth: +inf fill, a z-buffer pass over the unprojected maps of keyframes [0, counter), a finalize pass
// tracker -> projection -> mono.
// The z-buffer pass (zbuf_kernel, launch_zbuf) is also the whole of glorie_proj_depth (render.hip): it lives here
// because this unit compiles with contraction off, which the shared projection of camera.hiph then inherits.
#include <hip/hip_runtime.h>
// every fp32 operation rounded on its own, in the reference's order (as geom.hip): the unprojection is then bitwise
// equal to glorie_iproj, and the projection of the z-buffer pass keeps the bits it had in proj_depth_map
#pragma clang fp contract(off)
#include "camera.hiph"
#include "common.hiph"
#include "se3.hiph"

namespace {

using glorie::Pose;

constexpr int kThreads = 256;

// per-keyframe scratch of the scale: [0, 2B) the two int64 sums, then B int32 exponents (+ kExpBias), B uint32 counts
constexpr int kExpBias = 4096;

// keyframe of input point p if it is dirty and its pixel / keyframe indices are in range, else -1
__device__ __forceinline__ int dirty_frame(const int64_t* __restrict__ vidx, const int64_t* __restrict__ pj,
                                           const int64_t* __restrict__ pi, const uint8_t* __restrict__ dirty, long p,
                                           long n, int B, int H, int W) {
  if (p >= n) return -1;
  const int64_t v = vidx[p], j = pj[p], i = pi[p];
  if (v < 0 || v >= B || j < 0 || j >= H || i < 0 || i >= W) return -1;
  return dirty[v] ? (int)v : -1;
}

// depth of the point's pixel as get_depth_and_pose + `est_depth[~mask] = 0` compute it
__device__ __forceinline__ float frame_depth(const float* __restrict__ disps_up, const uint8_t* __restrict__ valid,
                                             int v, int64_t j, int64_t i, int H, int W) {
  const size_t px = ((size_t)v * H + (size_t)j) * W + (size_t)i;
  return valid[px] ? 1.0f / disps_up[px] : 0.0f;
}

// the two terms of get_scale for input point p of dirty keyframe v; false when the point has no valid depth (or a
// non-finite product, an infinite depth from a zero disparity, which would poison the integer sum: left out)
__device__ __forceinline__ bool scale_terms(const float* __restrict__ disps_up, const uint8_t* __restrict__ valid,
                                            const int64_t* __restrict__ pj, const int64_t* __restrict__ pi,
                                            const float* __restrict__ input_depth, long p, int v, int H, int W,
                                            double& pd, double& pp) {
  const float d = frame_depth(disps_up, valid, v, pj[p], pi[p], H, W);
  const double prev = (double)input_depth[p];
  pd = prev * (double)d;                                        // exact: 24 x 24 bit products
  pp = prev * prev;
  return d != 0.0f && isfinite(pd) && isfinite(pp);
}

__global__ __launch_bounds__(kThreads) void deform_range_kernel(
    const float* __restrict__ disps_up, const uint8_t* __restrict__ valid, const uint8_t* __restrict__ dirty, int B,
    int H, int W, const int64_t* __restrict__ vidx, const int64_t* __restrict__ pj, const int64_t* __restrict__ pi,
    const float* __restrict__ input_depth, long n, int* __restrict__ max_exp, unsigned* __restrict__ count) {
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;
  const int v = dirty_frame(vidx, pj, pi, dirty, p, n, B, H, W);
  int e = 0;
  bool has = false;
  if (v >= 0) {
    double pd, pp;
    has = scale_terms(disps_up, valid, pj, pi, input_depth, p, v, H, W, pd, pp);
    if (has) {
      int ea, eb;
      frexp(fabs(pd), &ea);                                    // |pd| < 2^ea
      frexp(pp, &eb);
      e = (ea > eb ? ea : eb) + kExpBias;
    }
  }
  const unsigned long long ballot = __ballot(has);
  const int v0 = __shfl(v, 0, 64);
  if (__all(v == v0)) {
    e = glorie::wave_max(e);
    if ((threadIdx.x & 63) == 0 && v0 >= 0 && ballot) {
      atomicMax(&max_exp[v0], e);
      atomicAdd(&count[v0], (unsigned)__popcll(ballot));
    }
  } else if (has) {
    atomicMax(&max_exp[v], e);
    atomicAdd(&count[v], 1u);
  }
}

__global__ __launch_bounds__(kThreads) void deform_scale_kernel(
    const float* __restrict__ disps_up, const uint8_t* __restrict__ valid, const uint8_t* __restrict__ dirty, int B,
    int H, int W, const int64_t* __restrict__ vidx, const int64_t* __restrict__ pj, const int64_t* __restrict__ pi,
    const float* __restrict__ input_depth, long n, unsigned long long* __restrict__ sums,
    const int* __restrict__ max_exp, const unsigned* __restrict__ count, unsigned long long* __restrict__ stats) {
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;
  const int v = dirty_frame(vidx, pj, pi, dirty, p, n, B, H, W);
  long long a = 0, b = 0;
  bool has = false;
  if (v >= 0) {
    double pd, pp;
    has = scale_terms(disps_up, valid, pj, pi, input_depth, p, v, H, W, pd, pp);
    if (has) {
      // every |term| * 2^e < 2^(61 - bits(count)): the keyframe's sum stays below 2^61
      const int e = 61 - (max_exp[v] - kExpBias) - (32 - __clz((int)count[v]));
      a = llrint(ldexp(pd, e));
      b = llrint(ldexp(pp, e));
    }
  }
  // points moved by this call (every dirty input point is re-placed)
  const unsigned long long moved = __ballot(v >= 0);
  if ((threadIdx.x & 63) == 0 && stats && moved) atomicAdd(stats, (unsigned long long)__popcll(moved));
  const int v0 = __shfl(v, 0, 64);
  const bool any_has = __any(has);
  if (__all(v == v0)) {
    a = glorie::wave_sum(a);
    b = glorie::wave_sum(b);
    if ((threadIdx.x & 63) == 0 && v0 >= 0 && any_has) {
      atomicAdd(&sums[2 * v0], (unsigned long long)a);
      atomicAdd(&sums[2 * v0 + 1], (unsigned long long)b);
    }
  } else if (has) {
    atomicAdd(&sums[2 * v], (unsigned long long)a);
    atomicAdd(&sums[2 * v + 1], (unsigned long long)b);
  }
}

// c2w of DepthVideo.get_pose (R from the stored world-to-camera quaternion, [R^T | -R^T t]) with columns 1 and 2
// negated (the renderer's OpenGL convention, `c2w[:3, 1:3] *= -1`)
struct C2W {
  float r[3][3];
  float t[3];
};

__device__ __forceinline__ C2W frame_c2w(const float* __restrict__ pose) {
  const float tx = pose[0], ty = pose[1], tz = pose[2];
  const float qx = pose[3], qy = pose[4], qz = pose[5], qw = pose[6];
  float R[3][3];
  R[0][0] = 1.0f - 2.0f * (qy * qy + qz * qz);
  R[0][1] = 2.0f * (qx * qy - qz * qw);
  R[0][2] = 2.0f * (qx * qz + qy * qw);
  R[1][0] = 2.0f * (qx * qy + qz * qw);
  R[1][1] = 1.0f - 2.0f * (qx * qx + qz * qz);
  R[1][2] = 2.0f * (qy * qz - qx * qw);
  R[2][0] = 2.0f * (qx * qz - qy * qw);
  R[2][1] = 2.0f * (qy * qz + qx * qw);
  R[2][2] = 1.0f - 2.0f * (qx * qx + qy * qy);
  C2W c;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) c.r[a][b] = (b == 0 ? 1.0f : -1.0f) * R[b][a];
    c.t[a] = -(R[0][a] * tx + R[1][a] * ty + R[2][a] * tz);
  }
  return c;
}

// torch.linspace(start, end, steps) in fp32, element s (the two-sided form of the ATen kernel)
__device__ __forceinline__ float linspace_f32(float start, float end, int steps, int s) {
  if (steps == 1) return start;
  const float step = (end - start) / (float)(steps - 1);
  const int half = steps / 2;
  return s < half ? start + step * (float)s : end - step * (float)(steps - s - 1);
}

__global__ __launch_bounds__(kThreads) void deform_apply_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps_up, const uint8_t* __restrict__ valid,
    const uint8_t* __restrict__ dirty, int B, int H, int W, const int64_t* __restrict__ vidx,
    const int64_t* __restrict__ pj, const int64_t* __restrict__ pi, float* __restrict__ input_depth,
    float* __restrict__ input_pos, long n, float* __restrict__ cloud_pos, int n_add, float near_s, float far_s,
    int fix_interval, float fx, float fy, float cx, float cy, const unsigned long long* __restrict__ sums) {
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;
  const int v = dirty_frame(vidx, pj, pi, dirty, p, n, B, H, W);
  if (v < 0) return;
  const int64_t j = pj[p], i = pi[p];
  float d = frame_depth(disps_up, valid, v, j, i, H, W);
  if (d == 0.0f) {
    // get_scale over the keyframe's points with a depth; none -> 1 (the reference divides 0 by 0: NaN positions)
    const long long spp = (long long)sums[2 * v + 1];
    const float s = spp != 0 ? (float)((double)(long long)sums[2 * v] / (double)spp) : 1.0f;
    d = s * input_depth[p];
  }
  const C2W c = frame_c2w(poses + (size_t)v * 7);
  // get_rays_from_uv: dirs = ((i - cx) / fx, -(j - cy) / fy, -1), rays_d = sum(dirs * c2w[:3, :3], -1)
  const float dx = ((float)i - cx) / fx, dy = -(((float)j - cy) / fy), dz = -1.0f;
  float rd[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) rd[a] = dx * c.r[a][0] + dy * c.r[a][1] + dz * c.r[a][2];
#pragma unroll
  for (int a = 0; a < 3; ++a) input_pos[p * 3 + a] = c.t[a] + rd[a] * d;
  input_depth[p] = d;
  for (int s = 0; s < n_add; ++s) {
    float z;
    if (fix_interval) {
      z = d + linspace_f32(-0.04f, 0.04f, n_add, s);
    } else {
      const float t = linspace_f32(0.0f, 1.0f, n_add, s);
      z = near_s * d * (1.0f - t) + far_s * d * t;
    }
    float* o = cloud_pos + ((size_t)p * n_add + s) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = c.t[a] + rd[a] * z;
  }
}

__global__ __launch_bounds__(kThreads) void iproj_dirty_kernel(const float* __restrict__ inv_poses,
                                                               const float* __restrict__ disps_up,
                                                               const float* __restrict__ intr,
                                                               const uint8_t* __restrict__ valid,
                                                               const uint8_t* __restrict__ dirty, int H, int W,
                                                               float* __restrict__ full_pcl,
                                                               uint8_t* __restrict__ full_mask) {
  const int b = blockIdx.y;
  if (!dirty[b]) return;
  const int HW = H * W;
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= HW) return;
  const Pose g = glorie::load_pose(inv_poses + (size_t)b * 7);
  const int y = k / W, x = k - y * W;
  const size_t px = (size_t)b * HW + k;
  glorie::iproj_pixel(g, x, y, disps_up[px], intr[0], intr[1], intr[2], intr[3], full_pcl + px * 3);
  full_mask[px] = valid[px] ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void clear_flags_kernel(uint8_t* __restrict__ dirty, int B) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b < B) dirty[b] = 0;
}

__global__ __launch_bounds__(kThreads) void fill_inf_kernel(unsigned* __restrict__ bits, int n) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k < n) bits[k] = 0x7f800000u;
}

// z-buffer projection of a point set into a pinhole view (neural_point.py:446-506, proj_depth_map): camera
// coordinates X_c = w2c X (OpenGL convention: the camera looks along -z; the x axis is flipped before the
// projection), pixel (u, v) = trunc(K X_c / z), depth = -z; the closest point per pixel wins.  The reference
// sorts all points by depth and takes the first of every unique pixel; here every point does one atomicMin on
// the bit pattern of its (positive) depth.  depth_bits must be pre-filled with +inf (0x7f800000).
// mask: optional; skip_row: the points are the pixels of [.., H, W] maps and image row skip_row of every map is left
// out (`full_mask[:, counter - mapping_window_size] = 0`; -1: no row)
__global__ __launch_bounds__(kThreads) void zbuf_kernel(const float* __restrict__ pts, const uint8_t* __restrict__ mask,
                                                        long n, int H, int W, int skip_row,
                                                        const float* __restrict__ w2c, float fx, float fy, float cx,
                                                        float cy, unsigned* __restrict__ depth_bits) {
  const long k = (long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= n || (mask && !mask[k])) return;
  if (skip_row >= 0 && (int)((k / W) % H) == skip_row) return;
  const glorie::Proj p = glorie::project(w2c, pts[k * 3 + 0], pts[k * 3 + 1], pts[k * 3 + 2], fx, fy, cx, cy, 1e-6f);
  if (!(p.u < (float)W && p.u >= 0.0f && p.v < (float)H && p.v >= 0.0f && -p.z > 0.0f)) return;
  const int ui = (int)p.u, vi = (int)p.v;
  atomicMin(&depth_bits[(size_t)vi * W + ui], __float_as_uint(-p.z));
}

// get_proxy_render_depth: the tracker's depth where > 0, else the projection where > 0, then (mono != NULL) the mono
// prior where the result is still 0
__global__ __launch_bounds__(kThreads) void proxy_finalize_kernel(const unsigned* __restrict__ depth_bits,
                                                                  const float* __restrict__ droid,
                                                                  const float* __restrict__ mono, int n,
                                                                  float* __restrict__ out) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const unsigned bits = depth_bits[k];
  const float proj = bits == 0x7f800000u ? 0.0f : __uint_as_float(bits);
  const float dr = droid[k];
  float p = dr;
  if (!(dr > 0.0f) && proj > 0.0f) p = proj;
  if (mono && p == 0.0f) p = mono[k];
  out[k] = p;
}

}  // namespace

int glorie::launch_zbuf(const float* points, const uint8_t* mask, long n, int H, int W, int skip_row, const float* w2c,
                        float fx, float fy, float cx, float cy, unsigned* depth_bits, hipStream_t st) {
  hipLaunchKernelGGL(zbuf_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, points, mask, n,
                     H, W, skip_row, w2c, fx, fy, cx, cy, depth_bits);
  return check_launch();
}

extern "C" size_t glorie_npc_deform_workspace(int B) {
  return B > 0 ? (size_t)B * (2 * sizeof(unsigned long long) + sizeof(int) + sizeof(unsigned)) : 0;
}

extern "C" int glorie_npc_deform(const float* poses, const float* disps_up, const uint8_t* valid, const uint8_t* dirty,
                                 int B, int H, int W, const int64_t* input_video_idx, const int64_t* input_j,
                                 const int64_t* input_i, float* input_depth, float* input_pos, long n,
                                 float* cloud_pos, long cloud_rows, int n_add, float near_end_surface,
                                 float far_end_surface, int fix_interval, float fx, float fy, float cx, float cy,
                                 void* workspace, unsigned long long* stats, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || n < 0 || n_add < 1 || cloud_rows < 0) return GLORIE_EINVAL;
  if (cloud_rows != n * (long)n_add) return GLORIE_EINVAL;      // plain add_points(pts) rows have no input point
  if (n == 0 || B == 0) return GLORIE_OK;
  if (!poses || !disps_up || !valid || !dirty || !input_video_idx || !input_j || !input_i || !input_depth ||
      !input_pos || !cloud_pos || !workspace)
    return GLORIE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  auto* sums = static_cast<unsigned long long*>(workspace);
  const int st = glorie::check_hip(hipMemsetAsync(sums, 0, glorie_npc_deform_workspace(B), s));
  if (st != GLORIE_OK) return st;
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
  int* max_exp = reinterpret_cast<int*>(sums + 2 * (size_t)B);
  unsigned* count = reinterpret_cast<unsigned*>(max_exp + B);
  hipLaunchKernelGGL(deform_range_kernel, grid, dim3(kThreads), 0, s, disps_up, valid, dirty, B, H, W, input_video_idx,
                     input_j, input_i, input_depth, n, max_exp, count);
  if (glorie::check_launch()) return GLORIE_EHIP;
  hipLaunchKernelGGL(deform_scale_kernel, grid, dim3(kThreads), 0, s, disps_up, valid, dirty, B, H, W, input_video_idx,
                     input_j, input_i, input_depth, n, sums, max_exp, count, stats);
  if (glorie::check_launch()) return GLORIE_EHIP;
  hipLaunchKernelGGL(deform_apply_kernel, grid, dim3(kThreads), 0, s, poses, disps_up, valid, dirty, B, H, W,
                     input_video_idx, input_j, input_i, input_depth, input_pos, n, cloud_pos, n_add, near_end_surface,
                     far_end_surface, fix_interval, fx, fy, cx, cy, sums);
  return glorie::check_launch();
}

extern "C" int glorie_iproj_dirty(const float* inv_poses, const float* disps_up, const float* intrinsics,
                                  const uint8_t* valid, uint8_t* dirty, int B, int H, int W, float* full_pcl,
                                  uint8_t* full_mask, int clear_flags, void* stream) {
  if (B < 0 || H <= 0 || W <= 0) return GLORIE_EINVAL;
  if (B == 0) return GLORIE_OK;
  if (!inv_poses || !disps_up || !intrinsics || !valid || !dirty || !full_pcl || !full_mask) return GLORIE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(iproj_dirty_kernel, dim3((unsigned)((H * W + kThreads - 1) / kThreads), (unsigned)B),
                     dim3(kThreads), 0, s, inv_poses, disps_up, intrinsics, valid, dirty, H, W, full_pcl, full_mask);
  if (glorie::check_launch()) return GLORIE_EHIP;
  if (!clear_flags) return GLORIE_OK;
  hipLaunchKernelGGL(clear_flags_kernel, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, dirty,
                     B);
  return glorie::check_launch();
}

extern "C" int glorie_proxy_depth(const float* full_pcl, const uint8_t* full_mask, int counter, int H, int W,
                                  int skip_row, const float* w2c, float fx, float fy, float cx, float cy,
                                  const float* droid_depth, const float* mono_depth, float* zbuf, float* out,
                                  void* stream) {
  if (counter < 0 || H <= 0 || W <= 0 || skip_row < -1 || skip_row >= H) return GLORIE_EINVAL;
  if (!droid_depth || !zbuf || !out) return GLORIE_EINVAL;
  if (counter > 0 && (!full_pcl || !full_mask || !w2c)) return GLORIE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  const dim3 grid_px((unsigned)((HW + kThreads - 1) / kThreads));
  unsigned* bits = reinterpret_cast<unsigned*>(zbuf);
  hipLaunchKernelGGL(fill_inf_kernel, grid_px, dim3(kThreads), 0, s, bits, HW);
  if (glorie::check_launch()) return GLORIE_EHIP;
  const long n = (long)counter * HW;
  if (n > 0 && glorie::launch_zbuf(full_pcl, full_mask, n, H, W, skip_row, w2c, fx, fy, cx, cy, bits, s))
    return GLORIE_EHIP;
  hipLaunchKernelGGL(proxy_finalize_kernel, grid_px, dim3(kThreads), 0, s, bits, droid_depth, mono_depth, HW, out);
  return glorie::check_launch();
}
