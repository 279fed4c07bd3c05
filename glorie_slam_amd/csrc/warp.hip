// Pixel-warping loss of the mapper (reference: src/mapper.py:326-388, projection src/utils/common.py:324-350).
//
// Every sampled ray's surface point X = o + d * depth is projected into the M frames of the mapping window; an entry
// (ray r, frame m) is kept when the projection (project of camera.hiph: common.py:336-350, uv = K p / (z + 1e-5),
// compiled here with the compiler's default contraction) lands more than 5 px inside the image, in front of the camera, in a frame
// other than the ray's own, and the ray has at least 4 such frames.  The kept entries' bilinear colour reads
// (grid_sample, align_corners=False, border padding) are compared with the ray's colour under smooth-L1 (beta 0.1) and
// averaged over 3 x the number of kept entries.
//
// Launches: pix_warp_fwd_kernel (one thread per ray: loss, kept count and the raw d loss / d depth of its ray, one
// fixed-order partial per workgroup), pix_warp_finish_kernel (one workgroup: the partials in index order -> loss and the
// gradient scale 1 / (3 count), both on the device), pix_warp_bwd_kernel (grad_depth = raw * g_out * scale).  No atomics:
// repeated calls are bitwise identical, and nothing the host sizes depends on the data (the term records into a hipGraph).
#include "camera.hiph"
#include "compact.hiph"

using namespace glorie;

namespace {

constexpr int kWarpThreads = 256;
constexpr int kWarpMaxFrames = 64;        // one bit per frame in the per-ray mask
constexpr int kWarpEdge = 5;              // pix_warping_edge (mapper.py:349)
constexpr float kWarpBeta = 0.1f;         // smooth_l1_loss(..., beta=0.1) (mapper.py:385)
constexpr float kProjEps = 1e-5f;

// w2c = inverse of the affine c2w [4,4] (bottom row 0 0 0 1), row-major 3x4, inverted in double.  torch.inverse of the
// reference agrees with it to fp32 rounding; a rigid c2w would allow R^T, the general form costs nothing here.
__device__ void affine_inverse(const float* c2w, float* w2c) {
  const double a = c2w[0], b = c2w[1], c = c2w[2], d = c2w[4], e = c2w[5], f = c2w[6], g = c2w[8], h = c2w[9],
               i = c2w[10];
  const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const double inv_det = 1.0 / (a * A + b * B + c * C);
  double R[9] = {A, -(b * i - c * h), b * f - c * e,
                 B, a * i - c * g, -(a * f - c * d),
                 C, -(a * h - b * g), a * e - b * d};
  for (int k = 0; k < 9; ++k) R[k] *= inv_det;
  const double t0 = c2w[3], t1 = c2w[7], t2 = c2w[11];
  for (int row = 0; row < 3; ++row) {
    w2c[row * 4 + 0] = (float)R[row * 3 + 0];
    w2c[row * 4 + 1] = (float)R[row * 3 + 1];
    w2c[row * 4 + 2] = (float)R[row * 3 + 2];
    w2c[row * 4 + 3] = (float)(-(R[row * 3 + 0] * t0 + R[row * 3 + 1] * t1 + R[row * 3 + 2] * t2));
  }
}

__device__ __forceinline__ float warp_texel(const float* img, int chw, int H, int W, int x, int y, int ch) {
  if (x < 0 || y < 0 || x >= W || y >= H) return 0.f;     // grid_sample's within_bounds: the corner contributes nothing
  return chw ? img[(size_t)ch * H * W + (size_t)y * W + x] : img[((size_t)y * W + x) * 3 + ch];
}

__global__ void __launch_bounds__(kWarpThreads)
pix_warp_fwd_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ depth,
                    const int64_t* __restrict__ ray_frame, int N, const float* __restrict__ c2ws,
                    const int64_t* __restrict__ frame_indices, int M, const float* __restrict__ images,
                    const float* const* __restrict__ frame_table, int chw, int H, int W, float fx, float fy, float cx,
                    float cy, const float* __restrict__ gt_color, double* __restrict__ part_loss,
                    long long* __restrict__ part_count, float* __restrict__ raw_grad) {
  __shared__ float w2c[kWarpMaxFrames][12];
  __shared__ int64_t fid[kWarpMaxFrames];
  __shared__ double red_loss[kWarpThreads];
  __shared__ long long red_count[kWarpThreads];
  const int tid = threadIdx.x;
  for (int m = tid; m < M; m += kWarpThreads) {
    affine_inverse(c2ws + 16 * m, w2c[m]);
    fid[m] = frame_indices[m];
  }
  __syncthreads();

  const int r = blockIdx.x * kWarpThreads + tid;
  float loss = 0.f, grad = 0.f;
  int kept = 0;
  if (r < N) {
    const float dep = depth[r];
    const int64_t own = ray_frame[r];
    const float ox = rays_o[3 * r], oy = rays_o[3 * r + 1], oz = rays_o[3 * r + 2];
    const float dx = rays_d[3 * r], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
    const float X = ox + dx * dep, Y = oy + dy * dep, Z = oz + dz * dep;
    uint64_t mask = 0;
    if (isfinite(dep)) {            // a non-finite depth projects nowhere (every comparison of the reference is false)
#pragma unroll 2                     // two frames per trip: their divisions overlap
      for (int m = 0; m < M; ++m) {
        const Proj p = project(w2c[m], X, Y, Z, fx, fy, cx, cy, kProjEps);
        const bool in = inside_edge(p.u, p.v, H, W, (float)kWarpEdge) && p.z < 0.f && fid[m] != own;
        if (in) mask |= 1ull << m;
      }
    }
    kept = __popcll(mask);
    if (kept < 4) {                 // mapper.py:367: at least 4 frames besides its own
      kept = 0;
      mask = 0;
    }
    const float g0 = gt_color[3 * r], g1 = gt_color[3 * r + 1], g2 = gt_color[3 * r + 2];
    for (int m = 0; m < M; ++m) {
      if (!((mask >> m) & 1ull)) continue;
      const float* w = w2c[m];
      const Proj p = project(w, X, Y, Z, fx, fy, cx, cy, kProjEps);
      // grid_sample's unnormalisation of u / W * 2 - 1 (align_corners=False), then the border clamp
      float ix = ((p.u / (float)W * 2.f - 1.f + 1.f) * (float)W - 1.f) * 0.5f;
      float iy = ((p.v / (float)H * 2.f - 1.f + 1.f) * (float)H - 1.f) * 0.5f;
      const float clip_x = (ix > 0.f && ix < (float)(W - 1)) ? 1.f : 0.f;
      const float clip_y = (iy > 0.f && iy < (float)(H - 1)) ? 1.f : 0.f;
      ix = fminf(fmaxf(ix, 0.f), (float)(W - 1));
      iy = fminf(fmaxf(iy, 0.f), (float)(H - 1));
      const float fx0 = floorf(ix), fy0 = floorf(iy);
      const int x0 = (int)fx0, y0 = (int)fy0;
      const float e = ix - fx0, s = iy - fy0, we = (fx0 + 1.f) - ix, ws = (fy0 + 1.f) - iy;
      const float* img = frame_table ? frame_table[m] : images + (size_t)m * H * W * 3;
      // d(a, b, c) / d depth = w2c_R . rays_d; u, v = (K row) . (-a, b, c) / z
      const float da = w[0] * dx + w[1] * dy + w[2] * dz;
      const float db = w[4] * dx + w[5] * dy + w[6] * dz;
      const float dc = w[8] * dx + w[9] * dy + w[10] * dz;
      const float du = (-fx * da + cx * dc - p.u * dc) / p.z;
      const float dv = (fy * db + cy * dc - p.v * dc) / p.z;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float vnw = warp_texel(img, chw, H, W, x0, y0, ch), vne = warp_texel(img, chw, H, W, x0 + 1, y0, ch);
        const float vsw = warp_texel(img, chw, H, W, x0, y0 + 1, ch), vse = warp_texel(img, chw, H, W, x0 + 1, y0 + 1, ch);
        const float val = vnw * we * ws + vne * e * ws + vsw * we * s + vse * e * s;
        const float gix = (vne - vnw) * ws + (vse - vsw) * s;
        const float giy = (vsw - vnw) * we + (vse - vne) * e;
        const float diff = val - (ch == 0 ? g0 : ch == 1 ? g1 : g2);
        const float ad = fabsf(diff);
        float dl;
        if (ad < kWarpBeta) {
          loss += 0.5f * ad * ad / kWarpBeta;
          dl = diff / kWarpBeta;
        } else {
          loss += ad - 0.5f * kWarpBeta;
          dl = diff > 0.f ? 1.f : -1.f;
        }
        grad += dl * (gix * clip_x * du + giy * clip_y * dv);
      }
    }
    raw_grad[r] = grad;
  }
  red_loss[tid] = (double)loss;
  red_count[tid] = kept;
  __syncthreads();
  for (int off = kWarpThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      red_loss[tid] += red_loss[tid + off];
      red_count[tid] += red_count[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part_loss[blockIdx.x] = red_loss[0];
    part_count[blockIdx.x] = red_count[0];
  }
}

__global__ void __launch_bounds__(kWarpThreads)
pix_warp_finish_kernel(const double* __restrict__ part_loss, const long long* __restrict__ part_count, int n_parts,
                       int nan_to_zero, float* __restrict__ loss, float* __restrict__ scale, int* __restrict__ count) {
  __shared__ double red_loss[kWarpThreads];
  __shared__ long long red_count[kWarpThreads];
  const int tid = threadIdx.x;
  double l = 0.0;
  long long c = 0;
  for (int i = tid; i < n_parts; i += kWarpThreads) {
    l += part_loss[i];
    c += part_count[i];
  }
  red_loss[tid] = l;
  red_count[tid] = c;
  __syncthreads();
  for (int off = kWarpThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      red_loss[tid] += red_loss[tid + off];
      red_count[tid] += red_count[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const long long n = red_count[0];
    // an empty selection: torch's mean of nothing is NaN and its gradient zero
    loss[0] = n > 0 ? (float)(red_loss[0] / (3.0 * (double)n)) : (nan_to_zero ? 0.f : __builtin_nanf(""));
    scale[0] = n > 0 ? (float)(1.0 / (3.0 * (double)n)) : 0.f;
    if (count) count[0] = (int)n;
  }
}

__global__ void pix_warp_bwd_kernel(const float* __restrict__ raw_grad, const float* __restrict__ scale,
                                    const float* __restrict__ grad_out, int N, float* __restrict__ grad_depth) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < N) grad_depth[r] = raw_grad[r] * (grad_out[0] * scale[0]);
}

inline int warp_parts(int N) { return (N + kWarpThreads - 1) / kWarpThreads; }

// workspace: per-workgroup loss double [parts] | kept count long long [parts]
struct WarpWs {
  Carver c;
  int parts;
  double* part_loss = c.take<double>(parts);
  long long* part_count = c.take<long long>(parts);
};

}  // namespace

extern "C" size_t glorie_pix_warp_workspace(int N) { return N < 0 ? 0 : carved_bytes<WarpWs>(warp_parts(N)); }

extern "C" int glorie_pix_warp_fwd(const float* rays_o, const float* rays_d, const float* depth, const int64_t* ray_frame,
                                   int N, const float* c2ws, const int64_t* frame_indices, int M, const float* images,
                                   const void* frame_table, int chw, int H, int W, float fx, float fy, float cx, float cy,
                                   const float* gt_color, int nan_to_zero, void* workspace, float* loss, float* raw_grad,
                                   float* scale, int* count, void* stream) {
  if (N < 0 || M < 0 || M > kWarpMaxFrames || H <= 2 * kWarpEdge || W <= 2 * kWarpEdge) return GLORIE_EINVAL;
  if (!loss || !scale) return GLORIE_EINVAL;
  const int parts = warp_parts(N);
  const WarpWs w{Carver(workspace), parts};
  if (N > 0) {
    if (!rays_o || !rays_d || !depth || !ray_frame || !gt_color || !raw_grad || !workspace) return GLORIE_EINVAL;
    if (M > 0 && (!c2ws || !frame_indices || (!images && !frame_table))) return GLORIE_EINVAL;
    hipLaunchKernelGGL(pix_warp_fwd_kernel, dim3(parts), dim3(kWarpThreads), 0, (hipStream_t)stream, rays_o, rays_d,
                       depth, ray_frame, N, c2ws, frame_indices, M, images,
                       reinterpret_cast<const float* const*>(frame_table), chw, H, W, fx, fy, cx, cy, gt_color,
                       w.part_loss, w.part_count, raw_grad);
    GLORIE_TRY(check_launch());
  }
  hipLaunchKernelGGL(pix_warp_finish_kernel, dim3(1), dim3(kWarpThreads), 0, (hipStream_t)stream, w.part_loss,
                     w.part_count, N > 0 ? parts : 0, nan_to_zero, loss, scale, count);
  return check_launch();
}

extern "C" int glorie_pix_warp_bwd(const float* raw_grad, const float* scale, const float* grad_out, int N,
                                   float* grad_depth, void* stream) {
  if (N < 0) return GLORIE_EINVAL;
  if (N == 0) return GLORIE_OK;
  if (!raw_grad || !scale || !grad_out || !grad_depth) return GLORIE_EINVAL;
  hipLaunchKernelGGL(pix_warp_bwd_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, raw_grad, scale,
                     grad_out, N, grad_depth);
  return check_launch();
}
