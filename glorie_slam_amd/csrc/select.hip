// Keyframe selection of the mapper: frustum feature selection and the keyframe overlap count
// (reference: src/mapper.py:126-174 Mapper.get_mask_from_c2w, :176-244 Mapper.keyframe_selection_overlap).
//
// Both take camera-to-world matrices in the renderer's OpenGL convention (what the reference passes after
// `c2w[:3, 1:3] *= -1`) and invert the rigid transform in the kernel: w2c = [R^T | -R^T t].  A point projects as in the
// reference: camera coordinates w2c . p, x negated, uv = K . cam, z = uv_z + 1e-5, uv = uv_xy / z (rigid_inverse,
// project and inside_edge of camera.hiph; compiled here with the compiler's default contraction).
//
// Frustum selection, four launches and one memset, no host synchronisation (the count stays on the device):
//   frustum_sample_kernel   one thread per point: project, sample the depth map bilinearly at (u, v) as
//                           cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) does - coordinates rounded to 1/32 px, weights
//                           and sum in fp32 (cv2 sums in its own order: the last bit may differ) - store (-z or -inf
//                           outside the edge band, sampled depth), and fold the sampled depth into a global maximum
//                           (an integer atomic max on an order-preserving key of the float: exact in any order)
//   frustum_mask_kernel     sampled depth 0 -> that maximum (`depths[zero_mask] = np.max(depths)`), keep when
//                           0 <= -z <= depth + 0.5; one kept count per workgroup (wave ballots, no atomics)
//   exclusive_scan_kernel   one workgroup: exclusive scan of the workgroup counts -> offsets and the total count
//   frustum_indices_kernel  (only when indices are asked for) the kept points' indices in ascending order
// The count, scan and rank steps are those of compact.hiph.
// Overlap count, one launch: overlap_count_kernel, one workgroup per keyframe, an integer sum over the ray samples.
// Every result is an integer decision or count: repeated calls are bitwise equal.
#include "camera.hiph"
#include "compact.hiph"

using namespace glorie;

namespace {

constexpr int kSelThreads = 256;          // 4 waves of 64
constexpr int kSelWaves = kSelThreads / 64;
constexpr float kProjEps = 1e-5f;         // z + 1e-5 (mapper.py, common.py)

__device__ __forceinline__ float depth_texel(const float* __restrict__ depth, int H, int W, int x, int y) {
  return (x < 0 || y < 0 || x >= W || y >= H) ? 0.f : depth[(size_t)y * W + x];
}

// cv2.remap(depth, u, v, INTER_LINEAR) with BORDER_CONSTANT 0 at one point: the map coordinate is rounded to a
// multiple of 1/32 px (INTER_BITS = 5, round to nearest even), neighbours outside the image read 0, a non-finite or far
// out coordinate samples 0
__device__ __forceinline__ float remap_linear(const float* __restrict__ depth, int H, int W, float u, float v) {
  if (!(u > -2.f && u < (float)W + 1.f && v > -2.f && v < (float)H + 1.f)) return 0.f;
  const int X = __float2int_rn(u * 32.f), Y = __float2int_rn(v * 32.f);
  const int x0 = X >> 5, y0 = Y >> 5;
  const float ax = (float)(X & 31) * (1.f / 32.f), ay = (float)(Y & 31) * (1.f / 32.f);
  const float w00 = (1.f - ay) * (1.f - ax), w01 = (1.f - ay) * ax, w10 = ay * (1.f - ax), w11 = ay * ax;
  return depth_texel(depth, H, W, x0, y0) * w00 + depth_texel(depth, H, W, x0 + 1, y0) * w01 +
         depth_texel(depth, H, W, x0, y0 + 1) * w10 + depth_texel(depth, H, W, x0 + 1, y0 + 1) * w11;
}

__global__ void __launch_bounds__(kSelThreads)
frustum_sample_kernel(const float* __restrict__ points, int n, const float* __restrict__ c2w, float fx, float fy,
                      float cx, float cy, int H, int W, float edge, const float* __restrict__ depth,
                      float2* __restrict__ zd, unsigned int* __restrict__ max_key) {
  const Rigid w = rigid_inverse(c2w);
  const int i = blockIdx.x * kSelThreads + threadIdx.x;
  unsigned int key = 0;
  if (i < n) {
    const Proj p = project(w.r, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], fx, fy,
                           cx, cy, kProjEps);
    const float s = remap_linear(depth, H, W, p.u, p.v);
    zd[i] = make_float2(inside_edge(p.u, p.v, H, W, edge) ? -p.z : -INFINITY, s);
    key = float_key(s);
  }
  // workgroup maximum, then one atomic per workgroup
  key = block_max<kSelWaves>(key);
  if (threadIdx.x == 0) atomicMax(max_key, key);
}

__global__ void __launch_bounds__(kSelThreads)
frustum_mask_kernel(const float2* __restrict__ zd, int n, const unsigned int* __restrict__ max_key,
                    unsigned char* __restrict__ mask, int* __restrict__ block_count) {
  __shared__ int red[kSelWaves];
  const float dmax = key_float(*max_key);
  const int i = blockIdx.x * kSelThreads + threadIdx.x;
  bool keep = false;
  if (i < n) {
    const float2 e = zd[i];
    const float d = e.y == 0.f ? dmax : e.y;
    keep = 0.f <= e.x && e.x <= d + 0.5f;
    mask[i] = keep ? 1 : 0;
  }
  wave_count(keep, red);
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = slot_sum(red, kSelWaves);
}

__global__ void __launch_bounds__(kSelThreads)
frustum_indices_kernel(const unsigned char* __restrict__ mask, int n, const int* __restrict__ offsets,
                       int64_t* __restrict__ indices) {
  __shared__ int wave_base[kSelWaves];
  const int i = blockIdx.x * kSelThreads + threadIdx.x;
  const bool keep = i < n && mask[i] != 0;
  const unsigned long long b = wave_count(keep, wave_base);
  __syncthreads();
  if (keep) indices[offsets[blockIdx.x] + block_rank(b, wave_base)] = i;
}

// one workgroup per keyframe: samples z = near (1 - t) + far t of every ray with depth > 0 (near = 0.8 d, far = d + 0.5,
// t = linspace(0, 1, n_samples)), counted when edge < u < W - edge, edge < v < H - edge and z < 0
__global__ void __launch_bounds__(kSelThreads)
overlap_count_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                     const float* __restrict__ depth, int R, int n_samples, const float* __restrict__ c2ws, float fx,
                     float fy, float cx, float cy, int H, int W, float edge, int* __restrict__ inside) {
  const Rigid w = rigid_inverse(c2ws + 16 * (size_t)blockIdx.x);
  const int total = R * n_samples;
  const float step = n_samples > 1 ? 1.f / (float)(n_samples - 1) : 0.f;
  int count = 0;
  for (int e = threadIdx.x; e < total; e += kSelThreads) {
    const int r = e / n_samples, s = e - r * n_samples;
    const float d = depth[r];
    if (!(d > 0.f)) continue;                                   // get_samples(..., depth_filter=True)
    // torch.linspace(0, 1, S): a single sample is the start; else the first half from the start, the rest from the end
    const float t = n_samples == 1 ? 0.f
                    : s < n_samples / 2 ? (float)s * step : 1.f - (float)(n_samples - 1 - s) * step;
    const float zs = (0.8f * d) * (1.f - t) + (d + 0.5f) * t;
    const Proj p = project(w.r, rays_o[3 * r] + rays_d[3 * r] * zs, rays_o[3 * r + 1] + rays_d[3 * r + 1] * zs,
                           rays_o[3 * r + 2] + rays_d[3 * r + 2] * zs, fx, fy, cx, cy, kProjEps);
    count += (inside_edge(p.u, p.v, H, W, edge) && p.z < 0.f) ? 1 : 0;
  }
  count = block_sum<kSelWaves>(count);
  if (threadIdx.x == 0) inside[blockIdx.x] = count;
}

inline int sel_blocks(int n) { return (n + kSelThreads - 1) / kSelThreads; }

// workspace layout: zd float2 [n] | block counts int [B] | offsets int [B] | max key uint (8-byte aligned pieces)
struct FrustumWs {
  Carver c;
  int n;
  float2* zd = c.take<float2>(n);
  int* block_count = c.take<int>(sel_blocks(n));
  int* offsets = c.take<int>(sel_blocks(n));
  unsigned int* max_key = c.take<unsigned int>(1);
};

__global__ void __launch_bounds__(kScanThreads)
exclusive_scan_kernel(const int* __restrict__ counts, int n, int* __restrict__ offsets, int* __restrict__ total) {
  const int* const in[1] = {counts};
  int* const out[1] = {offsets};
  int sum[1];
  block_exclusive_scan<1>(in, out, n, sum);
  if (total && threadIdx.x == 0) total[0] = sum[0];
}

}  // namespace

int glorie::launch_exclusive_scan(const int* counts, int n, int* offsets, int* total, hipStream_t st) {
  hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, counts, n, offsets, total);
  return check_launch();
}

extern "C" size_t glorie_frustum_select_workspace(int n) { return n < 0 ? 0 : carved_bytes<FrustumWs>(n); }

extern "C" int glorie_frustum_select(const float* points, int n, const float* c2w, float fx, float fy, float cx,
                                     float cy, int H, int W, float edge, const float* depth, void* workspace,
                                     unsigned char* mask, int* count, int64_t* indices, void* stream) {
  if (n < 0 || H <= 0 || W <= 0 || !count) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return check_hip(hipMemsetAsync(count, 0, sizeof(int), st));
  if (!points || !c2w || !depth || !workspace || !mask) return GLORIE_EINVAL;
  const int B = sel_blocks(n);
  const FrustumWs w{Carver(workspace), n};
  GLORIE_TRY(check_hip(hipMemsetAsync(w.max_key, 0, sizeof(unsigned int), st)));
  hipLaunchKernelGGL(frustum_sample_kernel, dim3(B), dim3(kSelThreads), 0, st, points, n, c2w, fx, fy, cx, cy, H, W,
                     edge, depth, w.zd, w.max_key);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(frustum_mask_kernel, dim3(B), dim3(kSelThreads), 0, st, w.zd, n, w.max_key, mask, w.block_count);
  GLORIE_TRY(check_launch());
  GLORIE_TRY(launch_exclusive_scan(w.block_count, B, w.offsets, count, st));
  if (indices) {
    hipLaunchKernelGGL(frustum_indices_kernel, dim3(B), dim3(kSelThreads), 0, st, mask, n, w.offsets, indices);
    GLORIE_TRY(check_launch());
  }
  return GLORIE_OK;
}

extern "C" int glorie_keyframe_overlap(const float* rays_o, const float* rays_d, const float* depth, int R,
                                       int n_samples, const float* c2ws, int K, float fx, float fy, float cx, float cy,
                                       int H, int W, float edge, int* inside, void* stream) {
  if (R < 0 || K < 0 || n_samples < 1 || H <= 0 || W <= 0) return GLORIE_EINVAL;
  if ((long long)R * n_samples > 0x7fffffffLL) return GLORIE_EINVAL;
  if (K == 0) return GLORIE_OK;
  if (!c2ws || !inside) return GLORIE_EINVAL;
  if (R > 0 && (!rays_o || !rays_d || !depth)) return GLORIE_EINVAL;
  hipLaunchKernelGGL(overlap_count_kernel, dim3(K), dim3(kSelThreads), 0, (hipStream_t)stream, rays_o, rays_d, depth,
                     R, n_samples, c2ws, fx, fy, cx, cy, H, W, edge, inside);
  return check_launch();
}
