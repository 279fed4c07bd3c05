// Mesh evaluation (reference: src/utils/eval_recon.py): area-weighted surface sampling, the moment sums of a
// point-to-point ICP step, the nearest-neighbour statistics behind accuracy / completion / completion ratio, a triangle
// rasteriser for the depth-L1 views, the projection test of the unseen points and the per-view depth-L1 accumulator.
//
// Sums: every sum that is reported is a per-workgroup fp64 partial (lanes -> wave -> workgroup in a fixed order) added by
//   ordered_sum in a second launch; no floating-point atomics, repeated calls are bitwise equal.
// Area CDF, 3 launches: a workgroup scans 256 areas, one workgroup scans the workgroup totals, a third launch adds them.
// Rasteriser, 4 launches (fill, small, large, resolve), all in fp64 from the fp32 inputs:
//   A triangle is never clipped into new vertices.  With the camera-space vertices v0, v1, v2 and the pixel's ray
//   d = ((u - cx) / fx, (v - cy) / fy, 1) the line t d meets the triangle's plane inside the triangle when
//   e0 = d . (v1 x v2), e1 = d . (v2 x v0), e2 = d . (v0 x v1) have one sign (zero included), at the camera-frame depth
//   z = v0 . (v1 x v2) / (e0 + e1 + e2); z_near < z <= z_far then keeps exactly the part in front of the near plane, which
//   is what clipping against z = z_near into one or two triangles keeps.  The clipped polygon is formed only to bound the
//   pixels that are visited.  The cross product of an edge is always taken with its end points in lexicographic order (and
//   negated when that swaps them), so two triangles that share an edge evaluate bit-identical edge values of opposite
//   sign: with inclusive edges there are no pin-holes, and double cover is harmless under the minimum.
//   One lane sets a triangle up and walks its pixel box when that has at most kSmallBox pixels; larger boxes are queued
//   (an integer atomic for the slot; the depth is a minimum, so the queue's order does not matter) and a second launch
//   spreads every queued triangle over up to kChunks workgroups.  Depth: atomicMin on the bits of the positive fp32 depth.
#include <float.h>
#include "compact.hiph"

using namespace glorie;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSmallBox = 256;                // pixels of a box one lane still walks by itself
constexpr int kChunks = 64;                   // workgroups one queued triangle is spread over, at most
constexpr int kChunkPixels = 4 * kThreads;    // pixels per workgroup that justify another one
constexpr int kSlots = 256;                   // grid.y of the large launch: queued triangles taken in parallel
constexpr unsigned kInfBits = 0x7f800000u;

inline int reduce_blocks(long long n) { return capped_blocks(n, kThreads); }

// the N sums of a workgroup's threads -> out[0..N); once per kernel (block_reduce is single use)
template <int N>
__device__ __forceinline__ void block_partials(const double (&s)[N], double* __restrict__ out) {
  const double t = block_sum<kWaves>(s);
  if (threadIdx.x < N) out[threadIdx.x] = t;
}

// out[s] = sum over the workgroups of partial[b * n_series + s]; n_blocks == 0 gives zeros
__global__ void __launch_bounds__(kThreads)
sum_finish_kernel(const double* __restrict__ partial, int n_blocks, int n_series, double* __restrict__ out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int s = wave; s < n_series; s += kWaves) {
    const double t = ordered_sum(partial + s, n_blocks, n_series);
    if (lane == 0) out[s] = t;
  }
}

// ---- triangles --------------------------------------------------------------------------------------------------------
struct Tri {
  double p[3][3];
  bool ok;
};

__device__ __forceinline__ Tri load_triangle(const float* __restrict__ vertices, int V, const int* __restrict__ faces,
                                             long long f) {
  Tri t;
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  t.ok = i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
  const int idx[3] = {t.ok ? i0 : 0, t.ok ? i1 : 0, t.ok ? i2 : 0};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) t.p[k][a] = t.ok ? (double)vertices[(size_t)idx[k] * 3 + a] : 0.0;
  return t;
}

// the differences of fp32 values are exact in fp64; products and sums are rounded
__device__ __forceinline__ double triangle_area(const Tri& t) {
#pragma clang fp contract(off)
  const double ax = t.p[1][0] - t.p[0][0], ay = t.p[1][1] - t.p[0][1], az = t.p[1][2] - t.p[0][2];
  const double bx = t.p[2][0] - t.p[0][0], by = t.p[2][1] - t.p[0][1], bz = t.p[2][2] - t.p[0][2];
  const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  return 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
}

// ---- area CDF -----------------------------------------------------------------------------------------------------------
// inclusive scan over the workgroup's 256 values (the last thread holds the total)
__device__ __forceinline__ double block_inclusive_scan(double v, double* sh) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) sh[wv] = inc;
  __syncthreads();
  double base = 0.0;
  for (int i = 0; i < wv; ++i) base += sh[i];
  return base + inc;
}

__global__ void __launch_bounds__(kThreads)
area_scan_kernel(const float* __restrict__ vertices, int V, const int* __restrict__ faces, long long F,
                 double* __restrict__ cdf, double* __restrict__ block_total, int* __restrict__ bad) {
  __shared__ double sh[kWaves];
  const long long f = (long long)blockIdx.x * kThreads + threadIdx.x;
  double a = 0.0;
  if (f < F) {
    const Tri t = load_triangle(vertices, V, faces, f);
    if (!t.ok) atomicOr(bad, 1);
    a = t.ok ? triangle_area(t) : 0.0;
  }
  const double inc = block_inclusive_scan(a, sh);
  if (f < F) cdf[f] = inc;
  if (threadIdx.x == kThreads - 1) block_total[blockIdx.x] = inc;
}

// exclusive scan of the workgroup totals, in place: thread t owns a contiguous run
__global__ void __launch_bounds__(kThreads)
area_offsets_kernel(double* __restrict__ block_total, int n_blocks) {
  __shared__ double sh[kWaves];
  const int run = (n_blocks + kThreads - 1) / kThreads;
  const int j0 = min(n_blocks, (int)threadIdx.x * run), j1 = min(n_blocks, j0 + run);
  double s = 0.0;
  for (int j = j0; j < j1; ++j) s += block_total[j];
  double base = block_inclusive_scan(s, sh) - s;
  for (int j = j0; j < j1; ++j) {
    const double v = block_total[j];
    block_total[j] = base;
    base += v;
  }
}

// out = {cdf[F-1], bad as a double}
__global__ void __launch_bounds__(kThreads)
area_add_kernel(double* __restrict__ cdf, long long F, const double* __restrict__ offsets, const int* __restrict__ bad,
                double* __restrict__ out) {
  const long long f = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const double v = blockIdx.x ? offsets[blockIdx.x] + cdf[f] : cdf[f];
  cdf[f] = v;
  if (f == F - 1) {
    out[0] = v;
    out[1] = (double)bad[0];
  }
}

// ---- sampling -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
mesh_sample_kernel(const float* __restrict__ vertices, int V, const int* __restrict__ faces, int F,
                   const double* __restrict__ cdf, const float* __restrict__ u, long long n, float* __restrict__ points,
                   int* __restrict__ face_of) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double total = cdf[F - 1];
  const double x = (double)u[3 * i] * total;
  int lo = 0, hi = F;
  while (lo < hi) {                                    // the first face with cdf > x
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] > x) hi = mid; else lo = mid + 1;
  }
  int f = min(lo, F - 1);
  Tri t = load_triangle(vertices, V, faces, f);
  // a face without area is never drawn: u0 = 1 (x = total) and the last bits of a parallel prefix sum could point at one
  for (int step = 0; step < 2 && (!t.ok || triangle_area(t) == 0.0); ++step) {
    const int dir = step ? -1 : 1;
    int g = f;
    while (g + dir >= 0 && g + dir < F) {
      g += dir;
      t = load_triangle(vertices, V, faces, g);
      if (t.ok && triangle_area(t) != 0.0) break;
    }
    f = g;
  }
  double a = (double)u[3 * i + 1], b = (double)u[3 * i + 2];
  if (a + b > 1.0) {
    a = 1.0 - a;
    b = 1.0 - b;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    points[3 * i + c] = t.ok ? (float)(t.p[0][c] + a * (t.p[1][c] - t.p[0][c]) + b * (t.p[2][c] - t.p[0][c])) : 0.f;
  face_of[i] = t.ok ? f : -1;
}

// ---- rigid transform ----------------------------------------------------------------------------------------------------
struct Mat34 {
  double m[12];
};

__global__ void __launch_bounds__(kThreads)
transform_points_kernel(Mat34 T, const float* __restrict__ in, long long n, float* __restrict__ out) {
#pragma clang fp contract(off)
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const double x = (double)in[3 * i], y = (double)in[3 * i + 1], z = (double)in[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
      out[3 * i + r] = (float)(((T.m[4 * r] * x + T.m[4 * r + 1] * y) + T.m[4 * r + 2] * z) + T.m[4 * r + 3]);
  }
}

// ---- ICP moments --------------------------------------------------------------------------------------------------------
// s = {count, sum p [3], sum q [3], sum p q^T [9] row-major, sum |p - q|^2}
__global__ void __launch_bounds__(kThreads)
icp_moments_kernel(const float* __restrict__ src, long long n, const float* __restrict__ tgt, long long m,
                   const int64_t* __restrict__ I, const float* __restrict__ D, float max_d2, double* __restrict__ partial) {
#pragma clang fp contract(off)
  double s[17];
#pragma unroll
  for (int q = 0; q < 17; ++q) s[q] = 0.0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const long long j = I[i];
    if (j < 0 || j >= m || !(D[i] < max_d2)) continue;
    double p[3], q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      p[a] = (double)src[3 * i + a];
      q[a] = (double)tgt[3 * j + a];
    }
    s[0] += 1.0;
    double d2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s[1 + a] += p[a];
      s[4 + a] += q[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) s[7 + 3 * a + b] += p[a] * q[b];
      const double d = p[a] - q[a];
      d2 += d * d;
    }
    s[16] += d2;
  }
  block_partials<17>(s, partial + (size_t)blockIdx.x * 17);
}

// ---- nearest-neighbour statistics -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
nn_stats_kernel(const float* __restrict__ D, long long Q, double threshold, double* __restrict__ partial) {
  double s[3] = {0.0, 0.0, 0.0};
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < Q; i += (long long)gridDim.x * kThreads) {
    const double d2 = (double)D[i];
    const double d = sqrt(d2);
    s[0] += d;
    s[1] += d < threshold ? 1.0 : 0.0;
    s[2] += d2;
  }
  block_partials<3>(s, partial + (size_t)blockIdx.x * 3);
}

// ---- rasteriser ---------------------------------------------------------------------------------------------------------
struct Camera {
  double fx, fy, cx, cy, z_near, z_far;
  int H, W;
};

struct RasterTri {
  double n[3][3];           // n[i] . d = e_i
  double det;
  int x0, x1, y0, y1;       // inclusive pixel box; x1 < x0: nothing to draw
};

__device__ __forceinline__ bool lex_less(const double* a, const double* b) {
  if (a[0] != b[0]) return a[0] < b[0];
  if (a[1] != b[1]) return a[1] < b[1];
  return a[2] < b[2];
}

// a x b with the end points in lexicographic order, negated when that swapped them
__device__ __forceinline__ void edge_cross(const double* a, const double* b, double* n) {
#pragma clang fp contract(off)
  const bool swap = lex_less(b, a);
  const double* p = swap ? b : a;
  const double* q = swap ? a : b;
  const double x = p[1] * q[2] - p[2] * q[1], y = p[2] * q[0] - p[0] * q[2], z = p[0] * q[1] - p[1] * q[0];
  n[0] = swap ? -x : x;
  n[1] = swap ? -y : y;
  n[2] = swap ? -z : z;
}

__device__ __forceinline__ RasterTri raster_setup(const float* __restrict__ vertices, int V, const int* __restrict__ faces,
                                                  long long f, const float* __restrict__ w2c, const Camera& cam) {
#pragma clang fp contract(off)
  RasterTri r;
  r.x0 = r.y0 = 0;
  r.x1 = r.y1 = -1;
  r.det = 0.0;
  const Tri t = load_triangle(vertices, V, faces, f);
  if (!t.ok) return r;
  double v[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a)
      v[k][a] = (((double)w2c[4 * a] * t.p[k][0] + (double)w2c[4 * a + 1] * t.p[k][1]) + (double)w2c[4 * a + 2] * t.p[k][2]) +
                (double)w2c[4 * a + 3];
  const double zn = cam.z_near;
  if (v[0][2] <= zn && v[1][2] <= zn && v[2][2] <= zn) return r;
  if (v[0][2] > cam.z_far && v[1][2] > cam.z_far && v[2][2] > cam.z_far) return r;
  // the box of the polygon in front of the near plane
  double ulo = DBL_MAX, uhi = -DBL_MAX, vlo = DBL_MAX, vhi = -DBL_MAX;
  auto add = [&](double x, double y, double z) {
    const double pu = cam.fx * x / z + cam.cx, pv = cam.fy * y / z + cam.cy;
    ulo = fmin(ulo, pu);
    uhi = fmax(uhi, pu);
    vlo = fmin(vlo, pv);
    vhi = fmax(vhi, pv);
  };
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double* a = v[k];
    const double* b = v[(k + 1) % 3];
    const bool fa = a[2] > zn, fb = b[2] > zn;
    if (fa) add(a[0], a[1], a[2]);
    if (fa != fb) {
      const double s = (zn - a[2]) / (b[2] - a[2]);
      add(a[0] + s * (b[0] - a[0]), a[1] + s * (b[1] - a[1]), zn);
    }
  }
  if (!(ulo <= uhi) || !(vlo <= vhi)) return r;               // also catches a NaN
  if (uhi < 0.0 || vhi < 0.0 || ulo > (double)(cam.W - 1) || vlo > (double)(cam.H - 1)) return r;
  edge_cross(v[1], v[2], r.n[0]);
  edge_cross(v[2], v[0], r.n[1]);
  edge_cross(v[0], v[1], r.n[2]);
  r.det = (v[0][0] * r.n[0][0] + v[0][1] * r.n[0][1]) + v[0][2] * r.n[0][2];
  r.x0 = (int)floor(fmax(ulo, 0.0));
  r.y0 = (int)floor(fmax(vlo, 0.0));
  r.x1 = (int)ceil(fmin(uhi, (double)(cam.W - 1)));
  r.y1 = (int)ceil(fmin(vhi, (double)(cam.H - 1)));
  return r;
}

__device__ __forceinline__ void raster_pixel(const RasterTri& r, const Camera& cam, int px, int py,
                                             unsigned* __restrict__ depth_bits) {
#pragma clang fp contract(off)
  const double dx = ((double)px - cam.cx) / cam.fx, dy = ((double)py - cam.cy) / cam.fy;
  const double e0 = (dx * r.n[0][0] + dy * r.n[0][1]) + r.n[0][2];
  const double e1 = (dx * r.n[1][0] + dy * r.n[1][1]) + r.n[1][2];
  const double e2 = (dx * r.n[2][0] + dy * r.n[2][1]) + r.n[2][2];
  const bool inside = (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
  if (!inside) return;
  const double s = (e0 + e1) + e2;
  if (s == 0.0) return;
  const double z = r.det / s;
  if (!(z > cam.z_near && z <= cam.z_far)) return;
  const unsigned bits = __float_as_uint((float)z);
  unsigned* cell = depth_bits + (size_t)py * cam.W + px;
  if (bits < *cell) atomicMin(cell, bits);
}

__global__ void __launch_bounds__(kThreads)
raster_fill_kernel(unsigned* __restrict__ depth_bits, long long n_pix, int* __restrict__ queue_count) {
  if (blockIdx.x == 0 && threadIdx.x == 0) queue_count[0] = 0;
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < n_pix; p += (long long)gridDim.x * kThreads)
    depth_bits[p] = kInfBits;
}

__global__ void __launch_bounds__(kThreads)
raster_small_kernel(const float* __restrict__ vertices, int V, const int* __restrict__ faces, int F,
                    const float* __restrict__ w2c, Camera cam, int policy, unsigned* __restrict__ depth_bits,
                    int* __restrict__ queue_count, int* __restrict__ queue) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const RasterTri r = raster_setup(vertices, V, faces, f, w2c, cam);
  if (r.x1 < r.x0 || r.y1 < r.y0) return;
  const long long box = (long long)(r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1);
  if (policy == 2 || (policy == 0 && box > kSmallBox)) {
    queue[atomicAdd(queue_count, 1)] = f;                     // at most F entries: every triangle queues itself once
    return;
  }
  for (int py = r.y0; py <= r.y1; ++py)
    for (int px = r.x0; px <= r.x1; ++px) raster_pixel(r, cam, px, py, depth_bits);
}

// workgroup (c, s): chunk c of the queued triangles s, s + gridDim.y, ...
__global__ void __launch_bounds__(kThreads)
raster_large_kernel(const float* __restrict__ vertices, int V, const int* __restrict__ faces, int F,
                    const float* __restrict__ w2c, Camera cam, unsigned* __restrict__ depth_bits,
                    const int* __restrict__ queue_count, const int* __restrict__ queue) {
  const int n_queued = min(queue_count[0], F);
  for (int j = blockIdx.y; j < n_queued; j += gridDim.y) {
    const int f = queue[j];
    if (f < 0 || f >= F) continue;
    const RasterTri r = raster_setup(vertices, V, faces, f, w2c, cam);
    if (r.x1 < r.x0 || r.y1 < r.y0) continue;
    const int w = r.x1 - r.x0 + 1;
    const long long box = (long long)w * (r.y1 - r.y0 + 1);
    const int chunks = (int)min((long long)kChunks, (box + kChunkPixels - 1) / kChunkPixels);
    if ((int)blockIdx.x >= chunks) continue;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < box; i += (long long)chunks * kThreads)
      raster_pixel(r, cam, r.x0 + (int)(i % w), r.y0 + (int)(i / w), depth_bits);
  }
}

__global__ void __launch_bounds__(kThreads)
raster_resolve_kernel(const unsigned* __restrict__ depth_bits, long long n_pix, float* __restrict__ depth) {
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < n_pix; p += (long long)gridDim.x * kThreads) {
    const unsigned b = depth_bits[p];
    depth[p] = b == kInfBits ? 0.f : __uint_as_float(b);
  }
}

// ---- check_proj ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
points_in_view_kernel(const float* __restrict__ points, long long n, const float* __restrict__ w2c, Camera cam, double edge,
                      int* __restrict__ count) {
#pragma clang fp contract(off)
  int c = 0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const double x = (double)points[3 * i], y = (double)points[3 * i + 1], z = (double)points[3 * i + 2];
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
      p[a] = (((double)w2c[4 * a] * x + (double)w2c[4 * a + 1] * y) + (double)w2c[4 * a + 2] * z) + (double)w2c[4 * a + 3];
    if (p[2] > 0.0) {
      const double pu = cam.fx * p[0] / p[2] + cam.cx, pv = cam.fy * p[1] / p[2] + cam.cy;
      c += (pu > edge && pu < (double)cam.W - edge && pv > edge && pv < (double)cam.H - edge) ? 1 : 0;
    }
  }
  c = block_sum<kWaves>(c);
  if (threadIdx.x == 0 && c) atomicAdd(count, c);
}

// ---- depth L1 -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
depth_l1_kernel(const float* __restrict__ gt, const float* __restrict__ rec, long long n_pix, double* __restrict__ partial) {
  double s[2] = {0.0, 0.0};
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < n_pix; p += (long long)gridDim.x * kThreads) {
    const float r = rec[p];
    if (r > 0.f) {
      s[0] += fabs((double)gt[p] - (double)r);
      s[1] += 1.0;
    }
  }
  block_partials<2>(s, partial + (size_t)blockIdx.x * 2);
}

__global__ void __launch_bounds__(64)
depth_l1_finish_kernel(const double* __restrict__ partial, int n_blocks, double* __restrict__ err, int* __restrict__ valid,
                       int view) {
  const double sum = ordered_sum(partial, n_blocks, 2);
  const double cnt = ordered_sum(partial + 1, n_blocks, 2);
  if (threadIdx.x == 0) {
    err[view] = cnt > 0.0 ? sum / cnt : 0.0;
    valid[view] = (int)cnt;
  }
}

bool make_camera(float fx, float fy, float cx, float cy, int H, int W, float z_near, float z_far, Camera* cam) {
  if (H <= 0 || W <= 0 || (long long)H * W > INT32_MAX || !(fx > 0.f) || !(fy > 0.f)) return false;
  cam->fx = fx;
  cam->fy = fy;
  cam->cx = cx;
  cam->cy = cy;
  cam->z_near = z_near;
  cam->z_far = z_far;
  cam->H = H;
  cam->W = W;
  return true;
}

// workspace of the area CDF: workgroup totals double [ceil(F / 256)] | out double [2] | bad int [2]
struct AreaWs {
  Carver c;
  int F;
  double* totals = c.take<double>((F + kThreads - 1) / kThreads);
  double* out = c.take<double>(2);
  int* bad = c.take<int>(2);
};

// workspace of the rasteriser: queue count int [2] | queue int [F]
struct RasterWs {
  Carver c;
  int F;
  int* queue_count = c.take<int>(2);
  int* queue = c.take<int>(F);
};

}  // namespace

extern "C" size_t glorie_mesh_area_cdf_workspace(int F) { return F <= 0 ? 0 : carved_bytes<AreaWs>(F); }

extern "C" int glorie_mesh_area_cdf(const float* vertices, int V, const int* faces, int F, double* cdf, void* workspace,
                                    double* total_out, void* stream) {
  if (V <= 0 || F <= 0 || !vertices || !faces || !cdf || !workspace || !total_out) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (F + kThreads - 1) / kThreads;
  const AreaWs w{Carver(workspace), F};
  GLORIE_TRY(check_hip(hipMemsetAsync(w.bad, 0, 2 * sizeof(int), st)));
  hipLaunchKernelGGL(area_scan_kernel, dim3(blocks), dim3(kThreads), 0, st, vertices, V, faces, (long long)F, cdf,
                     w.totals, w.bad);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(area_offsets_kernel, dim3(1), dim3(kThreads), 0, st, w.totals, blocks);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(area_add_kernel, dim3(blocks), dim3(kThreads), 0, st, cdf, (long long)F, w.totals, w.bad, w.out);
  GLORIE_TRY(check_launch());
  double host[2] = {0.0, 0.0};
  GLORIE_TRY(check_hip(hipMemcpyAsync(host, w.out, sizeof(host), hipMemcpyDeviceToHost, st)));
  GLORIE_TRY(check_hip(hipStreamSynchronize(st)));
  *total_out = host[0];
  return host[1] != 0.0 ? GLORIE_EINVAL : GLORIE_OK;
}

extern "C" int glorie_mesh_sample(const float* vertices, int V, const int* faces, int F, const double* cdf, const float* u,
                                  int n, float* points, int* face_of, void* stream) {
  if (V <= 0 || F <= 0 || n < 0 || !vertices || !faces || !cdf) return GLORIE_EINVAL;
  if (n == 0) return GLORIE_OK;
  if (!u || !points || !face_of) return GLORIE_EINVAL;
  hipLaunchKernelGGL(mesh_sample_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream,
                     vertices, V, faces, F, cdf, u, (long long)n, points, face_of);
  return check_launch();
}

extern "C" int glorie_transform_points(const double* T, const float* in, int n, float* out, void* stream) {
  if (!T || n < 0) return GLORIE_EINVAL;
  if (n == 0) return GLORIE_OK;
  if (!in || !out) return GLORIE_EINVAL;
  Mat34 m;
  for (int i = 0; i < 12; ++i) m.m[i] = T[i];
  hipLaunchKernelGGL(transform_points_kernel, dim3(reduce_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, m, in,
                     (long long)n, out);
  return check_launch();
}

extern "C" size_t glorie_icp_moments_workspace(int n) {
  if (n <= 0) return 0;
  return 17 * (size_t)reduce_blocks(n) * sizeof(double);
}

extern "C" int glorie_icp_moments(const float* src, int n, const float* tgt, int m, const int64_t* I, const float* D,
                                  float max_d2, void* workspace, double* out, void* stream) {
  if (n <= 0 || m <= 0 || !src || !tgt || !I || !D || !workspace || !out) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = reduce_blocks(n);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(icp_moments_kernel, dim3(blocks), dim3(kThreads), 0, st, src, (long long)n, tgt, (long long)m, I, D,
                     max_d2, partial);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(kThreads), 0, st, partial, blocks, 17, out);
  return check_launch();
}

extern "C" size_t glorie_nn_stats_workspace(int Q) {
  if (Q <= 0) return 0;
  return 3 * (size_t)reduce_blocks(Q) * sizeof(double);
}

extern "C" int glorie_nn_stats(const float* D, int Q, float threshold, void* workspace, double* out, void* stream) {
  if (Q < 0 || !out || (Q > 0 && (!D || !workspace))) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = Q > 0 ? reduce_blocks(Q) : 0;
  double* partial = reinterpret_cast<double*>(workspace);
  if (Q > 0) {
    hipLaunchKernelGGL(nn_stats_kernel, dim3(blocks), dim3(kThreads), 0, st, D, (long long)Q, (double)threshold, partial);
    GLORIE_TRY(check_launch());
  }
  hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(kThreads), 0, st, partial, blocks, 3, out);
  return check_launch();
}

extern "C" size_t glorie_mesh_depth_workspace(int F) { return F <= 0 ? 0 : carved_bytes<RasterWs>(F); }

extern "C" int glorie_mesh_depth(const float* vertices, int V, const int* faces, int F, const float* w2c, float fx, float fy,
                                 float cx, float cy, int H, int W, float z_near, float z_far, int policy, void* workspace,
                                 unsigned* depth_bits, float* depth, void* stream) {
  Camera cam;
  if (V <= 0 || F < 0 || !w2c || !depth_bits || !depth || policy < 0 || policy > 2) return GLORIE_EINVAL;
  if (F > 0 && (!vertices || !faces || !workspace)) return GLORIE_EINVAL;
  if (!make_camera(fx, fy, cx, cy, H, W, z_near, z_far, &cam) || !(z_near > 0.f) || !(z_far > z_near)) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long long n_pix = (long long)H * W;
  if (F > 0) {
    const RasterWs w{Carver(workspace), F};
    hipLaunchKernelGGL(raster_fill_kernel, dim3(reduce_blocks(n_pix)), dim3(kThreads), 0, st, depth_bits, n_pix,
                       w.queue_count);
    GLORIE_TRY(check_launch());
    hipLaunchKernelGGL(raster_small_kernel, dim3((F + kThreads - 1) / kThreads), dim3(kThreads), 0, st, vertices, V, faces, F,
                       w2c, cam, policy, depth_bits, w.queue_count, w.queue);
    GLORIE_TRY(check_launch());
    if (policy != 1) {
      hipLaunchKernelGGL(raster_large_kernel, dim3(kChunks, F < kSlots ? F : kSlots), dim3(kThreads), 0, st, vertices, V,
                         faces, F, w2c, cam, depth_bits, w.queue_count, w.queue);
      GLORIE_TRY(check_launch());
    }
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(reduce_blocks(n_pix)), dim3(kThreads), 0, st, depth_bits, n_pix, depth);
    return check_launch();
  }
  return check_hip(hipMemsetAsync(depth, 0, (size_t)n_pix * sizeof(float), st));
}

extern "C" int glorie_points_in_view(const float* points, int n, const float* w2c, float fx, float fy, float cx, float cy,
                                     int H, int W, float edge, int* count, void* stream) {
  Camera cam;
  if (n < 0 || !w2c || !count || (n > 0 && !points)) return GLORIE_EINVAL;
  if (!make_camera(fx, fy, cx, cy, H, W, 0.f, 0.f, &cam)) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  GLORIE_TRY(check_hip(hipMemsetAsync(count, 0, sizeof(int), st)));
  if (n == 0) return GLORIE_OK;
  hipLaunchKernelGGL(points_in_view_kernel, dim3(reduce_blocks(n)), dim3(kThreads), 0, st, points, (long long)n, w2c, cam,
                     (double)edge, count);
  return check_launch();
}

extern "C" size_t glorie_depth_l1_workspace(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  return 2 * (size_t)reduce_blocks((long long)H * W) * sizeof(double);
}

extern "C" int glorie_depth_l1_accumulate(const float* gt_depth, const float* rec_depth, int H, int W, void* workspace,
                                          double* err, int* valid, int view, void* stream) {
  if (H <= 0 || W <= 0 || view < 0 || !gt_depth || !rec_depth || !workspace || !err || !valid) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long long n_pix = (long long)H * W;
  const int blocks = reduce_blocks(n_pix);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(depth_l1_kernel, dim3(blocks), dim3(kThreads), 0, st, gt_depth, rec_depth, n_pix, partial);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(depth_l1_finish_kernel, dim3(1), dim3(64), 0, st, partial, blocks, err, valid, view);
  return check_launch();
}
