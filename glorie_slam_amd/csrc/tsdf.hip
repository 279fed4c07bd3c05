// Block-sparse TSDF volume: fusion of depth / colour frames and mesh extraction (reference: src/utils/generate_mesh.py,
// which drives Open3D's TSDF integration with RGB8 colour and depth_trunc 30; the update rule is restated in
// include/glorie_hip.h because Open3D is not part of this project).
//
// Layout: a dense int32 block table over the bound (nbz x nby x nbx, x fastest; -1 or a block id) and a pool of blocks of
// 8 x 8 x 8 voxels, voxel x fastest: tsdf f32 [n,512], weight f32 [n,512], rgb f32 [n,512,3] (0..255).  block_index[id]
// is the table index of a block.  Voxel (i,j,k) samples origin + (i + 0.5, j + 0.5, k + 0.5) * voxel_length.
//
// Allocate, four launches + a 12-byte read-back:
//   tsdf_flag_kernel     one thread per pixel: back-project, flag (a byte store of 1) every block that overlaps the box
//                        [p - sdf_trunc, p + sdf_trunc]; a pixel whose box leaves the grid is counted and flags nothing
//   tsdf_new_kernel      one thread per table entry: new = flagged and not yet allocated; one count per workgroup
//   tsdf_admit_kernel    one workgroup: exclusive scan of the counts; admits the frame only if it fits in max_blocks
//   tsdf_assign_kernel   new blocks get id = blocks before + rank: ascending in the table index
// Integrate, one launch: a workgroup of 512 threads per allocated block.  It first tests the block's bounding sphere
//   against the four side planes of the frustum and the depth range (conservative, uniform over the workgroup) and
//   leaves at once when the block cannot be seen; then one thread owns one voxel: no atomics, one pass.
// Extract, marching tetrahedra on the Kuhn split of every cell (count pass, (V, F) read-back, emit pass):
//   tsdf_order_*         the allocated blocks in ascending table index (flag -> count -> scan -> rank)
//   tsdf_count_kernel    a workgroup per block stages the 10^3 corner tile (corners -1..8: an owned edge is used when
//                        one of the up to four cells around it is valid, and those reach one voxel back) in LDS through
//                        the table, derives the validity of the 9^3 cells, and per cell the mask of owned edges with a
//                        vertex and the number of triangles; per-cell masks, in-block vertex prefixes and the block's
//                        (V, F) go to the workspace
//   tsdf_bases_kernel    exclusive scan of the per-block counts
//   tsdf_emit_kernel     recomputes the cell results and writes vertices, colours and faces at their canonical places
// The scans are block_exclusive_scan of compact.hiph; the one-array scan of the block order is launch_exclusive_scan, whose
// kernel is defined in select.hip (this file needs it linked, as libglorie_hip.so does).  Only integer atomics (two statistics counters): repeated runs
// are bitwise equal.
#include "compact.hiph"

using namespace glorie;

namespace {

constexpr int kBlock = 8;
constexpr int kVox = 512;                   // voxels of a block = threads of the per-block kernels
constexpr int kVoxWaves = kVox / 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 10;                   // corner tile of the extraction: corners -1..8
constexpr int kCells = 9;                   // cells -1..7

struct Grid {
  float ox, oy, oz, vl;
  int nbx, nby, nbz;
};
struct Cam {
  float fx, fy, cx, cy;
  int H, W;
};

// ---- allocate --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
tsdf_flag_kernel(const float* __restrict__ depth, Cam cam, const float* __restrict__ c2w, float depth_trunc,
                 float sdf_trunc, Grid g, unsigned char* __restrict__ flag, int* __restrict__ counters) {
  __shared__ int red[kWaves];
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  bool outside = false;
  if (pix < cam.H * cam.W) {
    const float d = depth[pix];
    if (d > 0.f && d <= depth_trunc) {
      const int v = pix / cam.W, u = pix - v * cam.W;
      const float x = ((float)u - cam.cx) / cam.fx * d, y = ((float)v - cam.cy) / cam.fy * d;
      const float p[3] = {c2w[0] * x + c2w[1] * y + c2w[2] * d + c2w[3], c2w[4] * x + c2w[5] * y + c2w[6] * d + c2w[7],
                          c2w[8] * x + c2w[9] * y + c2w[10] * d + c2w[11]};
      const float o[3] = {g.ox, g.oy, g.oz};
      const int nb[3] = {g.nbx, g.nby, g.nbz};
      const float size = (float)kBlock * g.vl;
      int lo[3], hi[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float l = floorf((p[a] - sdf_trunc - o[a]) / size), h = floorf((p[a] + sdf_trunc - o[a]) / size);
        // (a non-finite point compares false and counts as outside)
        if (!(l >= 0.f && h < (float)nb[a])) outside = true;
        lo[a] = (int)l;
        hi[a] = (int)h;
      }
      if (!outside) {
        for (int bz = lo[2]; bz <= hi[2]; ++bz)
          for (int by = lo[1]; by <= hi[1]; ++by)
            for (int bx = lo[0]; bx <= hi[0]; ++bx) flag[((size_t)bz * g.nby + by) * g.nbx + bx] = 1;
      }
    }
  }
  wave_count(outside, red);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = slot_sum(red, kWaves);
    if (c) atomicAdd(counters + 1, c);
  }
}

__global__ void __launch_bounds__(kThreads)
tsdf_new_kernel(const unsigned char* __restrict__ flag, const int* __restrict__ table, int n_table,
                int* __restrict__ wg_count) {
  __shared__ int red[kWaves];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool fresh = i < n_table && flag[i] != 0 && table[i] < 0;
  wave_count(fresh, red);
  __syncthreads();
  if (threadIdx.x == 0) wg_count[blockIdx.x] = slot_sum(red, kWaves);
}

// counters: [0] blocks in use, [1] pixels outside the bound (cumulative), [2] 1 when the last frame did not fit,
// [3] blocks that passed the culling of the last integration, [4] blocks the last frame asked for.
// admit[0] = id of the frame's first new block, or -1 when the frame is refused
__global__ void __launch_bounds__(kScanThreads)
tsdf_admit_kernel(const int* __restrict__ wg_count, int n_wg, int* __restrict__ wg_offset, int max_blocks,
                  int* __restrict__ counters, int* __restrict__ admit) {
  const int* const in[1] = {wg_count};
  int* const out[1] = {wg_offset};
  int sum[1];
  block_exclusive_scan<1>(in, out, n_wg, sum);
  if (threadIdx.x == 0) {
    const int used = counters[0];
    const bool fits = sum[0] <= max_blocks - used;
    admit[0] = fits ? used : -1;
    counters[2] = fits ? 0 : 1;
    counters[4] = sum[0];
    if (fits) counters[0] = used + sum[0];
  }
}

__global__ void __launch_bounds__(kThreads)
tsdf_assign_kernel(const unsigned char* __restrict__ flag, int* __restrict__ table, int n_table,
                   const int* __restrict__ wg_offset, const int* __restrict__ admit, int* __restrict__ block_index) {
  __shared__ int red[kWaves];
  const int base = admit[0];
  if (base < 0) return;                                           // uniform: the frame was refused
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool fresh = i < n_table && flag[i] != 0 && table[i] < 0;
  const unsigned long long b = wave_count(fresh, red);
  __syncthreads();
  if (fresh) {
    const int id = base + wg_offset[blockIdx.x] + block_rank(b, red);
    table[i] = id;
    block_index[id] = i;
  }
}

// ---- integrate -------------------------------------------------------------------------------------------------------
struct Pose {
  float r[9], t[3];                         // camera-to-world rotation (row major) and translation
};

__device__ __forceinline__ Pose load_pose(const float* __restrict__ c2w) {
  Pose p;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) p.r[3 * i + j] = c2w[4 * i + j];
    p.t[i] = c2w[4 * i + 3];
  }
  return p;
}

// p = R^T (X - t): the world-to-camera transform of a rigid camera-to-world matrix
__device__ __forceinline__ void to_camera(const Pose& c, float X, float Y, float Z, float& px, float& py, float& pz) {
  const float dx = X - c.t[0], dy = Y - c.t[1], dz = Z - c.t[2];
  px = c.r[0] * dx + c.r[3] * dy + c.r[6] * dz;
  py = c.r[1] * dx + c.r[4] * dy + c.r[7] * dz;
  pz = c.r[2] * dx + c.r[5] * dy + c.r[8] * dz;
}

// can a voxel of the block with centre (cx, cy, cz) in camera coordinates and bounding radius r be updated?  A voxel is
// updated only with p.z > 0, its projection inside the image and p.z < d + sdf_trunc <= depth_trunc + sdf_trunc; every
// such point lies on the inner side of the four planes through the camera centre and the image borders
__device__ __forceinline__ bool block_visible(float cx, float cy, float cz, float r, const Cam& cam, float z_max) {
  if (cz + r <= 0.f || cz - r > z_max) return false;
  const float tl = (-0.5f - cam.cx) / cam.fx, tr = ((float)cam.W - 0.5f - cam.cx) / cam.fx;
  const float tt = (-0.5f - cam.cy) / cam.fy, tb = ((float)cam.H - 0.5f - cam.cy) / cam.fy;
  if ((cx - tl * cz) * rsqrtf(1.f + tl * tl) < -r) return false;
  if ((tr * cz - cx) * rsqrtf(1.f + tr * tr) < -r) return false;
  if ((cy - tt * cz) * rsqrtf(1.f + tt * tt) < -r) return false;
  if ((tb * cz - cy) * rsqrtf(1.f + tb * tb) < -r) return false;
  return true;
}

__global__ void __launch_bounds__(kVox)
tsdf_integrate_kernel(const float* __restrict__ depth, const float* __restrict__ color, Cam cam,
                      const float* __restrict__ c2w, float depth_trunc, float sdf_trunc, Grid g,
                      const int* __restrict__ block_index, float* __restrict__ tsdf, float* __restrict__ weight,
                      float* __restrict__ rgb, int* __restrict__ counters) {
  const Pose c = load_pose(c2w);
  const int id = blockIdx.x;
  const int ti = block_index[id];
  const int bx = ti % g.nbx, by = (ti / g.nbx) % g.nby, bz = ti / (g.nbx * g.nby);
  {
    const float half = 0.5f * (float)kBlock * g.vl;
    float px, py, pz;
    to_camera(c, g.ox + (float)(bx * kBlock) * g.vl + half, g.oy + (float)(by * kBlock) * g.vl + half,
              g.oz + (float)(bz * kBlock) * g.vl + half, px, py, pz);
    // sqrt(3) * half, with 1 % and a voxel for the rounding of the centre and of the plane distances
    const float r = 1.7321f * half * 1.01f + g.vl;
    if (!block_visible(px, py, pz, r, cam, depth_trunc + sdf_trunc)) return;
  }
  if (threadIdx.x == 0) atomicAdd(counters + 3, 1);
  const int x = threadIdx.x & 7, y = (threadIdx.x >> 3) & 7, z = threadIdx.x >> 6;
  const float X = g.ox + ((float)(bx * kBlock + x) + 0.5f) * g.vl;
  const float Y = g.oy + ((float)(by * kBlock + y) + 0.5f) * g.vl;
  const float Z = g.oz + ((float)(bz * kBlock + z) + 0.5f) * g.vl;
  float px, py, pz;
  to_camera(c, X, Y, Z, px, py, pz);
  if (!(pz > 0.f)) return;
  const float u_f = cam.fx * px / pz + cam.cx + 0.5f, v_f = cam.fy * py / pz + cam.cy + 0.5f;
  if (!(u_f >= 1e-4f && u_f < (float)cam.W - 1e-4f && v_f >= 1e-4f && v_f < (float)cam.H - 1e-4f)) return;
  const int u = (int)u_f, v = (int)v_f;
  const size_t pix = (size_t)v * cam.W + u;
  const float d = depth[pix];
  if (!(d > 0.f) || d > depth_trunc) return;
  const float rx = ((float)u - cam.cx) / cam.fx, ry = ((float)v - cam.cy) / cam.fy;
  const float sdf = (d - pz) * sqrtf(1.f + rx * rx + ry * ry);
  if (sdf <= -sdf_trunc) return;
  const float fresh = fminf(1.f, sdf / sdf_trunc);
  const size_t vox = (size_t)id * kVox + threadIdx.x;
  const float w = weight[vox], w1 = w + 1.f;
  tsdf[vox] = (tsdf[vox] * w + fresh) / w1;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float col = floorf(fminf(fmaxf(color[3 * pix + ch], 0.f), 1.f) * 255.f);
    rgb[3 * vox + ch] = (rgb[3 * vox + ch] * w + col) / w1;
  }
  weight[vox] = w1;
}

// ---- extract ---------------------------------------------------------------------------------------------------------
// edges (p, q) of a positively oriented tetrahedron as 4 p + q, per inside mask (bit p: vertex p has tsdf < 0); the normal
// of every triangle points from the inside vertices to the outside ones; a negatively oriented tetrahedron swaps the
// last two vertices of each triangle
struct TetCase {
  unsigned char n, e[6];
};
__constant__ TetCase kTet[16] = {
    {0, {0, 0, 0, 0, 0, 0}},    {1, {1, 2, 3, 0, 0, 0}},   {1, {1, 7, 6, 0, 0, 0}},   {2, {2, 3, 7, 2, 7, 6}},
    {1, {2, 6, 11, 0, 0, 0}},   {2, {3, 1, 6, 3, 6, 11}},  {2, {1, 7, 11, 1, 11, 2}}, {1, {3, 7, 11, 0, 0, 0}},
    {1, {3, 11, 7, 0, 0, 0}},   {2, {1, 2, 11, 1, 11, 7}}, {2, {6, 1, 3, 6, 3, 11}},  {1, {2, 11, 6, 0, 0, 0}},
    {2, {2, 6, 7, 2, 7, 3}},    {1, {1, 6, 7, 0, 0, 0}},   {1, {1, 3, 2, 0, 0, 0}},   {0, {0, 0, 0, 0, 0, 0}}};
// the six orders (a, b, c) of the axis bits, as itertools.permutations((1, 2, 4)): corners (0, a, a|b, 7), and whether
// the order is an odd permutation (a negatively oriented tetrahedron)
__constant__ unsigned char kOrderA[6] = {1, 1, 2, 2, 4, 4};
__constant__ unsigned char kOrderAB[6] = {3, 5, 3, 6, 5, 6};
__constant__ unsigned char kOrderOdd[6] = {0, 1, 1, 0, 0, 1};
// corner reached by the owned edge of a slot, and the slot of a corner difference
__constant__ unsigned char kSlotCorner[7] = {1, 2, 4, 3, 5, 6, 7};
__constant__ unsigned char kCornerSlot[8] = {0, 0, 1, 3, 2, 4, 5, 6};

__device__ __forceinline__ int tile_at(int x, int y, int z) { return ((z + 1) * kTile + (y + 1)) * kTile + (x + 1); }
__device__ __forceinline__ int cell_at(int x, int y, int z) { return ((z + 1) * kCells + (y + 1)) * kCells + (x + 1); }

struct CellResult {
  int mask;        // bit s: the owned edge of slot s carries a vertex
  int faces;       // triangles of the cell
};

// Stages the corner tile of block (bx, by, bz) and the cell validity in LDS and returns this thread's cell result.
// st: tsdf of the corners, sv: corner allocated with weight > 0, cv: all 8 corners of the cell are.  All kVox threads.
__device__ __forceinline__ CellResult stage_block(const Grid& g, const int* __restrict__ table,
                                                  const float* __restrict__ tsdf, const float* __restrict__ weight, int bx,
                                                  int by, int bz, float* st, unsigned char* sv, unsigned char* cv) {
  const int tid = threadIdx.x;
  for (int e = tid; e < kTile * kTile * kTile; e += kVox) {
    const int lx = e % kTile - 1, ly = (e / kTile) % kTile - 1, lz = e / (kTile * kTile) - 1;
    const int gx = bx * kBlock + lx, gy = by * kBlock + ly, gz = bz * kBlock + lz;
    float t = 0.f;
    bool ok = false;
    if (gx >= 0 && gy >= 0 && gz >= 0 && gx < g.nbx * kBlock && gy < g.nby * kBlock && gz < g.nbz * kBlock) {
      const int id = table[((size_t)(gz >> 3) * g.nby + (gy >> 3)) * g.nbx + (gx >> 3)];
      if (id >= 0) {
        const size_t vox = (size_t)id * kVox + ((gz & 7) << 6 | (gy & 7) << 3 | (gx & 7));
        ok = weight[vox] > 0.f;
        t = tsdf[vox];
      }
    }
    st[e] = t;
    sv[e] = ok ? 1 : 0;
  }
  __syncthreads();
  for (int e = tid; e < kCells * kCells * kCells; e += kVox) {
    const int lx = e % kCells - 1, ly = (e / kCells) % kCells - 1, lz = e / (kCells * kCells) - 1;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) ok = ok && sv[tile_at(lx + (c & 1), ly + ((c >> 1) & 1), lz + (c >> 2))] != 0;
    cv[e] = ok ? 1 : 0;
  }
  __syncthreads();
  const int x = tid & 7, y = (tid >> 3) & 7, z = tid >> 6;
  CellResult r = {0, 0};
  const bool in0 = st[tile_at(x, y, z)] < 0.f;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    const int d = kSlotCorner[s];
    const bool in1 = st[tile_at(x + (d & 1), y + ((d >> 1) & 1), z + (d >> 2))] < 0.f;
    bool used = false;
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if ((o & d) == 0) used = used || cv[cell_at(x - (o & 1), y - ((o >> 1) & 1), z - (o >> 2))] != 0;
    if (used && in0 != in1) r.mask |= 1 << s;
  }
  if (cv[cell_at(x, y, z)]) {
    int inside = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) inside |= (st[tile_at(x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2))] < 0.f ? 1 : 0) << c;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const int a = kOrderA[q], ab = kOrderAB[q];
      const int m = (inside & 1) | ((inside >> a) & 1) << 1 | ((inside >> ab) & 1) << 2 | ((inside >> 7) & 1) << 3;
      r.faces += kTet[m].n;
    }
  }
  return r;
}

// exclusive prefix of v over the kVox threads of the workgroup (thread order) and the total; slot: kVoxWaves ints of LDS
__device__ __forceinline__ int block_prefix(int v, int* slot, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(inc, off, 64);
    if (lane >= off) inc += up;
  }
  __syncthreads();                                                // (the slots may still be read from the last call)
  if (lane == 63) slot[wave] = inc;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < kVoxWaves; ++k) {
    before += k < wave ? slot[k] : 0;
    total += slot[k];
  }
  return before + inc - v;
}

__global__ void __launch_bounds__(kThreads)
tsdf_order_count_kernel(const int* __restrict__ table, int n_table, int* __restrict__ wg_count) {
  __shared__ int red[kWaves];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  wave_count(i < n_table && table[i] >= 0, red);
  __syncthreads();
  if (threadIdx.x == 0) wg_count[blockIdx.x] = slot_sum(red, kWaves);
}

// order[r] = table index of the r-th allocated block in ascending table index; rank_of[id] = r
__global__ void __launch_bounds__(kThreads)
tsdf_order_rank_kernel(const int* __restrict__ table, int n_table, const int* __restrict__ wg_offset, int n_blocks,
                       int* __restrict__ order, int* __restrict__ rank_of) {
  __shared__ int red[kWaves];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int id = i < n_table ? table[i] : -1;
  const bool live = id >= 0 && id < n_blocks;
  const unsigned long long b = wave_count(live, red);
  __syncthreads();
  if (live) {
    const int r = wg_offset[blockIdx.x] + block_rank(b, red);
    if (r < n_blocks) {
      order[r] = i;
      rank_of[id] = r;
    }
  }
}

__global__ void __launch_bounds__(kVox)
tsdf_count_kernel(Grid g, const int* __restrict__ table, const float* __restrict__ tsdf,
                  const float* __restrict__ weight, const int* __restrict__ order, unsigned char* __restrict__ cell_mask,
                  unsigned short* __restrict__ cell_prefix, int* __restrict__ block_v, int* __restrict__ block_f) {
  __shared__ float st[kTile * kTile * kTile];
  __shared__ unsigned char sv[kTile * kTile * kTile], cv[kCells * kCells * kCells];
  __shared__ int slot[kVoxWaves];
  const int ti = order[blockIdx.x];
  const CellResult r = stage_block(g, table, tsdf, weight, ti % g.nbx, (ti / g.nbx) % g.nby, ti / (g.nbx * g.nby), st, sv,
                                   cv);
  int total_v, total_f;
  const int before = block_prefix(__popc(r.mask), slot, total_v);
  block_prefix(r.faces, slot, total_f);
  const size_t cell = (size_t)blockIdx.x * kVox + threadIdx.x;
  cell_mask[cell] = (unsigned char)r.mask;
  cell_prefix[cell] = (unsigned short)before;                     // at most 511 * 7
  if (threadIdx.x == 0) {
    block_v[blockIdx.x] = total_v;
    block_f[blockIdx.x] = total_f;
  }
}

// totals[0], totals[1] = V, F
__global__ void __launch_bounds__(kScanThreads)
tsdf_bases_kernel(const int* __restrict__ block_v, const int* __restrict__ block_f, int n, int* __restrict__ base_v,
                  int* __restrict__ base_f, int* __restrict__ totals) {
  const int* const in[2] = {block_v, block_f};
  int* const out[2] = {base_v, base_f};
  int sum[2];
  block_exclusive_scan<2>(in, out, n, sum);
  if (threadIdx.x == 0) {
    totals[0] = sum[0];
    totals[1] = sum[1];
  }
}

struct GridD {
  double ox, oy, oz, vl;
};

__global__ void __launch_bounds__(kVox)
tsdf_emit_kernel(Grid g, GridD gd, const int* __restrict__ table, const float* __restrict__ tsdf,
                 const float* __restrict__ weight, const float* __restrict__ rgb, const int* __restrict__ order,
                 const int* __restrict__ rank_of, const unsigned char* __restrict__ cell_mask,
                 const unsigned short* __restrict__ cell_prefix, const int* __restrict__ base_v,
                 const int* __restrict__ base_f, float* __restrict__ vertices, float* __restrict__ colors,
                 int* __restrict__ faces) {
  __shared__ float st[kTile * kTile * kTile];
  __shared__ unsigned char sv[kTile * kTile * kTile], cv[kCells * kCells * kCells];
  __shared__ int slot[kVoxWaves];
  const int tid = threadIdx.x;
  const int ti = order[blockIdx.x];
  const int bx = ti % g.nbx, by = (ti / g.nbx) % g.nby, bz = ti / (g.nbx * g.nby);
  const CellResult r = stage_block(g, table, tsdf, weight, bx, by, bz, st, sv, cv);
  int total;
  const int f_before = block_prefix(r.faces, slot, total);
  const int x = tid & 7, y = (tid >> 3) & 7, z = tid >> 6;
  const int v0 = base_v[blockIdx.x];
  if (r.mask) {
    // (the voxels of this block are those of table[ti])
    const size_t vox_a = (size_t)table[ti] * kVox + tid;
    const double ta = (double)st[tile_at(x, y, z)];
    int vid = v0 + (int)cell_prefix[(size_t)blockIdx.x * kVox + tid];
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      if (!(r.mask >> s & 1)) continue;
      const int d = kSlotCorner[s];
      const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
      const double tb = (double)st[tile_at(x + dx, y + dy, z + dz)];
      const double t = ta / (ta - tb);
      const int gx = bx * kBlock + x, gy = by * kBlock + y, gz = bz * kBlock + z;
      vertices[3 * (size_t)vid + 0] = (float)(gd.ox + gd.vl * ((double)gx + 0.5 + t * dx));
      vertices[3 * (size_t)vid + 1] = (float)(gd.oy + gd.vl * ((double)gy + 0.5 + t * dy));
      vertices[3 * (size_t)vid + 2] = (float)(gd.oz + gd.vl * ((double)gz + 0.5 + t * dz));
      const int hx = gx + dx, hy = gy + dy, hz = gz + dz;        // allocated: a valid cell uses the edge
      const int idb = table[((size_t)(hz >> 3) * g.nby + (hy >> 3)) * g.nbx + (hx >> 3)];
      const size_t vox_b = (size_t)idb * kVox + ((hz & 7) << 6 | (hy & 7) << 3 | (hx & 7));
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const double ca = (double)rgb[3 * vox_a + ch], cb = (double)rgb[3 * vox_b + ch];
        colors[3 * (size_t)vid + ch] = (float)((ca + t * (cb - ca)) / 255.0);
      }
      ++vid;
    }
  }
  if (r.faces) {
    int inside = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) inside |= (st[tile_at(x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2))] < 0.f ? 1 : 0) << c;
    size_t f = (size_t)base_f[blockIdx.x] + f_before;
    for (int q = 0; q < 6; ++q) {
      const int corner[4] = {0, kOrderA[q], kOrderAB[q], 7};
      const int m = (inside & 1) | ((inside >> corner[1]) & 1) << 1 | ((inside >> corner[2]) & 1) << 2 |
                    ((inside >> 7) & 1) << 3;
      const TetCase tc = kTet[m];
      for (int k = 0; k < tc.n; ++k) {
        int ids[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const int code = tc.e[3 * k + e];
          const int ca = corner[code >> 2], cb = corner[code & 3];
          const int s = kCornerSlot[cb & ~ca];
          // the owning cell: this cell moved by corner ca, possibly in a neighbouring block (allocated: this cell is valid)
          const int hx = bx * kBlock + x + (ca & 1), hy = by * kBlock + y + ((ca >> 1) & 1), hz = bz * kBlock + z + (ca >> 2);
          const int idn = table[((size_t)(hz >> 3) * g.nby + (hy >> 3)) * g.nbx + (hx >> 3)];
          const int rn = rank_of[idn];
          const size_t cell = (size_t)rn * kVox + ((hz & 7) << 6 | (hy & 7) << 3 | (hx & 7));
          const int mask = cell_mask[cell];
          ids[e] = base_v[rn] + (int)cell_prefix[cell] + __popc(mask & ((1 << s) - 1));
        }
        const bool odd = kOrderOdd[q] != 0;
        faces[3 * f + 0] = ids[0];
        faces[3 * f + 1] = odd ? ids[2] : ids[1];
        faces[3 * f + 2] = odd ? ids[1] : ids[2];
        ++f;
      }
    }
  }
}

inline int wgs(long long n) { return (int)((n + kThreads - 1) / kThreads); }

inline bool grid_ok(const float* origin, float vl, const int* nb) {
  if (!origin || !nb || !(vl > 0.f)) return false;
  if (nb[0] <= 0 || nb[1] <= 0 || nb[2] <= 0) return false;
  // voxel coordinates and the table index stay in int32
  if (nb[0] > (1 << 24) || nb[1] > (1 << 24) || nb[2] > (1 << 24)) return false;
  return (long long)nb[0] * nb[1] * nb[2] <= 0x7fffffffLL - kThreads;
}

inline Grid make_grid(const float* origin, float vl, const int* nb) {
  return Grid{origin[0], origin[1], origin[2], vl, nb[0], nb[1], nb[2]};
}

// workspace of the extraction: per table workgroup B = wgs(n_table), per allocated block n (at least one)
struct ExtractWs {
  Carver c;
  long long n_table;
  int n_blocks;
  size_t B = (size_t)wgs(n_table), n = (size_t)(n_blocks > 0 ? n_blocks : 1);
  int* wg_count = c.take<int>(B);
  int* wg_offset = c.take<int>(B);
  int* order = c.take<int>(n);
  int* rank_of = c.take<int>(n);
  int* block_v = c.take<int>(n);
  int* block_f = c.take<int>(n);
  int* base_v = c.take<int>(n);
  int* base_f = c.take<int>(n);
  int* totals = c.take<int>(2);
  unsigned short* cell_prefix = c.take<unsigned short>(n * kVox);
  unsigned char* cell_mask = c.take<unsigned char>(n * kVox);
};

// workspace of the allocation: flags u8 [n_table] | workgroup counts int [B] | offsets int [B] | admit int [2]
struct AllocateWs {
  Carver c;
  long long n_table;
  unsigned char* flag = c.take<unsigned char>((size_t)n_table);
  int* wg_count = c.take<int>((size_t)wgs(n_table));
  int* wg_offset = c.take<int>((size_t)wgs(n_table));
  int* admit = c.take<int>(2);
};

}  // namespace

extern "C" size_t glorie_tsdf_allocate_workspace(long n_table) {
  if (n_table <= 0 || n_table > 0x7fffffffLL - kThreads) return 0;
  return carved_bytes<AllocateWs>((long long)n_table);
}

extern "C" int glorie_tsdf_allocate(const float* depth, int H, int W, const float* c2w, float fx, float fy, float cx,
                                    float cy, float depth_trunc, float sdf_trunc, const float* origin,
                                    float voxel_length, const int* blocks_per_axis, int* table, int* block_index,
                                    int max_blocks, int* counters, void* workspace, int* n_blocks_out, void* stream) {
  if (!depth || !c2w || !table || !block_index || !counters || !workspace || !n_blocks_out) return GLORIE_EINVAL;
  if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL - kThreads || max_blocks <= 0) return GLORIE_EINVAL;
  if (!grid_ok(origin, voxel_length, blocks_per_axis) || !(sdf_trunc > 0.f)) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const Grid g = make_grid(origin, voxel_length, blocks_per_axis);
  const Cam cam{fx, fy, cx, cy, H, W};
  const int n_table = blocks_per_axis[0] * blocks_per_axis[1] * blocks_per_axis[2];
  const int B = wgs(n_table);
  const AllocateWs w{Carver(workspace), n_table};
  GLORIE_TRY(check_hip(hipMemsetAsync(w.flag, 0, (size_t)n_table, st)));
  hipLaunchKernelGGL(tsdf_flag_kernel, dim3(wgs((long long)H * W)), dim3(kThreads), 0, st, depth, cam, c2w, depth_trunc,
                     sdf_trunc, g, w.flag, counters);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(tsdf_new_kernel, dim3(B), dim3(kThreads), 0, st, w.flag, table, n_table, w.wg_count);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(tsdf_admit_kernel, dim3(1), dim3(kScanThreads), 0, st, w.wg_count, B, w.wg_offset, max_blocks,
                     counters, w.admit);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(tsdf_assign_kernel, dim3(B), dim3(kThreads), 0, st, w.flag, table, n_table, w.wg_offset, w.admit,
                     block_index);
  GLORIE_TRY(check_launch());
  int host[3] = {0, 0, 0};                                        // blocks in use, pixels outside, refused
  GLORIE_TRY(check_hip(hipMemcpyAsync(host, counters, sizeof(host), hipMemcpyDeviceToHost, st)));
  GLORIE_TRY(check_hip(hipStreamSynchronize(st)));
  *n_blocks_out = host[0];
  return host[2] ? GLORIE_ENOMEM : GLORIE_OK;
}

extern "C" int glorie_tsdf_integrate(const float* depth, const float* color, int H, int W, const float* c2w, float fx,
                                     float fy, float cx, float cy, float depth_trunc, float sdf_trunc,
                                     const float* origin, float voxel_length, const int* blocks_per_axis,
                                     const int* block_index, int n_blocks, float* tsdf, float* weight, float* rgb,
                                     int* counters, void* stream) {
  if (!depth || !color || !c2w || !block_index || !tsdf || !weight || !rgb || !counters) return GLORIE_EINVAL;
  if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL / 3 || n_blocks < 0) return GLORIE_EINVAL;
  if (!grid_ok(origin, voxel_length, blocks_per_axis) || !(sdf_trunc > 0.f)) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  GLORIE_TRY(check_hip(hipMemsetAsync(counters + 3, 0, sizeof(int), st)));
  if (n_blocks == 0) return GLORIE_OK;
  const Cam cam{fx, fy, cx, cy, H, W};
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(n_blocks), dim3(kVox), 0, st, depth, color, cam, c2w, depth_trunc,
                     sdf_trunc, make_grid(origin, voxel_length, blocks_per_axis), block_index, tsdf, weight, rgb,
                     counters);
  return check_launch();
}

extern "C" size_t glorie_tsdf_extract_workspace(long n_table, int n_blocks) {
  if (n_table <= 0 || n_table > 0x7fffffffLL - kThreads || n_blocks < 0) return 0;
  return carved_bytes<ExtractWs>((long long)n_table, n_blocks);
}

extern "C" int glorie_tsdf_extract_count(const float* origin, float voxel_length, const int* blocks_per_axis,
                                         const int* table, int n_blocks, const float* tsdf, const float* weight,
                                         void* workspace, int* counts_out, void* stream) {
  if (!table || !workspace || !counts_out || n_blocks < 0) return GLORIE_EINVAL;
  if (!grid_ok(origin, voxel_length, blocks_per_axis)) return GLORIE_EINVAL;
  counts_out[0] = counts_out[1] = 0;
  if (n_blocks == 0) return GLORIE_OK;
  if (!tsdf || !weight) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const Grid g = make_grid(origin, voxel_length, blocks_per_axis);
  const int n_table = blocks_per_axis[0] * blocks_per_axis[1] * blocks_per_axis[2];
  const int B = wgs(n_table);
  const ExtractWs w{Carver(workspace), n_table, n_blocks};
  hipLaunchKernelGGL(tsdf_order_count_kernel, dim3(B), dim3(kThreads), 0, st, table, n_table, w.wg_count);
  GLORIE_TRY(check_launch());
  GLORIE_TRY(launch_exclusive_scan(w.wg_count, B, w.wg_offset, nullptr, st));
  hipLaunchKernelGGL(tsdf_order_rank_kernel, dim3(B), dim3(kThreads), 0, st, table, n_table, w.wg_offset, n_blocks,
                     w.order, w.rank_of);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(tsdf_count_kernel, dim3(n_blocks), dim3(kVox), 0, st, g, table, tsdf, weight, w.order, w.cell_mask,
                     w.cell_prefix, w.block_v, w.block_f);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(tsdf_bases_kernel, dim3(1), dim3(kScanThreads), 0, st, w.block_v, w.block_f, n_blocks, w.base_v,
                     w.base_f, w.totals);
  GLORIE_TRY(check_launch());
  GLORIE_TRY(check_hip(hipMemcpyAsync(counts_out, w.totals, 2 * sizeof(int), hipMemcpyDeviceToHost, st)));
  return check_hip(hipStreamSynchronize(st));
}

extern "C" int glorie_tsdf_extract_emit(const double* origin, double voxel_length, const int* blocks_per_axis,
                                        const int* table, int n_blocks, const float* tsdf, const float* weight,
                                        const float* rgb, void* workspace, float* vertices, float* colors, int* faces,
                                        void* stream) {
  if (!origin || !blocks_per_axis || !table || !workspace || n_blocks < 0) return GLORIE_EINVAL;
  if (n_blocks == 0) return GLORIE_OK;
  if (!tsdf || !weight || !rgb || !vertices || !colors || !faces) return GLORIE_EINVAL;
  const float origin_f[3] = {(float)origin[0], (float)origin[1], (float)origin[2]};
  if (!grid_ok(origin_f, (float)voxel_length, blocks_per_axis)) return GLORIE_EINVAL;
  const Grid g = make_grid(origin_f, (float)voxel_length, blocks_per_axis);
  const GridD gd{origin[0], origin[1], origin[2], voxel_length};
  const int n_table = blocks_per_axis[0] * blocks_per_axis[1] * blocks_per_axis[2];
  const ExtractWs w{Carver(workspace), n_table, n_blocks};
  hipLaunchKernelGGL(tsdf_emit_kernel, dim3(n_blocks), dim3(kVox), 0, (hipStream_t)stream, g, gd, table, tsdf, weight,
                     rgb, w.order, w.rank_of, w.cell_mask, w.cell_prefix, w.base_v, w.base_f, vertices, colors, faces);
  return check_launch();
}
