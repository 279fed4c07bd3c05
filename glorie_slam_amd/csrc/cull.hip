// Mesh culling and cleaning: the per-vertex count of the views that see a vertex, the face rule on those counts, the
// order-preserving compaction of a mesh under a face mask, and connected components over shared vertex indices.
//
// Visibility, one launch for any number of views: one thread owns one vertex and walks the views, whose matrices a
//   workgroup stages in LDS in chunks of kViewChunk (every lane reads the same LDS address: a broadcast).  The count is a
//   register sum written (or added to what is there) once: no atomics, nothing depends on arrival order.  All arithmetic is
//   fp64 formed from the fp32 inputs, every operation rounded on its own, in the order of points_in_view_kernel
//   (recon.hip).  The pixel is compared as a double before it becomes an index, so a NaN or a huge coordinate never forms
//   an address.
// Compaction, _count (4 launches, one read-back) and _emit (2 launches): kept faces mark their vertices (plain stores of
//   1), wave ballots count the marks and the kept faces per workgroup, block_exclusive_scan (compact.hiph) turns the
//   counts into offsets, and a lane's place is its workgroup's offset plus its rank in the workgroup.
// Components, a lock-free union-find on the label array itself: every link points from a vertex to a smaller index, so
//   a chain strictly descends and every walk ends; a root is hooked under the smaller root of the other side with
//   atomicCAS, and a failed CAS returns the new parent, which is again smaller.  The root of a component is therefore its
//   smallest index.  A flatten pass writes the root to every vertex (concurrent writers only ever replace an ancestor by
//   an ancestor); the walks of the hooking pass halve their paths on the way.  Face counts are integer atomics at the
//   label vertex, one per run of equal labels a wave meets; the largest component is a 64-bit atomicMax over
//   (count << 32 | ~label).
#include "compact.hiph"

using namespace glorie;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCountBlocks = 2048;            // cap of the face-count grid: a wave then sums a run of faces on chip
constexpr int kViewChunk = 128;               // view matrices staged at once: 128 x 12 floats = 6 KiB of LDS

inline int blocks_of(long long n) { return (int)((n + kThreads - 1) / kThreads); }

struct VisCam {
  double fx, fy, cx, cy, z_near, z_far, eps;
  int H, W, edge, missing_sees;
};

// ---- visibility -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
mesh_visibility_kernel(const float* __restrict__ vertices, int V, const float* __restrict__ w2cs, int M, VisCam cam,
                       const float* const* __restrict__ depth_table, int accumulate, int* __restrict__ count) {
#pragma clang fp contract(off)
  __shared__ float sw[kViewChunk * 12];
  __shared__ const float* sdepth[kViewChunk];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < V;
  const double x = live ? (double)vertices[3 * (size_t)i] : 0.0;
  const double y = live ? (double)vertices[3 * (size_t)i + 1] : 0.0;
  const double z = live ? (double)vertices[3 * (size_t)i + 2] : 0.0;
  const double ulo = (double)cam.edge, uhi = (double)(cam.W - cam.edge), vhi = (double)(cam.H - cam.edge);
  int seen = 0;
  for (int m0 = 0; m0 < M; m0 += kViewChunk) {
    const int mc = min(kViewChunk, M - m0);
    __syncthreads();                                            // the previous chunk has been read
    for (int k = threadIdx.x; k < mc * 12; k += kThreads) sw[k] = w2cs[(size_t)(m0 + k / 12) * 16 + k % 12];
    if (depth_table)
      for (int k = threadIdx.x; k < mc; k += kThreads) sdepth[k] = depth_table[m0 + k];
    __syncthreads();
    if (!live) continue;
    for (int m = 0; m < mc; ++m) {
      const float* w = sw + m * 12;
      const double pz = (((double)w[8] * x + (double)w[9] * y) + (double)w[10] * z) + (double)w[11];
      if (!(pz > cam.z_near && pz <= cam.z_far)) continue;
      const double px = (((double)w[0] * x + (double)w[1] * y) + (double)w[2] * z) + (double)w[3];
      const double py = (((double)w[4] * x + (double)w[5] * y) + (double)w[6] * z) + (double)w[7];
      const double uf = floor((cam.fx * px / pz + cam.cx) + 0.5);
      const double vf = floor((cam.fy * py / pz + cam.cy) + 0.5);
      if (!(uf >= ulo && uf < uhi && vf >= ulo && vf < vhi)) continue;       // false for a NaN; edge >= 0 bounds the index
      bool sees = true;
      if (depth_table) {
        const float* dm = sdepth[m];
        if (dm) {                                                            // a null map: frustum only for this view
          const double d = (double)dm[(size_t)(int)vf * cam.W + (int)uf];
          sees = d > 0.0 ? pz <= d + cam.eps : (cam.missing_sees != 0);      // a NaN depth is a hole
        }
      }
      seen += sees ? 1 : 0;
    }
  }
  if (live) count[i] = accumulate ? count[i] + seen : seen;
}

// ---- the face rule ----------------------------------------------------------------------------------------------------------
struct FaceIdx {
  int a, b, c;
  bool ok;
};

__device__ __forceinline__ FaceIdx load_face(const int* __restrict__ faces, int V, long long f) {
  FaceIdx t;
  t.a = faces[3 * f];
  t.b = faces[3 * f + 1];
  t.c = faces[3 * f + 2];
  t.ok = t.a >= 0 && t.a < V && t.b >= 0 && t.b < V && t.c >= 0 && t.c < V;
  return t;
}

__global__ void __launch_bounds__(kThreads)
mesh_select_faces_kernel(const int* __restrict__ faces, int F, int V, const int* __restrict__ count, int min_views, int rule,
                         unsigned char* __restrict__ keep_face) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const FaceIdx t = load_face(faces, V, f);
  bool keep = false;
  if (t.ok) {
    const bool s0 = count[t.a] >= min_views, s1 = count[t.b] >= min_views, s2 = count[t.c] >= min_views;
    keep = rule == 0 ? (s0 && s1 && s2) : (s0 || s1 || s2);
  }
  keep_face[f] = keep ? 1 : 0;
}

// ---- compaction -------------------------------------------------------------------------------------------------------------
struct CompactWs {
  Carver c;
  int V, F;
  int* used = c.take<int>(V);                  // [V] 1 where a kept face refers to the vertex
  int* new_index = c.take<int>(V);             // [V]
  int* wgc_v = c.take<int>(blocks_of(V));      // [Bv] marks per workgroup, then their exclusive scan in wgo_v
  int* wgo_v = c.take<int>(blocks_of(V));
  int* wgc_f = c.take<int>(blocks_of(F));      // [Bf]
  int* wgo_f = c.take<int>(blocks_of(F));
  int* totals = c.take<int>(2);                // [2] V', F'
};

__device__ __forceinline__ bool face_kept(const int* __restrict__ faces, int F, int V,
                                          const unsigned char* __restrict__ keep_face, int f, FaceIdx* t) {
  if (f >= F) return false;
  *t = load_face(faces, V, f);
  return t->ok && keep_face[f] != 0;
}

// marks the vertices of the kept faces and counts the kept faces of the workgroup
__global__ void __launch_bounds__(kThreads)
compact_mark_kernel(const int* __restrict__ faces, int F, int V, const unsigned char* __restrict__ keep_face,
                    int* __restrict__ used, int* __restrict__ wgc_f) {
  __shared__ int slot[kWaves];
  FaceIdx t;
  const bool keep = face_kept(faces, F, V, keep_face, blockIdx.x * kThreads + threadIdx.x, &t);
  if (keep) used[t.a] = used[t.b] = used[t.c] = 1;
  wave_count(keep, slot);
  __syncthreads();
  if (threadIdx.x == 0) wgc_f[blockIdx.x] = slot_sum(slot, kWaves);
}

__global__ void __launch_bounds__(kThreads)
compact_vertex_count_kernel(const int* __restrict__ used, int V, int* __restrict__ wgc_v) {
  __shared__ int slot[kWaves];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  wave_count(i < V && used[i] != 0, slot);
  __syncthreads();
  if (threadIdx.x == 0) wgc_v[blockIdx.x] = slot_sum(slot, kWaves);
}

__global__ void __launch_bounds__(kScanThreads)
compact_scan_kernel(const int* __restrict__ wgc_v, int bv, int* __restrict__ wgo_v, const int* __restrict__ wgc_f, int bf,
                    int* __restrict__ wgo_f, int* __restrict__ totals) {
  int sum[1];
  {
    const int* const in[1] = {wgc_v};
    int* const out[1] = {wgo_v};
    block_exclusive_scan<1>(in, out, bv, sum);
  }
  if (threadIdx.x == 0) totals[0] = sum[0];
  __syncthreads();                                              // the second scan reuses the first one's LDS
  {
    const int* const in[1] = {wgc_f};
    int* const out[1] = {wgo_f};
    block_exclusive_scan<1>(in, out, bf, sum);
  }
  if (threadIdx.x == 0) totals[1] = sum[0];
}

__global__ void __launch_bounds__(kThreads)
compact_emit_vertices_kernel(const float* __restrict__ vertices, const float* __restrict__ colors, int V,
                             const int* __restrict__ used, const int* __restrict__ wgo_v, int n_out,
                             int* __restrict__ new_index, float* __restrict__ out_vertices,
                             float* __restrict__ out_colors) {
  __shared__ int slot[kWaves];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool keep = i < V && used[i] != 0;
  const unsigned long long b = wave_count(keep, slot);
  __syncthreads();
  if (i >= V) return;
  int r = -1;
  if (keep) {
    r = wgo_v[blockIdx.x] + block_rank(b, slot);
    if (r >= n_out) r = -1;                                     // the workspace belongs to another mask: write nothing
  }
  new_index[i] = r;
  if (r < 0) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    out_vertices[3 * (size_t)r + a] = vertices[3 * (size_t)i + a];
    if (colors) out_colors[3 * (size_t)r + a] = colors[3 * (size_t)i + a];
  }
}

__global__ void __launch_bounds__(kThreads)
compact_emit_faces_kernel(const int* __restrict__ faces, int F, int V, const unsigned char* __restrict__ keep_face,
                          const int* __restrict__ wgo_f, const int* __restrict__ new_index, int n_out,
                          int* __restrict__ out_faces) {
  __shared__ int slot[kWaves];
  FaceIdx t;
  const bool keep = face_kept(faces, F, V, keep_face, blockIdx.x * kThreads + threadIdx.x, &t);
  const unsigned long long b = wave_count(keep, slot);
  __syncthreads();
  if (!keep) return;
  const int r = wgo_f[blockIdx.x] + block_rank(b, slot);
  if (r >= n_out) return;
  out_faces[3 * (size_t)r] = new_index[t.a];
  out_faces[3 * (size_t)r + 1] = new_index[t.b];
  out_faces[3 * (size_t)r + 2] = new_index[t.c];
}

// ---- connected components ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int load_link(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void store_link(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x: links strictly descend, so the walk ends after at most x steps
__device__ __forceinline__ int find_root(const int* __restrict__ parent, int x) {
  int p = load_link(parent + x);
  while (p < x) {
    x = p;
    p = load_link(parent + x);
  }
  return x;
}

// the same walk with path halving: a vertex that already hangs under another one (it is no root and never becomes one
// again, so no compare-and-swap can succeed on it) is re-hung under its grandparent - an ancestor, smaller still
__device__ __forceinline__ int find_root_halving(int* __restrict__ parent, int x) {
  int p = load_link(parent + x);
  while (p < x) {
    const int g = load_link(parent + p);
    if (g < p) store_link(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

// joins the sets of a and b.  Every failed CAS hands back a smaller parent of the larger root; indices are bounded below
// by 0, so the loop ends whatever the other threads do
__device__ __forceinline__ void unite(int* __restrict__ parent, int a, int b) {
  a = find_root_halving(parent, a);
  b = find_root_halving(parent, b);
  while (a != b) {
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicCAS(parent + a, a, b);                // hook the larger root under the smaller
    if (old == a) return;
    a = find_root_halving(parent, old);
    b = find_root_halving(parent, b);
  }
}

__global__ void __launch_bounds__(kThreads)
cc_init_kernel(int V, int* __restrict__ label, int* __restrict__ faces_of, unsigned long long* __restrict__ best) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) best[0] = 0ull;
  if (i >= V) return;
  label[i] = i;
  faces_of[i] = 0;
}

__global__ void __launch_bounds__(kThreads)
cc_hook_kernel(const int* __restrict__ faces, int F, int V, int* __restrict__ label) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const FaceIdx t = load_face(faces, V, f);
  if (!t.ok) return;
  if (t.a != t.b) unite(label, t.a, t.b);
  if (t.b != t.c) unite(label, t.b, t.c);
}

__global__ void __launch_bounds__(kThreads)
cc_flatten_kernel(int V, int* __restrict__ label) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= V) return;
  store_link(label + i, find_root(label, i));
}

// A wave walks its share of the faces 64 at a time and keeps a running (label, count) pair, the same in all its lanes: the
// lanes that share the first pending lane's label retire together (at most 64 rounds per step, one per distinct label), and
// the pair goes to memory as one atomic only when the label changes - a mesh that is one component costs one atomic per
// wave, not one per face
__global__ void __launch_bounds__(kThreads)
cc_face_count_kernel(const int* __restrict__ faces, int F, int V, const int* __restrict__ label,
                     int* __restrict__ faces_of) {
  const int lane = threadIdx.x & 63;
  int run_lab = -1, run_cnt = 0;
  for (long long base = (long long)blockIdx.x * kThreads + (threadIdx.x - lane); base < F;
       base += (long long)gridDim.x * kThreads) {
    const long long f = base + lane;
    int lab = -1;
    if (f < F) {
      const FaceIdx t = load_face(faces, V, f);
      if (t.ok) lab = label[t.a];
    }
    bool pending = lab >= 0;
    for (int round = 0; round < 64; ++round) {
      const unsigned long long todo = __ballot(pending);
      if (todo == 0ull) break;
      const int lead_lab = __shfl(lab, __ffsll((long long)todo) - 1, 64);
      const bool mine = pending && lab == lead_lab;
      const int n = __popcll(__ballot(mine));
      if (lead_lab != run_lab) {
        if (run_cnt > 0 && lane == 0) atomicAdd(faces_of + run_lab, run_cnt);
        run_lab = lead_lab;
        run_cnt = 0;
      }
      run_cnt += n;
      if (mine) pending = false;
    }
  }
  if (run_cnt > 0 && lane == 0) atomicAdd(faces_of + run_lab, run_cnt);
}

__global__ void __launch_bounds__(kThreads)
cc_best_kernel(int V, const int* __restrict__ faces_of, unsigned long long* __restrict__ best) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= V) return;
  const int c = faces_of[i];
  if (c > 0) atomicMax(best, ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(~(unsigned)i));
}

__global__ void __launch_bounds__(kThreads)
cc_mask_kernel(const int* __restrict__ faces, int F, int V, const int* __restrict__ label, const int* __restrict__ faces_of,
               int min_faces, int keep_largest, const unsigned long long* __restrict__ best,
               unsigned char* __restrict__ keep_face) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const FaceIdx t = load_face(faces, V, f);
  bool keep = false;
  if (t.ok) {
    const int lab = label[t.a];
    keep = faces_of[lab] >= min_faces;
    if (keep_largest) {
      const unsigned long long k = best[0];
      keep = keep && k != 0ull && lab == (int)(~(unsigned)(k & 0xffffffffull));
    }
  }
  keep_face[f] = keep ? 1 : 0;
}

}  // namespace

extern "C" int glorie_mesh_visibility(const float* vertices, int V, const float* w2cs, int M, float fx, float fy, float cx,
                                      float cy, int H, int W, float z_near, float z_far, int edge, const void* depth_table,
                                      float eps, int depth_missing_sees, int accumulate, int* count, void* stream) {
  if (V <= 0 || M < 0 || !vertices || !count || (M > 0 && !w2cs)) return GLORIE_EINVAL;
  if (H <= 0 || W <= 0 || (long long)H * W > INT32_MAX || !(fx > 0.f) || !(fy > 0.f)) return GLORIE_EINVAL;
  if (edge < 0 || !(z_far > z_near) || !(eps == eps)) return GLORIE_EINVAL;
  if ((unsigned)depth_missing_sees > 1u || (unsigned)accumulate > 1u) return GLORIE_EINVAL;
  VisCam cam;
  cam.fx = fx;
  cam.fy = fy;
  cam.cx = cx;
  cam.cy = cy;
  cam.z_near = z_near;
  cam.z_far = z_far;
  cam.eps = eps;
  cam.H = H;
  cam.W = W;
  cam.edge = edge;
  cam.missing_sees = depth_missing_sees;
  hipLaunchKernelGGL(mesh_visibility_kernel, dim3(blocks_of(V)), dim3(kThreads), 0, (hipStream_t)stream, vertices, V, w2cs,
                     M, cam, reinterpret_cast<const float* const*>(depth_table), accumulate, count);
  return check_launch();
}

extern "C" int glorie_mesh_select_faces(const int* faces, int F, int V, const int* count, int min_views, int rule,
                                        uint8_t* keep_face, void* stream) {
  if (V <= 0 || F < 0 || !count || (unsigned)rule > 1u) return GLORIE_EINVAL;
  if (F == 0) return GLORIE_OK;
  if (!faces || !keep_face) return GLORIE_EINVAL;
  hipLaunchKernelGGL(mesh_select_faces_kernel, dim3(blocks_of(F)), dim3(kThreads), 0, (hipStream_t)stream, faces, F, V,
                     count, min_views, rule, keep_face);
  return check_launch();
}

// workspace (CompactWs): used int [V] | new_index int [V] | marks per workgroup and their offsets int [Bv] x 2 | kept faces
// per workgroup and their offsets int [Bf] x 2 | totals int [2], every piece 8-byte aligned
extern "C" size_t glorie_mesh_compact_workspace(int V, int F) {
  return (V <= 0 || F <= 0) ? 0 : carved_bytes<CompactWs>(V, F);
}

extern "C" int glorie_mesh_compact_count(const int* faces, int F, int V, const uint8_t* keep_face, void* workspace,
                                         int* counts_out, void* stream) {
  if (V <= 0 || F <= 0 || !faces || !keep_face || !workspace || !counts_out) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const CompactWs w{Carver(workspace), V, F};
  const int bv = blocks_of(V), bf = blocks_of(F);
  counts_out[0] = counts_out[1] = 0;
  GLORIE_TRY(check_hip(hipMemsetAsync(w.used, 0, (size_t)V * sizeof(int), st)));
  hipLaunchKernelGGL(compact_mark_kernel, dim3(bf), dim3(kThreads), 0, st, faces, F, V, keep_face, w.used, w.wgc_f);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(compact_vertex_count_kernel, dim3(bv), dim3(kThreads), 0, st, w.used, V, w.wgc_v);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, w.wgc_v, bv, w.wgo_v, w.wgc_f, bf, w.wgo_f,
                     w.totals);
  GLORIE_TRY(check_launch());
  GLORIE_TRY(check_hip(hipMemcpyAsync(counts_out, w.totals, 2 * sizeof(int), hipMemcpyDeviceToHost, st)));
  return check_hip(hipStreamSynchronize(st));
}

extern "C" int glorie_mesh_compact_emit(const float* vertices, const float* colors, const int* faces, int F, int V,
                                        const uint8_t* keep_face, void* workspace, int V_out, int F_out,
                                        float* out_vertices, float* out_colors, int* out_faces, void* stream) {
  if (V <= 0 || F <= 0 || V_out < 0 || F_out < 0 || V_out > V || F_out > F) return GLORIE_EINVAL;
  if (!vertices || !faces || !keep_face || !workspace) return GLORIE_EINVAL;
  if (V_out == 0 && F_out == 0) return GLORIE_OK;
  if ((V_out > 0 && !out_vertices) || (F_out > 0 && !out_faces) || (colors && V_out > 0 && !out_colors)) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const CompactWs w{Carver(workspace), V, F};
  hipLaunchKernelGGL(compact_emit_vertices_kernel, dim3(blocks_of(V)), dim3(kThreads), 0, st, vertices, colors, V, w.used,
                     w.wgo_v, V_out, w.new_index, out_vertices, out_colors);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(compact_emit_faces_kernel, dim3(blocks_of(F)), dim3(kThreads), 0, st, faces, F, V, keep_face, w.wgo_f,
                     w.new_index, F_out, out_faces);
  return check_launch();
}

extern "C" size_t glorie_mesh_components_workspace(void) { return sizeof(unsigned long long); }

extern "C" int glorie_mesh_components(const int* faces, int F, int V, int min_faces, int keep_largest, void* workspace,
                                      int* label, int* faces_of, uint8_t* keep_face, void* stream) {
  if (V <= 0 || F < 0 || !label || !faces_of || !workspace || (unsigned)keep_largest > 1u) return GLORIE_EINVAL;
  if (F > 0 && !faces) return GLORIE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* best = reinterpret_cast<unsigned long long*>(workspace);
  hipLaunchKernelGGL(cc_init_kernel, dim3(blocks_of(V)), dim3(kThreads), 0, st, V, label, faces_of, best);
  GLORIE_TRY(check_launch());
  if (F == 0) return GLORIE_OK;
  hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks_of(F)), dim3(kThreads), 0, st, faces, F, V, label);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks_of(V)), dim3(kThreads), 0, st, V, label);
  GLORIE_TRY(check_launch());
  hipLaunchKernelGGL(cc_face_count_kernel, dim3(min(blocks_of(F), kCountBlocks)), dim3(kThreads), 0, st, faces, F, V, label,
                     faces_of);
  GLORIE_TRY(check_launch());
  if (!keep_face) return GLORIE_OK;
  if (keep_largest) {
    hipLaunchKernelGGL(cc_best_kernel, dim3(blocks_of(V)), dim3(kThreads), 0, st, V, faces_of, best);
    GLORIE_TRY(check_launch());
  }
  hipLaunchKernelGGL(cc_mask_kernel, dim3(blocks_of(F)), dim3(kThreads), 0, st, faces, F, V, label, faces_of, min_faces,
                     keep_largest, best, keep_face);
  return check_launch();
}
