// Masked ray sampling and the depth gate of the per-keyframe mapping loop (reference: src/mapper.py:427-431 draws every
// window frame's pixels among the pixels of its render mask - get_samples / select_uv, src/utils/common.py:57-145, with
// mask.nonzero() and randint(count) - and :474-482 keeps the rays with depth <= min(10 median, 1.2 max)).  Done that way
// every window frame costs a host synchronisation per iteration (nonzero and boolean indexing size their results on the
// host).  Here nothing is sized by the data:
//
//   valid_index_kernel    once per window: per frame the bit mask of its valid pixels (depth > 0), 64 pixels a word in
//                         the reference's row-major order, and the exclusive prefix of the words' popcounts with the
//                         frame's valid count last: a rank table.  One workgroup of 16 waves per frame; a wave forms a
//                         word with one ballot over 64 coalesced loads and keeps 64 words (one per lane) before it
//                         stores them and their wave-local prefix coalesced; after one barrier every lane adds its
//                         wave's offset to the entries it wrote itself, so no thread reads another thread's stores.
//   sample_rays_kernel    every iteration: ray r of slot m maps its draw in [0, 2^31) to rank = (draw * count_m) >> 31
//                         (exact in int64), finds the word holding that rank by binary search in the prefix, the bit by
//                         popcount steps inside its own lane, and gathers what window_rays_kernel gathers through the
//                         same code (window_rays.hiph).  One wave per workgroup, one slot per workgroup, as there.
//   depth_gate_kernel     every iteration: the lower median of the positive depths by an exact radix select over the
//                         float bits (positive floats order as unsigned integers; 8 bits per pass, 4 passes), their
//                         maximum, the threshold, and keep = depth > 0 && depth <= threshold as 1 / 0 weights.  One
//                         workgroup; a wave counts a digit with eight ballots (the lanes that share a digit elect one
//                         of them to add their number to the wave's own LDS histogram), so there is no atomic; the bin
//                         that holds the rank is picked by radix.hiph's bin_pick.
//
// No host synchronisation, no atomics, no output sized by the data; every launch is on the caller's stream.
#include "radix.hiph"
#include "window_rays.hiph"

using namespace glorie;

namespace {

constexpr int kRayThreads = 64;        // one wave: the slot of a workgroup is uniform without any cross-lane step
constexpr int kIndexWaves = 16;        // valid_index_kernel: waves per frame
constexpr int kGateWaves = 16;         // depth_gate_kernel: waves of its one workgroup
constexpr long long kGateMaxN = 1LL << 22;

// ---- rank tables ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kIndexWaves * 64)
valid_index_kernel(const float* const* __restrict__ depth_table, int HW, int nw, int all_valid,
                   unsigned long long* __restrict__ words, int* __restrict__ prefix) {
  __shared__ int wave_total[kIndexWaves];
  const int m = blockIdx.x;                                           // frame (uniform)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* __restrict__ dmap = all_valid ? nullptr : depth_table[m];
  unsigned long long* __restrict__ wm = words + (size_t)m * nw;
  int* __restrict__ pm = prefix + (size_t)m * (nw + 1);

  // blocks of 64 words (4096 pixels); a wave takes a contiguous run of them
  const int blocks = (nw + 63) / 64, run = (blocks + kIndexWaves - 1) / kIndexWaves;
  const int b0 = min(wave * run, blocks), b1 = min(b0 + run, blocks);
  int base = 0;                                                       // valid pixels of this wave before block b (uniform)
  for (int b = b0; b < b1; ++b) {
    unsigned long long mine = 0ull;
#pragma unroll 8
    for (int q = 0; q < 64; ++q) {
      const long long p = ((long long)b * 64 + q) * 64 + lane;         // pixel j * W + i
      bool v = p < HW;
      if (v && !all_valid) v = dmap[p] > 0.0f;                        // NaN and negative depths are invalid
      const unsigned long long word = __ballot(v);
      if (lane == q) mine = word;
    }
    const int w = b * 64 + lane, cnt = __popcll(mine);
    int incl = cnt;                                                   // inclusive scan of the 64 popcounts
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (w < nw) {
      wm[w] = mine;
      pm[w] = base + incl - cnt;
    }
    base += __shfl(incl, 63, 64);
  }
  if (lane == 0) wave_total[wave] = base;
  __syncthreads();
  int offset = 0, total = 0;
  for (int q = 0; q < kIndexWaves; ++q) {
    if (q < wave) offset += wave_total[q];
    total += wave_total[q];
  }
  if (offset) {
    for (int b = b0; b < b1; ++b) {
      const int w = b * 64 + lane;
      if (w < nw) pm[w] += offset;                                    // the entry this very lane wrote above
    }
  }
  if (threadIdx.x == 0) pm[nw] = total;
}

// ---- one iteration's rays ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRayThreads)
sample_rays_kernel(const float* const* __restrict__ depth_table, const float* const* __restrict__ image_table,
                   const float* const* __restrict__ radius_table, const float* __restrict__ c2ws, int per, int chunks,
                   int chw, int H, int W, int nw, float fx, float fy, float cx, float cy,
                   const int64_t* __restrict__ draws, const unsigned long long* __restrict__ words,
                   const int* __restrict__ prefix, float const_radius, float* __restrict__ rays_o,
                   float* __restrict__ rays_d, float* __restrict__ depth, float* __restrict__ color,
                   float* __restrict__ radius, int64_t* __restrict__ ii, int64_t* __restrict__ jj) {
  const int m = blockIdx.x / chunks;                                  // window slot (uniform)
  const int k = (blockIdx.x - m * chunks) * kRayThreads + threadIdx.x;   // ray within the slot
  if (k >= per) return;
  const size_t r = (size_t)m * per + k;
  const unsigned long long* __restrict__ wm = words + (size_t)m * nw;
  const int* __restrict__ pm = prefix + (size_t)m * (nw + 1);
  const int HW = H * W;
  const long long count = min(max(pm[nw], 0), HW);                    // uniform; a bad table cannot send a ray outside

  int p = 0;
  if (count > 0) {
    long long q = draws[r];
    q = q < 0 ? 0 : (q > 0x7fffffffLL ? 0x7fffffffLL : q);
    const int rank = (int)((q * count) >> 31);                        // in [0, count)
    int lo = 0, hi = nw;                                              // prefix[lo] <= rank < prefix[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (pm[mid] <= rank) lo = mid; else hi = mid;
    }
    unsigned long long x = wm[lo];
    int kth = rank - pm[lo], pos = 0;                                 // the kth set bit of x, counted from bit 0
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const int c = __popcll(x & ((1ull << s) - 1ull));
      if (kth >= c) {
        kth -= c;
        x >>= s;
        pos += s;
      }
    }
    p = min(lo * 64 + pos, HW - 1);
  }
  const int j = p / W, i = p - j * W;
  gather_ray(c2ws + 16 * (size_t)m, depth_table[m], image_table[m], (radius && radius_table) ? radius_table[m] : nullptr,
             chw, H, W, fx, fy, cx, cy, i, j, r, const_radius, rays_o, rays_d, depth, color, radius);
  if (count == 0) depth[r] = 0.0f;                                    // a slot without a valid pixel: its rays carry no depth
  ii[r] = i;
  jj[r] = j;
}

// ---- the depth gate ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateWaves * 64)
depth_gate_kernel(const float* __restrict__ depth, int N, float* __restrict__ keep, float* __restrict__ stats) {
  __shared__ unsigned int hist[kGateWaves][256];
  __shared__ unsigned int total[256];
  __shared__ unsigned int pick[2];                                    // the selected digit, the rank inside it
  constexpr int T = kGateWaves * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  unsigned int key = 0u;            // the median's leading bits found so far
  unsigned int kth = 0u;            // its rank among the positive depths that share them
  unsigned int max_bits = 0u;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int b = tid; b < kGateWaves * 256; b += T) (&hist[0][0])[b] = 0u;
    __syncthreads();
    for (int base = 0; base < N; base += T) {                         // uniform trip count: every lane reaches the ballots
      const int idx = base + tid;
      const float d = idx < N ? depth[idx] : 0.0f;
      const unsigned int bits = __float_as_uint(d);
      bool in = d > 0.0f;                                             // NaN is out; +inf is a positive depth
      if (pass > 0) in = in && ((bits ^ key) >> (shift + 8)) == 0u;
      const unsigned int digit = (bits >> shift) & 255u;
      if (pass == 0 && in) max_bits = max(max_bits, bits);
      unsigned long long peers = __ballot(in);                        // the lanes that share this lane's digit
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const bool bit = (digit >> q) & 1u;
        const unsigned long long set = __ballot(in && bit);
        peers &= bit ? set : ~set;
      }
      if (in && lane == __ffsll((long long)peers) - 1) hist[wave][digit] += (unsigned int)__popcll(peers);
    }
    __syncthreads();
    if (tid < 256) {
      unsigned int s = 0u;
#pragma unroll
      for (int q = 0; q < kGateWaves; ++q) s += hist[q][tid];
      total[tid] = s;
    }
    __syncthreads();
    if (wave == 0) {
      // pass 0: the bins hold every positive depth, the rank is their lower median's; no positive depth at all: digit 256
      const BinPick p =
          bin_pick(total, [=](unsigned int n_in) { return pass == 0 ? (n_in ? (n_in - 1u) / 2u : 0u) : kth; });
      if (lane == 0) {
        pick[0] = p.digit;
        pick[1] = p.rank;
      }
    }
    __syncthreads();
    if (pick[0] == 256u) break;                                       // uniform
    key |= pick[0] << shift;
    kth = pick[1];
  }
  const bool none = pick[0] == 256u;
  const unsigned int mx = block_reduce_all<kGateWaves, MaxOp>(max_bits);

  float median = 0.0f, dmax = 0.0f, thr = 0.0f;
  if (!none) {
    median = __uint_as_float(key);
    dmax = __uint_as_float(mx);
    thr = fminf(10.0f * median, 1.2f * dmax);                         // two single products: nothing to contract
  }
  int kept = 0;
  for (int idx = tid; idx < N; idx += T) {
    const float d = depth[idx];
    const bool k = !none && d > 0.0f && d <= thr;
    keep[idx] = k ? 1.0f : 0.0f;
    kept += k ? 1 : 0;
  }
  const int all = block_sum<kGateWaves>(kept);
  if (tid == 0) {
    stats[0] = median;
    stats[1] = dmax;
    stats[2] = thr;
    stats[3] = (float)all;
  }
}

}  // namespace

extern "C" int glorie_valid_index_build(const void* depth_table, int M, int H, int W, int mode, uint64_t* words,
                                        int32_t* prefix, void* stream) {
  if (M < 0 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL - 4096) return GLORIE_EINVAL;
  if (mode != GLORIE_VALID_DEPTH && mode != GLORIE_VALID_ALL) return GLORIE_EINVAL;
  if (M == 0) return GLORIE_OK;
  if (!words || !prefix || (mode == GLORIE_VALID_DEPTH && !depth_table)) return GLORIE_EINVAL;
  const int HW = H * W, nw = (HW + 63) / 64;
  hipLaunchKernelGGL(valid_index_kernel, dim3((unsigned)M), dim3(kIndexWaves * 64), 0, (hipStream_t)stream,
                     reinterpret_cast<const float* const*>(depth_table), HW, nw, mode == GLORIE_VALID_ALL ? 1 : 0,
                     reinterpret_cast<unsigned long long*>(words), prefix);
  return check_launch();
}

extern "C" int glorie_sample_window_rays(const void* depth_table, const void* image_table, const void* radius_table,
                                         const float* c2ws, int M, int per, int chw, int H, int W, float fx, float fy,
                                         float cx, float cy, const int64_t* draws, const uint64_t* words,
                                         const int32_t* prefix, float const_radius, int want_radius, float* rays_o,
                                         float* rays_d, float* depth, float* color, float* radius, int64_t* ii, int64_t* jj,
                                         void* stream) {
  if (M < 0 || per < 0 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL - 4096) return GLORIE_EINVAL;
  if (M == 0 || per == 0) return GLORIE_OK;                           // N = 0: nothing is launched
  const long long chunks = ((long long)per + kRayThreads - 1) / kRayThreads;
  if ((long long)M * per > 0x7fffffffLL || (long long)M * chunks > 0x7fffffffLL) return GLORIE_EUNSUPPORTED;
  if (!depth_table || !image_table || !c2ws || !draws || !words || !prefix || !rays_o || !rays_d || !depth || !color ||
      !ii || !jj)
    return GLORIE_EINVAL;
  if (want_radius && !radius) return GLORIE_EINVAL;
  const int nw = (H * W + 63) / 64;
  hipLaunchKernelGGL(sample_rays_kernel, dim3((unsigned)(M * chunks)), dim3(kRayThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const float* const*>(depth_table),
                     reinterpret_cast<const float* const*>(image_table),
                     reinterpret_cast<const float* const*>(radius_table), c2ws, per, (int)chunks, chw ? 1 : 0, H, W, nw,
                     fx, fy, cx, cy, draws, reinterpret_cast<const unsigned long long*>(words), prefix, const_radius,
                     rays_o, rays_d, depth, color, want_radius ? radius : nullptr, ii, jj);
  return check_launch();
}

extern "C" int glorie_depth_gate(const float* depth, long long N, float* keep, float* stats, void* stream) {
  if (N < 0 || !stats) return GLORIE_EINVAL;
  if (N > kGateMaxN) return GLORIE_EUNSUPPORTED;
  if (N == 0) return GLORIE_OK;                                       // nothing is launched
  if (!depth || !keep) return GLORIE_EINVAL;
  hipLaunchKernelGGL(depth_gate_kernel, dim3(1), dim3(kGateWaves * 64), 0, (hipStream_t)stream, depth, (int)N, keep,
                     stats);
  return check_launch();
}
