// All-pairs correlation pyramid of an edge, built straight into the layout the lookup reads (scope row A1):
//   CorrBlock.__init__ / CorrBlock.corr   /root/reference/src/modules/droid_net/corr.py:26-41,67-76
//   corr[p][q] = fp16( sum_c fp16(f1[c][p] / 4) * fp16(f2[c][q] / 4) )     (autocast: fp16 GEMM, fp32 accumulation)
//   level l + 1 = avg_pool2d(level l, 2, 2) on fp16 tensors (fp32 average rounded to fp16)
// The reference (and round 1 of this repo) runs a library GEMM into a row-major [h1*w1][h2][w2] volume, three
// avg_pool2d launches, and this repo then re-tiled every level (pad + permute + copy: ~250 MB of traffic per edge).
// Here one launch per batch of new edges writes all four levels once, in the 4x8-tiled layout of
// corr_lookup_r3_tiled_kernel, into the SLOT of an arena (CorrArena): adding / removing edges never moves a
// volume again (factor_graph.py:126,161 copy all of them through boolean masks).
//
// Workgroup = 32 consecutive source pixels x 8 target rows (two tiled block rows of level 0 = one block row of level 1 =
// two rows of level 2 = one row of level 3), 4 waves.  The levels are computed in LDS by the front half this builder
// shares with the displacement-major one (corr_pyramid.hiph); the block rows leave LDS as 16-byte pieces, 640 contiguous
// bytes per (pixel, block row).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "corr_pyramid.hiph"

namespace glorie {

typedef CorrPad<0, 0, 0, 0> TiledPad;     // the write-out reads whole block rows: 16-byte pieces, conflict-free as they are

__global__ __launch_bounds__(256, 2) void corr_build_kernel(CorrBuildArgs a) {
  constexpr int PX = 32;
  extern __shared__ __attribute__((aligned(16))) _Float16 bsm[];
  const int tid = threadIdx.x;
  const int h = a.h, w = a.w, HW = h * w;
  const int e = blockIdx.z, grp = blockIdx.y, p0 = blockIdx.x * PX;
  const size_t sl = (size_t)a.slot[e];
  const CorrPyramidLds py = corr_pyramid_lds<TiledPad>(a.f, (int)a.ii[e], (int)a.jj[e], h, w, grp, a.num_levels, bsm,
                                                       [&](int k) { return min(p0 + k, HW - 1); });
  // ---- write-out: 16-byte pieces = one row of a 4x8 block; rows / blocks beyond the level's size are skipped ----
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    if (a.num_levels <= l) break;
    // py.lvl[l] [PX][rows][Wp]; level plane: [ceil(hl/4)][ceil(wl/8)][4][8]; global rows y0 .. y0 + rows - 1
    const int rows = 8 >> l, Wp = py.W[l], hl = h >> l, wl = w >> l, y0 = rows * grp;
    const int nbx = (wl + 7) >> 3, nby = (hl + 3) >> 2;
    const size_t plane = (size_t)nbx * nby * 32;
    const int per_px = rows * nbx;
    for (int idx = tid; idx < PX * per_px; idx += 256) {
      const int px = idx / per_px, r = idx - px * per_px;
      const int ly = r / nbx, bx = r - ly * nbx, y = y0 + ly;
      if (p0 + px >= HW || y >= hl) continue;
      const uint4 v = *reinterpret_cast<const uint4*>(py.lvl[l] + (size_t)px * py.stride[l] + ly * Wp + bx * 8);
      _Float16* d = a.lvl[l] + (sl * HW + p0 + px) * plane + ((size_t)(y >> 2) * nbx + bx) * 32 + (y & 3) * 8;
      *reinterpret_cast<uint4*>(d) = v;
    }
  }
}

}  // namespace glorie

using namespace glorie;

extern "C" int glorie_corr_build(const void* fmaps_cl, const int64_t* ii, const int64_t* jj, const int* slots,
                                 void* const* levels, int num_levels, int n_new, int h, int w, int C, void* stream) {
  // widths that are not multiples of 8 keep the torch builder
  return corr_build_launch<corr_build_kernel, TiledPad>(fmaps_cl, ii, jj, slots, levels, num_levels, n_new, h, w, C,
                                     stream, [&] { return (w & 7) ? 0 : (h * w + 31) / 32; });
}
