"""Scene builders and float64 references for the correlation kernels (numpy, CPU only; test infrastructure).

The hot correlation kernels differ from the oracle (oracle/corr.py) only where a summation ORDER is free: the fp32
accumulation of a 128-channel dot product on the matrix cores, and the fp32 accumulation of the fused 1x1 encoder.  The
scenes built here take that freedom away, so the tests that use them compare bit for bit:

  * order-free feature scenes: maps of small integers times 4.  After the product path's /4 every channel product of
    <f_i[p], pool_l(f_j)[q]> is an integer multiple of 4^-l and the sum of their magnitudes stays below 2^24 lsbs, so
    EVERY fp32 summation order gives the same exact number, and that number is representable in fp16.  The builder
    proves both claims on the scene it returns (`assert_order_free`) instead of trusting them;
  * encoder-exact scenes: all lookup values multiples of one lsb 2^-k with
    (max_row(sum|W|) max|corr| + max|b|) 2^k < 2^24, so W corr + b is exact in fp32 in any order and its fp16 rounding is
    unique (`encoder_reference` proves the bound on the scene it is given and returns the float64 result rounded once);
  * alt-corr integer scenes: integer features and quarter coordinates, the same argument for the fp32 path
    (`altcorr_exact_bound`).

`box_plan` mirrors the box rule of the volume-free kernel and is used ONLY to assert that a coordinate scene reaches the
branches it was written for; no expected value comes from it."""
import numpy as np

from oracle import corr as ocorr

F64 = np.float64

# ---- sizes shared by test_corr_ref.py (CPU) and test_gpu_corr_exact.py ------------------------------------------------------
SIZES8 = [(16, 24), (24, 32)]                      # multiples of the 8 x 8 source tile
SIZES_RAGGED_LEVELS = [(12, 16), (20, 24)]         # level 3 is 1 x 2 / 2 x 3, ragged heights at levels 2 and 3
SIZES_RAGGED = [(9, 17), (13, 22)]                 # no multiple of 8: half tiles, odd level widths
SIZES_ALL = SIZES8 + SIZES_RAGGED_LEVELS + SIZES_RAGGED
OTF_II = np.array([0, 1, 2, 1], np.int64)           # edge 3: ii == jj
OTF_JJ = np.array([1, 0, 0, 1], np.int64)
OTF_ENC_II = np.array([0, 1, 2, 0], np.int64)       # the encoder-exact scene of the volume-free lookup
OTF_ENC_JJ = np.array([1, 0, 0, 2], np.int64)


def _is_int(x):
    return bool(np.all(np.asarray(x, F64) == np.rint(np.asarray(x, F64))))


def _fp16_exact(x):
    x = np.asarray(x, F64)
    with np.errstate(over="ignore"):
        return bool(np.all(x.astype(np.float16).astype(F64) == x))


# ---- order-free feature scenes ---------------------------------------------------------------------------------------
def order_free_features(seed, F_, H, W, C=128, values=(-8, -4, 0, 4, 8), density=1.0, num_levels=4):
    """fp16 maps [F, C, H, W] of small integers times 4 (a fraction `density` of the channels non-zero per pixel), proven
    order-free for every ordered pair of frames"""
    rng = np.random.default_rng(seed)
    fm = rng.choice(np.asarray(values, F64), size=(F_, C, H, W))
    if density < 1.0:
        fm = fm * (rng.random((F_, C, H, W)) < density)
    fm = fm.astype(np.float16)
    pairs = [(i, j) for i in range(F_) for j in range(F_)]
    assert_order_free(fm, [p[0] for p in pairs], [p[1] for p in pairs], num_levels)
    return fm


def assert_order_free(fm, ii, jj, num_levels=4):
    """proof, in float64, that on these maps every level-l dot product <f_i[p], pool_l(f_j)[q]> of the product path is
    (1) the same exact fp32 number in ANY summation order and (2) exactly representable in fp16; also that the pooled
    pyramid itself is exact (no fp16 rounding in /4 or in any avg_pool step).  Returns max |dot|."""
    fm = np.asarray(fm)
    assert fm.dtype == np.float16
    levels = ocorr.otf_pyramid(fm, num_levels)                     # the oracle's fp16 pyramid of fm / 4
    exact = np.asarray(fm, F64) / 4.0
    worst = 0.0
    for l, fl in enumerate(levels):
        assert np.array_equal(fl.astype(F64), exact), f"level {l}: the fp16 pyramid rounds"
        lsb = 4.0 ** -l
        assert _is_int(exact / lsb), f"level {l}: values are no multiples of 4^-{l}"
        F_, C, hl, wl = exact.shape
        b_all = exact.reshape(F_, C, hl * wl)
        a_all = np.asarray(fm, F64).reshape(fm.shape[0], C, -1) / 4.0
        assert _is_int(a_all)
        for i, j in sorted(set(zip(map(int, ii), map(int, jj)))):
            # every partial sum, in any order, is a multiple of lsb bounded by sum_c |a_c b_c|: exact in fp32 below 2^24 lsbs
            bound = (np.abs(a_all[i]).T @ np.abs(b_all[j])).max()
            assert bound / lsb < 2.0 ** 24, f"level {l}, pair ({i},{j}): partial sums reach {bound / lsb} lsbs"
            dots = a_all[i].T @ b_all[j]                           # exact in float64 (integers of lsb below 2^53)
            assert _fp16_exact(dots), f"level {l}, pair ({i},{j}): a dot product is not an fp16 number"
            worst = max(worst, float(np.abs(dots).max()))
        if l + 1 < num_levels:                                      # exact 2 x 2 average of the level below
            h2, w2 = hl // 2, wl // 2
            e = exact[..., :2 * h2, :2 * w2]
            exact = (e[..., 0::2, 0::2] + e[..., 0::2, 1::2] + e[..., 1::2, 0::2] + e[..., 1::2, 1::2]) / 4.0
    return worst


def otf_volumes(fm, ii, jj, num_levels=4):
    """the virtual fp16 volumes of oracle.corr.corr_otf, [N, H, W, h_l, w_l] per level (float64 GEMM rounded to fp32, then
    to fp16, like the oracle): shared among the coordinate scenes of a test instead of being recomputed per scene"""
    levels = ocorr.otf_pyramid(fm, num_levels)
    F_, C, H, W = levels[0].shape
    vols = []
    for fl in levels:
        hl, wl = fl.shape[2:]
        a = levels[0].astype(F64).reshape(F_, C, H * W)
        b = fl.astype(F64).reshape(F_, C, hl * wl)
        v = np.stack([a[int(i)].T @ b[int(j)] for i, j in zip(ii, jj)])
        vols.append(v.astype(np.float32).astype(np.float16).reshape(len(ii), H, W, hl, wl))
    return vols


def otf_lookup(vols, coords, radius=3):
    """oracle.corr.corr_otf on precomputed volumes: coords [N, 2, H, W] -> [N, L * 49, H, W] fp16"""
    return ocorr.corr_lookup_pyramid(vols, coords, radius)


def lookup_f64(vols, coords, radius=3):
    """An independent restatement of the pyramid lookup: per OUTPUT (i, j) the four taps in the reference's order, every
    pinned step (corr_common.hiph) evaluated in float64 and rounded ONCE to its format: weight fp32 -> fp16, product -> fp16,
    sum -> fp16; a tap outside the map is skipped.  vols: fp16 levels [N, h, w, h_l, w_l] -> [N, L * 49, h, w] fp16"""
    coords = np.asarray(coords, np.float32)
    outs = []
    rd = 2 * radius + 1
    for l, vol in enumerate(vols):
        N, h1, w1, h2, w2 = vol.shape
        c = coords / np.float32(2 ** l)
        fx, fy = np.floor(c[:, 0]), np.floor(c[:, 1])
        dx, dy = c[:, 0] - fx, c[:, 1] - fy                          # fp32, like 1 - dx below (pinned fp32 steps)
        ex, ey = (np.float32(1) - dx).astype(F64), (np.float32(1) - dy).astype(F64)
        dx, dy = dx.astype(F64), dy.astype(F64)
        wts = [ex * ey, ex * dy, dx * ey, dx * dy]                   # taps (0,0), (0,+y), (+x,0), (+x,+y)
        wts = [w.astype(np.float32).astype(np.float16).astype(F64) for w in wts]
        x0 = fx.astype(np.int64) - radius
        y0 = fy.astype(np.int64) - radius
        n_i, y_i, x_i = np.meshgrid(np.arange(N), np.arange(h1), np.arange(w1), indexing="ij")
        out = np.zeros((N, rd, rd, h1, w1), np.float16)
        for i in range(rd):
            for j in range(rd):
                acc = np.zeros((N, h1, w1), F64)
                for (ox, oy), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), wts):
                    tx, ty = x0 + i + ox, y0 + j + oy
                    inb = (tx >= 0) & (tx < w2) & (ty >= 0) & (ty < h2)
                    s = vol[n_i, y_i, x_i, np.clip(ty, 0, h2 - 1), np.clip(tx, 0, w2 - 1)].astype(F64)
                    with np.errstate(over="ignore"):
                        prod = (s * wt).astype(np.float16).astype(F64)
                        new = (acc + prod).astype(np.float16).astype(F64)
                    acc = np.where(inb, new, acc)
                out[:, i, j] = acc.astype(np.float16)
        outs.append(out.reshape(N, rd * rd, h1, w1))
    return np.concatenate(outs, 1)


# ---- encoder-exact scenes --------------------------------------------------------------------------------------------
def encoder_reference(corr, weight, bias):
    """relu(W corr + b) of corr_encoder[0] in float64, rounded ONCE to fp16 - after proving that the scene is encoder-exact:
    corr [N, 196, h, w] fp16, weight [128, 196] and bias [128] (numbers the kernels hold exactly: fp16 weights, fp32 bias).
    Raises AssertionError if the bound fails.  Returns (out [N, 128, h, w] fp16, k, bound / 2^24)."""
    corr = np.asarray(corr)
    assert corr.dtype == np.float16 and np.all(np.isfinite(corr))
    c = corr.astype(F64)
    w = np.asarray(weight, F64).reshape(128, -1)
    b = np.asarray(bias, F64)
    assert _fp16_exact(w) and np.array_equal(b.astype(np.float32).astype(F64), b)
    assert _is_int(w), "integer weights expected (products then keep the lookup's lsb)"
    k = 0
    while not _is_int(c * 2.0 ** k):
        k += 1
        assert k <= 24
    assert _is_int(b * 2.0 ** k), "the bias is no multiple of the lookup's lsb"
    bound = (np.abs(w).sum(1).max() * np.abs(c).max() + np.abs(b).max()) * 2.0 ** k
    assert bound < 2.0 ** 24, f"not encoder-exact: lsb 2^-{k}, bound {bound / 2.0 ** 24:.3g} * 2^24"
    out = np.einsum("ok,nkyx->noyx", w, c) + b[None, :, None, None]
    assert _is_int(out * 2.0 ** k)
    return np.maximum(out, 0.0).astype(np.float16), k, bound / 2.0 ** 24


def integer_encoder(seed, lo, hi, bias_step=0.125, bias_max=2.0, density=1.0):
    """corr_encoder[0] parameters of an encoder-exact scene: integer weights [128, 196, 1, 1] in [lo, hi] (a fraction
    `density` of them kept, the others zero), bias multiples of bias_step in [-bias_max, bias_max]"""
    rng = np.random.default_rng(seed)
    w = rng.integers(lo, hi + 1, (128, 196, 1, 1)).astype(np.float32)
    w *= rng.random(w.shape) < density
    b = (rng.integers(-int(bias_max / bias_step), int(bias_max / bias_step) + 1, 128) * bias_step).astype(np.float32)
    return w, b


# ---- the box rule of corr_otf8_kernel -----------------------------------------------------------------------------------
SHARED, QUADS, SINGLES = 0, 1, 2
BOX_CAP = 320


def box_plan(coords, h, w, num_levels=4):
    """Mirror of the volume-free kernel's box rule for ONE edge: coords [2, h, w] float32.  Per 8 x 8 block (pixels clamped
    into the map) and level: window origins floor(clamp(c / 2^l, +-1e6)) - 3, box = min .. max + 7; the block shares the box
    if its area is <= 320, otherwise each 4 x 4 quadrant is tried, then its single pixels.
    Returns (branch [nby, nbx, L, 4] of SHARED / QUADS / SINGLES per quadrant, area [nby, nbx, L] of the whole-block box)."""
    coords = np.asarray(coords, np.float32)
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    branch = np.zeros((nby, nbx, num_levels, 4), np.int64)
    area = np.zeros((nby, nbx, num_levels), np.int64)
    ys = np.minimum(np.arange(nby * 8), h - 1)
    xs = np.minimum(np.arange(nbx * 8), w - 1)
    c = coords[:, ys][:, :, xs]                                     # [2, nby * 8, nbx * 8]
    for l in range(num_levels):
        s = np.clip(c * np.float32(1.0 / (1 << l)), np.float32(-1.0e6), np.float32(1.0e6))
        o = np.floor(s).astype(np.int64) - 3
        ob = o.reshape(2, nby, 8, nbx, 8)

        def box(v):                                                 # v [2, nby, ?, nbx, ?] -> area per block
            lo, hi = v.min(axis=(2, 4)), v.max(axis=(2, 4)) + 7
            return (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1)
        area[:, :, l] = box(ob)
        for q in range(4):
            qa = box(ob[:, :, 4 * (q >> 1):4 * (q >> 1) + 4, :, 4 * (q & 1):4 * (q & 1) + 4])
            branch[:, :, l, q] = np.where(area[:, :, l] <= BOX_CAP, SHARED, np.where(qa <= BOX_CAP, QUADS, SINGLES))
    return branch, area


# ---- coordinate scenes ---------------------------------------------------------------------------------------------------
def _grid(h, w):
    y, x = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    return y, x


def _blocked(h, w, step_x, step_y, off_x, off_y):
    """per 8 x 8 block: origin of the block + step * (position inside the block) + offset"""
    y, x = _grid(h, w)
    ly, lx = y % 8, x % 8
    return np.stack([(x - lx) + np.float32(step_x) * lx + np.float32(off_x),
                     (y - ly) + np.float32(step_y) * ly + np.float32(off_y)]).astype(np.float32)


def scene_box320(h, w):
    """(a) per-pixel steps of 1.75 px in x and 1.25 px in y inside a block: window origins span 12 x 8, box 20 x 16 = 320"""
    return _blocked(h, w, 1.75, 1.25, -2.0, -1.0)


def scene_box336(h, w):
    """(b) 1.875 px in x: box 21 x 16 = 336 - level 0 (only) falls back, all four quadrants fit"""
    return _blocked(h, w, 1.875, 1.25, -3.0, -1.0)


def scene_one_quadrant(h, w):
    """(c) smooth flow, but two pixels of quadrant 3 of every block look at opposite corners of the map: that quadrant goes to
    single pixels, the other three fit"""
    y, x = _grid(h, w)
    c = np.stack([x + 0.5, y + 0.25]).astype(np.float32)
    a = (y % 8 == 5) & (x % 8 == 6)
    b = (y % 8 == 6) & (x % 8 == 4)
    c[0][a], c[1][a] = 0.5, 0.25
    c[0][b], c[1][b] = w - 1.5, h - 1.75
    return c


def scene_scatter(h, w):
    """(d) every pixel discontinuous: targets scattered over the whole map"""
    y, x = _grid(h, w)
    return np.stack([(x * 7 + y * 13) % w + 0.25 * (x % 4), (y * 5 + x * 11) % h + 0.25 * (y % 4)]).astype(np.float32)


def scene_scatter_wide(h, w):
    """(d) scattered over the map and 64 px beyond it: single pixels at every level (the level-3 origins still spread)"""
    y, x = _grid(h, w)
    return np.stack([(x * 37 + y * 53) % (w + 128) - 64 + 0.25 * (x % 4),
                     (y * 29 + x * 43) % (h + 128) - 64 + 0.25 * (y % 4)]).astype(np.float32)


def scene_scale3(h, w):
    """(e) a scale of 3 about the map centre: levels 0 and 1 fall back (29 x 29, 18 x 18), levels 2 and 3 share a box; the
    outer thirds of the map look outside it"""
    y, x = _grid(h, w)
    return np.stack([3 * x - w + 0.5, 3 * y - h + 0.25]).astype(np.float32)


def scene_left(h, w):
    """(f) windows leaving the map on the left, partly and wholly; x = -0.25 where floor differs from truncation"""
    y, x = _grid(h, w)
    return np.stack([x - (w // 2) - 0.25, y + 0.5]).astype(np.float32)


def scene_right(h, w):
    """(f) ... on the right; x = w - 0.25 at pixel column w / 2"""
    y, x = _grid(h, w)
    return np.stack([x + (w // 2) - 0.25, y + 0.25]).astype(np.float32)


def scene_up(h, w):
    """(f) ... above: exact integers, y = -3.0 exactly at row h / 2 and 0.0 three rows below"""
    y, x = _grid(h, w)
    return np.stack([x + 0.0, y - (h // 2) - 3.0]).astype(np.float32)


def scene_down(h, w):
    """(f) ... below"""
    y, x = _grid(h, w)
    return np.stack([x + 1.0, y + (h // 2) + 0.5]).astype(np.float32)


def scene_huge(h, w):
    """(g) finite coordinates of large magnitude (+-1e5, +-1e7: a diverged pose), uniform inside some blocks and mixed with
    each other and with ordinary values in others: every output is an exact zero"""
    y, x = _grid(h, w)
    c = np.zeros((2, h, w), np.float32)
    q = (y >= h // 2) * 2 + (x >= w // 2)
    for k, (vx, vy) in enumerate([(1.0e5, 1.0e5), (-1.0e5, 3.0), (2.0, -1.0e7), (1.0e7, -1.0e7)]):
        c[0][q == k], c[1][q == k] = vx, vy
    odd = ((x + y) % 2 == 1) & (y < 8) & (x >= 8)                   # one block row that mixes both signs pixel by pixel
    c[0][odd] = -c[0][odd]
    return c


def scene_mirror(h, w):
    """(h) a map-wide displacement: the last rows and columns look at the first and the reverse, at every level, so the
    cyclic shift of the displacement-major layout wraps in both directions"""
    y, x = _grid(h, w)
    return np.stack([(w - 1) - x + 0.25, (h - 1) - y + 0.5]).astype(np.float32)


def scene_random(h, w, seed=0):
    """uniformly random coordinates whose margin is half a map"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-w / 2, w + w / 2, (h, w)), rng.uniform(-h / 2, h + h / 2, (h, w))]).astype(np.float32)


BORDER_SCENES = {"left": scene_left, "right": scene_right, "up": scene_up, "down": scene_down}

# scene -> what box_plan must report for it: `need` = (level, branch) pairs reached by at least one (block, quadrant); `area0` =
# range that the whole-block box area of at least one block has at level 0; `mixed0` = a block with one quadrant on single
# pixels and three that fit; `handover` = (la, lb): one block falls back at level la and shares a box at level lb
OTF_SCENES = {
    "box320": (scene_box320, dict(need=[(0, SHARED)], area0=(320, 320))),
    "box336": (scene_box336, dict(need=[(0, QUADS), (1, SHARED)], area0=(321, 336), handover=(0, 1))),
    "one_quadrant": (scene_one_quadrant, dict(need=[(0, QUADS), (0, SINGLES)], mixed0=True)),
    "scatter": (scene_scatter, dict(need=[(0, SINGLES)])),
    "scatter_wide": (scene_scatter_wide, dict(need=[(0, SINGLES), (1, SINGLES), (2, SINGLES), (3, SINGLES)])),
    "scale3": (scene_scale3, dict(need=[(0, QUADS), (1, QUADS), (2, SHARED), (3, SHARED)], handover=(1, 2))),
    "left": (scene_left, dict(need=[(0, SHARED)])),
    "right": (scene_right, dict(need=[(0, SHARED)])),
    "up": (scene_up, dict(need=[(0, SHARED)])),
    "down": (scene_down, dict(need=[(0, SHARED)])),
    "huge": (scene_huge, dict(need=[(0, SHARED), (0, SINGLES)])),
}


def check_plan(name, h, w, num_levels=4):
    """assert that scene `name` reaches, on an h x w map, every branch it was written for; returns (branch, area)"""
    fn, want = OTF_SCENES[name]
    branch, area = box_plan(fn(h, w), h, w, num_levels)
    for l, br in want.get("need", []):
        if l < num_levels:
            assert (branch[:, :, l] == br).any(), f"{name} {h}x{w}: no block takes branch {br} at level {l}"
    if "area0" in want:
        lo, hi = want["area0"]
        assert ((area[:, :, 0] >= lo) & (area[:, :, 0] <= hi)).any(), f"{name} {h}x{w}: level-0 areas {np.unique(area[:, :, 0])}"
        if lo > BOX_CAP:      # the fall-back with all four quadrants fitting
            ok = (area[:, :, 0] >= lo) & (area[:, :, 0] <= hi) & (branch[:, :, 0] == QUADS).all(-1)
            assert ok.any(), f"{name} {h}x{w}: no block in {lo}..{hi} whose four quadrants fit"
    if want.get("mixed0"):    # one quadrant on single pixels, the other three fitting, in the same block
        b0 = branch[:, :, 0]
        assert (((b0 == SINGLES).sum(-1) == 1) & ((b0 == QUADS).sum(-1) == 3)).any(), f"{name} {h}x{w}: no mixed block"
    if "handover" in want and want["handover"][1] < num_levels:
        la, lb = want["handover"]     # the same block falls back at level la and shares a box at level lb
        assert ((branch[:, :, la] != SHARED).all(-1) & (branch[:, :, lb] == SHARED).all(-1)).any(), f"{name} {h}x{w}: no hand-over"
    return branch, area


def otf_scene_coords(h, w, names=None):
    """coordinates [S * E, 2, h, w] of the scenes (each repeated for the E = 4 edges of OTF_II / OTF_JJ), the tiled edge
    lists, and the scene names in order"""
    names = list(OTF_SCENES) if names is None else list(names)
    E = len(OTF_II)
    coords = np.concatenate([np.repeat(OTF_SCENES[n][0](h, w)[None], E, 0) for n in names])
    return coords, np.tile(OTF_II, len(names)), np.tile(OTF_JJ, len(names)), names


def dm_scene_coords(h, w):
    """one edge per scene for the displacement-major lookup: (f) x 4, (g), (h), random with a margin of half a map (twice)"""
    names = ["left", "right", "up", "down", "huge", "mirror", "random0", "random1"]
    fields = [scene_left(h, w), scene_right(h, w), scene_up(h, w), scene_down(h, w), scene_huge(h, w), scene_mirror(h, w),
              scene_random(h, w, 0), scene_random(h, w, 1)]
    return np.stack(fields), names


def dm_volumes(seed, N, h, w):
    """random fp16 levels [N, h, w, h>>l, w>>l] that also hold -0.0 and fp16 subnormals in WHOLE planes (so that all four
    taps of every in-map output are such values: the reference's accumulator starts at +0 and never yields -0) and isolated
    +-65504"""
    rng = np.random.default_rng(seed)
    levels = []
    y, x = _grid(h, w)
    k = (y * w + x).astype(np.int64)
    for l in range(4):
        hl, wl = h >> l, w >> l
        v = rng.standard_normal((N, h, w, hl, wl)).astype(np.float16)
        v[:, k % 5 == 1] = np.float16(-0.0)
        sub = (rng.integers(-6, 7, (N, h, w, hl, wl)) * 2.0 ** -24).astype(np.float16)      # subnormals, +-0 among them
        sub[sub == 0] = np.float16(-0.0)
        v[:, k % 5 == 3] = sub[:, k % 5 == 3]
        if hl >= 4 and wl >= 4:                                     # isolated: no window blends two of them into an overflow
            v[:, k % 7 == 0, 0, 0] = np.float16(65504.0)
            v[:, k % 7 == 2, hl - 1, wl - 1] = np.float16(-65504.0)
        levels.append(v)
    return levels


def dm_integer_scene(seed, N, h, w):
    """encoder-exact scene of the displacement-major lookup: integer volumes in [-4, 4], coordinates multiples of 1/4"""
    rng = np.random.default_rng(seed)
    levels = [rng.integers(-4, 5, (N, h, w, h >> l, w >> l)).astype(np.float16) for l in range(4)]
    coords = np.stack([rng.integers(-4 * 4, 4 * (w + 4), (N, h, w)), rng.integers(-4 * 4, 4 * (h + 4), (N, h, w))], 1) / 4.0
    return levels, coords.astype(np.float32)


def otf_integer_scene(seed, F_, h, w):
    """encoder-exact scene of the volume-free lookup: +-4 in about 16 of the 128 channels, coordinates multiples of 1/2 that
    stay near the identity (shared boxes) on edge 0 and scatter on the others; edges OTF_ENC_II -> OTF_ENC_JJ (no ii == jj:
    a pixel's correlation with itself is the number of its non-zero channels, four times the other values)"""
    rng = np.random.default_rng(seed)
    fm = order_free_features(seed, F_, h, w, values=(-4, 4), density=0.125)
    y, x = _grid(h, w)
    E = len(OTF_II)
    coords = np.stack([rng.integers(-2 * 3, 2 * (w + 3), (E, h, w)), rng.integers(-2 * 3, 2 * (h + 3), (E, h, w))], 1) / 2.0
    coords[0] = np.stack([x + 1.5, y - 0.5])
    return fm, coords.astype(np.float32)


# ---- alt-corr ---------------------------------------------------------------------------------------------------------------
def altcorr_f64(fmap1, fmap2, coords, radius):
    """the oracle's loop nest (oracle.corr.altcorr_forward) in float64 throughout: fmap1 [B,H,W,C], fmap2 [B,H2,W2,C],
    coords [B,S,H,W,2] -> [B,S,(2r+1)^2,H,W] float64"""
    f1a = np.asarray(fmap1, np.float32).astype(F64)
    f2a = np.asarray(fmap2, np.float32).astype(F64)
    coords = np.asarray(coords, np.float32)
    B, H, W, C = f1a.shape
    _, H2, W2, _ = f2a.shape
    S = coords.shape[1]
    rd = 2 * radius + 1
    out = np.zeros((B, S, rd * rd, H, W), F64)
    x, y = coords[..., 0], coords[..., 1]
    fx, fy = np.floor(x), np.floor(y)
    dx, dy = (x - fx).astype(F64), (y - fy).astype(F64)
    bidx = np.arange(B)[:, None, None, None]
    for c0 in range(0, C, 32):
        f1 = f1a[..., c0:c0 + 32][:, None]
        for iy in range(rd + 1):
            for ix in range(rd + 1):
                h2 = fy.astype(np.int64) - radius + iy
                w2 = fx.astype(np.int64) - radius + ix
                inb = (h2 >= 0) & (h2 < H2) & (w2 >= 0) & (w2 < W2)
                f2 = f2a[bidx, np.clip(h2, 0, H2 - 1), np.clip(w2, 0, W2 - 1)][..., c0:c0 + 32]
                s = np.where(inb, (f1 * f2).sum(-1), 0.0)
                if iy > 0 and ix > 0:
                    out[:, :, (iy - 1) + rd * (ix - 1)] += s * (dy * dx)
                if iy > 0 and ix < rd:
                    out[:, :, (iy - 1) + rd * ix] += s * (dy * (1 - dx))
                if iy < rd and ix > 0:
                    out[:, :, iy + rd * (ix - 1)] += s * ((1 - dy) * dx)
                if iy < rd and ix < rd:
                    out[:, :, iy + rd * ix] += s * ((1 - dy) * (1 - dx))
    return out


def _lsb_exp(x, limit=40):
    """smallest k with x * 2^k integer"""
    k = 0
    while not _is_int(np.asarray(x, F64) * 2.0 ** k):
        k += 1
        assert k <= limit
    return k


def altcorr_exact_bound(fmap1, fmap2, coords):
    """proof that glorie_altcorr_fwd is order-free on this scene: features multiples of 2^-a / 2^-b, bilinear weights
    multiples of 2^-c (products of two fractions); every partial channel sum is bounded by S = max sum_c |f1 f2| over ALL
    pixel pairs, and so is every partial output (the four weights are non-negative and sum to 1), all of them multiples of
    2^-(a+b+c): with S 2^(a+b+c) < 2^24 every fp32 product, FMA and sum is exact, contracted or not.
    Returns the bound / 2^24."""
    f1 = np.asarray(fmap1, np.float32).astype(F64)
    f2 = np.asarray(fmap2, np.float32).astype(F64)
    c = np.asarray(coords, np.float32).astype(F64)
    a, b = _lsb_exp(f1), _lsb_exp(f2)
    frac = c - np.floor(c)
    cw = 2 * _lsb_exp(frac)
    B, C = f1.shape[0], f1.shape[-1]
    S = max((np.abs(f1[n]).reshape(-1, C) @ np.abs(f2[n]).reshape(-1, C).T).max() for n in range(B))
    bound = S * 2.0 ** (a + b + cw)
    assert bound < 2.0 ** 24, f"alt-corr scene is not exact: lsb 2^-{a + b + cw}, bound {bound / 2.0 ** 24:.3g} * 2^24"
    return bound / 2.0 ** 24


def altcorr_integer_scene(seed, B, S, H, W, H2, W2, C, fscale=1.0, amp=2, kind="random", density=1.0):
    """integer features (times fscale, a power of two) and quarter coordinates: `kind` random (margin 4 around the target
    map), a border scene of (f) on the TARGET map, or the huge coordinates of (g)"""
    rng = np.random.default_rng(seed)
    f1 = rng.integers(-amp, amp + 1, (B, H, W, C)).astype(np.float32)
    f2 = (rng.integers(-amp, amp + 1, (B, H2, W2, C)) * fscale).astype(np.float32)
    if density < 1.0:
        f1 *= rng.random(f1.shape) < density
        f2 *= rng.random(f2.shape) < density
    if kind == "random":
        c = np.stack([rng.integers(-16, 4 * (W2 + 4), (B, S, H, W)), rng.integers(-16, 4 * (H2 + 4), (B, S, H, W))], -1) / 4.0
    elif kind == "huge":
        c = np.broadcast_to(scene_huge(H, W).transpose(1, 2, 0)[None, None], (B, S, H, W, 2)).copy()
    else:       # a border scene, scaled from the source map onto the target map
        f = BORDER_SCENES[kind](H, W).transpose(1, 2, 0) * np.array([W2 / W, H2 / H], np.float32)
        c = np.broadcast_to((np.round(f * 4) / 4)[None, None], (B, S, H, W, 2)).copy()
        c += (np.arange(S, dtype=np.float32) * 0.75)[None, :, None, None, None]
    return f1, f2, c.astype(np.float32)


def altcorr_block_f64(fmaps, coords, ii, jj, num_levels=4, radius=3):
    """AltCorrBlock in float64: fmaps [F, C, H, W] (one batch), coords [N, H, W, S, 2], edges ii -> jj; the pyramid is
    avg_pool2d of fmaps / 4, level l is looked up at coords / 2^l.  Returns [N, L * 49, H, W, S] float64 and the per-level
    (f1, f2, coords) inputs for `altcorr_exact_bound`."""
    f = np.asarray(fmaps, np.float32).astype(F64) / 4.0
    coords = np.asarray(coords, np.float32)
    outs, inputs = [], []
    f1 = f[list(ii)].transpose(0, 2, 3, 1)
    for l in range(num_levels):
        f2 = f[list(jj)].transpose(0, 2, 3, 1)
        c = (coords / np.float32(2 ** l)).transpose(0, 3, 1, 2, 4)          # [N, S, H, W, 2]
        o = altcorr_f64(f1, f2, c, radius)                                    # [N, S, 49, H, W]
        outs.append(o.transpose(0, 2, 3, 4, 1))
        inputs.append((f1, f2, c))
        h2, w2 = f.shape[2] // 2, f.shape[3] // 2
        e = f[..., :2 * h2, :2 * w2]
        f = (e[..., 0::2, 0::2] + e[..., 0::2, 1::2] + e[..., 1::2, 0::2] + e[..., 1::2, 1::2]) / 4.0
    return np.concatenate(outs, 1), inputs


# (radius, C, S, (H, W), (H2, W2), kind): radius 3 with C % 4 == 0 runs altcorr_r3_kernel (channel tails: 40 = 32 + 8, 4),
# everything else altcorr_generic_kernel; H * W below, at and above the 64 pixels of a workgroup; targets down to 1 x 1
ALT_CASES = [
    (3, 128, 1, (9, 13), (9, 13), "random"), (3, 128, 3, (8, 8), (4, 4), "random"), (3, 40, 3, (9, 13), (4, 6), "left"),
    (3, 40, 1, (5, 7), (2, 3), "up"), (3, 4, 3, (5, 7), (1, 1), "random"), (3, 4, 1, (8, 8), (8, 8), "right"),
    (3, 128, 1, (9, 13), (1, 1), "down"), (3, 40, 3, (8, 8), (2, 2), "huge"), (3, 128, 3, (5, 7), (5, 7), "huge"),
    (2, 128, 3, (9, 13), (4, 6), "random"), (4, 32, 1, (8, 8), (8, 8), "random"), (3, 6, 3, (5, 7), (2, 3), "left"),
    (1, 130, 1, (9, 13), (1, 1), "random"), (2, 128, 1, (5, 7), (5, 7), "huge"), (4, 32, 3, (9, 13), (9, 13), "down"),
    (3, 6, 1, (8, 8), (1, 1), "up"), (1, 130, 3, (8, 8), (4, 4), "right"),
]


def altcorr_case(case, seed=0):
    radius, C, S, (H, W), (H2, W2), kind = case
    return altcorr_integer_scene(seed, 2, S, H, W, H2, W2, C, kind=kind)


def altcorr_block_scene(seed, h, w, S, integer_coords=False):
    """AltCorrBlock scene: 3 frames of +-4 in about 16 of 128 channels (order-free for OtfCorrBlock too), the 4 edges of
    OTF_II / OTF_JJ, coordinates [N, h, w, S, 2] multiples of 1/4 (or integers) within 3 px of the map"""
    rng = np.random.default_rng(seed)
    fm = order_free_features(seed, 3, h, w, values=(-4, 4), density=0.125)
    step = 1 if integer_coords else 4
    E = len(OTF_II)
    c = np.stack([rng.integers(-3 * step, step * (w + 3), (E, h, w, S)), rng.integers(-3 * step, step * (h + 3), (E, h, w, S))], -1)
    return fm, (c / float(step)).astype(np.float32)
