"""float64 restatement of the mapper's colour-gradient radii and gradient-ranked pixel draw (reference:
src/mapper.py:767-784, src/utils/common.py:96-118), the oracle of glorie_slam_amd/color_grad.py.

Gray is rgb . [0.2125, 0.7154, 0.0721]; the Sobel responses are [1,0,-1] x [1,2,1]/4 with the border pixel repeated
(scipy's mode='reflect' for a one-pixel reach); the radius maps interpolate the magnitude clipped to [0, float32(thr)]
(numpy clips a float32 map at the float32 threshold) between the nodes [0, 0.01, thr].  The top-M rule is the stable
order by (-key, index): equal keys at the boundary go to the lowest indices."""
import numpy as np


def gray(image):
    """[H,W,3] or [3,H,W] -> [H,W] float64"""
    im = np.asarray(image, dtype=np.float64)
    if im.shape[-1] != 3:
        im = np.moveaxis(im, 0, -1)
    return im @ np.array([0.2125, 0.7154, 0.0721])


def sobel_magnitude(image):
    g = np.pad(gray(image), 1, mode="edge")
    s = lambda a: (a[..., :-2] + 2 * a[..., 1:-1] + a[..., 2:]) / 4
    gy = s(g[2:, :]) - s(g[:-2, :])
    gx = (s(g[:, 2:].T) - s(g[:, :-2].T)).T
    return np.sqrt(gx ** 2 + gy ** 2)


def radius_map(mag, rmax, rmin, thr):
    x = np.clip(mag, 0.0, float(np.float32(thr)))
    return np.where(x <= 0.01, rmax, rmax + (rmin - rmax) / (thr - 0.01) * (x - 0.01))


def color_grad_maps_ref(image, color_grad_threshold=0.15, radius_add_max=0.08, radius_add_min=0.02,
                        radius_query_ratio=2.0, valid=None, depth_add=None, depth_query=None):
    """-> dict(grad, r_add, r_query) float64 [H,W], as glorie_color_grad_maps"""
    mag = sobel_magnitude(image)
    grad = mag.copy()
    if valid is not None:
        grad[~np.asarray(valid, dtype=bool)] = -1.0
    r_add = radius_map(mag, radius_add_max, radius_add_min, color_grad_threshold)
    r_query = radius_map(mag, radius_query_ratio * radius_add_max, radius_query_ratio * radius_add_min,
                         color_grad_threshold)
    if depth_add is not None:
        r_add = r_add / 3.0 * np.asarray(depth_add, dtype=np.float64)
    if depth_query is not None:
        r_query = r_query / 3.0 * np.asarray(depth_query, dtype=np.float64)
    return dict(grad=grad, r_add=r_add, r_query=r_query)


def top_indices_ref(keys, M):
    """the M largest keys' linear indices in ascending order (ties: lowest index first), and how many are >= 0"""
    k = np.asarray(keys).reshape(-1)
    if M > k.size:
        raise ValueError("M > n")
    order = np.lexsort((np.arange(k.size), -k.astype(np.float64)))[:M]
    sel = np.sort(order)
    return sel.astype(np.int64), int((k[sel] >= 0).sum())
