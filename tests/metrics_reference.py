"""float64 numpy statement of what t2v_image_metrics_u8 computes (include/t2v.h), written two independent ways, and the
seeded inputs the CPU and GPU tests share.

    SSIM (Wang, Bovik, Sheikh, Simoncelli 2004) per channel on the 8-bit values: window = outer product of
    g[i] = exp(-(i - 5)^2 / 4.5) normalised to sum 1; mx = sum w x, vx = sum w x^2 - mx^2, cxy = sum w x y - mx my;
    C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2; s = (2 mx my + C1)(2 cxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)),
    summed over the window positions that lie wholly inside the image and over the 3 channels.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

C1 = (0.01 * 255.0) ** 2
C2 = (0.03 * 255.0) ** 2
WIN = 11


def gaussian_window():
    g = np.exp(-(np.arange(WIN, dtype=np.float64) - 5.0) ** 2 / 4.5)
    return g / g.sum()


def _ssim_map(mx, my, exx, eyy, exy):
    vx, vy, cxy = exx - mx * mx, eyy - my * my, exy - mx * my
    return ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def ssim_direct(a, b):
    """(sum of s, number of positions x 3) with the 2-D window applied to every 11x11 patch; a, b: uint8 [H,W,>=3]"""
    H, W = a.shape[:2]
    if H < WIN or W < WIN:
        return 0.0, 0
    g = gaussian_window()
    w2 = np.outer(g, g)
    total = 0.0
    for ch in range(3):
        x = sliding_window_view(a[..., ch].astype(np.float64), (WIN, WIN))
        y = sliding_window_view(b[..., ch].astype(np.float64), (WIN, WIN))

        def m(v):
            return (v * w2).sum(axis=(2, 3))
        total += float(_ssim_map(m(x), m(y), m(x * x), m(y * y), m(x * y)).sum())
    return total, 3 * (H - WIN + 1) * (W - WIN + 1)


def ssim_separable(a, b):
    """the same sums with the window applied along rows, then along columns"""
    H, W = a.shape[:2]
    if H < WIN or W < WIN:
        return 0.0, 0
    g = gaussian_window()

    def blur(v):
        h = sum(g[j] * v[:, j:j + W - WIN + 1] for j in range(WIN))
        return sum(g[i] * h[i:i + H - WIN + 1] for i in range(WIN))
    total = 0.0
    for ch in range(3):
        x, y = a[..., ch].astype(np.float64), b[..., ch].astype(np.float64)
        total += float(_ssim_map(blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y)).sum())
    return total, 3 * (H - WIN + 1) * (W - WIN + 1)


def integer_sums(a, b):
    """(sse, sad) over channels 0..2, exact"""
    d = a[..., :3].astype(np.int64) - b[..., :3].astype(np.int64)
    return int((d * d).sum()), int(np.abs(d).sum())


def reference_row(a, b, box=None, ssim=ssim_separable):
    """{sse, sad, ssim_sum, ssim_n} of the pair cropped to box = (y0, y1, x0, x1), as floats"""
    if box is not None:
        a, b = a[box[0]:box[1], box[2]:box[3]], b[box[0]:box[1], box[2]:box[3]]
    sse, sad = integer_sums(a, b)
    s, n = ssim(a, b)
    return [float(sse), float(sad), s, float(n)]


def with_stride(img, cs, fill=77):
    """[H,W,3] -> [H,W,cs]; the pad channel holds bytes the kernel must not read into its sums"""
    if cs == 3:
        return np.array(img[..., :3])
    out = np.full(img.shape[:2] + (cs,), fill, np.uint8)
    out[..., :3] = img[..., :3]
    out[..., 3:] = (np.arange(img.shape[0] * img.shape[1]).reshape(img.shape[:2] + (1,)) * 37 + fill) % 256
    return out


def make_pair(kind, H, W, seed=0):
    """seeded uint8 [H,W,3] pairs.  noise: uniform bytes, b = clip(a + integers(-12, 13)).  smooth: a = clip(cumsum(
    integers(-3, 4), axis=1) + 128), b = clip(a + integers(-2, 3)) -- low variance, where float32 window sums fail.
    same: b == a."""
    rng = np.random.default_rng([seed, H, W, {"noise": 1, "smooth": 2, "same": 3}[kind]])
    if kind == "smooth":
        a = np.clip(np.cumsum(rng.integers(-3, 4, (H, W, 3)), axis=1) + 128, 0, 255)
        b = np.clip(a + rng.integers(-2, 3, (H, W, 3)), 0, 255)
    else:
        a = rng.integers(0, 256, (H, W, 3))
        b = a.copy() if kind == "same" else np.clip(a + rng.integers(-12, 13, (H, W, 3)), 0, 255)
    return a.astype(np.uint8), b.astype(np.uint8)
