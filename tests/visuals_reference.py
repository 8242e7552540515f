"""The definition ops.train_visuals (t2v_train_visuals_u8, include/t2v.h) is held to, in numpy: IMAGE and UNIT bytes in the
fp32 operation order of the kernel (they must be equal), FLOW bytes in float64 (equal wherever the value before rounding
is not within FRAGILE_EPS of a rounding boundary k + 0.5 -- the `fragile` mask --, +-1 there: atan2 and the other float64
operations of two correct libraries differ by ~1e-13 of that value), and the integer block mean of --display_scale.
Shared by tests/test_cpu_train_display.py and tests/test_gpu_train_display.py."""
import numpy as np

IMAGE, UNIT, FLOW = 0, 1, 2
FRAGILE_EPS = 1e-6


def image_bytes(x):
    """x [H,W,>=3] fp32 -> (uint8 [H,W,3], fragile = all False): util.tensor2im in fp32, truncating cast"""
    x = np.asarray(x, np.float32)[..., :3]
    v = (x + np.float32(1.0)) / np.float32(2.0) * np.float32(255.0)
    assert v.dtype == np.float32
    return np.clip(v, np.float32(0.0), np.float32(255.0)).astype(np.uint8), np.zeros(v.shape, bool)


def unit_bytes(x):
    """x [H,W] fp32 -> (uint8 [H,W,3], fragile = all False): x * 255 clipped in fp32, truncated, NaN -> 0, grey"""
    x = np.asarray(x, np.float32)
    v = x * np.float32(255.0)
    v = np.where(np.isnan(v), np.float32(0.0), np.clip(v, np.float32(0.0), np.float32(255.0))).astype(np.float32)
    b = v.astype(np.uint8)
    return np.repeat(b[..., None], 3, -1), np.zeros(b.shape + (3,), bool)


def flow_bytes(uv):
    """uv [H,W,>=2] fp32 (u, v in pixels) -> (uint8 [H,W,3], fragile [H,W,3]): HSV, S = 1, hue = direction, value = the
    magnitude normalised between its min and max over the panel's finite pixels; float64 from the fp32 inputs"""
    uv = np.asarray(uv, np.float32)
    u, v = uv[..., 0].astype(np.float64), uv[..., 1].astype(np.float64)
    finite = np.isfinite(u) & np.isfinite(v)
    with np.errstate(all="ignore"):
        m = np.sqrt(u * u + v * v)
        lo, hi = (m[finite].min(), m[finite].max()) if finite.any() else (np.inf, -np.inf)
        if hi > lo:
            V = np.where(finite, (m - lo) / (hi - lo), 0.0)
        else:
            V = np.zeros_like(m)
        a = np.arctan2(np.where(finite, v, 0.0), np.where(finite, u, 0.0))
        a = np.where(a < 0.0, a + 2.0 * np.pi, a)
        h6 = 3.0 * a / np.pi
        fl = np.floor(h6)
        f = h6 - fl
        i = fl.astype(np.int64) % 6
        one, zero = np.ones_like(f), np.zeros_like(f)
        table = [(one, f, zero), (1.0 - f, one, zero), (zero, one, f), (zero, 1.0 - f, one), (f, zero, one), (one, zero, 1.0 - f)]
        rgb = np.zeros(f.shape + (3,))
        for sector, cols in enumerate(table):
            for c in range(3):
                rgb[..., c] = np.where(i == sector, cols[c], rgb[..., c])
        pre = (255.0 * V)[..., None] * rgb
    frac = pre - np.floor(pre)
    fragile = np.abs(frac - 0.5) <= FRAGILE_EPS
    return np.floor(pre + 0.5).astype(np.uint8), fragile


def downscale(b, fragile, s):
    """(uint8 [H,W,3], fragile) -> the same at 1/s: (sum of the s x s bytes + s*s/2) // (s*s); fragile where any source is"""
    if s == 1:
        return b, fragile
    H, W = b.shape[:2]
    assert H % s == 0 and W % s == 0
    blocks = b.reshape(H // s, s, W // s, s, 3).astype(np.int64).sum((1, 3))
    frag = fragile.reshape(H // s, s, W // s, s, 3).any((1, 3))
    return ((blocks + s * s // 2) // (s * s)).astype(np.uint8), frag


def render(panels, scale=1):
    """panels = [(kind, array [H,W,cs] or [H,W], c0)] -> (uint8 [n,H/s,W/s,3], fragile of the same shape)"""
    out, frag = [], []
    for kind, x, c0 in panels:
        x = np.asarray(x, np.float32)
        if x.ndim == 2:
            x = x[..., None]
        if kind == IMAGE:
            b, fr = image_bytes(x[..., c0:c0 + 3])
        elif kind == UNIT:
            b, fr = unit_bytes(x[..., c0])
        else:
            b, fr = flow_bytes(x[..., c0:c0 + 2])
        b, fr = downscale(b, fr, scale)
        out.append(b)
        frag.append(fr)
    return np.stack(out), np.stack(frag)


def make_panels(H, W, seed):
    """The 8 panels of the kernel test: IMAGE from cs 12 at c0 6 and from cs 4, UNIT from channel 2 of cs 4 and from cs 1,
    a small-range (<= 0.5 px) and a large-range (<= 40 px) FLOW panel, a constant FLOW panel, and a FLOW panel with zeros,
    one NaN and one Inf pixel.  IMAGE / UNIT values are finite and leave [-1,1] / [0,1]."""
    rng = np.random.default_rng(seed)
    f32 = np.float32

    def flow(max_mag, cs):
        ang = rng.uniform(0.0, 2.0 * np.pi, (H, W))
        mag = rng.uniform(0.0, max_mag, (H, W))
        x = rng.standard_normal((H, W, cs))
        x[..., 0], x[..., 1] = mag * np.cos(ang), mag * np.sin(ang)
        return x.astype(f32)

    img12 = rng.uniform(-1.3, 1.3, (H, W, 12)).astype(f32)
    img4 = rng.uniform(-1.3, 1.3, (H, W, 4)).astype(f32)
    unit4 = rng.uniform(-0.2, 1.2, (H, W, 4)).astype(f32)
    unit1 = rng.uniform(-0.2, 1.2, (H, W)).astype(f32)
    small, large = flow(0.5, 4), flow(40.0, 2)
    const = np.empty((H, W, 4), f32)
    const[...] = (1.5, -2.25, 0.3, 0.0)
    holes = flow(3.0, 4)
    holes[:2, :, :2] = 0.0
    holes[H // 2, W // 3, 0] = np.nan
    holes[H // 3, W // 2, 1] = np.inf
    return [(IMAGE, img12, 6), (IMAGE, img4, 0), (UNIT, unit4, 2), (UNIT, unit1, 0), (FLOW, small, 0), (FLOW, large, 0),
            (FLOW, const, 0), (FLOW, holes, 0)]
