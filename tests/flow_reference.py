"""The dense Lucas-Kanade estimator of t2v_optical_flow (include/t2v.h) restated in torch on the CPU, in float64 or
float32, and the analytic image pairs its tests run on.  tests/test_cpu_optical_flow_ref.py checks the definition itself
(endpoint error and warp residual on known motions); tests/test_gpu_optical_flow.py checks the HIP kernels against it.

Convention: the flow lives on the current frame's grid and points into the previous frame, cur(x, y) ~ prev(x + u, y + v),
in pixels -- what ops.flow_warp / upstream's resample take."""
import math

import torch
import torch.nn.functional as F


def default_levels(h, w):
    """Pyramid levels of the default rule: halve (ceil) while the next level keeps min(h, w) >= 16, six at the most."""
    n = 1
    while n < 6 and min((h + 1) // 2, (w + 1) // 2) >= 16:
        h, w, n = (h + 1) // 2, (w + 1) // 2, n + 1
    return n


def _pool(x):
    return F.avg_pool2d(x[None, None], 3, 2, 1, count_include_pad=False)[0, 0]


def _smooth(x):
    """3x3 mean over the taps inside the image"""
    return F.avg_pool2d(x[None, None], 3, 1, 1, count_include_pad=False)[0, 0]


def _box(x, r):
    """window SUM over (2r+1)^2, zeros outside the image"""
    return F.avg_pool2d(x[None, None], 2 * r + 1, 1, r, divisor_override=1)[0, 0]


def bilinear(img, px, py):
    """img [h,w] at positions (px, py) (any shape), each clamped into the image first"""
    h, w = img.shape
    px = px.clamp(0, w - 1)
    py = py.clamp(0, h - 1)
    x0f, y0f = px.floor(), py.floor()
    fx, fy = px - x0f, py - y0f
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    top = (1 - fx) * img[y0, x0] + fx * img[y0, x1]
    bot = (1 - fx) * img[y1, x0] + fx * img[y1, x1]
    return (1 - fy) * top + fy * bot


def _grid(h, w, dtype):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
    return xs, ys


def warp(img, u, v):
    """img(x + u, y + v), bilinear, positions clamped into the image"""
    xs, ys = _grid(img.shape[0], img.shape[1], img.dtype)
    return bilinear(img, xs + u, ys + v)


def grey(img3):
    """[H,W,3] -> [H,W]: (R + G + B) / 3"""
    return (img3[..., 0] + img3[..., 1] + img3[..., 2]) / 3


def lk_flow(cur, prev, levels=None, iters=3, radius=3, lam=1e-3, dtype=torch.float64):
    """cur, prev: grey images [H,W].  -> (u, v), each [H,W] of `dtype`."""
    cur, prev = cur.to(dtype), prev.to(dtype)
    h, w = cur.shape
    levels = levels or default_levels(h, w)
    pyr = [(cur, prev)]
    for _ in range(levels - 1):
        pyr.append((_pool(pyr[-1][0]), _pool(pyr[-1][1])))
    n = float((2 * radius + 1) ** 2)
    u = v = None
    for c, p in reversed(pyr):
        hl, wl = c.shape
        if u is None:
            u, v = torch.zeros_like(c), torch.zeros_like(c)
        else:
            xs, ys = _grid(hl, wl, dtype)
            u, v = 2 * bilinear(u, xs / 2, ys / 2), 2 * bilinear(v, xs / 2, ys / 2)
        cx = F.pad(c[None, None], (1, 1, 1, 1), mode="replicate")[0, 0]
        gx = 0.5 * (cx[1:-1, 2:] - cx[1:-1, :-2])
        gy = 0.5 * (cx[2:, 1:-1] - cx[:-2, 1:-1])
        sxx = _box(gx * gx, radius) + lam * n
        syy = _box(gy * gy, radius) + lam * n
        sxy = _box(gx * gy, radius)
        det = sxx * syy - sxy * sxy
        for _ in range(iters):
            it = warp(p, u, v) - c
            bx, by = -_box(gx * it, radius), -_box(gy * it, radius)
            du = (syy * bx - sxy * by) / det
            dv = (sxx * by - sxy * bx) / det
            m = torch.sqrt(du * du + dv * dv).clamp(min=1.0)
            u, v = _smooth(u + du / m), _smooth(v + dv / m)
    return u, v


# ---------------------------------------------------------------------------------------------------------------------
# analytic image pairs: f(x, y) = tanh(sum_i a_i sin(k_i . (x, y) + phi_i) / sqrt(24)); cur = f, prev(p) = f(T^-1 p) for an
# affine T about the image centre, so the true flow T(x) - x is exact and no interpolation is involved
# ---------------------------------------------------------------------------------------------------------------------
N_WAVES = 24


def texture(seed=3):
    g = torch.Generator().manual_seed(seed)
    k = (torch.rand(N_WAVES, 2, generator=g, dtype=torch.float64) * 2 - 1) * 0.06 * 2 * math.pi
    a = torch.rand(N_WAVES, generator=g, dtype=torch.float64) + 0.5
    phi = torch.rand(N_WAVES, generator=g, dtype=torch.float64) * 2 * math.pi
    return k, a, phi


def _f(tex, x, y):
    k, a, phi = tex
    s = (a * torch.sin(x[..., None] * k[:, 0] + y[..., None] * k[:, 1] + phi)).sum(-1)
    return torch.tanh(s / math.sqrt(N_WAVES))


def affine_pair(h, w, angle=0.0, zoom=1.0, shift=(0.0, 0.0), seed=3):
    """-> (cur, prev, u_true, v_true), float64 [h,w].  T(x) = zoom * R(angle) (x - c) + c + shift."""
    tex = texture(seed)
    xs, ys = _grid(h, w, torch.float64)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    ca, sa = zoom * math.cos(angle), zoom * math.sin(angle)
    tx = ca * (xs - cx) - sa * (ys - cy) + cx + shift[0]
    ty = sa * (xs - cx) + ca * (ys - cy) + cy + shift[1]
    # T^-1 p
    det = ca * ca + sa * sa
    qx, qy = xs - cx - shift[0], ys - cy - shift[1]
    ix = (ca * qx + sa * qy) / det + cx
    iy = (-sa * qx + ca * qy) / det + cy
    return _f(tex, xs, ys), _f(tex, ix, iy), tx - xs, ty - ys


# name -> (image pair arguments, estimator arguments)
CASES = {
    "A": (dict(h=64, w=96, shift=(1.5, -2.25)), dict()),
    "B": (dict(h=85, w=64, angle=0.02, zoom=1.01, shift=(0.75, 0.5)), dict()),     # pyramid 85 -> 43 -> 22: odd sizes
    "C": (dict(h=48, w=40, shift=(-1.25, 0.75)), dict(iters=2, radius=2)),
}
# geometries at the edges of what the kernel accepts (compared with the restatement only: the functional bounds below were
# set for A, B and C): the smallest frame with the largest window (window wider than the frame, one level, one block), the
# largest window on more than one block and level (the LDS staging at its full extent), the smallest window on one level
EDGE_CASES = {
    "min_frame_r7": (dict(h=8, w=8, shift=(0.5, -0.25)), dict(radius=7, iters=2)),
    "r7_blocks": (dict(h=37, w=70, shift=(-0.75, 1.0)), dict(radius=7, iters=1, levels=2)),
    "r1_one_level": (dict(h=19, w=41, angle=0.03, shift=(0.25, 0.5)), dict(radius=1, levels=1)),
}
BORDER = 8
MAX_EPE = 0.25            # mean endpoint error, pixels, border removed
MAX_RESIDUAL_RATIO = 0.05  # mean |warp(prev, flow) - cur| over mean |prev - cur|, border removed

_memo = {}


def case(name):
    """-> dict(cur, prev, u_true, v_true, kw, u64, v64): the pair and the float64 estimate, computed once per process"""
    if name not in _memo:
        pair_kw, kw = CASES[name] if name in CASES else EDGE_CASES[name]
        cur, prev, ut, vt = affine_pair(**pair_kw)
        u, v = lk_flow(cur, prev, dtype=torch.float64, **kw)
        _memo[name] = dict(cur=cur, prev=prev, u_true=ut, v_true=vt, kw=kw, u64=u, v64=v)
    return _memo[name]


def functional_figures(c, u, v):
    """-> (mean endpoint error, residual ratio) of a flow (u, v) for case dict c, border removed"""
    u, v = u.double(), v.double()
    b = BORDER
    epe = torch.sqrt((u - c["u_true"]) ** 2 + (v - c["v_true"]) ** 2)[b:-b, b:-b].mean().item()
    res = (warp(c["prev"], u, v) - c["cur"]).abs()[b:-b, b:-b].mean().item()
    base = (c["prev"] - c["cur"]).abs()[b:-b, b:-b].mean().item()
    return epe, res / base


def rgb(img):
    """[H,W] float64 -> fp32 [H,W,3] whose channels differ and whose grey image is img (to fp32 rounding)"""
    return torch.stack([img, 0.8 * img, 1.2 * img], -1).float()


_memo_rgb = {}


def case_rgb(name):
    """What the kernel tests compare with: case(name) plus the fp32 three-channel frames the kernel is given (cur3, prev3),
    the float64 restatement on exactly those frames (u64, v64 replaced), the float32 restatement (u32, v32) and e32 = its
    maximum error against float64, in pixels.  Computed once per process; callers leave it unchanged."""
    if name not in _memo_rgb:
        c = dict(case(name))
        c["cur3"], c["prev3"] = rgb(c["cur"]), rgb(c["prev"])
        c["u64"], c["v64"] = lk_flow(grey(c["cur3"].double()), grey(c["prev3"].double()), dtype=torch.float64, **c["kw"])
        c["u32"], c["v32"] = lk_flow(grey(c["cur3"]), grey(c["prev3"]), dtype=torch.float32, **c["kw"])
        c["e32"] = max((c["u32"].double() - c["u64"]).abs().max().item(), (c["v32"].double() - c["v64"]).abs().max().item())
        _memo_rgb[name] = c
    return _memo_rgb[name]
