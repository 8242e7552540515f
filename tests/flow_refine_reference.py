"""The refined estimator of t2v_optical_flow_refined (include/t2v_flow_refine.h) restated in torch on the CPU, in float64 or float32:
flow_reference.lk_flow with a Horn-Schunck Jacobi refinement after every level's LK iterations.  Also the image pairs with
a textureless region that the refinement is there for, and the geometry cases its kernel tests run on.
tests/test_cpu_optical_flow_refine_ref.py checks the definition; tests/test_gpu_optical_flow_refine.py checks the HIP kernels
against it."""
import torch
import torch.nn.functional as F

import flow_reference as fr

ALPHA = 0.2
REFINE_ITERS = 64


def _neighbour_mean(x):
    """(N + S + E + W) / 6 + (NE + NW + SE + SW) / 12, neighbour indices clamped to the image (replicate)"""
    p = F.pad(x[None, None], (1, 1, 1, 1), mode="replicate")[0, 0]
    plus = p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, 2:] + p[1:-1, :-2]
    diag = p[:-2, 2:] + p[:-2, :-2] + p[2:, 2:] + p[2:, :-2]
    return plus / 6 + diag / 12


def lkhs_flow(cur, prev, levels=None, iters=3, radius=3, lam=1e-3, alpha=ALPHA, refine_iters=REFINE_ITERS,
              dtype=torch.float64):
    """cur, prev: grey images [H,W].  -> (u, v), each [H,W] of `dtype`.  refine_iters = 0 is fr.lk_flow, statement for
    statement."""
    cur, prev = cur.to(dtype), prev.to(dtype)
    h, w = cur.shape
    levels = levels or fr.default_levels(h, w)
    pyr = [(cur, prev)]
    for _ in range(levels - 1):
        pyr.append((fr._pool(pyr[-1][0]), fr._pool(pyr[-1][1])))
    n = float((2 * radius + 1) ** 2)
    u = v = None
    for c, p in reversed(pyr):
        hl, wl = c.shape
        if u is None:
            u, v = torch.zeros_like(c), torch.zeros_like(c)
        else:
            xs, ys = fr._grid(hl, wl, dtype)
            u, v = 2 * fr.bilinear(u, xs / 2, ys / 2), 2 * fr.bilinear(v, xs / 2, ys / 2)
        cx = F.pad(c[None, None], (1, 1, 1, 1), mode="replicate")[0, 0]
        gx = 0.5 * (cx[1:-1, 2:] - cx[1:-1, :-2])
        gy = 0.5 * (cx[2:, 1:-1] - cx[:-2, 1:-1])
        sxx = fr._box(gx * gx, radius) + lam * n
        syy = fr._box(gy * gy, radius) + lam * n
        sxy = fr._box(gx * gy, radius)
        det = sxx * syy - sxy * sxy
        for _ in range(iters):
            it = fr.warp(p, u, v) - c
            bx, by = -fr._box(gx * it, radius), -fr._box(gy * it, radius)
            du = (syy * bx - sxy * by) / det
            dv = (sxx * by - sxy * bx) / det
            m = torch.sqrt(du * du + dv * dv).clamp(min=1.0)
            u, v = fr._smooth(u + du / m), fr._smooth(v + dv / m)
        if refine_iters:
            u0, v0 = u, v
            it0 = fr.warp(p, u0, v0) - c
            den = alpha * alpha + gx * gx + gy * gy
            for _ in range(refine_iters):
                ub, vb = _neighbour_mean(u), _neighbour_mean(v)
                t = (gx * (ub - u0) + gy * (vb - v0) + it0) / den
                u, v = ub - gx * t, vb - gy * t
    return u, v


# ---------------------------------------------------------------------------------------------------------------------
# disc pairs: the texture of flow_reference with a flat disc cut out of it, field and disc moving together, so the true flow
# is the shift everywhere and the disc's inside has no gradient to estimate it from
# ---------------------------------------------------------------------------------------------------------------------
def disc_pair(h, w, rho, shift, seed=3):
    """-> (cur, prev, u_true, v_true, inner), float64 [h,w]; inner = the mask r < rho - 2 on cur's grid"""
    tex = fr.texture(seed)
    xs, ys = fr._grid(h, w, torch.float64)
    cx, cy = (w - 1) / 2, (h - 1) / 2

    def obj(x, y):
        r = torch.sqrt((x - cx) ** 2 + (y - cy) ** 2)
        s = ((r - rho) / 4).clamp(0, 1)
        return fr._f(tex, x, y) * (s * s * (3 - 2 * s))
    r = torch.sqrt((xs - cx) ** 2 + (ys - cy) ** 2)
    return (obj(xs, ys), obj(xs - shift[0], ys - shift[1]), torch.full_like(xs, shift[0]), torch.full_like(xs, shift[1]),
            r < rho - 2)


DISC_CASES = {
    "D1": dict(h=96, w=128, rho=20, shift=(1.5, -2.25)),
    "D2": dict(h=128, w=128, rho=36, shift=(1.5, -2.25)),
}
MAX_INNER_RATIO = 0.4      # refined inner mean EPE over the LK one (float64: 0.195 on D1, 0.229 on D2)

# geometries of the refinement kernel (csrc/optical_flow_refine.hip: a 16 x 16 tile):
# name -> (image pair arguments, estimator arguments)
GEOMETRY_CASES = {
    "g8x8_l2": (dict(h=8, w=8, shift=(0.5, -0.25)), dict(levels=2)),                 # a 4 x 4 level: smaller than any tile
    "g37x70_l2": (dict(h=37, w=70, shift=(-0.75, 1.0)), dict(levels=2)),             # tiles over both edges, several blocks
    "g85x64": (dict(h=85, w=64, angle=0.02, zoom=1.01, shift=(0.75, 0.5)), dict()),  # 85 -> 43 -> 22: odd sizes
    "g19x41_l1": (dict(h=19, w=41, angle=0.03, shift=(0.25, 0.5)), dict(levels=1)),
}

_memo = {}


def pair(name):
    """-> dict(cur, prev, u_true, v_true, kw[, inner]) of a case of fr.CASES, DISC_CASES or GEOMETRY_CASES"""
    if name not in _memo:
        if name in DISC_CASES:
            cur, prev, ut, vt, inner = disc_pair(**DISC_CASES[name])
            _memo[name] = dict(cur=cur, prev=prev, u_true=ut, v_true=vt, kw={}, inner=inner)
        else:
            pair_kw, kw = fr.CASES[name] if name in fr.CASES else GEOMETRY_CASES[name]
            cur, prev, ut, vt = fr.affine_pair(**pair_kw)
            _memo[name] = dict(cur=cur, prev=prev, u_true=ut, v_true=vt, kw=kw)
    return _memo[name]


def inner_epe(c, u, v):
    """mean endpoint error over the inside of the disc"""
    e = torch.sqrt((u.double() - c["u_true"]) ** 2 + (v.double() - c["v_true"]) ** 2)
    return e[c["inner"]].mean().item()


_memo_flow = {}


def flows64(name, refine_iters=REFINE_ITERS):
    """float64 estimate on the float64 pair: (u, v) of lkhs_flow; refine_iters = 0: of fr.lk_flow.  Once per process."""
    key = (name, refine_iters)
    if key not in _memo_flow:
        c = pair(name)
        if refine_iters:
            _memo_flow[key] = lkhs_flow(c["cur"], c["prev"], refine_iters=refine_iters, **c["kw"])
        else:
            _memo_flow[key] = fr.lk_flow(c["cur"], c["prev"], **c["kw"])
    return _memo_flow[key]


_memo_rgb = {}


def case_rgb(name, refine_iters=REFINE_ITERS):
    """What the kernel tests compare with: pair(name) plus the fp32 three-channel frames the kernel is given (cur3, prev3),
    the float64 restatement on exactly those frames (u64, v64), the float32 one (u32, v32) and e32 = its maximum error
    against float64, in pixels.  Computed once per process; callers leave it unchanged."""
    key = (name, refine_iters)
    if key not in _memo_rgb:
        c = dict(pair(name))
        c["cur3"], c["prev3"] = fr.rgb(c["cur"]), fr.rgb(c["prev"])
        kw = dict(c["kw"], refine_iters=refine_iters)
        c["u64"], c["v64"] = lkhs_flow(fr.grey(c["cur3"].double()), fr.grey(c["prev3"].double()), dtype=torch.float64, **kw)
        c["u32"], c["v32"] = lkhs_flow(fr.grey(c["cur3"]), fr.grey(c["prev3"]), dtype=torch.float32, **kw)
        c["e32"] = max((c["u32"].double() - c["u64"]).abs().max().item(), (c["v32"].double() - c["v64"]).abs().max().item())
        _memo_rgb[key] = c
    return _memo_rgb[key]
