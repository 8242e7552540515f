"""Float64 references, derived bounds, fp32 restatements and case tensors for the elementwise kernels of
text2video_amd/csrc/elementwise.hip: norm apply / join / add, the three norm-backward kernels, the flow-warp compositor and
its adjoint, the 3x3/s2 average pool, the pointwise activation backward and the masked-L1 / loss backward kernels.

A plain helper module (no fixtures, no hooks), shared by tests/test_cpu_elementwise_reference.py, which checks the references
against independent formulations, the bounds against injected faults and every case's buffers against extents(), and by
tests/test_gpu_elementwise_float64.py, which runs the kernels.  Per kernel:
  (a) a float64 reference taking the fp32 operands the kernel read;
  (b) an elementwise bound read off the kernel's arithmetic, the derivation next to the formula; gamma(n) counts every product
      and every sum as a rounding of its own, so it holds whether or not the compiler contracts a multiply-add (a contraction
      removes a rounding);
  (c) a restatement of the kernel's evaluation order in fp32 torch on the CPU (`*32`), with optional injected faults;
  (d) build_case(case, device): the exact tensors the GPU test passes;
  (e) extents(case): per argument, the number of floats the launcher and the kernel can index.
U, TINY, gamma(), sum_bound(), lazy_d64(), norm_pre64() and dy_front64() come from tests/kernel_variants.py."""
import collections
import math

import torch
import torch.nn.functional as F

import kernel_variants as kv
from kernel_variants import TINY, U, gamma, sum_bound

Case = collections.namedtuple("Case", "id kind p")
MARGIN = 64                      # floats of NaN on either side of an out= buffer (a multiple of 4: float4 stays aligned)
GRID_CAP = 2048 * 256            # grid_for(): at most 2048 blocks of 256 threads; past this a grid-stride loop iterates
LEAKY32 = kv.LEAKY32


def _c(id, kind, **p):
    return Case(id, kind, p)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id)) % 100003


def nan_margin(n, device):
    """a flat NaN buffer with MARGIN floats around n, and the view the kernel writes"""
    buf = torch.full((n + 2 * MARGIN,), float("nan"), dtype=torch.float32, device=device)
    return buf, buf[MARGIN:MARGIN + n]


def margins_untouched(buf):
    return bool(torch.isnan(buf[:MARGIN]).all() and torch.isnan(buf[-MARGIN:]).all())


def worst(err, bnd):
    """worst |error| / bound (a bound of exactly 0 admits an error of exactly 0 only)"""
    r = torch.where(bnd > 0, err / bnd.clamp(min=1e-300), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    return float(r.max())


def stats64(x):
    """(mean, rstd) [C, 2] of x [npix, C] in float64 (biased variance, eps 1e-5), rounded to fp32: the table the kernels read"""
    xd = x.double()
    m = xd.mean(0)
    v = ((xd - m) ** 2).mean(0)
    return torch.stack([m, 1.0 / torch.sqrt(v + 1e-5)], 1).float()


# ---- norm apply, join, add ------------------------------------------------------------------------------------------------
APPLY_CASES = [
    _c("apply_7x5_c4_relu0", "apply", H=7, W=5, C=4, relu=0, affine=False, nres=0, nimg=1, mean=0.0),
    _c("apply_7x5_c4_relu1", "apply", H=7, W=5, C=4, relu=1, affine=False, nres=0, nimg=1, mean=0.0),
    _c("apply_7x5_c4_relu2", "apply", H=7, W=5, C=4, relu=2, affine=False, nres=0, nimg=1, mean=0.0),
    _c("apply_11x13_c12_res2_relu2", "apply", H=11, W=13, C=12, relu=2, affine=True, nres=2, nimg=1, mean=0.0),
    _c("apply_9x7_c68_mean300", "apply", H=9, W=7, C=68, relu=0, affine=True, nres=1, nimg=1, mean=300.0),
    # n4 = 8200 * 64 = 524 800 float4: the last 512 are a second trip round the grid-stride loop
    _c("apply_82x100_c256_relu1", "apply", H=82, W=100, C=256, relu=1, affine=True, nres=1, nimg=1, mean=0.0),
    _c("apply_batch3_11x13_c12", "apply", H=11, W=13, C=12, relu=2, affine=True, nres=2, nimg=3, mean=0.0),
]
INPLACE_IDS = ("apply_11x13_c12_res2_relu2", "apply_82x100_c256_relu1")
JOIN_CASES = [
    _c("join_2x9x7_c64_a_affine", "join", H=9, W=7, C=64, nimg=2, affine=(True, False)),
    _c("join_2x9x7_c64_plain", "join", H=9, W=7, C=64, nimg=2, affine=(False, False)),
]


def _norm_side(g, nimg, npix, C, affine, mean, nres):
    x = torch.randn(nimg, npix, C, generator=g) * (1.0 + torch.rand(C, generator=g)) + mean + torch.randn(C, generator=g)
    mr = torch.stack([stats64(x[i]) for i in range(nimg)])
    ga = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0) if affine else None
    be = torch.randn(C, generator=g) if affine else None
    res = [torch.randn(nimg, npix, C, generator=g) for _ in range(nres)]
    return x, mr, ga, be, res


def apply64(x, mr, ga, be, relu, res1, res2):
    """[nimg, npix, C] images, each with its own table mr[i]: kv.lazy_d64 per image"""
    out = [kv.lazy_d64(x[i], mr[i], ga, be, relu, None if res1 is None else res1[i], None if res2 is None else res2[i])
           for i in range(x.shape[0])]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def join64(a, b):
    """(norm_a(ya) + ra) + (norm_b(yb) + rb): two lazy_d64 sums s_a, s_b with bounds e_a, e_b, then one more addition of the
    two computed values: |fl(sa~ + sb~) - (sa + sb)| <= e_a + e_b + u (|sa| + |sb| + e_a + e_b)"""
    sa, ea = apply64(a[0], a[1], a[2], a[3], 0, a[4], None)
    sb, eb = apply64(b[0], b[1], b[2], b[3], 0, b[4], None)
    return sa + sb, (ea + eb) * (1 + U) + U * (sa.abs() + sb.abs()) + TINY


def add64(a, b):
    """one correctly rounded addition"""
    s = a.double() + b.double()
    return s, U * s.abs() + TINY


def apply32(x, mr, ga, be, relu, res1, res2, fault=None):
    """inorm_apply_kernel's order in fp32: (x - mean) * rstd, * gamma + beta, activation, + res1, + res2.
    faults: 'table0' -- every image normalised with image 0's table; 'res2' -- res2 dropped"""
    outs = []
    for i in range(x.shape[0]):
        t = mr[0 if fault == "table0" else i]
        v = (x[i] - t[:, 0]) * t[:, 1]
        if ga is not None:
            v = v * ga + be
        if relu == 1:
            v = v.clamp(min=0)
        elif relu == 2:
            v = torch.where(v > 0, v, torch.tensor(LEAKY32, dtype=torch.float32) * v)
        if res1 is not None:
            v = v + res1[i]
        if res2 is not None and fault != "res2":
            v = v + res2[i]
        outs.append(v)
    return torch.stack(outs)


def join32(a, b):
    return apply32(a[0], a[1], a[2], a[3], 0, a[4], None) + apply32(b[0], b[1], b[2], b[3], 0, b[4], None)


# ---- norm backward ----------------------------------------------------------------------------------------------------------
_NB_SMALL = [(7, 5, 4), (12, 20, 12), (25, 40, 68), (25, 40, 132)]      # the C4 / 256 rounding; a last channel block not full
NORM_BWD_CASES = [_c("nbwd_%dx%d_c%d_relu%d_%s" % (H, W, C, relu, "affine" if aff else "plain"), "nbwd", H=H, W=W, C=C, relu=relu,
                     affine=aff) for (H, W, C) in _NB_SMALL for relu in (0, 1, 2) for aff in (False, True)] + [
    _c("nbwd_82x100_c64_relu1_affine", "nbwd", H=82, W=100, C=64, relu=1, affine=True),       # 129 slices wanted: the 128 cap
    _c("nbwd_41x100_c1024_relu2_plain", "nbwd", H=41, W=100, C=1024, relu=2, affine=False),   # 65 wanted: 1024 / ceil(C/64) = 64
]
PIN_CH = 1      # a channel whose every x is bit-equal to its mean (with beta == 0): pre == 0 exactly, the zero convention


def bwd_slices(npix, C):
    """launch_inorm_backward's pixel slices"""
    return max(1, min((npix + 63) // 64, 1024 // ((C + 63) // 64), 128))


def bwd_apply_blocks(npix, C, round_up=True):
    """launch_inorm_backward's block count for inorm_bwd_apply_kernel; round_up=False: without the lcm_blocks round-up"""
    C4 = C // 4
    threads = (npix * C4 + 7) // 8
    threads = (threads + C4 - 1) // C4 * C4
    blocks = (threads + 255) // 256
    if round_up and (blocks * 256) % C4 != 0:
        lcm = C4 // math.gcd(C4, 256)
        blocks = (blocks + lcm - 1) // lcm * lcm
    return blocks


def bwd_depth(npix, C):
    """the longest chain of additions a term of the per-channel sums meets: a thread's chain over its pixels
    (inorm_bwd_reduce_kernel: ceil(npix / (16 slices))), the block's 16 pixel lanes in turn (15; the first lands on 0),
    inorm_bwd_final_kernel's lane chain over ceil(slices / 4) partials, and its closing (a + b) + (c + d) (2)"""
    s = bwd_slices(npix, C)
    return -(-npix // (16 * s)) + 15 + -(-s // 4) + 2


def bwd_sums64(x, dy, mr, ga, be, relu):
    """S0 = sum g, S1 = sum g xhat per channel in float64, g = dy act'(gamma xhat + beta), and their bounds:
    sum_bound(sum |term|, bwd_depth) for the summation; the terms themselves: g is exact for relu 0 / 1 (a product by 1 or 0)
    and one rounding for the Leaky slope (float32(0.2) against 0.2 is 7.5e-9 relative, inside the u it is given: gamma(2));
    xhat has two roundings and g xhat one more (gamma(5) with the slope's two); inside dy_front64's `near` mask the kernel may
    take the other branch of the activation: + |dy| (1 - lo) there, times |xhat| for S1."""
    xh, pre, act, lo, near, r, g_ = kv.norm_pre64(x, mr, ga, be, relu)
    g = dy.double() * act
    npix, C = x.shape
    d = bwd_depth(npix, C)
    slack = near.double() * dy.double().abs() * (1.0 - lo)
    s0, s1 = g.sum(0), (g * xh).sum(0)
    a0, a1 = g.abs().sum(0), (g * xh).abs().sum(0)
    e0 = sum_bound(a0, d, npix) + gamma(2) * a0 + slack.sum(0)
    e1 = sum_bound(a1, d, npix) + gamma(5) * a1 + (slack * xh.abs()).sum(0) * (1 + gamma(3))
    return torch.stack([s0, s1], 1), torch.stack([e0, e1], 1)


def _bwd_terms32(x, dy, mr, ga, be, relu):
    xh = (x - mr[:, 0]) * mr[:, 1]
    g1 = ga if ga is not None else torch.ones(x.shape[1])
    b1 = be if be is not None else torch.zeros(x.shape[1])
    pre = g1 * xh + b1
    lo = torch.tensor(0.0 if relu == 1 else LEAKY32 if relu == 2 else 1.0, dtype=torch.float32)
    return xh, dy * torch.where(pre > 0, torch.tensor(1.0), lo)


def bwd_sums32(x, dy, mr, ga, be, relu, fault=None):
    """inorm_bwd_reduce_kernel + inorm_bwd_final_kernel in fp32, addition by addition.  fault 'tail': the pixels the 4-deep
    unrolled loop leaves to its tail loop are dropped"""
    npix, C = x.shape
    xh, g = _bwd_terms32(x, dy, mr, ga, be, relu)
    s = bwd_slices(npix, C)
    step = 16 * s
    iters = -(-npix // step)
    out = []
    for t in (g, g * xh):
        tp = torch.zeros(iters * step, C)
        tp[:npix] = t
        tp = tp.view(iters, s, 16, C)
        if fault == "tail":
            start = torch.arange(step).view(1, s, 16, 1)
            n_t = (npix - start + step - 1) // step                  # a thread's pixels
            it = torch.arange(iters).view(iters, 1, 1, 1)
            tp = tp * (it < 4 * (n_t // 4)).float()
        acc = torch.zeros(s, 16, C)
        for i in range(iters):
            acc = acc + tp[i]
        part = torch.zeros(s, C)
        for i in range(16):
            part = part + acc[:, i]
        k = -(-s // 4)
        pp = torch.zeros(k * 4, C)
        pp[:s] = part
        pp = pp.view(k, 4, C)
        lane = torch.zeros(4, C)
        for j in range(k):
            lane = lane + pp[j]
        out.append((lane[0] + lane[1]) + (lane[2] + lane[3]))
    return torch.stack(out, 1)


def bwd_dx32(x, dy, mr, ga, be, relu, sums, fault=None):
    """inorm_bwd_apply_kernel in fp32.  A thread forms its channel quad's terms once, from its FIRST index, and keeps them
    over the grid-stride loop: element i is computed with the quad of thread i % stride.  faults: 'stride' -- the block count
    without the launcher's lcm_blocks round-up, so the stride is no multiple of C4 and a thread's quad is off by
    stride % C4 after every trip; 'n-1' -- S1 / N taken with N - 1"""
    npix, C = x.shape
    C4 = C // 4
    stride = 256 * bwd_apply_blocks(npix, C, round_up=fault != "stride")
    i4 = torch.arange(npix * C4)
    quad = (i4 % stride) % C4
    ch = (quad[:, None] * 4 + torch.arange(4)).view(npix, C)           # the channel whose parameters element (p, c) is given
    invn = torch.tensor(1.0) / torch.tensor(float(npix))
    k0 = sums[:, 0] * invn
    k1 = sums[:, 1] * (torch.tensor(1.0) / torch.tensor(float(npix - 1)) if fault == "n-1" else invn)
    g1 = ga if ga is not None else torch.ones(C)
    b1 = be if be is not None else torch.zeros(C)
    m, r = mr[:, 0][ch], mr[:, 1][ch]
    xh = (x - m) * r
    pre = g1[ch] * xh + b1[ch]
    lo = torch.tensor(0.0 if relu == 1 else LEAKY32 if relu == 2 else 1.0, dtype=torch.float32)
    g = dy * torch.where(pre > 0, torch.tensor(1.0), lo)
    return r * g1[ch] * (g - k0[ch] - xh * k1[ch])


# ---- flow-warp compositor ---------------------------------------------------------------------------------------------------
# (prev_cs, prev_c0) cover {(3, 0), (4, 0), (6, 3), (8, 3), (12, 9)} across the small cases
WARP_CASES = [
    _c("warp_2x2", "warp", H=2, W=2, flow="inside2x2", std=0.0, cs=3, c0=0),
    _c("warp_2x37", "warp", H=2, W=37, flow="randn", std=3.0, cs=4, c0=0),
    _c("warp_37x2", "warp", H=37, W=2, flow="randn", std=3.0, cs=6, c0=3),
    _c("warp_17x23_std12", "warp", H=17, W=23, flow="randn", std=12.0, cs=8, c0=3),        # leaves the image
    _c("warp_64x64_zero", "warp", H=64, W=64, flow="zero", std=0.0, cs=12, c0=9),           # a kink on every pixel
    _c("warp_64x64_const", "warp", H=64, W=64, flow="const", std=0.0, cs=6, c0=3),          # flow exactly (3, -2)
    _c("warp_24x40_huge", "warp", H=24, W=40, flow="huge", std=2.0, cs=4, c0=0),            # +-1e6 in a few pixels
    _c("warp_19x21_edges", "warp", H=19, W=21, flow="edges", std=1.5, cs=8, c0=3),          # a row on W - 1, a column on H - 1
    _c("warp_513x1024", "warp", H=513, W=1024, flow="randn", std=4.0, cs=3, c0=0),          # 525 312 pixels: a second trip
]
K_POS = 4.0


def warp_pos64(fw):
    """The sampling position in float64 and the bound on the kernel's own.  In exact arithmetic warp_position() returns
    px = x + flow_x (the normalised grid and its un-normalisation cancel).  In fp32 it rounds seven times; in pixel units
    (one unit of the normalised grid is (W - 1) / 2 pixels, and sx = (W - 1) / 2 is exact):
      stepx = 2 / (W - 1) and stepx * x (or * (W - 1 - x)): two roundings of a value <= 1      -> 2 u (W - 1) / 2
      -1 + . (or 1 - .): |gx0| <= 1                                                            ->   u (W - 1) / 2
      flow / sx                                                                                ->   u |f|
      gx0 + .: <= 1 + |f| / sx                                                                 ->   u ((W - 1) / 2 + |f|)
      + 1: <= 2 + |f| / sx                                                                     ->   u ((W - 1) + |f|)
      / 2 exact, * (W - 1): <= (W - 1) + |f|                                                   ->   u ((W - 1) + |f|)
    together K_POS u ((W - 1) + |f|) with K_POS = 4, to first order; the factor (1 + 8 u) covers the products of the seven
    (1 + delta), 8 TINY a flushed intermediate.  A fused -1 + stepx * x removes one of the roundings."""
    H, W = fw.shape[:2]
    dev = fw.device
    fx, fy = fw[..., 0].double(), fw[..., 1].double()
    px = torch.arange(W, dtype=torch.float64, device=dev)[None, :] + fx
    py = torch.arange(H, dtype=torch.float64, device=dev)[:, None] + fy
    ex = K_POS * U * ((W - 1) + fx.abs()) * (1 + 8 * U) + 8 * TINY
    ey = K_POS * U * ((H - 1) + fy.abs()) * (1 + 8 * U) + 8 * TINY
    return px, py, ex, ey


def _cell(q, n):
    """the kernels' border rule on one axis: inside flag of the unclipped position, clamped position's cell i0, the clipped
    upper corner i1 = min(i0 + 1, n - 1) and the upper weight (0 outside the image and exactly on its last row / column)"""
    inside = (q >= 0) & (q <= n - 1)
    qc = q.clamp(0, n - 1)
    i0 = qc.floor()
    return inside, i0.long(), (i0 + 1).clamp(max=n - 1).long(), qc - i0


def _moved(p, e, n):
    """how far the clamped position can be from the reference's: min(e, length of [p - e, p + e] inside [0, n - 1])"""
    return torch.minimum(e, (p + e).clamp(0, n - 1) - (p - e).clamp(0, n - 1))


def _nbhd(M, y0, x0, r=2):
    """max of M [h, w, c] (>= 0) over rows y0 - r .. y0 + r, columns x0 - r .. x0 + r, gathered per pixel"""
    h, w = M.shape[:2]
    if h == 0 or w == 0:
        return torch.zeros(y0.shape + (M.shape[2],), dtype=M.dtype, device=M.device)
    P = F.max_pool2d(M.permute(2, 0, 1)[None], 2 * r + 1, 1, r)[0].permute(1, 2, 0)
    return P[y0.clamp(0, h - 1), x0.clamp(0, w - 1)]


def _taps(v, py, px, qx=None, qy=None):
    """corner values and weights of the cell holding (py, px); qx / qy: the cell (and inside flag) of another probe position
    on that axis, the weights still from (py, px)"""
    H, W = v.shape[:2]
    inx, x0, x1, wx1 = _cell(px if qx is None else qx, W)
    iny, y0, y1, wy1 = _cell(py if qy is None else qy, H)
    if qx is not None:
        wx1 = _cell(px, W)[3]
    if qy is not None:
        wy1 = _cell(py, H)[3]
    return (v[y0, x0], v[y0, x1], v[y1, x0], v[y1, x1]), (wx1, wy1), (inx, iny), (y0, y1, x0, x1)


def warp64(prev, c0, fw):
    """resample(prev[..., c0:c0+3], flow) written out at px = x + flow_x, py = y + flow_y in float64 (the CPU test holds it
    against oracle.generator_ref.resample in float64, which the GPU test compares with), and the bound of the kernel's value.
    The bilinear interpolant B is continuous, piecewise bilinear, constant outside the image on each axis.  The kernel
    evaluates it at its own position, up to _moved() away per axis: |B(p~) - B(p)| <= Lx dx + Ly dy with Lx, Ly the largest
    |difference of horizontal / vertical neighbours| over the cells within two of the reference's (dx, dy < 1 is asserted:
    the path from p to p~ stays inside that neighbourhood).  The tap sum: wx0 = 1 - wx1 (1 rounding; wx1 = px - floor(px) is
    exact), the weight product (2, with wy0: 3), the product with the tap (4), three additions (7), and the weights may sum to
    1 + 3 u: gamma(8) max|v| over the same neighbourhood."""
    v = prev[..., c0:c0 + 3].double()
    H, W = v.shape[:2]
    px, py, ex, ey = warp_pos64(fw)
    (v00, v10, v01, v11), (wx1, wy1), _, (y0, _, x0, _) = _taps(v, py, px)
    wx1, wy1 = wx1[..., None], wy1[..., None]
    warp = v00 * ((1 - wx1) * (1 - wy1)) + v10 * (wx1 * (1 - wy1)) + v01 * ((1 - wx1) * wy1) + v11 * (wx1 * wy1)
    dx, dy = _moved(px, ex, W), _moved(py, ey, H)
    assert float(dx.max()) < 0.5 and float(dy.max()) < 0.5, "the positional bound crosses more than one cell"
    Lx = _nbhd((v[:, 1:] - v[:, :-1]).abs(), y0, x0)
    Ly = _nbhd((v[1:] - v[:-1]).abs(), y0, x0)
    e = Lx * dx[..., None] + Ly * dy[..., None] + gamma(8) * _nbhd(v.abs(), y0, x0) + 8 * TINY
    return warp, e


def composite64(raw, fw, warp, e_warp):
    """out = raw w + warp (1 - w): raw w (1 rounding), 1 - w (1), its product with the warp (2, on top of the warp's own
    error), the sum (3): |1 - w| e_warp (1 + 3 u) + gamma(3) (|raw w| + |warp (1 - w)|)"""
    wt = fw[..., 2:3].double()
    r = raw[..., :3].double()
    out = r * wt + warp * (1 - wt)
    return out, (1 - wt).abs() * e_warp * (1 + 3 * U) + gamma(3) * ((r * wt).abs() + (warp * (1 - wt)).abs()) + 3 * TINY


def warp_backward64(d_out, d_warp, raw, fw, prev, c0):
    """The adjoint in float64.  Returns a dict:
      d_raw, e_raw       d_out w, one rounding
      d_w, e_w           sum_c d_out_c (raw_c - warp_c): the warp's own error (warp64), raw - warp (1), the product (2), three
                         additions (5): sum_c |d_out_c| e_warp_c (1 + 5 u) + gamma(5) sum_c |d_out_c| (|raw_c| + |warp_c|)
      d_fx, d_fy         LISTS of admissible values, e_fx, e_fy
      d_prev, e_prev
    Kink rule.  d B / d px is the slope of the cell the position falls in; it jumps where px crosses an integer, is 0 outside
    [0, W - 1] (the kernel's `inx`) and exactly on W - 1 (both corners clip to the same pixel).  A pixel whose float64 position
    is within the positional bound of such a point has two admissible one-sided derivatives.  The candidates are the slopes of
    the cells holding px - ex, px and px + ex (2 ex < 1: no other cell is within reach), each evaluated with the y weights of
    the reference position: d B / d px is continuous in py (also across rows, and where py is clamped), so the y side enters
    only through Lxy dy, Lxy the largest mixed second difference nearby.  d_flow_x therefore depends on the x side alone
    and d_flow_y on the y side alone: testing each against its own candidates is testing the up to four (x side, y side)
    combinations, and no pixel is left out.
    Roundings of d_flow_x: g_c = d_out_c (1 - w) + d_warp_c (3), v10 - v00 (1), wy0 (1) and their product (3), the bracket's
    sum (4), times g_c (8), three additions (11): sum_c G_c (gamma(11) max|slope| + Lxy dy), G_c = |d_out_c (1 - w)| + |d_warp_c|.
    d_prev: pixel -> tap weights are products of two hat functions of the position, 1-Lipschitz in each coordinate, so a
    contribution moves by at most G_c (dx + dy) on any tap within one of the reference's four, plus gamma(8) for its roundings
    (g_c 3, the weight 3, the product 1, and 1 to spare); the atomic accumulation is a sum in no fixed order:
    sum_bound(sum |contribution|, n) with n the number of contributions that can land on the tap (counted on the reference's
    taps and their neighbours)."""
    H, W = fw.shape[:2]
    dev = fw.device
    v = prev[..., c0:c0 + 3].double()
    zero = torch.zeros(H, W, 3, dtype=torch.float64, device=dev)
    go = d_out[..., :3].double() if d_out is not None else zero
    gw = d_warp[..., :3].double() if d_warp is not None else zero
    wt = fw[..., 2:3].double() if d_out is not None else torch.zeros(H, W, 1, dtype=torch.float64, device=dev)
    rw = raw[..., :3].double() if raw is not None else zero
    g = go * (1 - wt) + gw
    G = (go * (1 - wt)).abs() + gw.abs()
    px, py, ex, ey = warp_pos64(fw)
    dxm, dym = _moved(px, ex, W), _moved(py, ey, H)
    warp, e_warp = warp64(prev, c0, fw)
    res = {"d_raw": go * wt, "e_raw": U * (go * wt).abs() + TINY}
    res["d_w"] = (go * (rw - warp)).sum(-1)
    res["e_w"] = (go.abs() * e_warp).sum(-1) * (1 + 5 * U) + gamma(5) * (go.abs() * (rw.abs() + warp.abs())).sum(-1) + 5 * TINY
    (_, _, _, _), _, _, (y0, _, x0, _) = _taps(v, py, px)
    Dx, Dy = v[:, 1:] - v[:, :-1], v[1:] - v[:-1]
    Dxy = (Dx[1:] - Dx[:-1]).abs()
    Lxy = _nbhd(Dxy, y0, x0)
    fxs, fys = [], []
    for s in (-1.0, 0.0, 1.0):
        (a00, a10, a01, a11), (_, wy1), (inx, _), _ = _taps(v, py, px, qx=px + s * ex)
        wy1 = wy1[..., None]
        fxs.append((g * ((1 - wy1) * (a10 - a00) + wy1 * (a11 - a01))).sum(-1) * inx.double())
        (b00, b10, b01, b11), (wx1, _), (_, iny), _ = _taps(v, py, px, qy=py + s * ey)
        wx1 = wx1[..., None]
        fys.append((g * ((1 - wx1) * (b01 - b00) + wx1 * (b11 - b10))).sum(-1) * iny.double())
    res["d_fx"], res["d_fy"] = fxs, fys
    res["e_fx"] = (G * (gamma(11) * _nbhd(Dx.abs(), y0, x0) + Lxy * dym[..., None])).sum(-1) + 11 * TINY
    res["e_fy"] = (G * (gamma(11) * _nbhd(Dy.abs(), y0, x0) + Lxy * dxm[..., None])).sum(-1) + 11 * TINY
    # d_prev: scatter g_c w_tap onto the reference's four taps
    _, (wx1, wy1), _, (y0, y1, x0, x1) = _taps(v, py, px)
    wts = ((1 - wx1) * (1 - wy1), wx1 * (1 - wy1), (1 - wx1) * wy1, wx1 * wy1)
    idx = (y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1)
    dp = torch.zeros(H * W, 3, dtype=torch.float64, device=dev)
    ab = torch.zeros_like(dp)
    er = torch.zeros_like(dp)
    cnt = torch.zeros(H * W, 1, dtype=torch.float64, device=dev)
    eg = (G * ((dxm + dym)[..., None] + gamma(8))).reshape(-1, 3)
    for w_, i_ in zip(wts, idx):
        dp.index_add_(0, i_.reshape(-1), (g * w_[..., None]).reshape(-1, 3))
        ab.index_add_(0, i_.reshape(-1), (G * w_[..., None]).reshape(-1, 3))
        er.index_add_(0, i_.reshape(-1), eg)
        cnt.index_add_(0, i_.reshape(-1), torch.ones(H * W, 1, dtype=torch.float64, device=dev))
    box = lambda t: (F.avg_pool2d(t.view(H, W, -1).permute(2, 0, 1)[None], 3, 1, 1, count_include_pad=True)[0] * 9).permute(1, 2, 0)
    E, N = box(er), box(cnt)
    res["d_prev"] = dp.view(H, W, 3)
    res["e_prev"] = E + kv.C_DIRECT * U * N * (ab.view(H, W, 3) + E) + (N + 8) * TINY      # sum_bound with a per-tap depth
    return res


def warp_position32(fw):
    """warp_position() of elementwise.hip in fp32, operation by operation (unfused)"""
    H, W = fw.shape[:2]
    f32 = lambda t: torch.tensor(float(t), dtype=torch.float32)

    def axis(n, flow):
        s = f32(n - 1) / f32(2.0)
        step = f32(2.0) / f32(n - 1)
        i = torch.arange(n)
        g0 = torch.where(i < n // 2, f32(-1.0) + step * i.float(), f32(1.0) - step * (n - 1 - i).float())
        return g0, s

    gx0, sx = axis(W, None)
    gy0, sy = axis(H, None)
    gx = gx0[None, :] + fw[..., 0] / sx
    gy = gy0[:, None] + fw[..., 1] / sy
    return ((gx + f32(1.0)) / f32(2.0)) * f32(W - 1), ((gy + f32(1.0)) / f32(2.0)) * f32(H - 1)


def warp32(raw, fw, prev, c0, fault=None):
    """warp_composite_kernel in fp32: (out | None, warp).  fault 'c0': the channels read from prev_c0 - 1 (or + 1 at 0)"""
    H, W = fw.shape[:2]
    if fault == "c0":
        c0 = c0 - 1 if c0 > 0 else c0 + 1
    v = prev[..., c0:c0 + 3]
    px, py = warp_position32(fw)
    px, py = px.clamp(0, W - 1), py.clamp(0, H - 1)
    x0, y0 = px.floor().long(), py.floor().long()
    wx1, wy1 = (px - px.floor())[..., None], (py - py.floor())[..., None]
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    okx, oky = (x0 + 1 < W)[..., None], (y0 + 1 < H)[..., None]
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    wv = v[y0, x0] * (wx0 * wy0)
    wv = torch.where(okx, wv + v[y0, x1] * (wx1 * wy0), wv)
    wv = torch.where(oky, wv + v[y1, x0] * (wx0 * wy1), wv)
    wv = torch.where(okx & oky, wv + v[y1, x1] * (wx1 * wy1), wv)
    if raw is None:
        return None, wv
    wt = fw[..., 2:3]
    return raw[..., :3] * wt + wv * (1.0 - wt), wv


def warp_backward32(d_out, d_warp, raw, fw, prev, c0, fault=None):
    """warp_composite_backward_kernel in fp32: (d_raw | None, d_fw [H, W, 3], d_prev [H, W, 3]).  faults: 'wy' -- wy0 and wy1
    swapped in d_flow_x; 'c0' -- prev_c0 off by one"""
    H, W = fw.shape[:2]
    if fault == "c0":
        c0 = c0 - 1 if c0 > 0 else c0 + 1
    v = prev[..., c0:c0 + 3]
    upx, upy = warp_position32(fw)
    inx, iny = (upx >= 0) & (upx <= W - 1), (upy >= 0) & (upy <= H - 1)
    px, py = upx.clamp(0, W - 1), upy.clamp(0, H - 1)
    x0, y0 = px.floor().long(), py.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    wx1, wy1 = (px - px.floor())[..., None], (py - py.floor())[..., None]
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    z = torch.zeros(H, W, 3)
    go = d_out[..., :3] if d_out is not None else z
    gw = d_warp[..., :3] if d_warp is not None else z
    wt = fw[..., 2:3] if d_out is not None else torch.zeros(H, W, 1)
    rw = raw[..., :3] if raw is not None else z
    g = go * (1.0 - wt) + gw
    v00, v10, v01, v11 = v[y0, x0], v[y0, x1], v[y1, x0], v[y1, x1]
    warp = v00 * (wx0 * wy0) + v10 * (wx1 * wy0) + v01 * (wx0 * wy1) + v11 * (wx1 * wy1)
    a, b = (wy1, wy0) if fault == "wy" else (wy0, wy1)
    tx = g * (a * (v10 - v00) + b * (v11 - v01))
    ty = g * (wx0 * (v01 - v00) + wx1 * (v11 - v10))
    tw = go * (rw - warp)
    s3 = lambda t: (t[..., 0] + t[..., 1]) + t[..., 2]
    d_fw = torch.stack([torch.where(inx, s3(tx), torch.tensor(0.0)), torch.where(iny, s3(ty), torch.tensor(0.0)),
                        s3(tw) if d_out is not None else torch.zeros(H, W)], -1)
    dp = torch.zeros(H * W, 3)
    for w_, i_ in (((wx0 * wy0), y0 * W + x0), ((wx1 * wy0), y0 * W + x1), ((wx0 * wy1), y1 * W + x0), ((wx1 * wy1), y1 * W + x1)):
        dp.index_add_(0, i_.reshape(-1), (g * w_).reshape(-1, 3))
    return (go * wt if d_out is not None else None), d_fw, dp.view(H, W, 3)


def closest(got, cands):
    """|got - candidate| of the nearest admissible value"""
    return torch.stack([(got - c).abs() for c in cands]).min(0).values


# ---- 3x3 / stride 2 average pool -----------------------------------------------------------------------------------------------
POOL_CASES = [
    _c("pool_1x1_c3", "pool", H=1, W=1, C=3, fwd=True, bwd=True),
    _c("pool_2x3_c1", "pool", H=2, W=3, C=1, fwd=True, bwd=True),
    _c("pool_7x9_c3", "pool", H=7, W=9, C=3, fwd=True, bwd=True),
    _c("pool_16x16_c12", "pool", H=16, W=16, C=12, fwd=True, bwd=True),
    _c("pool_fwd_258x258_c32", "pool", H=258, W=258, C=32, fwd=True, bwd=False),      # 129 * 129 * 32 = 532 512 outputs
    _c("pool_bwd_128x129_c32", "pool", H=128, W=129, C=32, fwd=False, bwd=True),      # 528 384 inputs
]


def pool_dims(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _pool_counts(H, W, device):
    Ho, Wo = pool_dims(H, W)
    oy, ox = torch.arange(Ho, device=device), torch.arange(Wo, device=device)
    ny = torch.minimum(2 * oy + 1, torch.tensor(H - 1, device=device)) - (2 * oy - 1).clamp(min=0) + 1
    nx = torch.minimum(2 * ox + 1, torch.tensor(W - 1, device=device)) - (2 * ox - 1).clamp(min=0) + 1
    return (ny[:, None] * nx[None, :])[..., None]


def _pool_windows(xp, Ho, Wo, order=((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2))):
    """the nine strided views of the zero-padded map [H + 2 (+1), W + 2 (+1), C]: window tap (ky, kx) of every output"""
    return [xp[ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] for ky, kx in order]


def _padded(x, dtype):
    H, W, C = x.shape
    Ho, Wo = pool_dims(H, W)
    xp = torch.zeros(2 * Ho + 2, 2 * Wo + 2, C, dtype=dtype, device=x.device)
    xp[1:1 + H, 1:1 + W] = x
    return xp


def pool64(x):
    """AvgPool2d(3, 2, 1, count_include_pad=False): the sum of the taps inside the image over their number.  The kernel adds
    them in window order onto 0 (<= 8 roundings) and divides (9): gamma(9) sum|x| / n"""
    H, W, _ = x.shape
    Ho, Wo = pool_dims(H, W)
    n = _pool_counts(H, W, x.device).double()
    s = sum(_pool_windows(_padded(x.double(), torch.float64), Ho, Wo))
    a = sum(_pool_windows(_padded(x.double().abs(), torch.float64), Ho, Wo))
    return s / n, gamma(9) * a / n + 9 * TINY


def pool32(x, fault=None):
    """avgpool3s2_kernel in fp32 (a tap outside the image adds an exact 0).  fault 'nine': the divisor is 9 everywhere"""
    H, W, _ = x.shape
    Ho, Wo = pool_dims(H, W)
    s = torch.zeros(Ho, Wo, x.shape[2])
    for t in _pool_windows(_padded(x, torch.float32), Ho, Wo):
        s = s + t
    return s / (torch.full((Ho, Wo, 1), 9.0) if fault == "nine" else _pool_counts(H, W, "cpu").float())


def pool_backward64(dy, H, W):
    """each input pixel sums dy / n over the <= 4 windows that hold it: a rounded quotient each, three additions (the first
    lands on 0): gamma(4) sum |dy / n|"""
    Ho, Wo = pool_dims(H, W)
    q = dy.double() / _pool_counts(H, W, dy.device).double()
    out = []
    for t in (q, q.abs()):
        dp = torch.zeros(2 * Ho + 2, 2 * Wo + 2, dy.shape[2], dtype=torch.float64, device=dy.device)
        for view in _pool_windows(dp, Ho, Wo):
            view += t
        out.append(dp[1:1 + H, 1:1 + W])
    return out[0], gamma(4) * out[1] + 4 * TINY


def pool_backward32(dy, H, W, fault=None):
    """avgpool3s2_backward_kernel in fp32: a pixel's windows in (oy, ox) order, i.e. window taps in descending (ky, kx)"""
    Ho, Wo = pool_dims(H, W)
    q = dy / (torch.full((Ho, Wo, 1), 9.0) if fault == "nine" else _pool_counts(H, W, "cpu").float())
    dp = torch.zeros(2 * Ho + 2, 2 * Wo + 2, dy.shape[2])
    for view in _pool_windows(dp, Ho, Wo, order=[(ky, kx) for ky in (2, 1, 0) for kx in (2, 1, 0)]):
        view += q
    return dp[1:1 + H, 1:1 + W]


# ---- activation backward ---------------------------------------------------------------------------------------------------------
ACT_CASES = [_c("act_mode%d_n%d" % (m, n), "act", mode=m, n=n, slope={0: 0.37, 1: 1.0, 2: 1.0, 3: 0.2, 4: 20.0}[m])
             for m in (0, 1, 2, 3, 4) for n in (1, 1001, 524292) if not (m == 4 and n % 4)] + [     # 524 292 > GRID_CAP, % 4 == 0
    _c("act_mode4_n4", "act", mode=4, n=4, slope=20.0), _c("act_mode4_n1000", "act", mode=4, n=1000, slope=20.0)]   # mode 4: n % 4 == 0


def act64(dy, y, mode, slope):
    """act_backward_kernel, from the OUTPUT y.  slope32 = float32(slope) is what the kernel multiplies by.
      1 tanh:    g (1 - y y): y y (1), 1 - . (2), the product (3); the subtraction's rounding is relative to |1 - y y| and the
                 square's to y y: gamma(3) |g| (|1 - y y| + y y)   (y = +-1 gives exactly 0 either way)
      2 sigmoid: (g y) (1 - y): three roundings, each relative: gamma(3) |g y (1 - y)|
      3 leaky:   y > 0 ? g : g slope: one rounding
      4 flow / weight head on [., 4] storage: channels 0, 1 g slope; channel 2 the sigmoid's; channel 3 exactly 0
      0 (scale): g slope: one rounding"""
    g, v = dy.double(), y.double()
    s = float(torch.tensor(slope, dtype=torch.float32))
    sig, e_sig = g * v * (1 - v), gamma(3) * (g * v * (1 - v)).abs() + 3 * TINY
    lin, e_lin = g * s, U * (g * s).abs() + TINY
    if mode == 1:
        return g * (1 - v * v), gamma(3) * g.abs() * ((1 - v * v).abs() + v * v) + 3 * TINY
    if mode == 2:
        return sig, e_sig
    if mode == 3:
        return torch.where(v > 0, g, lin), torch.where(v > 0, torch.zeros_like(g), e_lin)
    if mode == 4:
        c = torch.arange(g.numel(), device=g.device) & 3
        z = torch.zeros_like(g)
        return torch.where(c < 2, lin, torch.where(c == 2, sig, z)), torch.where(c < 2, e_lin, torch.where(c == 2, e_sig, z))
    return lin, e_lin


def act32(dy, y, mode, slope):
    s = torch.tensor(slope, dtype=torch.float32)
    sig = dy * y * (1.0 - y)
    if mode == 1:
        return dy * (1.0 - y * y)
    if mode == 2:
        return sig
    if mode == 3:
        return torch.where(y > 0, dy, dy * s)
    if mode == 4:
        c = torch.arange(dy.numel()) & 3
        return torch.where(c < 2, dy * s, torch.where(c == 2, sig, torch.zeros_like(dy)))
    return dy * s


# ---- masked L1 and the loss backward kernels ---------------------------------------------------------------------------------------
_ML1_CH = [(4, 0, 2), (4, 2, 1), (8, 3, 3)]          # (cs, c0, C)
ML1_CASES = [_c("ml1_20x28_cs%d_c%d_C%d_%s" % (cs, c0, C, v), "ml1", H=20, W=28, cs=cs, c0=c0, C=C, b=v != "nob", mask=v != "nomask")
             for (cs, c0, C) in _ML1_CH for v in ("full", "nob", "nomask")] + [
    _c("ml1_257x512_cs4_c0_C2", "ml1", H=257, W=512, cs=4, c0=0, C=2, b=True, mask=True)]     # 526 336 floats: past the cap
LOSS_BWD_CASES = [_c("lossbwd_op%d_n%d" % (op, n), "lossbwd", op=op, n=n) for op in (0, 1) for n in (1001, 524289)]


def ml1_depth(n):
    """reduce_masked_l1_kernel + reduce_final_kernel: a thread's chain over ceil(n / (256 g)) positions, 6 shuffle levels and
    the 4 wave sums (block_sum), then the same over the g partials"""
    g = max(1, min((n + 255) // 256, 2048))
    return -(-n // (256 * g)) + 10 + -(-g // 256) + 10


def ml1_64(a, b, mask, c0, C):
    """sum over pixels and channels [c0, c0 + C) of mask |a - b|: the terms round twice (the difference, the product by the
    mask), the two-level sum by sum_bound at ml1_depth"""
    d = (a.double() - (b.double() if b is not None else 0.0)).abs()[..., c0:c0 + C]
    t = d * mask.double()[..., None] if mask is not None else d
    A = t.abs().sum()
    return t.sum(), sum_bound(A, ml1_depth(a.numel()), a.numel()) + gamma(2) * A


def _block_sum32(s):
    """block_sum(): s [..., 256] -> [...]: xor-shuffle tree per 64-lane wave (lane 0's value), then the 4 waves in turn"""
    w = s.reshape(s.shape[:-1] + (4, 64))
    for o in (32, 16, 8, 4, 2, 1):
        idx = torch.arange(64) ^ o
        w = w + w[..., idx]
    t = torch.zeros(s.shape[:-1])
    for i in range(4):
        t = t + w[..., i, 0]
    return t


def ml1_32(a, b, mask, c0, C, fault=None):
    """the two kernels in fp32.  fault 'c0': the channel window taken from channel 0"""
    cs = a.shape[-1]
    n = a.numel()
    if fault == "c0":
        c0 = 0
    d = (a - (b if b is not None else 0.0)).abs()
    if mask is not None:
        d = mask[..., None] * d
    ch = torch.arange(cs)
    d = (d * ((ch >= c0) & (ch < c0 + C)).float()).reshape(-1)
    g = max(1, min((n + 255) // 256, 2048))
    it = -(-n // (256 * g))
    dp = torch.zeros(it * g * 256)
    dp[:n] = d
    dp = dp.view(it, g, 256)
    s = torch.zeros(g, 256)
    for i in range(it):
        s = s + dp[i]
    part = _block_sum32(s)
    k = -(-g // 256)
    pp = torch.zeros(k * 256)
    pp[:g] = part
    pp = pp.view(k, 256)
    s = torch.zeros(256)
    for i in range(k):
        s = s + pp[i]
    return _block_sum32(s)


def ml1_backward32(a, b, mask, c0, C, scale):
    """masked_l1_backward_kernel: sign(a - b) scale mask inside [c0, c0 + C), exactly 0 outside.  One product: the kernel's
    bits (there is nothing to fuse it with)"""
    d = a - (b if b is not None else 0.0)
    s = torch.tensor(scale, dtype=torch.float32, device=a.device)
    g = torch.where(d > 0, s, torch.where(d < 0, -s, torch.zeros_like(s)))
    if mask is not None:
        g = g * mask[..., None]
    ch = torch.arange(a.shape[-1], device=a.device)
    return torch.where((ch >= c0) & (ch < c0 + C), g, torch.zeros_like(g))


def loss_backward64(a, b, c, scale, op):
    """op 0: (2 scale) (a - c): the doubling is exact, the difference and the product round: gamma(2).  op 1: scale sign(a - b),
    exact"""
    s = float(torch.tensor(scale, dtype=torch.float32))
    if op == 0:
        r = 2.0 * s * (a.double() - float(torch.tensor(c, dtype=torch.float32)))
        return r, gamma(2) * r.abs() + 2 * TINY
    r = s * torch.sign(a.double() - b.double())
    return r, torch.zeros_like(r)


def loss_backward32(a, b, c, scale, op):
    s = torch.tensor(scale, dtype=torch.float32)
    if op == 0:
        return torch.tensor(2.0) * s * (a - torch.tensor(c, dtype=torch.float32))
    return s * torch.sign(a - b)


# ---- the cases' tensors and the extents of what the kernels index ----------------------------------------------------------------
ALL_CASES = APPLY_CASES + JOIN_CASES + NORM_BWD_CASES + WARP_CASES + POOL_CASES + ACT_CASES + ML1_CASES + LOSS_BWD_CASES
BY_ID = {c.id: c for c in ALL_CASES}


def _warp_flow(p, g):
    H, W = p["H"], p["W"]
    f = torch.zeros(H, W, 2)
    if p["flow"] in ("randn", "huge", "edges"):
        f = torch.randn(H, W, 2, generator=g) * p["std"]
    if p["flow"] == "const":
        f[..., 0], f[..., 1] = 3.0, -2.0
    if p["flow"] == "inside2x2":     # three of the four pixels sample inside the single cell, the fourth leaves it on both axes
        f[:] = torch.tensor([[[0.3, 0.6], [-0.25, 0.5]], [[0.5, -0.75], [0.4, 0.2]]])
    if p["flow"] == "huge":
        for (y, x, fx, fy) in ((0, 0, 1e6, 0.5), (3, 7, -1e6, -1e6), (23, 39, 0.25, 1e6), (11, 20, -1e6, 2.0), (12, 1, 1e6, -1e6)):
            f[y, x, 0], f[y, x, 1] = fx, fy
    if p["flow"] == "edges":
        f[5, :, 0] = (W - 1) - torch.arange(W).float()          # row 5 samples exactly on the last column
        f[:, 8, 1] = (H - 1) - torch.arange(H).float()          # column 8 exactly on the last row
        f[9, :, 0] = -torch.arange(W).float()                   # row 9 exactly on column 0
        f[:, 3, 1] = -torch.arange(H).float()                   # column 3 exactly on row 0
    return f


def build_case(case, device):
    """the tensors the GPU test passes for `case` (built on the CPU from the case's own seed, then moved), by argument name"""
    p, g = case.p, _gen(_seed(case))
    t = {}
    if case.kind == "apply":
        npix = p["H"] * p["W"]
        x, mr, ga, be, res = _norm_side(g, p["nimg"], npix, p["C"], p["affine"], p["mean"], p["nres"])
        t = dict(x=x, mean_rstd=mr, gamma=ga, beta=be, res1=res[0] if res else None, res2=res[1] if len(res) > 1 else None)
    elif case.kind == "join":
        npix = p["H"] * p["W"]
        for tag, aff in zip("ab", p["affine"]):
            x, mr, ga, be, res = _norm_side(g, p["nimg"], npix, p["C"], aff, 0.0, 1)
            t.update({tag + "_y": x, tag + "_mean_rstd": mr, tag + "_gamma": ga, tag + "_beta": be, tag + "_res": res[0]})
    elif case.kind == "nbwd":
        npix, C = p["H"] * p["W"], p["C"]
        x = torch.randn(npix, C, generator=g) * (1.0 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
        x[:, PIN_CH] = 0.75                                   # the pinned channel: mean == x exactly, rstd = 1 / sqrt(eps)
        ga = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0) if p["affine"] else None
        be = torch.randn(C, generator=g) * 0.5 if p["affine"] else None
        if be is not None:
            be[PIN_CH] = 0.0
        t = dict(x=x, dy=torch.randn(npix, C, generator=g), mean_rstd=stats64(x), gamma=ga, beta=be,
                 d_beta=torch.randn(C, generator=g), d_gamma=torch.randn(C, generator=g))
    elif case.kind == "warp":
        H, W = p["H"], p["W"]
        fw = torch.zeros(H, W, 4)
        fw[..., :2] = _warp_flow(p, g)
        fw[..., 2] = torch.rand(H, W, generator=g)
        fw[0, 0, 2], fw[-1, -1, 2] = 0.0, 1.0
        raw = torch.randn(H, W, 4, generator=g)
        raw[..., 3] = 0.0
        t = dict(raw=raw, fw=fw, prev=torch.randn(H, W, p["cs"], generator=g), d_out=torch.randn(H, W, 4, generator=g),
                 d_warp=torch.randn(H, W, 4, generator=g))
    elif case.kind == "pool":
        Ho, Wo = pool_dims(p["H"], p["W"])
        t = dict(x=torch.randn(p["H"], p["W"], p["C"], generator=g), dy=torch.randn(Ho, Wo, p["C"], generator=g))
    elif case.kind == "act":
        n = p["n"]
        y = torch.tanh(torch.randn(n, generator=g)) if p["mode"] in (1, 3, 0) else torch.sigmoid(torch.randn(n, generator=g))
        special = torch.tensor([-1.0, 0.0, 1.0] if p["mode"] != 2 and p["mode"] != 4 else [0.0, 1.0, 0.0])
        k = min(n, 3)
        y[:k] = special[:k]
        if n > 8:
            y[-7:-4] = special
            if p["mode"] == 4:
                y[2], y[6] = 0.0, 1.0                         # the sigmoid channel at exactly 0 and 1
        t = dict(dy=torch.randn(n, generator=g), y=y)
    elif case.kind == "ml1":
        H, W, cs = p["H"], p["W"], p["cs"]
        a = torch.randn(H, W, cs, generator=g)
        b = torch.randn(H, W, cs, generator=g)
        tie = torch.rand(H, W, cs, generator=g) < 0.1
        b = torch.where(tie, a, b)                            # some a == b: sign 0
        if not p["b"]:
            a = torch.where(tie, torch.zeros_like(a), a)      # (against no b: some exact zeros)
        mask = torch.rand(H, W, generator=g)
        mask[0, :5] = 0.0
        t = dict(a=a, b=b if p["b"] else None, mask=mask if p["mask"] else None)
    elif case.kind == "lossbwd":
        a = torch.randn(p["n"], generator=g)
        b = torch.randn(p["n"], generator=g)
        b[::7] = a[::7]
        t = dict(a=a, b=b)
    return {k: (v.contiguous().to(device) if v is not None else None) for k, v in t.items()}


def extents(case):
    """Floats each argument of `case`'s launches can be indexed at, read off the kernels' index expressions:
      apply / join / add (inorm_apply_kernel, add_kernel): image im, float4 i < n4 = npix C / 4 -> x, res, y [nimg npix C];
        tables mean_rstd + im 2 C4, float4 2 c4 + 1 < 2 C4 -> nimg 2 C; gamma, beta float4 c4 < C4 -> C.  C % 4 == 0.
      norm backward: x, dy, dx at (p C4 + q) float4, p < npix, q < C4 -> npix C; mean_rstd, sums float2 c < C -> 2 C; gamma, beta
        C; partial[(blockIdx.y C + c)] float2, blockIdx.y < slices <= 128 -> slices C 2 <= 128 C 2; d_beta, d_gamma C.
      warp: raw, fw, out, warp_out, d_* float4 i < H W -> H W 4; prev, d_prev at ((y W + x) prev_cs + prev_c0 + c), y < H, x < W,
        c < 3, prev_c0 + 3 <= prev_cs -> H W prev_cs.  H, W >= 2.
      avgpool: x, dx [H W C]; y, dy [Ho Wo C], Ho = (H - 1) / 2 + 1.
      act / loss backward: n each.  masked L1: a, b, da npix cs; mask npix; partials one per block, <= 2048; out 1."""
    p = case.p
    if case.kind == "apply":
        n, C = p["nimg"] * p["H"] * p["W"] * p["C"], p["C"]
        assert C % 4 == 0
        return dict(x=n, res1=n if p["nres"] > 0 else 0, res2=n if p["nres"] > 1 else 0, out=n, mean_rstd=p["nimg"] * 2 * C,
                    gamma=C if p["affine"] else 0, beta=C if p["affine"] else 0)
    if case.kind == "join":
        n, C = p["nimg"] * p["H"] * p["W"] * p["C"], p["C"]
        assert C % 4 == 0
        e = dict(out=n, sum=n)
        for tag, aff in zip("ab", p["affine"]):
            e.update({tag + "_y": n, tag + "_res": n, tag + "_mean_rstd": p["nimg"] * 2 * C, tag + "_gamma": C if aff else 0,
                      tag + "_beta": C if aff else 0})
        return e
    if case.kind == "nbwd":
        npix, C = p["H"] * p["W"], p["C"]
        assert C % 4 == 0
        return dict(x=npix * C, dy=npix * C, dx=npix * C, mean_rstd=2 * C, sums=2 * C, gamma=C if p["affine"] else 0,
                    beta=C if p["affine"] else 0, scratch=bwd_slices(npix, C) * C * 2, d_beta=C, d_gamma=C)
    if case.kind == "warp":
        assert p["H"] >= 2 and p["W"] >= 2 and 0 <= p["c0"] and p["c0"] + 3 <= p["cs"]
        n = p["H"] * p["W"]
        return dict(raw=4 * n, fw=4 * n, out=4 * n, warp_out=4 * n, d_out=4 * n, d_warp=4 * n, d_raw=4 * n, d_fw=4 * n,
                    prev=n * p["cs"], d_prev=n * p["cs"])
    if case.kind == "pool":
        Ho, Wo = pool_dims(p["H"], p["W"])
        return dict(x=p["H"] * p["W"] * p["C"], y=Ho * Wo * p["C"], dy=Ho * Wo * p["C"], dx=p["H"] * p["W"] * p["C"])
    if case.kind == "act":
        assert p["mode"] != 4 or p["n"] % 4 == 0
        return dict(dy=p["n"], y=p["n"], dpre=p["n"])
    if case.kind == "ml1":
        assert p["c0"] >= 0 and p["c0"] + p["C"] <= p["cs"]
        npix = p["H"] * p["W"]
        return dict(a=npix * p["cs"], b=npix * p["cs"] if p["b"] else 0, mask=npix if p["mask"] else 0, da=npix * p["cs"],
                    scratch=max(1, min((npix * p["cs"] + 255) // 256, 2048)), out=1)
    if case.kind == "lossbwd":
        return dict(a=p["n"], b=p["n"], da=p["n"])
    raise KeyError(case.kind)


def allocated(case):
    """what text2video_amd/ops.py allocates itself for `case` (read off ops.py): outputs empty_like their input, the norm
    backward's sums [C, 2] and scratch 128 C 2, the reductions' 2048-float scratch.  Where the size is the contract's own (every
    output), it must equal extents(); the two scratch buffers are sized for the largest launch and must cover it."""
    p, e = case.p, extents(case)
    if case.kind == "nbwd":
        return dict(dx=(p["H"] * p["W"] * p["C"], True), sums=(2 * p["C"], True), scratch=(128 * p["C"] * 2, False))
    if case.kind == "warp":
        n = p["H"] * p["W"]
        return dict(out=(4 * n, True), warp_out=(4 * n, True), d_raw=(4 * n, True), d_fw=(4 * n, True), d_prev=(n * p["cs"], True))
    if case.kind == "pool":
        Ho, Wo = pool_dims(p["H"], p["W"])
        return dict(y=(((p["H"] + 2 - 3) // 2 + 1) * ((p["W"] + 2 - 3) // 2 + 1) * p["C"], True), dx=(e["dx"], True))
    if case.kind == "act":
        return dict(dpre=(p["n"], True))
    if case.kind == "ml1":
        return dict(da=(e["da"], True), scratch=(2048, False), out=(1, True))
    if case.kind == "lossbwd":
        return dict(da=(p["n"], True))
    return {}
