"""The norm finalize's grouped form (inorm_finalize_kernel with gridDim.y > 1 + inorm_finalize_merge_kernel,
csrc/elementwise.hip) restated in float64: which partial a pixel belongs to, which group pools which partial, the
pooled-moment formula, and the faults that form can have.  A plain helper module (numpy only) for
tests/test_cpu_norm_finalize_grouped.py and tests/test_gpu_norm_finalize_grouped.py.

A partial is (mean, M2) of up to 128 output pixels: 8 consecutive 4x4 tiles of the F(4x4) output transform's tile grid
(row-major tiles; a ragged map's edge tiles hold fewer pixels), or BM consecutive pixels (row-major) of the direct kernel.
With a scratch buffer and nparts >= 2048 the launch has G = groups(nparts, C) block rows; block row g pools the partials
g*64 + sl + 64*G*j (slice sl = 0..63, j = 0, 1, ...), i.e. the 64-partial block b = part // 64 goes to group b % G, and
the merge kernel adds scratch rows g*C + c over g in order."""
import numpy as np

SLICES = 64
MAX_GROUPS = 64
EPS = 1e-5
RTOL, ATOL = 2e-5, 2e-6          # tests/test_gpu_norm_finalize_direct.py's tolerance for a finalize


def groups(nparts, C):
    """finalize_groups() with a scratch buffer given"""
    if nparts < 2048:
        return 1
    return max(1, min(nparts // 512, 512 // -(-C // 16), MAX_GROUPS))


def partial_map(H, W, wm=4, BM=None):
    """(int [H, W]: the partial, inside its image, that output pixel (y, x) is pooled in; partials per image, padding ones
    included).  wm: the tile edge of a Winograd producer; BM: the rows per partial of the direct kernel instead"""
    ys, xs = np.mgrid[0:H, 0:W]
    if BM is not None:
        return (ys * W + xs) // BM, -(-H * W // BM)
    TH, TW = -(-H // wm), -(-W // wm)
    per = 128 // (wm * wm)
    T = TH * TW
    a, b = -(-T // 64) * 64, -(-T // 128) * 128          # wino_pad_tiles
    Tp = a if (b - a) * 8 >= b else b
    return ((ys // wm) * TW + xs // wm) // per, Tp // per


def group_map(part, nparts_image, batch, C):
    """int [batch, H, W]: the group that pools each pixel's partial; G"""
    G = groups(batch * nparts_image, C)
    glob = np.stack([part + i * nparts_image for i in range(batch)])
    return (glob // SLICES) % G, G


def stripes(gmap, G, C, sigma=1.0):
    """float64 [batch, H, W, C]: a component that is constant inside each finalize group and steps by sigma from one group
    to the next; channel c meets the groups' levels rotated by c, so every channel has the same variance"""
    level = (gmap[..., None] + np.arange(C)) % G
    return sigma * (level - (G - 1) / 2.0)


def partials64(y, part, nparts_image):
    """y float64 [batch, H, W, C] -> (mean [P, C], M2 [P, C], n [P]) over P = batch * nparts_image partials (n = 0: padding)"""
    batch, H, W, C = y.shape
    P = batch * nparts_image
    idx = np.stack([part + i * nparts_image for i in range(batch)]).reshape(-1)
    flat = y.reshape(-1, C)
    n = np.bincount(idx, minlength=P).astype(np.float64)
    mean, m2 = np.zeros((P, C)), np.zeros((P, C))
    for c in range(C):
        mean[:, c] = np.bincount(idx, weights=flat[:, c], minlength=P) / np.maximum(n, 1)
        m2[:, c] = np.bincount(idx, weights=(flat[:, c] - mean[idx, c]) ** 2, minlength=P)
    return mean, m2, n


FAULTS = ("a group dropped", "a group counted twice", "scratch row g*16+c for g*C+c", "pixel count taken as uniform")


def pooled64(mean, m2, n, G, fault=None, eps=EPS):
    """(mean [C], rstd [C]) by the kernels' pooled-moment formula in float64, group by group; `fault`: one of FAULTS"""
    P, C = mean.shape
    if fault == "pixel count taken as uniform":
        n = np.where(n > 0, 128.0, 0.0)
    ref = mean[0]
    d = mean - ref
    grp = (np.arange(P) // SLICES) % G
    rows = np.zeros((G, C, 4))
    for g in range(G):
        k = grp == g
        nk = n[k][:, None]
        rows[g, :, 0] = nk.sum()
        rows[g, :, 1] = (nk * d[k]).sum(0)
        rows[g, :, 2] = (nk * d[k] * d[k]).sum(0)
        rows[g, :, 3] = (m2[k] * (nk > 0)).sum(0)
    flat = rows.reshape(G * C, 4)
    tot = np.zeros((C, 4))
    for g in range(G):
        if fault == "a group dropped" and g == G - 1:
            continue
        row = flat[g * 16 + np.arange(C)] if fault == "scratch row g*16+c for g*C+c" else rows[g]
        tot += row
        if fault == "a group counted twice" and g == 0:
            tot += row
    s0, s1, s2, sm2 = tot.T
    md = s1 / s0
    var = np.maximum(sm2 + s2 - s1 * md, 0.0) / s0
    return ref + md, 1.0 / np.sqrt(var + eps)


def tolerance(want):
    return ATOL + RTOL * np.abs(want)
