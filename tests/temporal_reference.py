"""float64 numpy statement of what t2v_temporal_metrics_u8 computes (include/t2v.h), written two independent ways
(vectorised, and a plain per-pixel loop), and the seeded inputs the CPU and GPU tests share.

    For a pixel p = (x, y) of the region, f = flow_fwd(p): q = p + f; p is INSIDE when f is finite and q lies in
    [0, W-1] x [0, H-1]; bq = bilinear(flow_bwd; q); p is VALID when it is inside, bq is finite and
    |f + bq|^2 <= 0.01 (|f|^2 + |bq|^2) + 0.5.  Row = {n_valid, warp_sse_a, warp_sse_b, n_flow, epe_sum, tdiff_sse}:
    warp_sse_x = sum over valid p and 3 channels of (x_cur(p) - bilinear(x_prev; q))^2; n_flow / epe_sum over all p where f
    and flow_a(p) are finite: their number and sum |flow_a(p) - f|; tdiff_sse = sum over all p and 3 channels of
    ((a_cur - a_prev) - (b_cur - b_prev))^2.  A box restricts p, not the taps.
"""
import math

import numpy as np

COLUMNS = ("n_valid", "warp_sse_a", "warp_sse_b", "n_flow", "epe_sum", "tdiff_sse")
INTEGER_COLUMNS = (0, 3, 5)
FLOAT_COLUMNS = (1, 2, 4)
MIN_MARGIN = 1e-9          # every case handed out keeps the validity test this far from equality (a condition on the inputs)


def _bilinear(img, qx, qy, dt):
    """img [H,W] or [H,W,C] (already of dtype dt) at positions inside the image (qx, qy: [N])"""
    H, W = img.shape[:2]
    x0f, y0f = np.floor(qx), np.floor(qy)
    fx, fy = (qx - x0f).astype(dt), (qy - y0f).astype(dt)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    if img.ndim == 3:
        fx, fy = fx[:, None], fy[:, None]
    one = dt(1.0)
    top = (one - fx) * img[y0, x0] + fx * img[y0, x1]
    bot = (one - fx) * img[y1, x0] + fx * img[y1, x1]
    return (one - fy) * top + fy * bot


def _pixel_terms(a_cur, a_prev, b_cur, b_prev, f, b, fa, dt=np.float64):
    """per-pixel planes: inside, bq finite, lhs, rhs (of the validity test; NaN where not inside), wa, wb (warp squares,
    0 where not inside), flow_ok, epe, td -- everything the row is summed from"""
    H, W = a_cur.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    fu, fv = f[..., 0].astype(dt), f[..., 1].astype(dt)
    f_ok = np.isfinite(fu) & np.isfinite(fv)
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = xs.astype(dt) + fu, ys.astype(dt) + fv
        inside = f_ok & (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
    lhs, rhs = np.full((H, W), np.nan), np.full((H, W), np.nan)
    bq_ok = np.zeros((H, W), bool)
    wa, wb = np.zeros((H, W), dt), np.zeros((H, W), dt)
    idx = np.nonzero(inside)
    px, py = qx[idx], qy[idx]
    with np.errstate(invalid="ignore", over="ignore"):
        bq = _bilinear(b[..., :2].astype(dt), px, py, dt)
        bu, bv = bq[:, 0], bq[:, 1]
        su, sv = fu[idx] + bu, fv[idx] + bv
        lhs[idx] = su * su + sv * sv
        rhs[idx] = dt(0.01) * ((fu[idx] * fu[idx] + fv[idx] * fv[idx]) + (bu * bu + bv * bv)) + dt(0.5)
    bq_ok[idx] = np.isfinite(bu) & np.isfinite(bv)
    for cur, prev, dst in ((a_cur, a_prev, wa), (b_cur, b_prev, wb)):
        d = cur[..., :3].astype(dt)[idx] - _bilinear(prev[..., :3].astype(dt), px, py, dt)
        dst[idx] = (d * d).sum(axis=1) if dt is np.float64 else (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    flow_ok, epe = np.zeros((H, W), bool), np.zeros((H, W), dt)
    if fa is not None:
        gu, gv = fa[..., 0].astype(dt), fa[..., 1].astype(dt)
        flow_ok = f_ok & np.isfinite(gu) & np.isfinite(gv)
        j = np.nonzero(flow_ok)
        with np.errstate(over="ignore"):
            du, dv = gu[j] - fu[j], gv[j] - fv[j]
            epe[j] = np.sqrt(du * du + dv * dv)
    d = (a_cur[..., :3].astype(np.int64) - a_prev[..., :3]) - (b_cur[..., :3].astype(np.int64) - b_prev[..., :3])
    td = (d * d).sum(axis=2)
    return inside, bq_ok, lhs, rhs, wa, wb, flow_ok, epe, td


def _region(H, W, box):
    m = np.zeros((H, W), bool)
    y0, y1, x0, x1 = (0, H, 0, W) if box is None else box
    m[y0:y1, x0:x1] = True
    return m


def reference_row(a_cur, a_prev, b_cur, b_prev, f, b, fa, box=None, dtype=np.float64):
    """the row of the region (the frame, or box = (y0, y1, x0, x1)), vectorised; images uint8 [H,W,>=3], flows [H,W,>=2],
    fa may be None.  dtype=np.float32 evaluates the definition in float32 instead (the per-pixel terms AND the sums)."""
    inside, bq_ok, lhs, rhs, wa, wb, flow_ok, epe, td = _pixel_terms(a_cur, a_prev, b_cur, b_prev, f, b, fa, dtype)
    reg = _region(*a_cur.shape[:2], box)
    with np.errstate(invalid="ignore"):
        valid = reg & inside & bq_ok & (lhs <= rhs)
    fl = reg & flow_ok
    return [float(valid.sum()), float(wa[valid].sum(dtype=dtype)), float(wb[valid].sum(dtype=dtype)), float(fl.sum()),
            float(epe[fl].sum(dtype=dtype)), float(td[reg].sum())]


def reference_row_loop(a_cur, a_prev, b_cur, b_prev, f, b, fa, box=None):
    """the same row, pixel by pixel in plain Python floats (float64), straight from the definition"""
    H, W = a_cur.shape[:2]
    y0, y1, x0, x1 = (0, H, 0, W) if box is None else box
    n_valid = n_flow = tdiff = 0
    sse_a = sse_b = epe = 0.0

    def tap(img, c, qx, qy):
        ix, iy = int(math.floor(qx)), int(math.floor(qy))
        jx, jy = min(ix + 1, W - 1), min(iy + 1, H - 1)
        fx, fy = qx - ix, qy - iy
        top = (1.0 - fx) * float(img[iy, ix, c]) + fx * float(img[iy, jx, c])
        bot = (1.0 - fx) * float(img[jy, ix, c]) + fx * float(img[jy, jx, c])
        return (1.0 - fy) * top + fy * bot

    for y in range(y0, y1):
        for x in range(x0, x1):
            for c in range(3):
                d = (int(a_cur[y, x, c]) - int(a_prev[y, x, c])) - (int(b_cur[y, x, c]) - int(b_prev[y, x, c]))
                tdiff += d * d
            fu, fv = float(f[y, x, 0]), float(f[y, x, 1])
            f_ok = math.isfinite(fu) and math.isfinite(fv)
            if fa is not None and f_ok:
                gu, gv = float(fa[y, x, 0]), float(fa[y, x, 1])
                if math.isfinite(gu) and math.isfinite(gv):
                    n_flow += 1
                    epe += math.sqrt((gu - fu) * (gu - fu) + (gv - fv) * (gv - fv))
            if not f_ok:
                continue
            qx, qy = x + fu, y + fv
            if not (0.0 <= qx <= W - 1 and 0.0 <= qy <= H - 1):
                continue
            bu, bv = tap(b, 0, qx, qy), tap(b, 1, qx, qy)
            if not (math.isfinite(bu) and math.isfinite(bv)):
                continue
            if (fu + bu) ** 2 + (fv + bv) ** 2 <= 0.01 * ((fu * fu + fv * fv) + (bu * bu + bv * bv)) + 0.5:
                n_valid += 1
                for c in range(3):
                    sse_a += (float(a_cur[y, x, c]) - tap(a_prev, c, qx, qy)) ** 2
                    sse_b += (float(b_cur[y, x, c]) - tap(b_prev, c, qx, qy)) ** 2
    return [float(n_valid), sse_a, sse_b, float(n_flow), epe, float(tdiff)]


def margin(a_cur, a_prev, b_cur, b_prev, f, b, fa=None):
    """rhs - lhs of the validity test for the inside pixels whose bq is finite (1-D)"""
    inside, bq_ok, lhs, rhs = _pixel_terms(a_cur, a_prev, b_cur, b_prev, f, b, fa)[:4]
    m = inside & bq_ok
    return rhs[m] - lhs[m]


def fractions(case):
    """(share of pixels inside, share valid) of a case"""
    inside, bq_ok, lhs, rhs = _pixel_terms(*case["images"], case["f"], case["b"], None)[:4]
    with np.errstate(invalid="ignore"):
        return inside.mean(), (inside & bq_ok & (lhs <= rhs)).mean()


def with_stride(img, cs, fill=77):
    """[H,W,3] -> [H,W,cs]; the pad channel holds bytes the kernel must not read into its sums"""
    if cs == 3:
        return np.array(img[..., :3])
    out = np.full(img.shape[:2] + (cs,), fill, np.uint8)
    out[..., :3] = img[..., :3]
    out[..., 3:] = (np.arange(img.shape[0] * img.shape[1]).reshape(img.shape[:2] + (1,)) * 37 + fill) % 256
    return out


def make_flows(H, W, seed):
    """-> (flow_fwd, flow_bwd, flow_a), fp32 [H,W,4]: smooth sinusoidal forward flow of a few px scaled by min(1, min(H,W)/32),
    a band of columns pushed out of the frame (W >= 32), rows pushed out at the top (H >= 32); flow_bwd = -flow_fwd +
    N(0, 0.15) with a 9x15 block offset by 2 px (occluded); flow_a = flow_fwd + a smooth px-sized difference + N(0, 0.3).
    Channels 2, 3 hold values no sum may depend on."""
    rng = np.random.default_rng([seed, H, W, 7])
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    s = min(1.0, min(H, W) / 32.0)
    ph = rng.uniform(0, 2 * np.pi, 4)
    u = s * (1.6 * np.sin(2 * np.pi * xs / max(W, 48) + ph[0]) + 0.9 * np.cos(2 * np.pi * ys / max(H, 48) * 1.3 + ph[1]))
    v = s * (1.2 * np.cos(2 * np.pi * ys / max(H, 48) + ph[2]) + 0.8 * np.sin(2 * np.pi * xs / max(W, 48) * 0.7 + ph[3]))
    if W >= 32:
        u[:, W // 2:W // 2 + max(2, W // 12)] += 2.0 * W
    if H >= 32:
        v[:max(2, H // 10), :] -= H
    f = np.zeros((H, W, 4), np.float32)
    f[..., 0], f[..., 1], f[..., 2], f[..., 3] = u, v, 123.0, -7.5
    b = np.zeros((H, W, 4), np.float32)
    b[..., :2] = -np.stack([u, v], -1) + rng.normal(0.0, 0.15, (H, W, 2))
    if W >= 32:       # (the band's huge values would otherwise leak into the taps of its neighbours)
        b[..., 0] = np.where(np.abs(b[..., 0]) > W, rng.normal(0.0, 0.15, (H, W)), b[..., 0])
    if H >= 32:
        b[..., 1] = np.where(np.abs(b[..., 1]) > H / 2, rng.normal(0.0, 0.15, (H, W)), b[..., 1])
    by, bx = H // 3, W // 3
    b[by:by + 9, bx:bx + 15, :2] += 2.0
    b[..., 2], b[..., 3] = -55.0, 9.25
    fa = np.zeros((H, W, 4), np.float32)
    fa[..., 0] = f[..., 0] + 0.6 * np.sin(xs / 5.0) + rng.normal(0.0, 0.3, (H, W))
    fa[..., 1] = f[..., 1] + 0.4 * np.cos(ys / 7.0) + rng.normal(0.0, 0.3, (H, W))
    fa[..., 2], fa[..., 3] = 31.0, -1.0
    return f, b, fa


def make_images(kind, H, W, seed):
    """-> (a_cur, a_prev, b_cur, b_prev) uint8 [H,W,3].  noise: independent uniform bytes for the real pair, a = clip(b +
    integers(-12, 13)).  smooth: cumsum(integers(-3, 4)) + 128 along the rows for b_prev, b_cur = b_prev shifted by a few
    levels of slow change, a = clip(b + integers(-2, 3))."""
    rng = np.random.default_rng([seed, H, W, {"noise": 1, "smooth": 2}[kind]])
    if kind == "smooth":
        b_prev = np.clip(np.cumsum(rng.integers(-3, 4, (H, W, 3)), axis=1) + 128, 0, 255)
        b_cur = np.clip(b_prev + np.cumsum(rng.integers(-1, 2, (H, W, 3)), axis=0), 0, 255)
        a_prev = np.clip(b_prev + rng.integers(-2, 3, (H, W, 3)), 0, 255)
        a_cur = np.clip(b_cur + rng.integers(-2, 3, (H, W, 3)), 0, 255)
    else:
        b_prev, b_cur = rng.integers(0, 256, (H, W, 3)), rng.integers(0, 256, (H, W, 3))
        a_prev = np.clip(b_prev + rng.integers(-12, 13, (H, W, 3)), 0, 255)
        a_cur = np.clip(b_cur + rng.integers(-12, 13, (H, W, 3)), 0, 255)
    return tuple(t.astype(np.uint8) for t in (a_cur, a_prev, b_cur, b_prev))


_memo = {}


def make_case(kind, H, W, seed=1):
    """-> dict(images=(a_cur, a_prev, b_cur, b_prev), f, b, fa, row): the inputs (read-only) and the float64 row of the whole
    frame, computed once per process.  Asserts the condition the tests' equalities rest on: no inside pixel's validity test
    is closer to equality than MIN_MARGIN (two float64 evaluations differ by ~1e-15), so n_valid is unambiguous."""
    key = (kind, H, W, seed)
    if key not in _memo:
        images = make_images(kind, H, W, seed)
        f, b, fa = make_flows(H, W, seed)
        for t in images + (f, b, fa):
            t.setflags(write=False)
        m = margin(*images, f, b)
        assert m.size and np.abs(m).min() >= MIN_MARGIN, ("choose another seed", key, float(np.abs(m).min()) if m.size else None)
        _memo[key] = dict(images=images, f=f, b=b, fa=fa, row=tuple(reference_row(*images, f, b, fa)))
    return _memo[key]


def check_margin(images, f, b):
    """the same condition for inputs a test builds itself (hostile flows)"""
    m = margin(*images, f, b)
    assert m.size and np.abs(m).min() >= MIN_MARGIN, float(np.abs(m).min()) if m.size else None
