"""Every stage kernel of the Winograd F(4x4,3x3), F(2x2,3x3) and polyphase F(4,2) pipelines against float64, one stage at a
time, at a shape proven -- by the profiler, in the same test -- to select it.  The cases, references and bounds live in
tests/kernel_variants.py (PIPE_CASES); tests/test_cpu_kernel_variants.py checks the transform matrices and that the references
see the faults they are meant to catch.

Per case:
  * workspace, outputs and side outputs start as NaN; the stage runs on its own (its inputs made by the earlier stages first,
    outside the profiled window) under torch.profiler, and exactly the expected instantiations of PIPE_FAMILIES run;
  * the stage's input and output are read out of the workspace (V [pos][T][Cin], then M [pos][T][Cout]; the weight gradient's
    V [36][batch Tp][x_cs], Md [36][batch Tp][Cout], dU [36][Cout_p][Kp]; the data gradient's dV [36][Tp][x_cs], then the
    padded map), the float64 reference is formed from the fp32 values the kernel read, and |got - ref| <= bound elementwise;
    a failure names the worst ratio and its [pos, tile, channel] index;
  * padding rows and padding channels the stage writes are exactly 0, no real element stays NaN, and statistics partials go
    through instance_norm_finalize within stats_bounds.
The large float64 GEMM references run on the device."""
import pytest
import torch
import torch.nn.functional as F

import kernel_variants as kv

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _dev():
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return torch.device("cuda:0")


def _profiled(fn):
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {kv.normalise(e.name) for e in prof.events() if "t2v::" in e.name}


def _check(what, got, ref, bnd):
    """elementwise |got - ref| <= bnd; NaN anywhere fails; the message names the worst element"""
    got, ref, bnd = got.double(), ref.double().to(got.device), bnd.double().to(got.device)
    assert got.shape == ref.shape == bnd.shape, (what, got.shape, ref.shape, bnd.shape)
    nan = ~torch.isfinite(got)
    assert not nan.any(), "%s: %d elements left unwritten / not finite, first at %s" % (
        what, int(nan.sum()), [int(i) for i in torch.nonzero(nan)[0]])
    ratio = (got - ref).abs() / bnd
    worst = ratio.max().item()
    at = [int(i) for i in torch.nonzero(ratio == ratio.max())[0]]
    print("%s: worst |got - ref| / bound %.3g at %s" % (what, worst, at))
    assert worst <= 1.0, "%s: worst |got - ref| / bound = %.3g at index %s (got %.9g, ref %.9g, bound %.3g)" % (
        what, worst, at, got[tuple(at)].item(), ref[tuple(at)].item(), bnd[tuple(at)].item())
    return worst


def _rand(g, *shape, scale=1.0, offset=0.0):
    return torch.randn(*shape, generator=g) * scale + offset


SLOPE = 0.2       # the LeakyReLU slope of the "lrelu" output case


def _desc(ops, c):
    if c.algo in ("down", "up"):
        return ops.conv_desc(c.H, c.W, c.Cin, c.Cout, 3, 2, 1, ops.PAD_ZERO, c.algo == "up", algo=ops.ALGO_POLYPHASE)
    lrelu = "lrelu" in c.opts
    return ops.conv_desc(c.H, c.W, c.Cin, c.Cout, 3, 1, c.pad, ops.PAD_REFLECT if c.reflect else ops.PAD_ZERO,
                         act=ops.ACT_LRELU if lrelu else ops.ACT_NONE, act_scale=SLOPE if lrelu else 1.0,
                         algo=ops.ALGO_WINOGRAD_F4 if c.algo == "F4" else ops.ALGO_WINOGRAD)


def _geometry(c):
    """positions P, real tiles per image T, rows per position Tt, TH, TW, Ho, Wo, output matrix A"""
    if c.algo in ("down", "up"):
        up = c.algo == "up"
        TH, TW = (-(-c.H // 4), -(-c.W // 4)) if up else (-(-(c.H // 2) // 4), -(-(c.W // 2) // 4))
        Ho, Wo = (2 * c.H, 2 * c.W) if up else (c.H // 2, c.W // 2)
        T = TH * TW
        return 81, T, kv.pad_tiles(T), TH, TW, Ho, Wo, kv.PP["kAU" if up else "kAD"]
    m = 4 if c.algo == "F4" else 2
    Ho, Wo = c.H + 2 * c.pad - 2, c.W + 2 * c.pad - 2
    TH, TW = -(-Ho // m), -(-Wo // m)
    T = TH * TW
    Tt = kv.pad_tiles(c.nimg * T) if c.nimg > 1 else kv.pad_tiles(T)
    return (m + 2) ** 2, T, Tt, TH, TW, Ho, Wo, (kv.F4 if m == 4 else kv.F2)["kAT"]


def _weight(g, c):
    """torch-layout weight: [Cout][Cin][3][3], ConvTranspose2d's [Cin][Cout][3][3] for "up" """
    shape = (c.Cin, c.Cout, 3, 3) if c.algo == "up" else (c.Cout, c.Cin, 3, 3)
    return _rand(g, *shape, scale=(9 * c.Cin) ** -0.5)


def _norm_inputs(g, c):
    """per-image (mean, rstd) table with mean != 0, gamma / beta (beta != 0) if "affine", residual if "res" """
    mr = torch.stack([_rand(g, c.nimg, c.Cin, scale=0.5, offset=0.3), torch.rand(c.nimg, c.Cin, generator=g) + 0.5], -1)
    gm = _rand(g, c.Cin, scale=0.5, offset=1.0) if "affine" in c.opts else None
    bt = _rand(g, c.Cin, scale=0.5, offset=0.2) if "affine" in c.opts else None
    res = _rand(g, c.nimg, c.H, c.W, c.Cin) if "res" in c.opts else None
    return mr, gm, bt, res


def _run_forward(ops, c, desc, x, pu, b, ws, y, stats, stages, lazy):
    """one forward call: the plain staged entry for one image without a norm, the batch entry otherwise"""
    if lazy is None and c.nimg == 1:
        return ops.conv2d_winograd(x[0], pu, b, desc, stats=stats, out=y[0], workspace=ws, stages=stages)
    mr, gm, bt, res, xout = lazy if lazy is not None else (None,) * 5
    return ops.conv2d_winograd_batch(x, pu, b, desc, ws, stats=stats, out=y, stages=stages, mean_rstd=mr, gamma=gm, beta=bt,
                                     relu=int("relu" in c.opts), res=res, xout=xout)


def _forward_case(c, t2v_env):
    from text2video_amd import ops
    dev = _dev()
    for k, v in c.env:
        t2v_env(k, v)
    g = torch.Generator().manual_seed(11)
    desc = _desc(ops, c)
    P, T, Tt, TH, TW, Ho, Wo, A = _geometry(c)
    x = _rand(g, c.nimg, c.H, c.W, c.Cin, offset=0.25)
    w, b = _weight(g, c), _rand(g, c.Cout, scale=0.1)
    xd, bd = x.to(dev), b.to(dev)
    pu = ops.pack_conv_weight(w.to(dev), desc, c.Cin)
    ws = ops.winograd_batch_workspace(desc, c.Cin, c.nimg, dev).fill_(NAN)
    y = torch.full((c.nimg, Ho, Wo, c.Cout), NAN, device=dev)
    lazy = None
    if "relu" in c.opts or "res" in c.opts or "affine" in c.opts:
        mr, gm, bt, res = _norm_inputs(g, c)
        xout = torch.full_like(xd, NAN) if res is not None else None
        lazy = (mr.to(dev).contiguous(), None if gm is None else gm.to(dev), None if bt is None else bt.to(dev),
                None if res is None else res.to(dev), xout)
    nv, nm = P * Tt * c.Cin, P * Tt * c.Cout
    V, M = ws[:nv].view(P, Tt, c.Cin), ws[nv:nv + nm].view(P, Tt, c.Cout)
    rows = c.nimg * T
    hint = "hint" in c.opts
    old_hint = ops.set_overlap_hint(1) if hint else None
    try:
        stages = {"input": 1, "gemm": 2, "output": 4}[c.stage]
        if stages > 1:
            _run_forward(ops, c, desc, xd, pu, bd, ws, y, None, stages - 1 if stages == 2 else 3, lazy)
            torch.cuda.synchronize()
            (M if stages == 2 else y).fill_(NAN)
        stats = None
        if "stats" in c.opts:
            n_st = ops.conv_stats_buffer(desc, dev).numel()
            stats = torch.full((c.nimg * n_st,), NAN, device=dev)
        ran = _profiled(lambda: _run_forward(ops, c, desc, xd, pu, bd, ws, y, stats, stages, lazy))
    finally:
        if hint:
            ops.set_overlap_hint(old_hint)
    got = {n for n in ran if kv.family(n) in kv.PIPE_FAMILIES}
    assert got == set(c.expect), "expected %s, ran %s" % (list(c.expect), sorted(ran))

    if c.stage == "input":
        Vc = V.double().cpu()
        for i in range(c.nimg):
            d = e_d = None
            if lazy is not None:
                d, e_d = kv.lazy_d64(x[i], lazy[0][i].cpu(), None if lazy[1] is None else lazy[1].cpu(),
                                     None if lazy[2] is None else lazy[2].cpu(), "relu" in c.opts,
                                     None if lazy[3] is None else lazy[3][i].cpu())
                if lazy[4] is not None:     # mode 2: the side output is the block output norm(x) + res, every pixel written
                    _check("%s xout[%d]" % (c.id, i), lazy[4][i].cpu(), d, e_d)
            if c.algo in ("down", "up"):
                up = c.algo == "up"
                ref, _, _ = kv.polyphase_input64(x[i].double(), c.H, c.W, up, d=d)
                aab, _, _ = kv.polyphase_input64(x[i].double().abs(), c.H, c.W, up, d=None if d is None else d.abs(),
                                                 absolute=True)
                ed = None if e_d is None else kv.polyphase_input64(e_d, c.H, c.W, up, absolute=True)[0]
                n = kv.nnz_rows(kv.PP["kBU" if up else "kBD"])
            else:
                BT = (kv.F4 if c.algo == "F4" else kv.F2)["kBT"]
                m = 4 if c.algo == "F4" else 2
                ref, _, _ = kv.wino_input64(x[i].double(), c.H, c.W, c.pad, c.reflect, m=m, BT=BT, d=d)
                aab, _, _ = kv.wino_input64(x[i].double().abs(), c.H, c.W, c.pad, c.reflect, m=m, BT=BT.abs(),
                                            d=None if d is None else d.abs())
                ed = None if e_d is None else kv.wino_input64(e_d, c.H, c.W, c.pad, c.reflect, m=m, BT=BT.abs())[0]
                n = kv.nnz_rows(BT)
            r0 = i * (T if c.nimg > 1 else 0)
            _check("%s V[pos, tile, c] image %d" % (c.id, i), Vc[:, r0:r0 + T], ref, kv.input_bound(aab, n, ed))
        assert (Vc[:, rows:] == 0).all(), "%s: V padding rows [%d, %d) must be exactly 0" % (c.id, rows, Tt)
    elif c.stage == "gemm":
        Ub = pu.view(P, -1, c.Cin)[:, :c.Cout]
        ref = kv.gemm64(V[:, :rows], Ub)
        _check("%s M[pos, tile, n]" % c.id, M[:, :rows], ref, kv.gemm_bound(V[:, :rows], Ub, c.Cin))
    else:
        Mc = M.double().cpu()
        n_st = ops.conv_stats_buffer(desc, dev).numel()
        for i in range(c.nimg):
            r0 = i * T
            ref, aab = kv.output64(Mc[:, r0:r0 + T], A, TH, TW, Ho, Wo, b)
            slope = SLOPE if "lrelu" in c.opts else None
            bnd = kv.output_bound(aab, kv.nnz_rows(A), slope)
            if slope is not None:
                ref = kv.leaky64(ref, slope)
                assert (ref < 0).any() and (ref > 0).any(), "%s: both branches of the activation" % c.id
            _check("%s y[y, x, n] image %d" % (c.id, i), y[i].cpu(), ref, bnd)
            if stats is not None:
                mr = ops.instance_norm_finalize(stats[i * n_st:(i + 1) * n_st], desc).view(-1, 2).double().cpu()
                parts = n_st // (2 * c.Cout)
                m_, s_, e_m, e_s = kv.stats_bounds(ref.permute(2, 0, 1), bnd.permute(2, 0, 1), parts)
                _check("%s mean image %d" % (c.id, i), mr[:, 0], m_, e_m)
                _check("%s rstd image %d" % (c.id, i), mr[:, 1], s_, e_s)


def _weight_case(c):
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(12)
    if c.stage == "weight_adjoint":       # the data-gradient conv (zero pad 2) of a Cout -> Cin layer: w [Cin][Cout][3][3]
        desc = ops.conv_desc(c.H, c.W, c.Cin, c.Cout, 3, 1, 2, ops.PAD_ZERO, algo=ops.ALGO_WINOGRAD_F4)
        w = _rand(g, c.Cin, c.Cout, 3, 3)
        out = {}
        ran = _profiled(lambda: out.setdefault("u", ops.pack_conv_weight(w.to(dev), desc, c.Cin, adjoint=True)))
        rows, K, ref = c.Cout, c.Cin, kv.weight64(w, kv.F4["kG"], transposed_layout=True, flip=True)
        aab = kv.weight64(w.abs(), kv.F4["kG"].abs(), transposed_layout=True, flip=True)
        P = 36
    elif c.stage == "weight_transposed":   # U^T of the forward layer: rows its Cin, K its Cout
        desc = ops.conv_desc(c.H, c.W, c.Cin, c.Cout, 3, 1, 1, ops.PAD_REFLECT, algo=ops.ALGO_WINOGRAD_F4)
        assert ops.backward_data_winograd_supported(desc, c.Cin, c.Cout)
        w = _rand(g, c.Cout, c.Cin, 3, 3)
        out = {}
        ran = _profiled(lambda: out.setdefault("u", ops.pack_conv_weight_transposed(w.to(dev), desc, c.Cin)))
        rows, K, ref = c.Cin, c.Cout, kv.weight64(w, kv.F4["kG"], transposed_layout=True)
        aab = kv.weight64(w.abs(), kv.F4["kG"].abs(), transposed_layout=True)
        P = 36
    else:
        desc = _desc(ops, c)
        w = _weight(g, c)
        out = {}
        ran = _profiled(lambda: out.setdefault("u", ops.pack_conv_weight(w.to(dev), desc, c.Cin)))
        G = kv.PP["kGU"] if c.algo == "up" else kv.PP["kGD"] if c.algo == "down" else (kv.F4 if c.algo == "F4" else kv.F2)["kG"]
        up = c.algo == "up"
        rows, K, ref = c.Cout, c.Cin, kv.weight64(w, G, transposed_layout=up)
        aab = kv.weight64(w.abs(), G.abs(), transposed_layout=up)
        P = G.shape[0] ** 2
    got = {n for n in ran if kv.family(n) in kv.PIPE_FAMILIES}
    assert got == set(c.expect), "expected %s, ran %s" % (list(c.expect), sorted(ran))
    u = out["u"].double().cpu()
    Ks = K if c.stage != "weight_transposed" else -(-K // 32) * 32
    u = u.view(P, -1, Ks)
    bnd = kv.weight_bound_f2(aab) if c.algo == "F2" else kv.weight_bound(ref, aab)
    _check("%s U[pos, n, c]" % c.id, u[:, :rows, :K], ref, bnd)
    assert (u[:, rows:] == 0).all() and (u[:, :, K:] == 0).all(), "%s: padding rows / channels of U must be 0" % c.id


def _wgrad_common(ops, c, dev):
    desc = ops.conv_desc(c.H, c.W, c.Cin, c.Cout, 3, 1, 1, ops.PAD_REFLECT, algo=ops.ALGO_WINOGRAD_F4)
    assert ops.backward_weight_winograd_supported(desc, c.Cin, c.Cout)
    Tp = kv.pad_tiles(-(-c.H // 4) * -(-c.W // 4))
    Tt = c.batch * Tp
    ws = ops.backward_weight_winograd_workspace(desc, c.Cin, c.batch, dev).fill_(NAN)
    nv, nm = 36 * Tt * c.Cin, 36 * Tt * c.Cout
    return desc, Tp, Tt, ws, ws[:nv].view(36, Tt, c.Cin), ws[nv:nv + nm].view(36, Tt, c.Cout), nv + nm


def _dy_case(c):
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(13)
    desc, Tp, Tt, ws, V, Md, _ = _wgrad_common(ops, c, dev)
    Ho, Wo = c.H, c.W
    T = -(-Ho // 4) * -(-Wo // 4)
    dy = _rand(g, Ho, Wo, c.Cout)
    e_front = None
    if c.stage == "dy":
        ran = _profiled(lambda: ops.conv2d_backward_weight_winograd_dy(dy.to(dev), desc, ws, c.batch, c.slot, c.Cin))
        d64 = dy.double()
    else:
        xo = _rand(g, Ho, Wo, c.Cout, offset=0.3)
        mr = torch.stack([_rand(g, c.Cout, scale=0.2, offset=0.3), torch.rand(c.Cout, generator=g) + 0.5], -1)
        gm = _rand(g, c.Cout, scale=0.5, offset=1.0) if "affine" in c.opts else None
        bt = _rand(g, c.Cout, scale=0.5, offset=0.2) if "affine" in c.opts else None
        sums = _rand(g, c.Cout, 2, scale=float(Ho * Wo) ** 0.5)
        relu = 1 if "relu" in c.opts else 0
        todev = lambda t: None if t is None else t.to(dev).contiguous()
        ran = _profiled(lambda: ops.conv2d_backward_weight_winograd_dy_norm(
            todev(xo), todev(dy), todev(mr), todev(gm), todev(bt), relu, todev(sums), desc, ws, c.batch, c.slot, c.Cin))
        d64, e_front = kv.dy_front64(dy, xo, mr, gm, bt, relu, sums, Ho * Wo)
    got = {n for n in ran if kv.family(n) in kv.PIPE_FAMILIES}
    assert got == set(c.expect), "expected %s, ran %s" % (list(c.expect), sorted(ran))
    ref, aab = kv.dy64(d64, Ho, Wo)
    ed = None if e_front is None else kv.dy64(e_front, Ho, Wo)[1]
    Mc = Md.double().cpu()
    r0 = c.slot * Tp
    _check("%s Md[pos, tile, n]" % c.id, Mc[:, r0:r0 + T], ref, kv.dy_bound(aab, ed))
    assert (Mc[:, r0 + T:r0 + Tp] == 0).all(), "%s: padding rows of the slot must be exactly 0" % c.id
    others = torch.cat([Mc[:, :r0], Mc[:, r0 + Tp:]], 1)
    assert torch.isnan(others).all(), "%s: rows of other slots written" % c.id
    assert torch.isnan(V.cpu()).all(), "%s: V written by the dy transform" % c.id


def _wgrad_case(c, t2v_env):
    from text2video_amd import ops
    dev = _dev()
    for k, v in c.env:
        t2v_env(k, v)
    g = torch.Generator().manual_seed(14)
    desc, Tp, Tt, ws, V, Md, du0 = _wgrad_common(ops, c, dev)
    x = _rand(g, c.batch, c.H, c.W, c.Cin).to(dev)
    dy = _rand(g, c.batch, c.H, c.W, c.Cout).to(dev)
    ops.conv2d_backward_weight_winograd_stages(x, dy, desc, ws, c.batch, 0, reduce=False)
    torch.cuda.synchronize()
    ws[du0:].fill_(NAN)
    out = {}
    ran = _profiled(lambda: out.setdefault("dw", ops.conv2d_backward_weight_winograd_reduce(desc, ws, c.batch, c.Cin, c.Cout)))
    got = {n for n in ran if kv.family(n) in kv.PIPE_FAMILIES}
    assert got == set(c.expect), "expected %s, ran %s" % (list(c.expect), sorted(ran))
    Cout_p, Kp = -(-c.Cout // 128) * 128, -(-c.Cin // 32) * 32
    dU = ws[du0:du0 + 36 * Cout_p * Kp].view(36, Cout_p, Kp)[:, :c.Cout, :c.Cin]
    assert torch.isfinite(V).all() and torch.isfinite(Md).all()
    # V of each image, written by winograd4_input_kernel<0, *> in its slot of the batch-wide tile list
    T = -(-c.H // 4) * -(-c.W // 4)
    Vc, n4 = V.double().cpu(), kv.nnz_rows(kv.F4["kBT"])
    for i in range(c.batch):
        xi = x[i].double().cpu()
        ref_v, _, _ = kv.wino_input64(xi, c.H, c.W, 1, True)
        aab = kv.wino_input64(xi.abs(), c.H, c.W, 1, True, BT=kv.F4["kBT"].abs())[0]
        _check("%s V[pos, tile, c] slot %d" % (c.id, i), Vc[:, i * Tp:i * Tp + T], ref_v, kv.input_bound(aab, n4))
        assert (Vc[:, i * Tp + T:(i + 1) * Tp] == 0).all(), "%s: V padding rows of slot %d must be exactly 0" % (c.id, i)
    MdT = Md.transpose(1, 2)
    ref = kv.gemm64(MdT, V.transpose(1, 2))             # dU[xi][n][c] = sum_t Md[xi][t][n] V[xi][t][c]
    _check("%s dU[pos, n, c]" % c.id, dU, ref, kv.gemm_bound(MdT, V.transpose(1, 2), Tt))
    r64, a64 = kv.dw64(dU.double())
    _check("%s dw[n, c, i, j]" % c.id, out["dw"], r64, kv.weight_bound(r64, a64))


def _dgrad_case(c, t2v_env):
    from text2video_amd import ops
    dev = _dev()
    for k, v in c.env:
        t2v_env(k, v)
    g = torch.Generator().manual_seed(15)
    desc, Tp, Tt, ws, V, Md, _ = _wgrad_common(ops, c, dev)
    assert ops.backward_data_winograd_supported(desc, c.Cin, c.Cout)
    fw = "fw" in c.opts
    if fw:
        assert ops.backward_data_winograd_takes_forward_weights(desc, c.Cin, c.Cout)
    TH, TW = c.H // 4, c.W // 4
    T = TH * TW
    w = _rand(g, c.Cout, c.Cin, 3, 3, scale=(9 * c.Cout) ** -0.5).to(dev)
    dy = _rand(g, c.H, c.W, c.Cout).to(dev)
    ops.conv2d_backward_weight_winograd_dy(dy, desc, ws, c.batch, c.slot, c.Cin)
    if fw:
        ut = ops.pack_conv_weight(w, ops.with_algo(desc, ops.ALGO_WINOGRAD_F4), c.Cin)
        B = ut.view(36, c.Cout, c.Cin).transpose(1, 2)                 # [K = Cout][N = Cin] read as B
    else:
        ut = ops.pack_conv_weight_transposed(w, desc, c.Cin)
        B = ut.view(36, -(-c.Cin // 128) * 128, -(-c.Cout // 32) * 32)[:, :c.Cin, :c.Cout]
    scratch = ops.backward_data_winograd_scratch(desc, c.Cin, dev).fill_(NAN)
    torch.cuda.synchronize()
    out = {}
    ran = _profiled(lambda: out.setdefault("dx", ops.conv2d_backward_data_winograd(desc, c.batch, c.slot, ws, c.Cin, ut,
                                                                                   forward_weights=fw, scratch=scratch)))
    got = {n for n in ran if kv.family(n) in kv.PIPE_FAMILIES}
    assert got == set(c.expect), "expected %s, ran %s" % (list(c.expect), sorted(ran))
    nv = 36 * Tp * c.Cin
    dV = scratch[:nv].view(36, Tp, c.Cin)
    dxp = scratch[nv:nv + (c.H + 2) * (c.W + 2) * c.Cin].view(c.H + 2, c.W + 2, c.Cin)
    A = Md[:, c.slot * Tp:c.slot * Tp + T]
    _check("%s dV[pos, tile, c]" % c.id, dV[:, :T], kv.gemm64(A, B), kv.gemm_bound(A, B, c.Cout))
    ref, aab = kv.dgrad_output64(dV[:, :T].double(), TH, TW)
    _check("%s dxp[y, x, c]" % c.id, dxp, ref, kv.dgrad_output_bound(aab))
    # the reflect-pad adjoint folds dxp into dx: <= 4 terms per pixel, 3 roundings
    fold, fold_a = kv.reflect_fold(dxp.double()), kv.reflect_fold(dxp.double().abs())
    _check("%s dx[y, x, c]" % c.id, out["dx"], fold, kv.gamma(3) * fold_a + 3 * kv.TINY)


@pytest.mark.parametrize("case", kv.PIPE_CASES, ids=[c.id for c in kv.PIPE_CASES])
def test_pipeline_stage_against_float64(case, t2v_env):
    if case.stage in ("input", "gemm", "output"):
        _forward_case(case, t2v_env)
    elif case.stage.startswith("weight"):
        _weight_case(case)
    elif case.stage in ("dy", "dy_norm"):
        _dy_case(case)
    elif case.stage == "wgrad":
        _wgrad_case(case, t2v_env)
    else:
        assert case.stage == "dgrad", case.stage
        _dgrad_case(case, t2v_env)


def _dgrad_end_to_end(H, W, Cin, Cout):
    """ops.conv2d_backward_data_winograd's dx against autograd's input gradient of the ReflectionPad(1) conv in float64,
    under dgrad_bound(): A dy A^T, the GEMM with U^T, the scatter and the reflect-pad fold, all in one"""
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(17)
    desc = ops.conv_desc(H, W, Cin, Cout, 3, 1, 1, ops.PAD_REFLECT, algo=ops.ALGO_WINOGRAD_F4)
    assert ops.backward_data_winograd_supported(desc, Cin, Cout)
    w = _rand(g, Cout, Cin, 3, 3, scale=(9 * Cout) ** -0.5)
    dy = _rand(g, H, W, Cout)
    ws = ops.backward_weight_winograd_workspace(desc, Cin, 1, dev).fill_(NAN)
    ops.conv2d_backward_weight_winograd_dy(dy.to(dev), desc, ws, 1, 0, Cin)
    dx = ops.conv2d_backward_data_winograd(desc, 1, 0, ws, Cin, ops.pack_conv_weight_transposed(w.to(dev), desc, Cin)).cpu()
    x0 = torch.zeros(1, Cin, H, W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(x0, (1,) * 4, mode="reflect"), w.double())
    (ref,) = torch.autograd.grad(y, x0, dy.double().permute(2, 0, 1)[None])
    ref = ref[0].permute(1, 2, 0)
    _check("F4_dgrad end to end dx[y, x, c]", dx, ref, kv.dgrad_bound(dy, w) + 2.0 ** -40 * ref.abs())


def _wgrad_end_to_end(H, W, Cin, Cout):
    """the dw of conv2d_backward_weight_winograd_stages against autograd's weight gradient of the ReflectionPad(1) conv in
    float64, under wgrad_bound(): a batch of two images through V, A dy A^T, the reduction over tiles and G^T dU G"""
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(18)
    B = 2
    desc = ops.conv_desc(H, W, Cin, Cout, 3, 1, 1, ops.PAD_REFLECT, algo=ops.ALGO_WINOGRAD_F4)
    x, dy = _rand(g, B, H, W, Cin), _rand(g, B, H, W, Cout)
    ws = ops.backward_weight_winograd_workspace(desc, Cin, B, dev).fill_(NAN)
    dw = ops.conv2d_backward_weight_winograd_stages(x.to(dev), dy.to(dev), desc, ws, B, 0, reduce=True).cpu()
    w0 = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(x.double().permute(0, 3, 1, 2), (1,) * 4, mode="reflect"), w0)
    (ref,) = torch.autograd.grad(y, w0, dy.double().permute(0, 3, 1, 2))
    Tp = kv.pad_tiles(-(-H // 4) * -(-W // 4))
    _check("F4_wgrad end to end dw[n, c, i, j]", dw, ref, kv.wgrad_bound(x, dy, Tp) + 2.0 ** -40 * ref.abs())


@pytest.mark.parametrize("algo,H,W,Cin,Cout", kv.E2E_CASES, ids=[e[0] for e in kv.E2E_CASES])
def test_pipeline_end_to_end_against_float64(algo, H, W, Cin, Cout):
    """the whole pipeline against F.conv2d / conv_transpose2d / autograd in float64 under pipeline_bound() (the data and weight
    gradients: dgrad_bound(), wgrad_bound()): a wrong transform matrix or adjoint (which the stage cases, each checked
    against the header's own matrices, cannot see) shows here"""
    if algo == "F4_dgrad":
        return _dgrad_end_to_end(H, W, Cin, Cout)
    if algo == "F4_wgrad":
        return _wgrad_end_to_end(H, W, Cin, Cout)
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(16)
    c = kv._pc("e2e", "e2e", algo, H, W, Cin, Cout, ())
    desc = _desc(ops, c)
    x = _rand(g, H, W, Cin)
    w, b = _weight(g, c), _rand(g, Cout, scale=0.1)
    pu = ops.pack_conv_weight(w.to(dev), desc, Cin)
    y = ops.conv2d_winograd(x.to(dev), pu, b.to(dev), desc).cpu()
    xd = x.permute(2, 0, 1)[None].double()
    if algo == "up":
        ref = F.conv_transpose2d(xd, w.double(), b.double(), stride=2, padding=1, output_padding=1)
    elif algo == "down":
        ref = F.conv2d(xd, w.double(), b.double(), stride=2, padding=1)
    else:
        ref = F.conv2d(F.pad(xd, (1,) * 4, mode="reflect"), w.double(), b.double())
    ref = ref[0].permute(1, 2, 0)
    bnd = kv.pipeline_bound(x, w, b, algo) + 2.0 ** -40 * ref.abs()
    _check("%s end to end y[y, x, n]" % algo, y, ref, bnd)
