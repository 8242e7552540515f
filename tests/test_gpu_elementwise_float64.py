"""The elementwise kernels of csrc/elementwise.hip against float64, at their edges: norm apply (single, in place, batch, the
encoder join and add_kernel), the three norm-backward kernels, the flow-warp compositor and its adjoint, the 3x3/s2 average
pool, act_backward and the masked-L1 / loss backward kernels.  The cases, the float64 references, the bounds (each derived from
the kernel's arithmetic, none fitted) and the buffers' extents live in tests/elementwise_reference.py;
tests/test_cpu_elementwise_reference.py checks them without a GPU.  Every test prints its worst |error| / bound
(profiles/elementwise_float64.txt keeps them); where ops takes out=, the output sits between NaN margins that must stay NaN."""
import pytest
import torch

import elementwise_reference as er
import kernel_variants as kv
from test_gpu_kernel_variants import _dev, _launch_profiled

pytestmark = pytest.mark.gpu

_ids = lambda cases: [c.id for c in cases]


def _report(case, what, err, bnd):
    r = er.worst(err, bnd)
    print("elementwise %-34s %-22s worst |got - ref| / bound %.3g" % (case.id if hasattr(case, "id") else case, what, r))
    return r


def _inside(case, what, got, ref, bnd):
    assert torch.isfinite(got).all(), "%s %s: output left unwritten (NaN poison)" % (case.id, what)
    err = (got.double() - ref).abs()
    r = _report(case, what, err, bnd)
    assert r <= 1.0, "%s %s: worst |got - ref| / bound = %.3g (max |got - ref| %.3g)" % (case.id, what, r, err.max().item())


def _side(t, tag):
    return tuple(t[tag + "_" + k] for k in ("y", "mean_rstd", "gamma", "beta", "res"))


# ---- norm apply ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.APPLY_CASES, ids=_ids(er.APPLY_CASES))
def test_norm_apply_against_float64(case):
    from text2video_amd import ops
    dev, p = _dev(), case.p
    t = er.build_case(case, dev)
    x, mr, nimg = t["x"], t["mean_rstd"], p["nimg"]
    assert all(v is None or v.numel() >= er.extents(case)[k] for k, v in t.items())
    buf, out = er.nan_margin(x.numel(), dev)
    out = out.view(x.shape)
    if nimg == 1:
        call = lambda: ops.instance_norm_apply(x[0], mr[0], t["gamma"], t["beta"], None if t["res1"] is None else t["res1"][0],
                                               None if t["res2"] is None else t["res2"][0], p["relu"], out=out[0])
    else:
        call = lambda: ops.instance_norm_apply(x, mr, t["gamma"], t["beta"], t["res1"], t["res2"], p["relu"], out=out, nimg=nimg)
    ran = _launch_profiled(call)
    assert "t2v::inorm_apply_kernel" in ran, sorted(ran)
    assert er.margins_untouched(buf), "%s: a NaN margin was written" % case.id
    ref, bnd = er.apply64(x, mr, t["gamma"], t["beta"], p["relu"], t["res1"], t["res2"])
    _inside(case, "y", out, ref, bnd)
    if nimg > 1:       # the batch form: image i with table i, the bits of the single call
        for i in range(nimg):
            one = ops.instance_norm_apply(x[i], mr[i], t["gamma"], t["beta"], t["res1"][i], t["res2"][i], p["relu"])
            assert torch.equal(one, out[i]), "image %d of the batch differs from its single call" % i
    if case.id in er.INPLACE_IDS:      # out = x, as the discriminator and conv_norm_act call it
        xc = x[0].clone()
        got = ops.instance_norm_apply(xc, mr[0], t["gamma"], t["beta"], None if t["res1"] is None else t["res1"][0],
                                      None if t["res2"] is None else t["res2"][0], p["relu"], out=xc)
        assert got.data_ptr() == xc.data_ptr() and torch.equal(xc, out[0]), "%s: in place differs from out of place" % case.id


@pytest.mark.parametrize("case", er.JOIN_CASES, ids=_ids(er.JOIN_CASES))
def test_norm_join_is_two_applies_and_an_add(case):
    from text2video_amd import ops
    dev, p = _dev(), case.p
    t = er.build_case(case, dev)
    a, b = _side(t, "a"), _side(t, "b")
    buf, out = er.nan_margin(a[0].numel(), dev)
    out = out.view(a[0].shape)
    ran = _launch_profiled(lambda: ops.instance_norm_join(a, b, nimg=p["nimg"], out=out))
    assert "t2v::inorm_apply_kernel" in ran and "t2v::add_kernel" not in ran, sorted(ran)
    assert er.margins_untouched(buf)
    sa = ops.instance_norm_apply(a[0], a[1], a[2], a[3], res1=a[4], nimg=p["nimg"])
    sb = ops.instance_norm_apply(b[0], b[1], b[2], b[3], res1=b[4], nimg=p["nimg"])
    sbuf, two = er.nan_margin(sa.numel(), dev)
    two = two.view(sa.shape)
    ran = _launch_profiled(lambda: ops.add(sa, sb, out=two))
    assert "t2v::add_kernel" in ran, sorted(ran)
    assert er.margins_untouched(sbuf)
    assert torch.equal(two, sa + sb), "add_kernel is one fp32 addition"
    ref, bnd = er.add64(sa, sb)
    _inside(case, "add", two, ref, bnd)
    assert torch.equal(out, two), "%s: the join differs from add(apply(a), apply(b)) at %d places" % (case.id, (out != two).sum())
    ref, bnd = er.join64(a, b)
    _inside(case, "join", out, ref, bnd)


def test_add_strides_past_the_grid_cap():
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    n = er.GRID_CAP * 4 + 2048            # n4 = GRID_CAP + 512
    a, b = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    buf, out = er.nan_margin(n, dev)
    ops.add(a, b, out=out)
    assert er.margins_untouched(buf) and torch.equal(out, a + b)


# ---- norm backward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.NORM_BWD_CASES, ids=_ids(er.NORM_BWD_CASES))
def test_norm_backward_against_float64(case):
    from text2video_amd import ops
    dev, p = _dev(), case.p
    t = er.build_case(case, dev)
    x, dy, mr, ga, be, relu = t["x"], t["dy"], t["mean_rstd"], t["gamma"], t["beta"], p["relu"]
    npix, C = x.shape
    ext = er.extents(case)
    assert ext["scratch"] <= 128 * C * 2 and x.numel() == ext["x"] == ext["dx"]
    buf, out = er.nan_margin(x.numel(), dev)
    out = out.view(x.shape)
    res = {}
    ran = _launch_profiled(lambda: res.setdefault("r", ops.instance_norm_backward(x, dy, mr, ga, be, relu, out=out)))
    assert {"t2v::inorm_bwd_reduce_kernel", "t2v::inorm_bwd_final_kernel", "t2v::inorm_bwd_apply_kernel"} <= ran, sorted(ran)
    dx, sums = res["r"]
    assert dx.data_ptr() == out.data_ptr() and er.margins_untouched(buf), "%s: a NaN margin was written" % case.id
    s64, es = er.bwd_sums64(x, dy, mr, ga, be, relu)
    _inside(case, "sums", sums, s64, es)
    dx64, ed = kv.dy_front64(dy, x, mr, ga, be, relu, sums, npix)          # from the kernel's own fp32 sums
    _inside(case, "dx", dx, dx64, ed)

    # the pinned channel: x == mean bit for bit and beta == 0, so pre == 0 exactly: ReLU' = 0, Leaky' = 0.2 (`pre > 0`)
    c = er.PIN_CH
    r_ga = mr[c, 1].double() * (ga[c].double() if ga is not None else 1.0)
    k0 = (sums[c, 0] * (torch.tensor(1.0, device=dev) / torch.tensor(float(npix), device=dev))).double()
    if relu == 1:
        assert sums[c, 0] == 0 and sums[c, 1] == 0, "ReLU' at pre == 0 must be 0: sums %s" % sums[c].tolist()
        assert (dx[:, c] == 0).all()
    elif relu == 2:
        g = dy[:, c].double() * kv.LEAKY32
        A = g.abs().sum()
        e0 = kv.sum_bound(A, er.bwd_depth(npix, C), npix) + kv.gamma(2) * A          # no `near` slack: the branch is pinned
        assert (sums[c, 0].double() - g.sum()).abs() <= e0 and sums[c, 1] == 0
        want = r_ga * (g - k0)          # xhat == 0: rstd gamma (g - k0); g (1), k0 (2), the difference, the two products
        assert ((dx[:, c].double() - want).abs() <= kv.gamma(6) * r_ga.abs() * (g.abs() + k0.abs()) + 6 * kv.TINY).all()

    # sums_only: the same sums bit for bit, no dx
    dx2, sums2 = ops.instance_norm_backward(x, dy, mr, ga, be, relu, sums_only=True)
    assert dx2 is None and torch.equal(sums2, sums)
    # affine_into: overwrite writes the two sums, accumulate holds fl32(prior + sum)
    for overwrite in (True, False):
        d_beta, d_gamma = t["d_beta"].clone(), t["d_gamma"].clone()
        dx3, sums3 = ops.instance_norm_backward(x, dy, mr, ga, be, relu, affine_into=(d_beta, d_gamma, overwrite))
        assert torch.equal(sums3, sums) and torch.equal(dx3, dx)
        if overwrite:
            assert torch.equal(d_beta, sums[:, 0]) and torch.equal(d_gamma, sums[:, 1])
        else:
            assert torch.equal(d_beta, t["d_beta"] + sums[:, 0]) and torch.equal(d_gamma, t["d_gamma"] + sums[:, 1])


# ---- flow warp ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.WARP_CASES, ids=_ids(er.WARP_CASES))
def test_flow_warp_forward_and_backward_against_float64(case):
    from oracle.generator_ref import resample
    from text2video_amd import ops
    dev, p = _dev(), case.p
    t = er.build_case(case, dev)
    raw, fw, prev, c0, cs = t["raw"], t["fw"], t["prev"], p["c0"], p["cs"]
    H, W = p["H"], p["W"]
    big = H * W > er.GRID_CAP
    ext = er.extents(case)
    assert prev.numel() == ext["prev"] and fw.numel() == ext["fw"] and raw.numel() == ext["raw"] and c0 + 3 <= cs

    w_ref = resample(prev[..., c0:c0 + 3].double().permute(2, 0, 1)[None], fw[..., :2].double().permute(2, 0, 1)[None])[0].permute(1, 2, 0)
    w64, e = er.warp64(prev, c0, fw)
    assert torch.allclose(w64, w_ref, rtol=1e-11, atol=1e-11)
    o64, eo = er.composite64(raw, fw, w_ref, e)
    buf, out = er.nan_margin(raw.numel(), dev)
    out = out.view(raw.shape)
    res = {}
    ran = _launch_profiled(lambda: res.setdefault("r", ops.flow_warp_composite(raw, fw, prev, c0, want_warp=True, out=out)))
    assert "t2v::warp_composite_kernel" in ran, sorted(ran)
    _, warp = res["r"]
    assert er.margins_untouched(buf)
    _inside(case, "composite out", out[..., :3], o64, eo)
    _inside(case, "composite warp", warp[..., :3], w_ref, e)
    assert (out[..., 3] == 0).all() and (warp[..., 3] == 0).all(), "the padding channel must be written as 0"
    if p["flow"] == "zero":      # the identity: the bound is the positional error through the local slope, plus the tap sum
        _inside(case, "identity", warp[..., :3], prev[..., c0:c0 + 3].double(), e)
    if not big:
        wbuf, wout = er.nan_margin(raw.numel(), dev)
        wout = wout.view(raw.shape)
        ops.flow_warp(fw, prev, c0, out=wout)
        assert er.margins_untouched(wbuf) and (wout[..., 3] == 0).all()
        _inside(case, "flow_warp", wout[..., :3], w_ref, e)

    modes = {"composite": (t["d_out"], None, raw)}
    if not big:
        modes["warp_only"] = (None, t["d_warp"], None)
    for mode, (do, dw, rw) in modes.items():
        r = er.warp_backward64(do, dw, rw, fw, prev, c0)
        ran = _launch_profiled(lambda: res.__setitem__("b", ops.flow_warp_composite_backward(do, dw, rw, fw, prev, c0, want_d_prev=True)))
        assert "t2v::warp_composite_backward_kernel" in ran, sorted(ran)
        d_raw, d_fw, d_prev = res["b"]
        assert torch.isfinite(d_fw).all() and torch.isfinite(d_prev).all()
        # the kink rule: inside the bound of one of the admissible one-sided derivatives, every pixel compared
        for k, name in ((0, "d_fx"), (1, "d_fy")):
            rr = _report(case, mode + " " + name, er.closest(d_fw[..., k].double(), r[name]), r["e" + name[1:]])
            assert rr <= 1.0, "%s %s %s: worst ratio %.3g" % (case.id, mode, name, rr)
        assert (d_fw[..., 3] == 0).all()
        _inside(case, mode + " d_prev", d_prev[..., c0:c0 + 3], r["d_prev"], r["e_prev"])
        other = torch.ones(cs, dtype=torch.bool, device=dev)
        other[c0:c0 + 3] = False
        assert (d_prev[..., other] == 0).all(), "d_prev outside [c0, c0 + 3) must stay exactly 0"
        if do is not None:
            _inside(case, mode + " d_w", d_fw[..., 2], r["d_w"], r["e_w"])
            _inside(case, mode + " d_raw", d_raw[..., :3], r["d_raw"], r["e_raw"])
            assert (d_raw[..., 3] == 0).all()
        else:
            assert d_raw is None and (d_fw[..., 2] == 0).all()


# ---- average pool -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.POOL_CASES, ids=_ids(er.POOL_CASES))
def test_avgpool_forward_and_backward_against_float64(case):
    from text2video_amd import ops
    dev, p = _dev(), case.p
    t = er.build_case(case, dev)
    H, W, C = p["H"], p["W"], p["C"]
    ext = er.extents(case)
    assert t["x"].numel() == ext["x"] and t["dy"].numel() == ext["dy"]
    if p["fwd"]:
        res = {}
        ran = _launch_profiled(lambda: res.setdefault("y", ops.avgpool3x3s2(t["x"])))
        assert "t2v::avgpool3s2_kernel" in ran, sorted(ran)
        assert tuple(res["y"].shape) == er.pool_dims(H, W) + (C,) and res["y"].numel() == ext["y"]
        ref, bnd = er.pool64(t["x"])
        _inside(case, "y", res["y"], ref, bnd)
    if p["bwd"]:
        res = {}
        ran = _launch_profiled(lambda: res.setdefault("dx", ops.avgpool3x3s2_backward(t["dy"], H, W)))
        assert "t2v::avgpool3s2_backward_kernel" in ran, sorted(ran)
        ref, bnd = er.pool_backward64(t["dy"], H, W)
        _inside(case, "dx", res["dx"], ref, bnd)


# ---- pointwise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.ACT_CASES, ids=_ids(er.ACT_CASES))
def test_act_backward_against_float64(case):
    from text2video_amd import ops
    dev, p = _dev(), case.p
    t = er.build_case(case, dev)
    assert t["dy"].numel() == t["y"].numel() == er.extents(case)["dpre"] and (p["mode"] != 4 or p["n"] % 4 == 0)
    got = ops.act_backward(t["dy"], t["y"], p["mode"], p["slope"])
    ref, bnd = er.act64(t["dy"], t["y"], p["mode"], p["slope"])
    _inside(case, "dpre", got, ref, bnd)
    if p["mode"] == 4:
        assert (got.view(-1, 4)[:, 3] == 0).all()
    if p["mode"] == 1:
        assert (got[t["y"].abs() == 1] == 0).all(), "tanh' at y = +-1 is exactly 0"


@pytest.mark.parametrize("case", er.ML1_CASES, ids=_ids(er.ML1_CASES))
def test_masked_l1_and_its_backward_against_float64(case):
    from text2video_amd import ops
    dev, p = _dev(), case.p
    t = er.build_case(case, dev)
    a, b, mask, c0, C = t["a"], t["b"], t["mask"], p["c0"], p["C"]
    ext = er.extents(case)
    assert a.numel() == ext["a"] and ext["scratch"] <= 2048 and c0 + C <= p["cs"]
    res = {}
    ran = _launch_profiled(lambda: res.setdefault("s", ops.sum_abs_diff_masked(a, b, mask, c0, C)))
    assert {"t2v::reduce_masked_l1_kernel", "t2v::reduce_final_kernel"} <= ran, sorted(ran)
    ref, bnd = er.ml1_64(a, b, mask, c0, C)
    _inside(case, "sum", res["s"][0], ref, bnd)
    ran = _launch_profiled(lambda: res.setdefault("d", ops.sum_abs_diff_masked_backward(a, b, mask, c0, C, 0.37)))
    assert "t2v::masked_l1_backward_kernel" in ran, sorted(ran)
    want = er.ml1_backward32(a, b, mask, c0, C, 0.37)
    assert torch.equal(res["d"], want), "%s: the backward is exact; differs at %d places" % (case.id, (res["d"] != want).sum())


@pytest.mark.parametrize("case", er.LOSS_BWD_CASES, ids=_ids(er.LOSS_BWD_CASES))
def test_loss_backward_past_the_grid_cap(case):
    from text2video_amd import ops
    dev, p = _dev(), case.p
    t = er.build_case(case, dev)
    res = {}
    if p["op"] == 0:
        ran = _launch_profiled(lambda: res.setdefault("d", ops.sum_sq_diff_const_backward(t["a"], 0.25, 0.37)))
    else:
        ran = _launch_profiled(lambda: res.setdefault("d", ops.sum_abs_diff_backward(t["a"], t["b"], 0.37)))
    assert "t2v::loss_backward_kernel" in ran, sorted(ran)
    ref, bnd = er.loss_backward64(t["a"], t["b"], 0.25, 0.37, p["op"])
    _inside(case, "da", res["d"], ref, bnd)


# ---- what the host refuses before any launch -----------------------------------------------------------------------------------
def test_new_entries_refuse_bad_contracts_on_the_host():
    """only what is refused BEFORE a launch: no shape outside a contract reaches the GPU"""
    from text2video_amd import ops
    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev)
    x, mr, ga = z(2, 6, 8), z(2, 8, 2), z(8)
    with pytest.raises(ValueError):
        ops.instance_norm_apply(z(2, 6, 6), z(2, 6, 2), nimg=2)                       # C % 4
    with pytest.raises(ValueError):
        ops.instance_norm_apply(x, z(8, 2), nimg=2)                                   # one table for two images
    with pytest.raises(ValueError):
        ops.instance_norm_apply(x, mr, res1=z(6, 8), nimg=2)                          # a residual of one image
    with pytest.raises(ValueError):
        ops.instance_norm_apply(x, mr, gamma=ga, nimg=2)                              # gamma without beta
    with pytest.raises(ValueError):
        ops.instance_norm_apply(x, mr, nimg=4)                                        # 2 * 6 pixels are no 4 images
    side = (x, mr, None, None, z(2, 6, 8))
    with pytest.raises(ValueError):
        ops.instance_norm_join(side, (x, mr, ga, None, z(2, 6, 8)), nimg=2)           # gamma without beta
    with pytest.raises(ValueError):
        ops.instance_norm_join(side, (x, z(8, 2), None, None, z(2, 6, 8)), nimg=2)    # a wrong table
    with pytest.raises(ValueError):
        ops.instance_norm_join(side, (x, mr, None, None, None), nimg=2)               # no residual
    with pytest.raises(ValueError):
        ops.instance_norm_join((z(2, 6, 6), z(2, 6, 2), None, None, z(2, 6, 6)), (z(2, 6, 6), z(2, 6, 2), None, None, z(2, 6, 6)), nimg=2)
    with pytest.raises(ValueError):
        ops.add(z(6), z(6))                                                           # n % 4
    with pytest.raises(ValueError):
        ops.add(z(8), z(12))
    # the C entries themselves: a status, nothing launched
    c = ops.context()
    s, P = ops._stream(), ops._p
    y = z(2, 6, 8)
    lib = c.lib
    bad = [
        lib.t2v_add(c.handle, s, P(x), P(x), P(y), 6),
        lib.t2v_add(c.handle, s, P(x), None, P(y), 8),
        lib.t2v_instance_norm_apply_batch(c.handle, s, P(x), P(mr), None, None, None, None, P(y), 6, 6, 0, 2),
        lib.t2v_instance_norm_apply_batch(c.handle, s, P(x), P(mr), None, None, None, None, P(y), 0, 8, 0, 2),
        lib.t2v_instance_norm_apply_batch(c.handle, s, P(x), P(mr), None, None, None, None, P(y), 6, 8, 0, 0),
        lib.t2v_instance_norm_apply_batch(c.handle, s, P(x), P(mr), P(ga), None, None, None, P(y), 6, 8, 0, 2),
        lib.t2v_instance_norm_apply_batch(c.handle, s, P(x), None, None, None, None, None, P(y), 6, 8, 0, 2),
        lib.t2v_instance_norm_join(c.handle, s, P(x), P(mr), None, None, P(y), P(x), P(mr), None, P(ga), P(y), P(y), 6, 8, 2),
        lib.t2v_instance_norm_join(c.handle, s, P(x), P(mr), None, None, None, P(x), P(mr), None, None, P(y), P(y), 6, 8, 2),
        lib.t2v_instance_norm_join(c.handle, s, P(x), P(mr), None, None, P(y), P(x), P(mr), None, None, P(y), P(y), 6, 6, 2),
        lib.t2v_instance_norm_join(c.handle, s, P(x), P(mr), None, None, P(y), P(x), P(mr), None, None, P(y), P(y), 6, 8, 0),
    ]
    assert all(st != 0 for st in bad), bad
    torch.cuda.synchronize()
    assert (y == 0).all()
