"""Every reachable instantiation of the direct convolution kernels (conv_igemm_kernel<Cfg, MODE, STATS, REFLECT, RING>,
conv_stem7x7_kernel, conv_head7x7_strip_kernel, conv_cout1_kernel) against float64, at a shape proven -- by the profiler,
in the same test -- to select it.  The cases and the bound live in tests/kernel_variants.py; tests/test_cpu_kernel_variants.py
checks that the cases cover every compiled instantiation and that the bound sees the faults it is meant to catch.

Per case:
  * the launch runs under torch.profiler: the expected instantiation ran, and no other instantiation of the four direct
    conv families did;
  * elementwise |y - r| <= C_DIRECT u K A + K tiny against the conv in float64 (r), A being the same conv on |x|, |w|, |b|
    in float64 and K the products per output plus the bias (kernel_variants.C_DIRECT: the gamma bound of a K-term fma
    chain summed in any order, with unfused products);
  * output and statistics buffers start as NaN.  The contract on output channels [Cout, y_cs), y_cs = Cout rounded up to 4
    (what every caller passes): the implicit-GEMM, head and one-channel kernels write them as 0.  The stem kernel's Cout
    is 64 or 128, so it has no such channels;
  * STATS cases: the partials through instance_norm_finalize give every image's per-channel mean and rstd within
    kernel_variants.stats_bounds of the float64 values."""
import pytest
import torch

import kernel_variants as kv

pytestmark = pytest.mark.gpu

DIRECT_FAMILIES = ("conv_igemm_kernel", "conv_stem7x7_kernel", "conv_head7x7_strip_kernel", "conv_cout1_kernel")


def _dev():
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return torch.device("cuda:0")


def _launch_profiled(fn):
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {kv.normalise(e.name) for e in prof.events() if "t2v::" in e.name}


def _direct_conv_kernels(names):
    return {n for n in names if kv.family(n) in DIRECT_FAMILIES}


@pytest.mark.parametrize("case", kv.CONV_CASES, ids=[c.id for c in kv.CONV_CASES])
def test_direct_conv_variant_against_float64(case):
    from text2video_amd import ops
    dev = _dev()
    x, w, b = kv.case_tensors(case)
    ref = kv.conv64(case, x, w, b)                         # [B, Cout, Ho, Wo] float64
    bnd = kv.bound(case, x, w, b)
    desc = ops.conv_desc(case.H, case.W, case.Cin, case.Cout, case.k, case.stride, case.pad,
                         ops.PAD_REFLECT if case.reflect else ops.PAD_ZERO, case.transposed, ops.ACT_NONE, 1.0,
                         output_padding=case.op)
    assert ops.conv_out_dims(desc) == tuple(ref.shape[2:])
    xcs = kv.x_cs(case)
    xs = torch.zeros(case.batch, case.H, case.W, xcs)
    xs[..., :case.Cin] = x.permute(0, 2, 3, 1)
    xs = xs.to(dev)
    pw = ops.pack_conv_weight(w.to(dev), desc, xcs)
    bd = b.to(dev)
    ycs = ops.round_up(case.Cout, 4)
    ho, wo = ref.shape[2:]
    y = torch.full((case.batch, ho, wo, ycs), float("nan"), device=dev)
    n = ops.conv_stats_buffer(desc, dev).numel() if case.stats else 0
    sb = torch.full((case.batch * n,), float("nan"), device=dev) if case.stats else None
    if case.batch == 1:
        ran = _launch_profiled(lambda: ops.conv2d(xs[0], pw, bd, desc, y_cs=ycs, stats=sb, out=y[0]))
    else:
        ran = _launch_profiled(lambda: ops.conv2d_batch(xs, pw, bd, desc, y_cs=ycs, stats=sb, out=y))
    assert _direct_conv_kernels(ran) == {case.expect}, "expected %s, ran %s" % (case.expect, sorted(ran))

    got = y[..., :case.Cout].permute(0, 3, 1, 2).double().cpu()
    assert torch.isfinite(got).all(), "output left unwritten (NaN poison) at %d places" % (~torch.isfinite(got)).sum()
    err = (got - ref).abs()
    ratio = err / bnd
    assert ratio.max().item() <= 1.0, "worst |y - r| / bound = %.3g at [b, c, y, x] = %s (max |y - r| %.3g)" % (
        ratio.max().item(), [int(i) for i in torch.nonzero(ratio == ratio.max())[0]], err.max().item())
    if ycs > case.Cout:
        assert (y[..., case.Cout:] == 0).all(), "output channels [Cout, y_cs) must be written as 0"

    if case.stats:
        for i in range(case.batch):
            mr = ops.instance_norm_finalize(sb[i * n:(i + 1) * n], desc).view(-1, 2).double().cpu()
            m, s, e_m, e_s = kv.stats_bounds(ref[i], bnd[i], parts=max(n // (2 * case.Cout), 1))
            dm, ds = (mr[:, 0] - m).abs(), (mr[:, 1] - s).abs()
            assert (dm <= e_m).all(), "image %d mean: worst |d| / bound %.3g" % (i, (dm / e_m).max().item())
            assert (ds <= e_s).all(), "image %d rstd: worst |d| / bound %.3g" % (i, (ds / e_s).max().item())


def test_scalar_channel_forms_against_float64():
    """Three kernels no other GPU test reaches, each pinned by the profiler: reflect_pad_backward_kernel<float> (channel
    counts that are no multiple of 4), scale_kernel (exact: a power-of-two factor) and bn_running_update_kernel (BatchNorm2d's
    running statistics from a (mean, rstd) table: momentum average, unbiased variance = (1 / rstd^2 - eps) n / (n - 1))."""
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 3, 5, 7, dtype=torch.float64, generator=g, requires_grad=True)
    yp = torch.nn.functional.pad(x, (2, 2, 2, 2), mode="reflect")
    d = torch.randn(*yp.shape, generator=g).double()         # fp32 values: the upload is exact
    yp.backward(d)
    dxp = d[0].permute(1, 2, 0).float().contiguous().to(dev)
    out = {}
    ran = _launch_profiled(lambda: out.setdefault("dx", ops.reflect_pad_backward(dxp, 2)))
    assert "t2v::reflect_pad_backward_kernel<float>" in ran, sorted(ran)
    got = out["dx"].permute(2, 0, 1).double().cpu()
    # each input pixel sums at most 4 padded-map gradients (3 roundings)
    assert ((got - x.grad[0]).abs() <= 3.03 * kv.U * 4 * d.abs().max()).all()

    v = torch.randn(1000, generator=g).to(dev)
    want = v.double() * 0.25
    ran = _launch_profiled(lambda: ops.scale_(v, 0.25))
    assert "t2v::scale_kernel" in ran, sorted(ran)
    assert torch.equal(v.double(), want)

    C, n, mom, eps = 37, 96, 0.1, 1e-5
    mr = torch.stack([torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5], 1)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    var = 1.0 / mr[:, 1].double() ** 2 - eps
    want_m = (1 - mom) * rm.double() + mom * mr[:, 0].double()
    want_v = (1 - mom) * rv.double() + mom * var * n / (n - 1)
    rmd, rvd = rm.to(dev), rv.to(dev)
    ran = _launch_profiled(lambda: ops.batch_norm_update_running(mr.to(dev), rmd, rvd, n, mom, eps))
    assert "t2v::bn_running_update_kernel" in ran, sorted(ran)
    # ~6 roundings on the variance path (square, divide, subtract, two multiplies, the average), 3 on the mean's
    assert ((rmd.double().cpu() - want_m).abs() <= 8 * kv.U * (rm.double().abs() + mr[:, 0].double().abs())).all()
    assert ((rvd.double().cpu() - want_v).abs() <= 16 * kv.U * (rv.double() + var.abs() * n / (n - 1))).all()


def test_layout_and_reduction_forms_against_float64():
    """More single-purpose kernels, each pinned by the profiler and checked against a plain reference of its own:
    reflect_pad_backward_kernel<float4> (channels a multiple of 4), nhwc_to_nchw / copy_channels (exact moves),
    accumulate / unzip2 (one fp32 addition each: equal to torch's), and reduce_partial_kernel<0> / <1> + reduce_final_kernel
    (sum (x - c)^2 and sum |a - b|: within gamma(k) sum|terms|, k = 28 the two-level reduction's longest chain of roundings)."""
    from text2video_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 8, 6, 9, dtype=torch.float64, generator=g, requires_grad=True)
    yp = torch.nn.functional.pad(x, (2, 2, 2, 2), mode="reflect")       # (the entry point asks H, W > 2 pad)
    d = torch.randn(*yp.shape, generator=g).double()         # fp32 values: the upload is exact
    yp.backward(d)
    dxp = d[0].permute(1, 2, 0).float().contiguous().to(dev)
    out = {}
    ran = _launch_profiled(lambda: out.setdefault("dx", ops.reflect_pad_backward(dxp, 2)))
    assert "t2v::reflect_pad_backward_kernel<HIP_vector_type<float,4u>>" in ran, sorted(ran)
    assert ((out["dx"].permute(2, 0, 1).double().cpu() - x.grad[0]).abs() <= 3.03 * kv.U * 4 * d.abs().max()).all()

    hwc = torch.randn(7, 5, 12, generator=g).to(dev)
    ran = _launch_profiled(lambda: out.setdefault("chw", ops.nhwc_to_nchw(hwc, 10)))
    assert "t2v::nhwc_to_nchw_kernel" in ran, sorted(ran)
    assert torch.equal(out["chw"], hwc[..., :10].permute(2, 0, 1))
    dst = torch.full((7, 5, 8), float("nan"), device=dev)
    ran = _launch_profiled(lambda: ops.copy_channels(hwc, 3, dst, 1, 5))
    assert "t2v::copy_channels_kernel" in ran, sorted(ran)
    assert torch.equal(dst[..., 1:6], hwc[..., 3:8]) and torch.isnan(dst[..., 0]).all() and torch.isnan(dst[..., 6:]).all()

    a, b = torch.randn(4099, generator=g).to(dev), torch.randn(4099, generator=g).to(dev)
    want = a + b
    ran = _launch_profiled(lambda: ops.accumulate_(a, b))
    assert "t2v::accumulate_kernel" in ran, sorted(ran)
    assert torch.equal(a, want)
    src = torch.randn(37, 2, generator=g).to(dev)
    d0, d1 = torch.randn(37, generator=g).to(dev), torch.randn(37, generator=g).to(dev)
    w0, w1 = d0 + src[:, 0], d1 + src[:, 1]
    ran = _launch_profiled(lambda: ops.unzip2_(src, d0, d1))
    assert "t2v::unzip2_kernel" in ran, sorted(ran)
    assert torch.equal(d0, w0) and torch.equal(d1, w1)

    n = 300001
    p, q = torch.randn(n, generator=g), torch.randn(n, generator=g)
    for form, fn, terms in ((0, lambda: ops.sum_sq_diff_const(p.to(dev), 0.75), (p.double() - 0.75) ** 2),
                            (1, lambda: ops.sum_abs_diff(p.to(dev), q.to(dev)), (p.double() - q.double()).abs())):
        ran = _launch_profiled(lambda: out.__setitem__("s", fn()))
        assert {"t2v::reduce_partial_kernel<%d>" % form, "t2v::reduce_final_kernel"} <= ran, sorted(ran)
        # |got - sum| <= gamma(k) sum|terms|, k the longest chain of fp32 roundings a term goes through in launch_reduce's two
        # levels (csrc/elementwise.hip; no fused multiply-add): the difference and the square / |.| (2); thread j of
        # reduce_partial_kernel adds elements j, j + grid*256, ...: ceil(n / (grid*256)) adds with grid = min(ceil(n / 256),
        # 2048); block_sum's six shuffle levels and four wave sums (10); reduce_final_kernel's ceil(grid / 256) strided adds
        # and its own block_sum (10).  n = 300001: grid 1172, k = 2 + 1 + 10 + 5 + 10 = 28 -- not n + 2: a dropped block of
        # 256 elements (8.5e-4 of the sum) passed the old bound (1.9 % of it) and is 500x this one (1.7e-6)
        grid = min(-(-n // 256), 2048)
        k = 2 + -(-n // (grid * 256)) + 10 + -(-grid // 256) + 10
        assert k == 28
        bound = k * kv.U / (1 - k * kv.U) * terms.abs().sum().item()
        err = abs(out["s"].item() - terms.sum().item())
        print("reduce form %d: |got - f64| / bound %.3g (k = %d)" % (form, err / bound, k))
        assert err <= bound
        assert bound < kv.C_DIRECT * kv.U * (n + 2) * terms.abs().sum().item() / 1e4     # (what this assertion used to allow)


WGRAD_CASES = [
    # id, B, H, W, Cin, Cout, k, stride, pad, reflect, transposed, expected kernel
    ("rb3x3_reflect", 2, 16, 16, 64, 128, 3, 1, 1, True, False, "t2v::conv_wgrad_kernel<true,16,4>"),
    ("stem7x7_reflect_cin9", 1, 20, 20, 9, 32, 7, 1, 3, True, False, "t2v::conv_wgrad_kernel<true,16,4>"),
    ("down3x3_s2_zero_odd", 2, 17, 15, 32, 64, 3, 2, 1, False, False, "t2v::conv_wgrad_kernel<false,16,4>"),
    ("disc4x4_s2_p2", 2, 16, 16, 8, 64, 4, 2, 2, False, False, "t2v::conv_wgrad_kernel<false,16,4>"),
    ("convT3x3", 2, 8, 8, 64, 32, 3, 2, 1, False, True, "t2v::conv_wgrad_kernel<false,16,4>"),
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_direct_weight_gradient_against_float64(case):
    """conv_wgrad_kernel<REFLECT, 16, 4> (conv2d_backward_weight): dW = sum over images and output pixels of dy * x, pinned
    by the profiler and compared elementwise with float64: |dW - r| <= C_DIRECT u K A + K tiny, K = B Ho Wo products per
    weight (any summation order, including the split reduction), A = the same gradient from |x| and |dy|."""
    from text2video_amd import ops
    _, B, H, W, Cin, Cout, k, stride, pad, reflect, transposed, kernel = case
    dev = _dev()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, Cin, H, W, generator=g).double()      # fp32 values: the uploads below are exact
    w0 = torch.zeros(*((Cin, Cout, k, k) if transposed else (Cout, Cin, k, k)), dtype=torch.float64)

    def fwd(xx, ww):
        if transposed:
            return torch.nn.functional.conv_transpose2d(xx, ww, stride=2, padding=pad, output_padding=1)
        if reflect:
            return torch.nn.functional.conv2d(torch.nn.functional.pad(xx, (pad,) * 4, mode="reflect"), ww, stride=stride)
        return torch.nn.functional.conv2d(xx, ww, stride=stride, padding=pad)
    ho, wo = fwd(x, w0).shape[2:]
    dy = torch.randn(B, Cout, ho, wo, generator=g).double()
    ww = w0.clone().requires_grad_()
    (ref,) = torch.autograd.grad(fwd(x, ww), ww, dy)
    wa = w0.clone().requires_grad_()
    (A,) = torch.autograd.grad(fwd(x.abs(), wa), wa, dy.abs())
    K = B * ho * wo
    bnd = kv.sum_bound(A, K)
    desc = ops.conv_desc(H, W, Cin, Cout, k, stride, pad, ops.PAD_REFLECT if reflect else ops.PAD_ZERO, transposed)
    xcs, ycs = ops.round_up(Cin, 4), ops.round_up(Cout, 4)
    xs = torch.zeros(B, H, W, xcs)
    xs[..., :Cin] = x.float().permute(0, 2, 3, 1)
    dys = torch.zeros(B, ho, wo, ycs)
    dys[..., :Cout] = dy.float().permute(0, 2, 3, 1)
    xs, dys = xs.to(dev), dys.to(dev)
    out = {}
    ran = _launch_profiled(lambda: out.setdefault("dw", ops.conv2d_backward_weight(xs, dys, desc)))
    assert {n for n in ran if kv.family(n) in ("conv_wgrad_kernel", "wino_wgrad_sk_kernel")} == {kernel}, sorted(ran)
    got = ops.unpack_conv_weight(out["dw"], desc, xcs).double().cpu()
    assert got.shape == ref.shape
    ratio = ((got - ref).abs() / bnd).max().item()
    assert ratio <= 1.0, "worst |dW - r| / bound = %.3g" % ratio
