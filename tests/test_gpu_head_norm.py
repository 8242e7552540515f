"""The 7x7 head on a RAW decoder output with a pending norm (t2v_conv2d_forward_head_norm, ops.conv2d_head_norm): the halo-tile
kernel normalises every plane it stages in LDS instead of reading a map an apply pass wrote.

Per case (Cin 128 | 64, tanh | flow-and-sigmoid epilogue, with | without gamma and beta, a geometry with ragged 16x16 tiles and
one that is a multiple of 16):
  * bit-equal to instance_norm_apply followed by the plain head, both outputs poisoned with NaN first;
  * under torch.profiler the lazy call runs conv_head7x7_strip_kernel<Cin> and no inorm_apply_kernel;
  * within a float64 bound of norm -> ReLU -> reflect-padded conv -> activation, derived below from the kernel's arithmetic
    with kernel_variants' own pieces (the head's summation depth, the K-term sum bound, gamma(n))."""

import pytest
import torch

import kernel_variants as kv

pytestmark = pytest.mark.gpu

GEOMETRIES = {"ragged_37x53": (37, 53), "mult16_32x48": (32, 48)}


def _profiled(fn):
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {kv.normalise(e.name) for e in prof.events() if "t2v::" in e.name}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _float64_reference_and_bound(case, x, mr, gamma, beta, w, b, act, act_scale):
    """r [Cout, H, W] and the elementwise bound on |y - r|, everything in float64 from the fp32 operands the kernel reads.

    Norm (transform_common.h: norm_apply): z = relu(fl(fl(fl(x - m) * s) * g) + b)) -- two roundings without gamma / beta,
    four with: each rounding is relative to what it rounds, so |z_fl - z| <= gamma(n) (|x - m| |s| |g| + |b|) =: e_z with
    n = 2 | 4, ReLU being 1-Lipschitz and exact (kernel_variants.gamma; + one TINY per rounding for flushed results).
    Conv (conv_head.hip): the 49 * Cin products and the bias are summed along chains of depth kv.depth(case) -- the tree the
    docstring of kernel_variants.depth reads off the kernel -- so with Z = |z| + e_z >= |z_fl|
        |v_fl - v| <= sum |w| e_z                       (the exact conv of the norm's error)
                    + kv.sum_bound(conv64(Z, |w|, |b|), depth, terms)       (the fp32 sum of the products of z_fl).
    Activation: tanh is 1-Lipschitz, the flow channels are v * act_scale (one more rounding), the weight channel
    1 / (1 + exp(-v)) is 1/4-Lipschitz.  ocml's tanhf and expf are specified to 2 ulp or better; 4 u |tanh| covers tanhf and
    the store; the sigmoid goes through expf (2 ulp), an add, a divide and a negation-free rest: <= 5 u relative on a value
    <= 1.  Those evaluation terms are added to the Lipschitz image of the pre-activation bound."""
    x64, w64, b64 = x.double(), w.double(), b.double()
    m, s = mr[:, 0].double().view(-1, 1, 1), mr[:, 1].double().view(-1, 1, 1)
    v = (x64 - m) * s
    mag = (x64 - m).abs() * s.abs()
    n = 2
    if gamma is not None:
        g64, bt64 = gamma.double().view(-1, 1, 1), beta.double().view(-1, 1, 1)
        v = v * g64 + bt64
        mag = mag * g64.abs() + bt64.abs()
        n = 4
    z = v.clamp(min=0)
    e_z = kv.gamma(n) * mag + n * kv.TINY
    pre = kv.conv64(case, z[None], w64, b64)[0]
    e_in = kv.conv64(case, e_z[None], w64.abs(), torch.zeros_like(b64))[0]
    A = kv.conv64(case, (z.abs() + e_z)[None], w64.abs(), b64.abs())[0]
    e_pre = e_in + kv.sum_bound(A, kv.depth(case), kv.terms(case))
    if act == "tanh":
        r = torch.tanh(pre)
        bnd = e_pre + 4 * kv.U * r.abs() + kv.TINY
    else:
        r = torch.cat([pre[:2] * act_scale, torch.sigmoid(pre[2:3])])
        bnd = torch.cat([abs(act_scale) * e_pre[:2] + kv.U * r[:2].abs() + kv.TINY,
                         0.25 * e_pre[2:3] + 5 * kv.U * r[2:3].abs() + kv.TINY])
    return r, bnd


@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("act", ["tanh", "flow"])
@pytest.mark.parametrize("cin", [128, 64])
def test_head_on_raw_map_is_apply_then_head(cin, act, affine, geom):
    from text2video_amd import ops
    assert torch.cuda.is_available(), "GPU test without a GPU"
    dev = torch.device("cuda:0")
    H, W = GEOMETRIES[geom]
    case = kv._case("head_norm", H, W, cin, 3, 7, 1, 3, True, False, False, kv.head(cin))
    x, w, b = kv.case_tensors(case, seed=cin + H)
    g = torch.Generator().manual_seed(7 * cin + W)
    # a conv output before its norm: every channel with a mean and a spread of its own
    x = x[0] * (0.5 + 2.0 * torch.rand(cin, 1, 1, generator=g)) + 3.0 * torch.randn(cin, 1, 1, generator=g)
    mean = x.double().mean((1, 2))
    rstd = 1.0 / torch.sqrt(x.double().var((1, 2), unbiased=False) + 1e-5)
    mr = torch.stack([mean, rstd], 1).float().contiguous()                     # [C][2], as the finalize kernels write it
    gamma = (1.0 + 0.3 * torch.randn(cin, generator=g)) if affine else None
    beta = (0.2 * torch.randn(cin, generator=g)) if affine else None
    act_id, act_scale = (ops.ACT_TANH, 1.0) if act == "tanh" else (ops.ACT_FLOW_W, 20.0)
    desc = ops.conv_desc(H, W, cin, 3, 7, 1, 3, ops.PAD_REFLECT, False, act_id, act_scale)
    xd = x.permute(1, 2, 0).contiguous().to(dev)
    mrd = mr.to(dev)
    gd = gamma.to(dev) if affine else None
    bd = beta.to(dev) if affine else None
    pw = ops.pack_conv_weight(w.to(dev), desc, cin)
    bias = b.to(dev)

    want = torch.full((H, W, 4), float("nan"), device=dev)
    ops.conv2d(ops.instance_norm_apply(xd, mrd, gd, bd, relu=True), pw, bias, desc, y_cs=4, out=want)
    got = torch.full((H, W, 4), float("nan"), device=dev)
    ran = _profiled(lambda: ops.conv2d_head_norm(xd, pw, bias, desc, mrd, gd, bd, relu=True, y_cs=4, out=got))
    assert kv.head(cin) in ran and "t2v::inorm_apply_kernel" not in ran, sorted(ran)
    assert torch.isfinite(got).all() and torch.isfinite(want).all(), "output left unwritten (NaN poison)"
    assert torch.equal(_bits(got), _bits(want)), "lazy head differs from apply + head at %d values (max |d| %.3g)" % (
        (_bits(got) != _bits(want)).sum().item(), (got - want).abs().max().item())
    assert (got[..., 3] == 0).all()

    r, bnd = _float64_reference_and_bound(case, x, mr, gamma, beta, w, b, act, act_scale)
    err = (got[..., :3].permute(2, 0, 1).double().cpu() - r).abs()
    ratio = err / bnd
    print("head_norm cin %d %s %s %s: worst |y - r| / bound = %.3g (max |y - r| %.3g)"
          % (cin, act, "affine" if affine else "plain", geom, ratio.max().item(), err.max().item()))
    assert ratio.max().item() <= 1.0, "worst |y - r| / bound = %.3g at [c, y, x] = %s (max |y - r| %.3g)" % (
        ratio.max().item(), [int(i) for i in torch.nonzero(ratio == ratio.max())[0]], err.max().item())


def test_head_norm_rejects_what_the_head_kernel_does_not_take():
    from text2video_amd import ops
    dev = torch.device("cuda:0")
    x = torch.zeros(8, 8, 12, device=dev)                         # 12 channels: the implicit-GEMM kernel's shape, not the head's
    desc = ops.conv_desc(8, 8, 12, 3, 7, 1, 3, ops.PAD_REFLECT, False, ops.ACT_TANH, 1.0)
    pw = ops.pack_conv_weight(torch.zeros(3, 12, 7, 7, device=dev), desc, 12)
    with pytest.raises(RuntimeError, match="head7x7"):
        ops.conv2d_head_norm(x, pw, torch.zeros(3, device=dev), desc, torch.ones(12, 2, device=dev))
