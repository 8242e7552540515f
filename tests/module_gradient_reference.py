"""Float64 reference, kink masks, bounds, fp32 restatement and case table for the discriminator's Python backward layer
(text2video_amd/train.py: _ConvBlock, _norm_adjoint, _bias_gradient, _weight_gradient, _data_gradient and
TrainableDiscriminator with groups / bn_times / pt_skip / frozen).

A plain helper module (no fixtures, no hooks), shared by tests/test_cpu_module_gradient_reference.py, which checks the
reference against plain autograd, the near-kink cap of every case, the conditioning claim about one flipped LeakyReLU
element and the bound against injected faults, and by tests/test_gpu_module_gradients.py, which runs the HIP modules.

The comparison:
  * the reference is the project's own oracle module (oracle.generator_ref.MultiscaleDiscriminator: stock torch.nn) in
    float64, with every nn.LeakyReLU replaced by `_MaskedLeaky`: the true leaky ReLU forward, a backward that multiplies by
    1 or 0.2 according to a SUPPLIED mask.  TrainableDiscriminator.forward returns every stage output, so the sign of each
    activated stage output is the slope the HIP backward used; the float64 reference differentiated with those slopes has
    no kink left to disagree about;
  * the loss is the linear functional sum <R_ij, feat_ij> over all stage outputs with fixed random R_ij: every stage's
    gradient entry is exercised and no second family of kinks is added;
  * error per tensor: ||g - g64||_2 / ||g64||_2;
  * bound per tensor: FACTOR x the error of the same masked module evaluated by torch in fp32 on the CPU with the same masks
    (another correct fp32 implementation that shares no code with the kernels), with a floor of FLOOR (8 units of fp32
    roundoff) so that a tensor the fp32 evaluation happens to hit exactly does not fail.  FACTOR = 4 allows for two
    correct fp32 implementations summing in different orders;
  * the kink: a HIP mask may differ from the float64 sign only where |z64| <= delta (near_kink), delta = 5 x the forward
    tolerance asserted for that stage's output, taken per element: 5 x bound(e32) x rms(y64).  A stage output that meets
    its forward tolerance has an rms error of at most bound(e32) x rms(y64), and the negative side of the activation
    carries slope 0.2, so an error of that size in y is one of 5 x that in z.  At most KINK_CAP elements of a case may lie
    there (a condition on the case's seeds, checked on the CPU, not a measurement)."""
import collections
import copy

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24            # unit roundoff of fp32
SLOPE = 0.2
FACTOR = 4.0
# The floor stands for what a correct fp32 evaluation reaches where the CPU evaluation happens to land on the float64 value:
# the tensors concerned are short reductions (the bias gradient of the one-channel logits: 150 .. 700 seeds), which torch's
# vectorised pairwise sum hits to < 0.2 u.  A correct reduction that adds n same-sign terms in a fixed serial order -- one
# thread adds the up to 256 pixel lanes of a block in channel_sum's partial kernels -- has a relative rounding error of
# u sqrt(n) / 3 rms (each of the n additions rounds a partial sum of i / n of the total by u / sqrt(3) rms): 5.3 u for n = 256.
# 8 u is 1.5 x that rms.  (First set to 4 u without that count: the 216-term logits bias gradient of grouped3's coarse scale,
# 4.9 u from the serial chain against 0.9 u from torch, then failed by the floor alone.)
FLOOR = 8.0 * U
KINK_CAP = 8
N_LAYERS = 3              # every case: five stages per scale, the first four activated

# id; module: num_D, ndf, norm, cin (logical input channels) in xcs channels of NHWC storage; input: B x H x W, channels
# [zero_from:] zero; form: groups / bn_times (passes in one batch), calls (forward calls in one graph), pt_skip + off
# (param_gradients_off: a pass-through backward), frozen; w_seed / x_seed: weights and input;  init: "affine" draws the norm
# biases from N(0, 0.1) (every affine term exercised), "trainer" keeps what Vid2VidTrainer draws (norm bias 0)
Case = collections.namedtuple("Case", "id num_D ndf norm cin xcs B H W groups bn_times calls pt_skip off frozen w_seed x_seed "
                                      "zero_from init")


def _c(id, num_D=2, ndf=16, norm="batch", cin=6, xcs=8, B=2, H=45, W=37, groups=1, bn_times=None, calls=1, pt_skip=0,
       off=False, frozen=False, w_seed=11, x_seed=12, zero_from=None, init="affine"):
    return Case(id, num_D, ndf, norm, cin, xcs, B, H, W, groups, bn_times, calls, pt_skip, off, frozen, w_seed, x_seed,
                zero_from, init)


CASES = [
    _c("plain_bn"),
    _c("plain_in", norm="instance", w_seed=13, x_seed=14),
    _c("temporal13", cin=13, xcs=16, H=48, W=32, zero_from=9, w_seed=3, x_seed=4),
    _c("grouped3", B=6, groups=3, bn_times=[1, 2, 2], w_seed=15, x_seed=16),
    _c("two_calls", B=4, calls=2, w_seed=17, x_seed=18),
    _c("passthrough", B=6, groups=3, bn_times=[1, 2, 2], pt_skip=2, off=True, w_seed=15, x_seed=16),
    _c("passthrough_in", norm="instance", B=3, pt_skip=1, off=True, w_seed=19, x_seed=20),
    _c("frozen", frozen=True, w_seed=21, x_seed=22),
    _c("wide_storage", cin=3, xcs=8, H=33, W=29, w_seed=23, x_seed=24),
    _c("capped_ndf", num_D=3, ndf=32, B=1, H=64, W=48, w_seed=25, x_seed=26),
    # D_f's geometry.  The seeded ones take the weights as Vid2VidTrainer(seed=s) draws D_f's (discriminator_state_dict with
    # seed s + 2) and the first frame's 128 x 128 face crop of the clip the full-size tests draw for that seed
    _c("face128", num_D=1, ndf=64, B=1, H=128, W=128, w_seed=31, x_seed=32, init="trainer"),
    _c("face128_seed5", num_D=1, ndf=64, B=1, H=128, W=128, w_seed=5, x_seed=5, init="trainer"),
    _c("face128_seed6", num_D=1, ndf=64, B=1, H=128, W=128, w_seed=6, x_seed=6, init="trainer"),
    _c("face128_seed7", num_D=1, ndf=64, B=1, H=128, W=128, w_seed=7, x_seed=7, init="trainer"),
]
BY_ID = {c.id: c for c in CASES}
FACE_SEED_CASES = [c for c in CASES if c.id.startswith("face128_seed")]


# ------------------------------------------------------------------------------------------------------------------
# case tensors
# ------------------------------------------------------------------------------------------------------------------
def stage_channels(case, scale):
    """Cout of the five stages of result[scale] (result[0] is the finest scale: the module's scale num_D - 1)"""
    nd = min(case.ndf * 2 ** scale, 64)
    return [nd, min(nd * 2, 512), min(nd * 4, 512), min(nd * 8, 512), 1]


def stage_shapes(case):
    """[scale][layer] -> (C, h, w): k4 p2 convs of stride 2, 2, 2, 1, 1; the 3x3 / s2 / p1 pool between two scales"""
    out, h, w = [], case.H, case.W
    for i in range(case.num_D):
        hh, ww, row = h, w, []
        for j, C in enumerate(stage_channels(case, i)):
            hh, ww = (hh // 2 + 1, ww // 2 + 1) if j < N_LAYERS else (hh + 1, ww + 1)
            row.append((C, hh, ww))
        out.append(row)
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return out


def pass_slices(case):
    """the independent forward passes of the case: slices of the batch, each with batch statistics of its own"""
    P = case.groups * case.calls
    n = case.B // P
    assert n * P == case.B
    return [slice(g * n, (g + 1) * n) for g in range(P)]


def zero_bias_names(case):
    """conv biases in front of a norm layer: the norm removes the channel mean, their gradient is exactly zero"""
    return ["scale%d_layer%d.0.bias" % (i, j) for i in range(case.num_D) for j in range(1, N_LAYERS + 1)]


def _face_crop(seed):
    """pose channels 6..8 and the real frame of the first image on the face box of a 512 x 512 clip, drawn as
    tests/test_gpu_device_oracle.py draws the clip of `seed` (its _pose / _frames with data_seed = 10 (seed - 5))"""
    H = W = 512
    ds = 10 * (seed - 5)
    rng = np.random.default_rng(51 + ds)
    pose = torch.from_numpy(np.where(rng.random((2, 1, H, W)) < 0.02, rng.uniform(-1, 1, (2, 9, H, W)), -1.0).astype(np.float32))
    real = torch.tanh(torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(52 + ds)))
    ys, xs = H // 8, (W - 128) // 2
    return torch.cat([pose[:1, 6:9, ys:ys + 128, xs:xs + 128], real[:1, :, ys:ys + 128, xs:xs + 128]], 1).contiguous()


_BUILT = {}


def build_case(case):
    """-> dict(sd, ref, x, seeds): the state dict (upstream names, fp32), the oracle module holding it (fp32, CPU, train
    mode), the input [B, cin, H, W] and the seeds R[scale][layer] of the loss, all fp32 on the CPU.  Built once per case
    and shared: nothing may write into it."""
    if case.id in _BUILT:
        return _BUILT[case.id]
    from oracle.generator_ref import MultiscaleDiscriminator
    from text2video_amd.train import discriminator_state_dict
    seeded_face = case.id.startswith("face128_seed")
    sd = discriminator_state_dict(case.cin, case.ndf, N_LAYERS, case.num_D, case.norm, case.w_seed + (2 if seeded_face else 0))
    g = torch.Generator().manual_seed(1000 + case.x_seed)
    if case.init == "affine":
        for k in sorted(sd):
            if k.endswith(".1.bias"):
                sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
    ref = MultiscaleDiscriminator(case.cin, case.ndf, N_LAYERS, case.num_D, case.norm)
    missing, unexpected = ref.load_state_dict(sd, strict=False)
    assert not unexpected and all(("running" in k or "num_batches" in k) for k in missing), (missing, unexpected)
    ref.train()
    if seeded_face:
        x = _face_crop(case.x_seed)
    else:
        x = torch.tanh(torch.randn(case.B, case.cin, case.H, case.W, generator=g))
    if case.zero_from is not None:
        x[:, case.zero_from:] = 0
    # (a mean of 0.5: the bias gradients of the two layers without a norm are sums of seeds, which would otherwise cancel)
    seeds = [[torch.randn(case.B, C, h, w, generator=g) + 0.5 for (C, h, w) in row] for row in stage_shapes(case)]
    _BUILT[case.id] = dict(sd=sd, ref=ref, x=x, seeds=seeds)
    return _BUILT[case.id]


def to_nhwc(t, cs):
    """[B, C, h, w] -> [B, h, w, cs], the storage channels beyond C zero"""
    out = torch.zeros(t.shape[0], t.shape[2], t.shape[3], cs, dtype=t.dtype, device=t.device)
    out[..., :t.shape[1]] = t.permute(0, 2, 3, 1)
    return out


def to_nchw(t, C):
    """the logical channels of an NHWC tensor as [B, C, h, w]"""
    return t[..., :C].permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------------
# the masked oracle module
# ------------------------------------------------------------------------------------------------------------------
class _MaskedLeaky(torch.autograd.Function):
    """forward: the true leaky ReLU of z.  backward: dy times 1 where `mask`, times `slope` elsewhere."""

    @staticmethod
    def forward(ctx, z, mask, slope):
        ctx.save_for_backward(mask)
        ctx.slope = slope
        return F.leaky_relu(z, slope)

    @staticmethod
    def backward(ctx, dy):
        mask, = ctx.saved_tensors
        return torch.where(mask, dy, dy * ctx.slope), None, None


def masked_discriminator(ref_module, masks=None):
    """-> run(x) -> (feats, zs): the stage outputs result[scale][layer] of `ref_module` (a MultiscaleDiscriminator in any
    dtype, on any device) and the pre-activations z of the activated stages (None for the logits), as parts of one autograd
    graph in which every nn.LeakyReLU differentiates with masks[scale][layer] (a bool tensor of the stage output's shape:
    True = slope 1).  masks=None, or None for a stage: the sign of z itself, which is plain autograd."""
    def run(x):
        feats, zs = [], []
        for i in range(ref_module.num_D):
            cur, row, zrow = x, [], []
            for j in range(ref_module.n_layers + 2):
                z = None
                for m in getattr(ref_module, "scale%d_layer%d" % (ref_module.num_D - 1 - i, j)):
                    if isinstance(m, torch.nn.LeakyReLU):
                        z = cur
                        mk = None if masks is None else masks[i][j]
                        mk = (z > 0) if mk is None else mk.to(z.device)
                        assert mk.shape == z.shape and mk.dtype == torch.bool, (i, j, mk.shape, z.shape)
                        cur = _MaskedLeaky.apply(z, mk, m.negative_slope)
                    else:
                        cur = m(cur)
                row.append(cur)
                zrow.append(z)
            feats.append(row)
            zs.append(zrow)
            if i != ref_module.num_D - 1:
                x = ref_module.downsample(x)
        return feats, zs
    return run


Result = collections.namedtuple("Result", "feats zs dx grads")


def _linear_loss(feats, seeds, sl, skip, device, dtype):
    loss = 0.0
    for frow, srow in zip(feats, seeds):
        for f, R in zip(frow, srow):
            R = R.to(device=device, dtype=dtype).clone()
            R[:skip] = 0
            loss = loss + (R[sl] * f).sum()
    return loss


def reference(case, data, dtype, device="cpu", masks=None, skip=0, module_fn=masked_discriminator):
    """The case through the masked oracle module in `dtype` on `device`: one independent forward call per pass of the case
    (pass_slices: its own batch statistics), the linear loss summed over the passes, so the parameter gradients are summed
    over them.  skip: the seeds of the leading `skip` images are zero (what a pass-through backward with pt_skip reaches).
    -> Result(feats[scale][layer] over the whole batch, zs likewise, dx, {upstream parameter name: gradient}), detached."""
    mod = copy.deepcopy(data["ref"]).to(device=device, dtype=dtype).train()
    x = data["x"].to(device=device, dtype=dtype).requires_grad_(True)
    loss, fs, zz = 0.0, [], []
    for sl in pass_slices(case):
        mk = None if masks is None else [[None if m is None else m[sl] for m in row] for row in masks]
        feats, zs = module_fn(mod, mk)(x[sl])
        loss = loss + _linear_loss(feats, data["seeds"], sl, skip, device, dtype)
        fs.append(feats)
        zz.append(zs)
    names = [k for k, _ in mod.named_parameters()]
    g = torch.autograd.grad(loss, [x] + [p for _, p in mod.named_parameters()])

    def cat(parts):
        return [[None if parts[0][i][j] is None else torch.cat([p[i][j] for p in parts]).detach()
                 for j in range(len(parts[0][i]))] for i in range(len(parts[0]))]
    return Result(cat(fs), cat(zz), g[0].detach(), {k: t.detach() for k, t in zip(names, g[1:])})


def own_masks(res):
    """the float64 (or any) evaluation's own signs: z > 0 for the four activated stages, None for the logits"""
    return [[None if z is None else (z > 0) for z in row] for row in res.zs]


def masks_from_features(feats, z64=None):
    """feat > 0 for the four activated stages of each scale ([B, C, h, w] tensors; None for the logits).  An exact zero in
    a feature is either side: the float64 sign `z64[scale][layer] > 0` is taken there (plain False without z64)."""
    out = []
    for i, row in enumerate(feats):
        mrow = []
        for j, f in enumerate(row):
            if j == len(row) - 1:
                mrow.append(None)
                continue
            mk = f > 0
            if z64 is not None:
                zref = z64[i][j].to(f.device)
                mk = torch.where(f == 0, zref > 0, mk)
            mrow.append(mk)
        out.append(mrow)
    return out


def near_kink(z64, delta):
    """the elements of a stage whose float64 pre-activation lies within `delta` of the kink"""
    return z64.abs() <= delta


def rel_err(g, g64):
    """||g - g64||_2 / ||g64||_2 in float64"""
    g64 = g64.double().cpu()
    return ((g.double().cpu() - g64).norm() / g64.norm()).item()


def bound(e32):
    return max(FACTOR * e32, FLOOR)


def kink_delta(y32, y64):
    """near_kink's delta of a stage from its output in an fp32 evaluation and in float64 (module docstring)"""
    y64 = y64.double().cpu()
    return 5.0 * bound(rel_err(y32, y64)) * (y64.norm() / y64.numel() ** 0.5).item()


def kink_deltas(r32, r64):
    """[scale][layer] -> delta of the activated stages from an fp32 and the float64 evaluation (None for the logits)"""
    return [[None if z is None else kink_delta(y32, y64) for y32, y64, z in zip(frow32, frow64, zrow)]
            for frow32, frow64, zrow in zip(r32.feats, r64.feats, r64.zs)]


def near_kink_count(r64, deltas):
    return sum(int(near_kink(z, d).sum().item()) for zrow, drow in zip(r64.zs, deltas) for z, d in zip(zrow, drow) if z is not None)


def gradient_tensors(case, res):
    """{name: tensor} of what a case compares with float64: dx and, unless the form delivers no parameter gradients (a
    pass-through or frozen backward), every parameter gradient whose true value is not zero"""
    zero = set(zero_bias_names(case))
    out = {"dx": res.dx}
    if not (case.off or case.frozen):
        out.update({k: v for k, v in res.grads.items() if k not in zero})
    return out


# ------------------------------------------------------------------------------------------------------------------
# fp32 restatement of the backward pass train.py wires together, with injected faults
# ------------------------------------------------------------------------------------------------------------------
FAULTS = ("group_stats_whole_batch", "image_stats_shifted", "drop_mean_dy", "slope_on_positive", "bias_sum_dc",
          "skipped_rows_carry", "pool_div9")


def _conv_grads(x, w, dc, stride):
    """(dx, dw) of y = conv2d(x, w, stride, padding 2) by torch's own conv adjoints"""
    dx = torch.nn.grad.conv2d_input(x.shape, w, dc, stride=stride, padding=2)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dc, stride=stride, padding=2)
    return dx, dw


def restated_backward(case, data, masks, skip=0, fault=None, fault_layer=2, dtype=torch.float32):
    """What _ConvBlock.backward computes, layer by layer, restated with torch on the CPU: conv + bias, statistics per pass
    (batch norm) or per image (instance norm), affine, leaky ReLU forward; backward through the supplied masks, the norm's
    adjoint  dc = rstd (g - mean(g) - xhat mean(g xhat)),  g = gamma dy',  d beta = sum dy', d gamma = sum dy' xhat, an exactly
    zero bias gradient in front of a norm, torch's conv adjoints, the count_include_pad=False pool's adjoint; images below
    `skip` are left out of the backward and their rows of dx are zero.  fault: one of FAULTS, in layer `fault_layer` of every
    scale where a layer is meant.  -> Result (feats and zs of the forward, dx, gradients)."""
    assert fault is None or fault in FAULTS
    sd = {k: v.to(dtype) for k, v in data["sd"].items()}
    x0 = data["x"].to(dtype)
    B = x0.shape[0]
    if case.norm == "batch":
        groups = pass_slices(case)
    else:
        groups = [slice(b, b + 1) for b in range(B)]
    strides = [2] * N_LAYERS + [1, 1]
    grads = {}
    feats_all, zs_all = [], []
    xin = x0
    pools = []          # inputs of the pools, finest first
    per_scale = []
    for i in range(case.num_D):
        mi = case.num_D - 1 - i
        cur, saved, row, zrow = xin, [], [], []
        for j in range(N_LAYERS + 2):
            pre = "scale%d_layer%d" % (mi, j)
            w, b = sd[pre + ".0.weight"], sd[pre + ".0.bias"]
            c = F.conv2d(cur, w, b, stride=strides[j], padding=2)
            normed = 1 <= j <= N_LAYERS
            st = None
            if normed:
                gamma, beta = sd.get(pre + ".1.weight"), sd.get(pre + ".1.bias")
                mean, rstd = torch.empty(B, c.shape[1], 1, 1, dtype=dtype), torch.empty(B, c.shape[1], 1, 1, dtype=dtype)
                for sl in groups:
                    m_ = c[sl].mean((0, 2, 3), keepdim=True)
                    v_ = ((c[sl] - m_) ** 2).mean((0, 2, 3), keepdim=True)
                    mean[sl], rstd[sl] = m_, (v_ + 1e-5).rsqrt()
                xhat = (c - mean) * rstd
                z = xhat if gamma is None else xhat * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
                st = (mean, rstd, gamma)
            else:
                z = c
            y = F.leaky_relu(z, SLOPE) if j <= N_LAYERS else z
            saved.append((cur, w, c, st, pre, strides[j]))
            row.append(y)
            zrow.append(z if j <= N_LAYERS else None)
            cur = y
        feats_all.append(row)
        zs_all.append(zrow)
        per_scale.append(saved)
        if i != case.num_D - 1:
            pools.append(xin)
            xin = F.avg_pool2d(xin, 3, stride=2, padding=1, count_include_pad=False)
    live = slice(skip, B)
    dx_scales = []
    for i in range(case.num_D):
        saved = per_scale[i]
        dy = None
        for j in reversed(range(N_LAYERS + 2)):
            xj, w, c, st, pre, stride = saved[j]
            R = data["seeds"][i][j].to(dtype)
            dy = R[live] if dy is None else dy + R[live]
            if j <= N_LAYERS:
                mk = masks[i][j][live]
                if fault == "slope_on_positive" and j == fault_layer:
                    dy = dy * SLOPE
                else:
                    dy = torch.where(mk, dy, dy * SLOPE)
            if st is None:
                dc = dy
                grads[pre + ".0.bias"] = dc.sum((0, 2, 3))
            else:
                mean, rstd, gamma = st
                hit = j == fault_layer
                if fault == "group_stats_whole_batch" and hit:
                    m_ = c.mean((0, 2, 3), keepdim=True)
                    v_ = ((c - m_) ** 2).mean((0, 2, 3), keepdim=True)
                    mean, rstd = m_.expand_as(mean), (v_ + 1e-5).rsqrt().expand_as(rstd)
                if fault == "image_stats_shifted" and hit and skip:      # statistics of image i for image skip + i
                    mean = torch.cat([mean[:skip], mean[:B - skip]])
                    rstd = torch.cat([rstd[:skip], rstd[:B - skip]])
                xhat = ((c - mean) * rstd)[live]
                rs = rstd[live]
                if gamma is not None:
                    grads[pre + ".1.bias"] = dy.sum((0, 2, 3))
                    grads[pre + ".1.weight"] = (dy * xhat).sum((0, 2, 3))
                    g = dy * gamma.view(1, -1, 1, 1)
                else:
                    g = dy
                dc = torch.empty_like(g)
                for sl in groups:
                    lo, hi = max(sl.start, skip) - skip, sl.stop - skip
                    if hi <= lo:
                        continue
                    s_ = slice(lo, hi)
                    m1 = g[s_].mean((0, 2, 3), keepdim=True)
                    m2 = (g[s_] * xhat[s_]).mean((0, 2, 3), keepdim=True)
                    if fault == "drop_mean_dy" and hit:
                        m1 = torch.zeros_like(m1)
                    dc[s_] = rs[s_] * (g[s_] - m1 - xhat[s_] * m2)
                grads[pre + ".0.bias"] = dc.sum((0, 2, 3)) if (fault == "bias_sum_dc" and hit) else torch.zeros(c.shape[1], dtype=dtype)
            dxj, dw = _conv_grads(xj[live], w, dc, stride)
            grads[pre + ".0.weight"] = dw
            dy = dxj
        dxi = torch.zeros_like(saved[0][0])
        dxi[live] = dy
        if fault == "skipped_rows_carry" and skip:
            dxi[:skip] = dxi[skip:2 * skip]
        dx_scales.append(dxi)
    # the pools' adjoints, coarsest first: every input pixel of a window gets dy / (the window's count of inside pixels)
    dcur = dx_scales[-1]
    for i in reversed(range(case.num_D - 1)):
        xp = pools[i]
        ones = torch.ones(1, 1, xp.shape[2], xp.shape[3], dtype=dtype)
        cnt = F.avg_pool2d(ones, 3, stride=2, padding=1, count_include_pad=True) * 9.0
        if fault == "pool_div9":
            cnt = torch.full_like(cnt, 9.0)
        spread = F.conv_transpose2d((dcur / cnt).reshape(-1, 1, dcur.shape[2], dcur.shape[3]), torch.ones(1, 1, 3, 3, dtype=dtype),
                                    stride=2, padding=1,
                                    output_padding=(xp.shape[2] - ((dcur.shape[2] - 1) * 2 + 1), xp.shape[3] - ((dcur.shape[3] - 1) * 2 + 1)))
        dcur = dx_scales[i] + spread.reshape(xp.shape)
    return Result(feats_all, zs_all, dcur, grads)


# ------------------------------------------------------------------------------------------------------------------
# the figures file
# ------------------------------------------------------------------------------------------------------------------
def format_rows(case_id, rows, counts):
    """rows: [(tensor, hip error or None, fp32 shared-mask error, bound)], counts: {name: int} -> text lines"""
    out = ["%s  %s" % (case_id, "  ".join("%s=%d" % kv for kv in sorted(counts.items())))]
    for name, eh, e32, bnd in rows:
        hip = "%.3e" % eh if eh is not None else "    -    "
        ratio = "%.2f" % (eh / bnd) if eh is not None else " -  "
        out.append("    %-34s hip %s  fp32 %.3e  bound %.3e  hip/bound %s" % (name, hip, e32, bnd, ratio))
    return out
