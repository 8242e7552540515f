"""The Python layer that wires the kernels into the discriminators' backward pass (text2video_amd/train.py: _ConvBlock,
_norm_adjoint, _bias_gradient, _weight_gradient, _data_gradient, TrainableDiscriminator with groups / bn_times / pt_skip /
frozen) against float64 with SHARED kink masks: the sign of every activated stage output the HIP module returns is the slope
its backward used, and the float64 reference (tests/module_gradient_reference.py: the oracle module with a masked LeakyReLU
adjoint, evaluated by torch on the device) differentiates with those slopes.  No tensor is left out for being small, none
is allowed to be off because a LeakyReLU element near zero took the other slope.

Per case, in this order: forward (every stage output), masks (every disagreement with the float64 sign lies in the
near-kink set, at most KINK_CAP of them), backward (dx and every parameter gradient, tensor by tensor, ||g - g64|| / ||g64||
within 4 x what the same masked module gives in fp32 torch on the CPU, floor 8 u), exact facts (zero bias gradients in front
of a norm, zero rows of dx below pt_skip, zero storage channels of dx, no parameter gradient in the pass-through and frozen
forms) and, where the case is meant to reach a particular path, that it did."""
import contextlib

import pytest
import torch

import kernel_variants as kv
import module_gradient_reference as mg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _exact_fp32():
    """the float64 reference on the device: ATen's native kernels + rocBLAS (no MIOpen: the fp64 path has no solvers)"""
    old = (torch.backends.cudnn.enabled, torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.enabled = False
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cudnn.enabled, torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = old


class _Calls:
    """counts the calls of the ops entries a case is meant to reach (restored on exit)"""

    def __init__(self):
        self.norm_backward, self.zero_rows, self.wgrad_batches, self.kernels = [], [], [], set()

    @contextlib.contextmanager
    def watching(self, profile):
        from text2video_amd import ops
        nb, zr, wg = ops.instance_norm_backward, ops.zero_, ops.conv2d_backward_weight

        def norm_backward(x, dy, mr, *a, **k):
            self.norm_backward.append((x.shape[0] if x.dim() == 4 else 1, k.get("out") is not None))
            return nb(x, dy, mr, *a, **k)

        def zero_(x):
            self.zero_rows.append(x.shape[0])
            return zr(x)

        def wgrad(x, dy, *a, **k):
            self.wgrad_batches.append(x.shape[0] if x.dim() == 4 else 1)
            return wg(x, dy, *a, **k)
        ops.instance_norm_backward, ops.zero_, ops.conv2d_backward_weight = norm_backward, zero_, wgrad
        try:
            if profile:
                torch.cuda.synchronize()
                with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                    yield
                    torch.cuda.synchronize()
                self.kernels = {kv.family(e.name) for e in prof.events() if "t2v::" in e.name}
            else:
                yield
        finally:
            ops.instance_norm_backward, ops.zero_, ops.conv2d_backward_weight = nb, zr, wg


def _hip_run(case, data):
    """-> (feats[scale][layer] as [B, C, h, w] on the device, dx [B, H, W, xcs], {name: gradient or None}, the module's
    parameters, _Calls of the backward pass).  The forms as the trainer uses them: inside a batched_weight_gradients scope,
    the pass-through backward under param_gradients_off, the gradients flushed after the pass."""
    from text2video_amd import ops, train as T
    hip = T.TrainableDiscriminator(case.cin, data["sd"], case.ndf, mg.N_LAYERS, case.num_D, case.norm, DEV)
    named = hip.named_upstream_parameters()
    params = list(named.values())
    xh = mg.to_nhwc(data["x"], case.xcs).to(DEV).requires_grad_(True)
    seeds = [[mg.to_nhwc(R, ops.round_up(R.shape[1], 4)).to(DEV) for R in row] for row in data["seeds"]]
    calls = _Calls()
    with T.batched_weight_gradients(params):
        if case.calls > 1:
            parts = [hip(xh[sl]) for sl in mg.pass_slices(case)]
            outs = [f for p in parts for row in p for f in row]
            sds = [R[sl] for sl in mg.pass_slices(case) for row in seeds for R in row]
            feats = [[torch.cat([p[i][j] for p in parts]) for j in range(len(parts[0][i]))] for i in range(len(parts[0]))]
        else:
            feats = hip(xh, frozen=case.frozen, groups=case.groups, bn_times=case.bn_times, pt_skip=case.pt_skip)
            outs = [f for row in feats for f in row]
            sds = [R for row in seeds for R in row]
        with calls.watching(profile=case.id == "two_calls"):
            with (T.param_gradients_off(params) if case.off else contextlib.nullcontext()):
                g = torch.autograd.grad(outs, [xh] + params, grad_outputs=sds, allow_unused=True)
            gp = T.flush_pending_weight_gradients(params, g[1:])
    torch.cuda.synchronize()
    ops.check_async_errors()
    shapes = mg.stage_shapes(case)
    feats = [[mg.to_nchw(f.detach(), shapes[i][j][0]) for j, f in enumerate(row)] for i, row in enumerate(feats)]
    return feats, g[0], dict(zip(named.keys(), gp)), params, calls


@pytest.mark.parametrize("case", mg.CASES, ids=[c.id for c in mg.CASES])
def test_discriminator_gradients_against_float64_with_shared_masks(case):
    data = mg.build_case(case)
    skip = case.pt_skip if case.off else 0
    r64 = mg.reference(case, data, torch.float64, DEV, skip=skip)
    r32 = mg.reference(case, data, torch.float32, "cpu", skip=skip)
    feats, dx, grads, params, calls = _hip_run(case, data)
    failures, lines = [], []

    # 1. forward
    rows = []
    for i, row in enumerate(feats):
        for j, f in enumerate(row):
            assert f.shape == r64.feats[i][j].shape, (i, j, f.shape, r64.feats[i][j].shape)
            eh, e32 = mg.rel_err(f, r64.feats[i][j]), mg.rel_err(r32.feats[i][j], r64.feats[i][j])
            rows.append(("feat[%d][%d]" % (i, j), eh, e32, mg.bound(e32)))
    failures += ["forward %s: %.3e > %.3e" % (n, eh, b) for n, eh, _, b in rows if not eh <= b]

    # 2. masks
    deltas = mg.kink_deltas(r32, r64)
    masks = mg.masks_from_features(feats, r64.zs)
    own = mg.own_masks(r64)
    differ = outside = 0
    for i, row in enumerate(masks):
        for j, mk in enumerate(row):
            if mk is None:
                continue
            d = mk != own[i][j]
            differ += int(d.sum().item())
            outside += int((d & ~mg.near_kink(r64.zs[i][j], deltas[i][j])).sum().item())
    counts = {"near_kink": mg.near_kink_count(r64, deltas), "mask_disagreements": differ, "outside_near_kink": outside}

    # 3. backward, under the HIP masks
    r64m = mg.reference(case, data, torch.float64, DEV, masks=masks, skip=skip)
    r32m = mg.reference(case, data, torch.float32, "cpu", masks=[[None if m is None else m.cpu() for m in row] for row in masks],
                        skip=skip)
    want_params = not (case.off or case.frozen)
    g64, g32 = mg.gradient_tensors(case, r64m), mg.gradient_tensors(case, r32m)
    got = {"dx": mg.to_nchw(dx, case.cin)}
    got.update({k: grads[k] for k in g64 if k != "dx"})
    assert len(g64) == (1 + len(grads) - len(mg.zero_bias_names(case)) if want_params else 1)
    brow = []
    for k in g64:
        assert got[k] is not None, "%s: no gradient delivered" % k
        assert got[k].shape == g64[k].shape, (k, got[k].shape, g64[k].shape)
        eh, e32 = mg.rel_err(got[k], g64[k]), mg.rel_err(g32[k], g64[k])
        brow.append((k, eh, e32, mg.bound(e32)))
    failures += ["backward %s: %.3e > %.3e" % (n, eh, b) for n, eh, _, b in brow if not eh <= b]
    lines = mg.format_rows(case.id, rows + brow, counts)
    print("\n" + "\n".join("MODGRAD " + ln for ln in lines))

    assert outside == 0 and differ <= mg.KINK_CAP, counts
    assert not failures, failures

    # 4. exact facts
    if want_params:
        for k in mg.zero_bias_names(case):
            assert grads[k] is not None and torch.count_nonzero(grads[k]).item() == 0, k
            wk = k.replace(".0.bias", ".0.weight")
            assert r64m.grads[k].norm().item() <= 1e-9 * r64m.grads[wk].norm().item(), k
    else:
        assert all(v is None for v in grads.values()), [k for k, v in grads.items() if v is not None]
        assert all(p.grad is None for p in params)
    if skip:
        assert torch.count_nonzero(dx[:skip]).item() == 0
        assert torch.count_nonzero(dx[skip:]).item() > 0
    if case.xcs > case.cin:
        assert torch.count_nonzero(dx[..., case.cin:]).item() == 0

    # 5. the path the case is for
    n_norm = mg.N_LAYERS * case.num_D          # normed layers, all scales
    n_conv = (mg.N_LAYERS + 2) * case.num_D
    if case.id in ("grouped3", "passthrough"):
        gB, live = case.B // case.groups, case.groups - skip // (case.B // case.groups)
        assert calls.norm_backward == [(gB, True)] * (n_norm * live), calls.norm_backward
    if case.id == "passthrough_in":
        assert calls.norm_backward == [(1, True)] * (n_norm * (case.B - skip)), calls.norm_backward
    if skip:
        assert calls.zero_rows == [skip] * n_conv, calls.zero_rows      # the img0 zero fill of every layer's dx
        assert calls.wgrad_batches == []
    if case.id == "two_calls":
        # the paired path: the two uses of a layer reduce in ONE launch over both calls' images
        assert calls.wgrad_batches == [case.B] * n_conv, calls.wgrad_batches
        assert "conv_wgrad_kernel" in calls.kernels, sorted(calls.kernels)
    if case.id == "plain_bn":
        assert calls.wgrad_batches == [case.B] * n_conv and calls.norm_backward == [(case.B, False)] * n_norm
    if case.id == "wide_storage":
        from text2video_amd import ops
        assert ops.round_up(case.cin, 4) != case.xcs
