"""The generators' backward pass (text2video_amd/train.py: TrainableGenerator, TrainableLocalGenerator, TwoScaleGenerator
through _ConvBlock, _CatParams, _WarpComposite; text2video_amd/gradients.py: the Winograd-domain weight gradient reduced on
the spot, collected over the frames, with the kept input transform and the lazy gradient in front of the norm, the transposed
data gradient, the paired direct weight gradient, the flush) against float64 with SHARED ReLU masks: the sign of every
relu=1 norm-apply output of the HIP forward is the decision its backward takes, and the float64 reference
(tests/generator_gradient_reference.py: the oracle with masked ReLU sites, evaluated by torch on the device) differentiates
with those decisions.  No tensor is left out for being small, none is allowed to be off because a ReLU element near zero
fell on the other side.

Per case, in this order: forward (fake, raw, flow, weight and every ReLU layer's output), masks (every disagreement with the
float64 sign lies in the near-kink set), backward (every parameter gradient -- and the coarse-feature gradients of the G1
cases -- tensor by tensor, ||g - g64|| / ||g64|| within 4 x what the YARDSTICK gives: the same masked module in fp32 torch on
the CPU with the ResnetBlock convs restated in the noisiest Winograd form the HIP path takes, floor 8 u), exact facts (zero
bias gradients in front of a norm, no gradient for G0's heads in the pair, none for a frozen G0) and that the path the case
is for was reached.  `step2` cases run two steps with unchanged weights and compare both with the one reference;
g0_fewer_uses runs its first step with the flow branch on both frames (so that two uses are expected) and compares the
second, which runs it once.

Measured on an MI355X (profiles/generator_gradients_float64.txt has every row): all 972 rows inside their bounds, hip/bound
at most 0.57 (the second norm bias of the encoders' ResnetBlock in g0_ragged_step), median 0.27; mask disagreements 0 in the
direct and F(2x2) cases and 1 .. 4 of 1.4 .. 4.4 million ReLU elements where F(4x4) runs, all of them near the kink; 0.1 .. 0.7 s per case (2.3 s for the first, which loads the library)."""
import contextlib

import pytest
import torch

import generator_gradient_reference as gg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COUNTED = ("conv2d_backward_weight_pair", "conv2d_backward_weight_winograd", "conv2d_backward_weight_winograd_stages",
           "conv2d_backward_weight_winograd_dy_norm", "conv2d_backward_weight_winograd_reduce", "conv2d_backward_data_winograd",
           "avgpool3x3s2")


@pytest.fixture(autouse=True)
def _exact_fp32():
    """the float64 reference on the device: ATen's native kernels + rocBLAS (no MIOpen: the fp64 path has no solvers)"""
    old = (torch.backends.cudnn.enabled, torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.enabled = False
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cudnn.enabled, torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = old


class _Watch:
    """wraps ops entries (restored on exit): records the output of every relu=1 norm-apply call while `recording`, counts
    the calls of the entries a case is meant to reach"""

    def __init__(self):
        self.sites, self.with_res, self.recording = [], 0, False
        self.calls = {k: 0 for k in COUNTED}
        self.forward_weights, self.unfilled = [], []

    @contextlib.contextmanager
    def watching(self):
        from text2video_amd import gradients, ops
        saved = {k: getattr(ops, k) for k in COUNTED + ("instance_norm_apply",)}
        zero_unfilled = gradients._zero_unfilled_slots
        apply_ = saved["instance_norm_apply"]

        def norm_apply(x, mean_rstd, gamma=None, beta=None, res1=None, res2=None, relu=False, out=None, nimg=None):
            y = apply_(x, mean_rstd, gamma, beta, res1=res1, res2=res2, relu=relu, out=out, nimg=nimg)
            if self.recording and int(relu) == 1:
                assert res2 is None and nimg is None
                t = y
                if res1 is not None:
                    # y = relu(norm(c)) + res: the same elementwise, stateless entry once more without the residual gives the
                    # forward's own decision bits
                    t = apply_(x, mean_rstd, gamma, beta, res1=None, relu=relu, out=torch.empty_like(y))
                    self.with_res += 1
                self.sites.append(t)
            return y

        def counted(name):
            def call(*a, **k):
                self.calls[name] += 1
                if name == "conv2d_backward_data_winograd":
                    self.forward_weights.append(bool(k.get("forward_weights", False)))
                return saved[name](*a, **k)
            return call

        def zero_unfilled_slots(col):
            self.unfilled.append(sum(1 for f in col.filled if not f))
            return zero_unfilled(col)

        ops.instance_norm_apply = norm_apply
        for k in COUNTED:
            setattr(ops, k, counted(k))
        gradients._zero_unfilled_slots = zero_unfilled_slots
        try:
            yield self
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
            gradients._zero_unfilled_slots = zero_unfilled


def _build_hip(case, data):
    """-> (module, {name as the reference names it: parameter})"""
    from text2video_amd import train as T
    sp = gg.specs(case)
    if case.net == "g0":
        net = T.TrainableGenerator(sp[0], data["sds"][0], DEV)
        named = dict(net.named_upstream_parameters())
    elif case.net == "g1":
        net = T.TrainableLocalGenerator(sp[0], data["sds"][0], DEV)
        named = dict(net.named_upstream_parameters())
    else:
        net = T.TwoScaleGenerator(T.TrainableGenerator(sp[0], data["sds"][0], DEV), T.TrainableLocalGenerator(sp[1], data["sds"][1], DEV))
        named = {"G0." + k: p for k, p in net.G0.named_upstream_parameters().items()}
        named.update({"G1." + k: p for k, p in net.G1.named_upstream_parameters().items()})
        if case.frozen:
            for p in net.G0.parameters():
                p.requires_grad_(False)
    return net, named


def _hip_step(case, data, net, named, frames):
    """one forward / backward of the case's frames in its form -> (outs[frame] {name: [1, C, H, W]}, sites[frame]: per ReLU
    site the layer's output [1, C, h, w] or None where the HIP forward did not run it, {name: gradient or None}, _Watch)"""
    from text2video_amd import ops, train as T
    trained = {k: p for k, p in named.items() if p.requires_grad}
    params = list(trained.values())
    HW = float(case.H * case.W)
    watch = _Watch()
    scope = contextlib.nullcontext() if case.form == "plain" else T.batched_weight_gradients(params)
    outs, sites, heads, coarse = [], [], [], []
    with watch.watching(), scope:
        for fr, (raw_only, need_flow) in zip(data["frames"], frames):
            pose, prev = gg.to_nhwc(fr["pose"], 12).to(DEV), gg.to_nhwc(fr["prev"], 8).to(DEV)
            watch.sites, watch.recording = [], True
            if case.net == "g0":
                fake, raw, fw = net(pose, prev, use_raw_only=raw_only, full=True, need_flow=need_flow)
            elif case.net == "g1":
                ic = gg.to_nhwc(fr["img_c"], case.ngf_global).to(DEV).requires_grad_(True)
                fc = None if case.no_flow else gg.to_nhwc(fr["flow_c"], case.ngf_global).to(DEV).requires_grad_(True)
                coarse += [("img_feat_coarse", ic)] + ([] if fc is None else [("flow_feat_coarse", fc)])
                fake, raw, fw = net(pose, prev, ic, fc, use_raw_only=raw_only, full=True, need_flow=need_flow)
            else:
                fake, raw, fw, fake0, _ = net(pose, (prev, gg.to_nhwc(fr["prev0"], 8).to(DEV)), use_raw_only=raw_only,
                                              need_flow=need_flow)
                assert not fake0.requires_grad
            watch.recording = False
            if case.no_flow:
                assert raw is None and fw is None       # (raw, None, None)
            raw = fake if raw is None else raw
            assert (fake is raw) == (raw_only or case.no_flow)
            out = {"fake": gg.to_nchw(fake.detach(), 3), "raw": gg.to_nchw(raw.detach(), 3)}
            seeds = [(fake, gg.to_nhwc(fr["R_fake"], 4).to(DEV) / HW), (raw, gg.to_nhwc(fr["R_raw"], 4).to(DEV) / HW)]
            if not case.no_flow and need_flow:
                out.update(flow=gg.to_nchw(fw.detach(), 3)[:, :2], weight=gg.to_nchw(fw.detach(), 3)[:, 2:3])
                # flow_w is (flow_x, flow_y, weight, 0): the padding channel's seed is zero
                seeds.append((fw, gg.to_nhwc(torch.cat([fr["R_flow"], fr["R_weight"]], 1), 4).to(DEV) / HW))
            else:
                assert fw is None
            for t, s in seeds:      # (fake is raw in a raw-only frame: one output, the two seeds added)
                hit = [i for i, (u, _) in enumerate(heads) if u is t]
                if hit:
                    heads[hit[0]] = (t, heads[hit[0]][1] + s)
                else:
                    heads.append((t, s))
            outs.append(out)
            # the sites: per net the ones it ran, in order, then None for a flow branch it left out
            row, k = [], 0
            for sp, (H, W) in zip(gg.specs(case), gg.net_sizes(case)):
                ran, full = gg.site_shapes(sp, H, W, flow=need_flow), gg.site_shapes(sp, H, W)
                for (C, h, w) in ran:
                    t = watch.sites[k]
                    k += 1
                    t = t.unsqueeze(0) if t.dim() == 3 else t
                    assert tuple(t.shape) == (1, h, w, C), (len(row), tuple(t.shape), (C, h, w))
                    row.append(gg.to_nchw(t.detach(), C))
                row += [None] * (len(full) - len(ran))
            assert k == len(watch.sites), (k, len(watch.sites))
            sites.append(row)
        wanted = params + [t for _, t in coarse]
        g = torch.autograd.grad([t for t, _ in heads], wanted, grad_outputs=[s for _, s in heads], allow_unused=True)
        gp = list(g[:len(params)])
        if case.form != "plain":
            gp = T.flush_pending_weight_gradients(params, gp)
    torch.cuda.synchronize()
    ops.check_async_errors()
    grads = dict(zip(trained.keys(), gp))
    for (k, t), gi in zip(coarse, g[len(params):]):
        assert gi.shape[-1] == case.ngf_global      # (the coarse features carry no padding channel)
        grads[k] = gg.to_nchw(gi, case.ngf_global)
    return outs, sites, grads, watch


@pytest.mark.parametrize("case", gg.CASES, ids=[c.id for c in gg.CASES])
def test_generator_gradients_against_float64_with_shared_masks(case, monkeypatch):
    from text2video_amd import gradients, ops
    if case.direct:
        monkeypatch.setenv("T2V_CONV_ALGO", "1")
    else:
        monkeypatch.delenv("T2V_CONV_ALGO", raising=False)
    algos = gg.layer_algorithms(case)            # (also: no layer of the case takes the polyphase form)
    assert tuple(a["level"] for a in algos) == case.wino, [(a["fwd"], a["dgrad"], a["transposed"]) for a in algos]
    data = gg.build_case(case)
    r64 = gg.evaluate(case, data, torch.float64, DEV)
    y32 = gg.evaluate(case, data, torch.float32, "cpu", yardstick=True)
    net, named = _build_hip(case, data)
    steps = []
    if case.id == "g0_fewer_uses":
        # two uses of the flow branch are expected from here on (not compared: another loss)
        _hip_step(case, data, net, named, [(True, True)] * len(case.frames))
    else:
        steps.append(_hip_step(case, data, net, named, case.frames))
    if case.form == "step2":
        steps.append(_hip_step(case, data, net, named, case.frames))
    deltas = gg.kink_deltas(y32, r64)
    failures, refs = [], None
    for n, (outs, sites, grads, watch) in enumerate(steps):
        # (g0_fewer_uses compares its second step alone)
        tag = case.id if case.form != "step2" else "%s step %d" % (case.id, n + 1 + (2 - len(steps)))
        # 1. forward
        rows = []
        for f, out in enumerate(outs):
            assert set(out) == set(r64.outs[f])
            for k in gg.OUT_NAMES:
                if k in out:
                    assert out[k].shape == r64.outs[f][k].shape, (k, out[k].shape)
                    e32 = gg.rel_err(y32.outs[f][k], r64.outs[f][k])
                    rows.append(("%s[%d]" % (k, f), gg.rel_err(out[k], r64.outs[f][k]), e32, gg.bound(e32)))
            assert len(sites[f]) == len(r64.zs[f])
            for i, y in enumerate(sites[f]):
                if y is not None:
                    y64 = torch.relu(r64.zs[f][i])
                    e32 = gg.rel_err(torch.relu(y32.zs[f][i]), y64)
                    rows.append(("relu[%d][%d]" % (f, i), gg.rel_err(y, y64), e32, gg.bound(e32)))
        failures += ["%s forward %s: %.3e > %.3e" % (tag, nm, eh, b) for nm, eh, _, b in rows if not eh <= b]

        # 2. masks
        masks = [[None if y is None else (y > 0) for y in row] for row in sites]
        differ = outside = near = sited = 0
        for f, row in enumerate(masks):
            for i, mk in enumerate(row):
                if mk is None:
                    continue
                z64 = r64.zs[f][i]
                assert mk.shape == z64.shape, (f, i, mk.shape, z64.shape)
                nk = gg.near_kink(z64, deltas[f][i])
                d = mk != (z64 > 0)
                differ += int(d.sum().item())
                outside += int((d & ~nk).sum().item())
                near += int(nk.sum().item())
                sited += mk.numel()
        counts = {"relu_elements": sited, "near_kink": near, "mask_disagreements": differ, "outside_near_kink": outside}

        # 3. backward, under the HIP masks (a second step with the same masks: the same reference)
        if refs is None or not all((a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))
                                   for ra, rb in zip(refs[0], masks) for a, b in zip(ra, rb)):
            r64m = gg.evaluate(case, data, torch.float64, DEV, masks=masks)
            y32m = gg.evaluate(case, data, torch.float32, "cpu", yardstick=True,
                               masks=[[None if m is None else m.cpu() for m in row] for row in masks])
            refs = (masks, r64m, y32m)
        _, r64m, y32m = refs
        g64 = gg.gradient_tensors(case, r64m)
        bnd = gg.bounds(case, y32m, r64m)
        brow = []
        for k in g64:
            assert grads.get(k) is not None, "%s: no gradient delivered" % k
            assert grads[k].shape == g64[k].shape, (k, grads[k].shape, g64[k].shape)
            brow.append((k, gg.rel_err(grads[k], g64[k]), bnd[k][0], bnd[k][1]))
        failures += ["%s backward %s: %.3e > %.3e" % (tag, nm, eh, b) for nm, eh, _, b in brow if not eh <= b]
        print("\n" + "\n".join("GENGRAD " + ln for ln in gg.format_rows(tag, rows + brow, counts)))
        assert outside == 0, counts

        # 4. exact facts
        zero = [k for k in gg.zero_bias_names(case) if k in r64m.grads]
        assert len(g64) + len(zero) == sum(1 for v in r64m.grads.values() if v is not None)
        for k in zero:
            assert grads[k] is not None and torch.count_nonzero(grads[k]).item() == 0, k
            assert r64m.grads[k].norm().item() <= 1e-9 * r64m.grads[k.replace(".bias", ".weight")].norm().item(), k
        absent = sorted(k for k, v in grads.items() if v is None)
        assert absent == sorted(k for k, v in r64m.grads.items() if v is None)
        if case.net == "pair":
            assert case.frozen or (len(absent) == 6 and all(k.startswith("G0.model_final_") for k in absent))
            assert not case.frozen or not any(k.startswith("G0.") for k in grads)
        assert all(p.grad is None for p in named.values())

        # 5. the path the case is for
        c, a = watch.calls, algos[-1]
        nres = sum(2 for k in named if k.endswith("conv_block.1.weight"))          # 3x3 stride-1 layers, all nets
        uses = len(case.frames)
        if case.direct:
            assert all(c[k] == 0 for k in COUNTED if "winograd" in k), c
        if case.id == "g0_direct_pair_in":
            assert c["conv2d_backward_weight_pair"] > 0 and data["sds"][0].get("model_down_seg.2.weight") is None, c
        if case.id == "g0_wino":
            # no step scope: each node reduces on the spot; the data gradient is the full-correlation F(4x4) convolution
            assert a["fwd"] == a["dgrad"] == ops.ALGO_WINOGRAD_F4
            assert c["conv2d_backward_weight_winograd"] == nres and c["conv2d_backward_weight_winograd_stages"] == 0, c
            assert c["conv2d_backward_data_winograd"] == 0, c
        if case.id == "g0_ragged_step":
            h, w = a["desc"].H, a["desc"].W
            assert a["fwd"] == ops.ALGO_WINOGRAD_F4 and h % 4 and w % 4 and not a["transposed"]
            assert c["conv2d_backward_weight_winograd_stages"] == nres * uses, c
            assert c["conv2d_backward_weight_winograd"] == c["conv2d_backward_weight_winograd_dy_norm"] == 0, c
            assert c["conv2d_backward_data_winograd"] == 0, c
        if case.id == "g0_kept_lazy":
            assert a["fwd"] == ops.ALGO_WINOGRAD_F4 and a["transposed"]
            assert c["conv2d_backward_data_winograd"] == nres * uses, c
            want_fw = a["takes_forward_weights"] and gradients.switch("T2V_DGRAD_FORWARD_WEIGHTS")
            assert watch.forward_weights == [bool(want_fw)] * (nres * uses), (want_fw, watch.forward_weights)
            if n == 0:      # no expectation yet: the collected, un-kept form
                assert c["conv2d_backward_weight_winograd_stages"] == nres * uses and c["conv2d_backward_weight_winograd_dy_norm"] == 0, c
            else:           # V kept by the forward pass, the gradient in front of the norm formed inside the transform of dy
                assert c["conv2d_backward_weight_winograd_dy_norm"] == nres * uses and c["conv2d_backward_weight_winograd_stages"] == 0, c
                assert c["conv2d_backward_weight_winograd_reduce"] == nres, c
        if case.id == "g0_fewer_uses":
            # the flow branch's ResnetBlock (2 layers) filled one of its two kept slots: the other one zeroed before the reduction
            assert sorted(watch.unfilled) == [0] * (nres - 2) + [1] * 2, watch.unfilled
            assert c["conv2d_backward_weight_winograd_reduce"] == nres, c
        if case.net == "g1":
            assert watch.with_res == 1      # relu(norm(c)) + res in the second encoder
        if case.net == "pair":
            assert c["avgpool3x3s2"] == uses and watch.with_res == uses
            assert algos[0]["fwd"] == ops.ALGO_DIRECT and a["fwd"] == ops.ALGO_WINOGRAD_F4
            assert c["conv2d_backward_weight_winograd_stages"] > 0 and c["conv2d_backward_data_winograd"] > 0, c
    assert not failures, failures
