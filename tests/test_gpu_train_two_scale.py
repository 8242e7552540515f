"""Two-scale training (--n_scales_spatial 2, --niter_fix_global) on the GPU: the local enhancer G1 alone and one train
iteration of G0 + G1 + the multiscale discriminator against torch autograd over the CPU oracle modules, the frozen phase,
and the trainer end to end (determinism, the G0 / G1 checkpoint pair through Vid2VidModelG, the carried FIFOs).

Bounds (tests/test_gpu_train_step.py's): frames <= 1e-4, losses <= 1e-4 relative, gradient error relative to the tensor's
max <= 2e-3 worst with a median <= 1e-4 where every ResnetBlock conv is direct and <= 4e-4 where Winograd runs; gradients
whose reference max is <= 1e-5 are skipped, and only conv biases in front of a norm (mathematically zero) may be.

Seeds.  The bounds assume no pre-activation on a ReLU / LeakyReLU kink, so each case's seed was searched on the CPU: the
oracle evaluated in fp32 and in fp64, a seed kept only where fp32-against-fp64 stays inside HALF of every bound above.
Outcome (seeds 11, 12, 13 for each G1 case; 3, 4, 5 for the pair; all nine passed, the first of each is used):
  G1 cases, seed 11: gradients worst 1.4e-6 .. 3.7e-6, median 0.7e-6 .. 1.0e-6 of the tensor's max; the smallest
      non-bias gradient has max 6e-4 (nothing but the zero-gradient biases falls under the 1e-5 skip rule);
  G0 + G1 + D, seed 3: frames 4e-6, gradients worst 1.7e-5 (G1.model_final_flow.1.bias), median 1.9e-6; 102 tensors
      compared, 32 zero-gradient biases skipped, smallest other gradient max 2.6e-3.
"""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand(*shape, seed=0, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def _nhwc(x_bchw, cs):
    """[B,C,H,W] cpu -> [B,H,W,cs] device"""
    B, C, H, W = x_bchw.shape
    out = torch.zeros(B, H, W, cs, device="cuda:0")
    out[..., :C] = x_bchw.detach().float().permute(0, 2, 3, 1).cuda()
    return out


def _nchw(t, c):
    """[B,H,W,cs] device -> [B,c,H,W] cpu"""
    return t.detach()[..., :c].permute(0, 3, 1, 2).cpu()


from oracle.optim_ref import adam_041_step as _adam_041   # pinned to the reference's torch-0.4.1 adam.py


def _zero_gradient_biases(spec):
    """conv biases in front of a norm layer: the norm removes the channel mean, their gradient is rounding noise"""
    from text2video_amd.generator import layer_keys
    return {ck + ".bias" for ck, nk, _ in layer_keys(spec) if nk is not None}


def _compare_gradients(got, ref, may_skip, median_bound, tag, scale=1.0):
    """got / ref: {name: gradient}; -> (worst, median) of the errors relative to each reference tensor's max.  `scale` < 1:
    the seed search's half bounds."""
    errs, skipped = {}, set()
    for k, r in ref.items():
        assert got[k] is not None, (tag, k)
        if r.abs().max().item() <= 1e-5:
            skipped.add(k)
            continue
        errs[k] = (got[k].double().cpu() - r.double()).abs().max().item() / r.abs().max().item()
    assert skipped <= may_skip, (tag, "skipped beyond the zero-gradient biases", sorted(skipped - may_skip))
    worst, med = max(errs.values()), float(np.median(list(errs.values())))
    top = sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    print(tag, "largest relative gradient errors:", ["%s %.1e" % kv for kv in top], "median %.1e" % med,
          "(%d tensors, %d skipped)" % (len(errs), len(skipped)))
    assert worst <= 2e-3 * scale and med <= median_bound * scale, (tag, worst, med)
    return worst, med


# ------------------------------------------------------------------------------------------------------------------
# (a) G1 alone
# ------------------------------------------------------------------------------------------------------------------
# (H, W, ngf_global, n_blocks_local, norm, no_flow, seed)
G1_CASES = {
    "32x32_ngf64_winograd-batch_flow": (32, 32, 64, 2, "batch", False, 11),
    "32x32_ngf64_winograd-instance_noflow": (32, 32, 64, 2, "instance", True, 11),
    "32x48_ngf32-batch_flow": (32, 48, 32, 1, "batch", False, 11),
    "32x48_ngf32-instance_noflow": (32, 48, 32, 1, "instance", True, 11),
}


def _g1_spec(case):
    from text2video_amd.generator import GeneratorSpec
    H, W, ngf_global, blocks, norm, no_flow, seed = case
    return GeneratorSpec(ngf=ngf_global // 2, n_blocks=blocks, no_flow=no_flow, norm=norm, is_local=True, scale=1)


def _g1_inputs(case):
    H, W, ngf_global, blocks, norm, no_flow, seed = case
    inp = {"pose": _rand(1, 9, H, W, seed=seed + 1).clamp(-1, 1),
           # non-zero previous frames: an all-zero prev image makes the image encoder's norm layers 0/0
           "prev": torch.tanh(_rand(1, 6, H, W, seed=seed + 2)),
           # the coarse scale's decoder outputs are relu(norm(.)): non-negative, unit scale
           "img_c": torch.relu(_rand(1, ngf_global, H // 2, W // 2, seed=seed + 3)),
           "flow_c": torch.relu(_rand(1, ngf_global, H // 2, W // 2, seed=seed + 4))}
    # the loss: a fixed linear functional of every output (the coefficients play the role of a loss network's gradient)
    for i, (name, c) in enumerate((("fake", 3), ("raw", 3), ("flow", 2), ("weight", 1))):
        inp["d_" + name] = _rand(1, c, H, W, seed=seed + 5 + i)
    return inp


def _g1_oracle(case, dtype=torch.float32):
    """-> (outputs {name: tensor}, loss, gradients {parameter name | img_feat_coarse | flow_feat_coarse: tensor})"""
    from oracle.generator_ref import CompositeLocalGenerator
    from text2video_amd.generator import synthetic_state_dict
    H, W, ngf_global, blocks, norm, no_flow, seed = case
    # flow_gain 0.05: flows of a few pixels behind this scale's x40 multiplier, as a trained network predicts
    sd = synthetic_state_dict(_g1_spec(case), seed, "vid2vid", flow_gain=0.05)
    net = CompositeLocalGenerator(9, 3, 6, ngf_global, blocks, 1, no_flow, norm).train()
    missing = net.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all("running_" in k or "num_batches" in k for k in missing.missing_keys)
    net = net.to(dtype)
    inp = {k: v.to(dtype) for k, v in _g1_inputs(case).items()}
    ic, fc = inp["img_c"].requires_grad_(), inp["flow_c"].requires_grad_()
    fake, flow, weight, raw, _, _ = net(inp["pose"], inp["prev"], ic, fc, False)
    outs = {"fake": fake, "raw": raw}
    if not no_flow:
        outs.update(flow=flow, weight=weight)
        assert flow.abs().max().item() < 8.0 and flow.abs().mean().item() > 0.05
    loss = sum((v * inp["d_" + k]).sum() for k, v in outs.items()) / (H * W)
    names = [k for k, _ in net.named_parameters()] + ["img_feat_coarse"] + ([] if no_flow else ["flow_feat_coarse"])
    grads = torch.autograd.grad(loss, list(net.parameters()) + [ic] + ([] if no_flow else [fc]))
    return {k: v.detach() for k, v in outs.items()}, loss.detach(), dict(zip(names, grads)), sd


def _g1_winograd(case):
    """whether the ResnetBlock convs of this case leave the direct kernel (the median bound follows)"""
    from text2video_amd import ops
    H, W, ngf_global = case[:3]
    return ops.best_conv_algo(ops.conv_desc(H // 2, W // 2, ngf_global, ngf_global, 3, 1, 1, ops.PAD_REFLECT), ngf_global)


@pytest.mark.parametrize("name", list(G1_CASES))
def test_local_generator_matches_autograd_oracle(name):
    from text2video_amd import ops
    from text2video_amd import train as T
    case = G1_CASES[name]
    H, W, ngf_global, blocks, norm, no_flow, seed = case
    algo = _g1_winograd(case)
    if ngf_global == 64:    # 64-channel ResnetBlock convs on a 16x16 map: Winograd F(2x2,3x3), forward and data gradient
        assert algo == ops.ALGO_WINOGRAD
    ref_out, ref_loss, ref_g, sd = _g1_oracle(case)
    spec = _g1_spec(case)
    net = T.TrainableLocalGenerator(spec, sd, "cuda:0")
    inp = _g1_inputs(case)
    ic = _nhwc(inp["img_c"], ngf_global).requires_grad_()
    fc = _nhwc(inp["flow_c"], ngf_global).requires_grad_()
    fake, raw, fw = net(_nhwc(inp["pose"], 12), _nhwc(inp["prev"], 8), ic, None if no_flow else fc, use_raw_only=False,
                        full=True)
    got_out = {"fake": fake[..., :3], "raw": fake[..., :3] if no_flow else raw[..., :3]}
    if no_flow:
        assert raw is None and fw is None
    else:
        got_out.update(flow=fw[..., :2], weight=fw[..., 2:3])
    for k, r in ref_out.items():
        err = (_nchw(got_out[k], r.shape[1]) - r).abs().max().item()
        print(name, k, "max |delta| %.1e" % err)
        # (flow is in pixels: relative to its size)
        assert err <= 1e-4 * (max(1.0, r.abs().max().item()) if k == "flow" else 1.0), (k, err)
    loss = sum((got_out[k] * _nhwc(inp["d_" + k], r.shape[1])).sum() for k, r in ref_out.items()) / (H * W)
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * max(1, abs(ref_loss.item()))
    params = net.named_upstream_parameters()
    grads = torch.autograd.grad(loss, list(params.values()) + [ic] + ([] if no_flow else [fc]), allow_unused=True)
    got = dict(zip(list(params) + ["img_feat_coarse", "flow_feat_coarse"], grads))
    for k in ("img_feat_coarse", "flow_feat_coarse"):
        if k in ref_g:
            got[k] = _nchw(got[k], ngf_global)
    assert set(ref_g) == set(got)
    # (the 32x48 case's 32-channel blocks on 16x24 take F(2x2) too -- `algo` says so -- and keep the tighter bound all the same)
    _compare_gradients(got, ref_g, _zero_gradient_biases(spec), 4e-4 if ngf_global == 64 else 1e-4, name)


# ------------------------------------------------------------------------------------------------------------------
# (b) one two-frame iteration of G0 + G1 + MultiscaleDiscriminator(num_D 2)
# ------------------------------------------------------------------------------------------------------------------
PAIR_SEED = 3


def _pair_specs():
    from text2video_amd.generator import GeneratorSpec
    return (GeneratorSpec(ngf=32, n_downsample=2, n_blocks=2, no_flow=False, norm="batch"),
            GeneratorSpec(ngf=16, n_downsample=2, n_blocks=2, no_flow=False, norm="batch", is_local=True, scale=1))


def _pair_inputs(seed=PAIR_SEED):
    H = W = 64
    return {"poses": _rand(2, 9, H, W, seed=seed + 1).clamp(-1, 1),          # two frames (two sliding windows)
            "real": torch.tanh(_rand(2, 3, H, W, seed=seed + 2)),
            "prev1": torch.tanh(_rand(1, 6, H, W, seed=seed + 3)),             # non-zero previous frames on both scales
            "prev0": torch.tanh(_rand(1, 6, H // 2, W // 2, seed=seed + 4))}


def _pair_oracle(seed=PAIR_SEED, dtype=torch.float32):
    """frame 1 raw-only, frame 2 through both scales' compositors; LSGAN + feature matching on the finest scale's frames"""
    from oracle.generator_ref import CompositeGenerator, CompositeLocalGenerator, MultiscaleDiscriminator, weights_init
    from text2video_amd.generator import synthetic_state_dict
    s0, s1 = _pair_specs()
    torch.manual_seed(0)        # the discriminator's conv biases keep torch's default init: seeded, as the one-scale test does
    sd0 = synthetic_state_dict(s0, seed, "vid2vid", flow_gain=0.1)
    sd1 = synthetic_state_dict(s1, seed + 30, "vid2vid", flow_gain=0.05)
    G0 = CompositeGenerator(9, 3, 6, 32, 2, 2, False, "batch").train()
    G1 = CompositeLocalGenerator(9, 3, 6, 32, 2, 1, False, "batch").train()
    G0.load_state_dict(sd0, strict=False)
    G1.load_state_dict(sd1, strict=False)
    Dr = MultiscaleDiscriminator(6, 16, 3, 2, "batch").train()
    gen = torch.Generator().manual_seed(7)
    Dr.apply(lambda m: weights_init(m, gen))
    dsd = {k: v.clone() for k, v in Dr.state_dict().items() if "running" not in k and "num_batches" not in k}
    G0, G1, Dr = G0.to(dtype), G1.to(dtype), Dr.to(dtype)
    inp = {k: v.to(dtype) for k, v in _pair_inputs(seed).items()}
    pool = torch.nn.AvgPool2d(3, stride=2, padding=[1, 1], count_include_pad=False)
    mse, l1 = torch.nn.MSELoss(), torch.nn.L1Loss()

    def gan(pred, real_target):
        return sum(mse(p[-1], torch.ones_like(p[-1]) if real_target else torch.zeros_like(p[-1])) for p in pred)

    def fm(pf, pr):
        return sum(0.5 * 1.0 * l1(pf[i][j], pr[i][j].detach()) * 10.0 for i in range(2) for j in range(4))

    p1, p0 = inp["prev1"], inp["prev0"]
    fine, coarse = [], []
    for f in range(2):
        o0 = G0(pool(inp["poses"][f:f + 1]), p0, f == 0)
        o1 = G1(inp["poses"][f:f + 1], p1, o0[4], o0[5], f == 0)
        fine.append(o1[0])
        coarse.append(o0[0].detach())
        p0 = torch.cat([p0[:, 3:], o0[0].detach()], 1)
        p1 = torch.cat([p1[:, 3:], o1[0].detach()], 1)
    fake = torch.cat(fine, 0)
    A = inp["poses"][:, 6:9]
    pred_real = Dr(torch.cat([A, inp["real"]], 1))
    pred_fake_d = Dr(torch.cat([A, fake.detach()], 1))
    loss_D = 0.5 * (gan(pred_fake_d, False) + gan(pred_real, True))
    pred_fake_g = Dr(torch.cat([A, fake], 1))
    loss_G = gan(pred_fake_g, True) + fm(pred_fake_g, pred_real)
    named = [("G0." + k, p) for k, p in G0.named_parameters()] + [("G1." + k, p) for k, p in G1.named_parameters()]
    gG = torch.autograd.grad(loss_G, [p for _, p in named], allow_unused=True)
    grads = {k: g for (k, _), g in zip(named, gG)}
    heads = sorted(k for k, g in grads.items() if g is None)
    assert heads and all(k.startswith("G0.model_final_") for k in heads)       # upstream: G0's heads get no gradient
    return {"fake": fake.detach(), "coarse": torch.cat(coarse, 0), "loss_G": loss_G.detach(), "loss_D": loss_D.detach(),
            "grads": {k: g for k, g in grads.items() if g is not None}, "heads": heads,
            "params": {k: p.detach() for k, p in named}, "sd0": sd0, "sd1": sd1, "dsd": dsd}


def test_two_scale_train_iteration_matches_autograd_oracle():
    from text2video_amd import ops
    from text2video_amd import train as T
    # G1's 32-channel ResnetBlock convs on the 32x32 map take F(4x4,3x3) -- with it the Winograd-domain weight gradient and the
    # transposed-Winograd data gradient; G0's 128-channel ones on 8x8 stay direct
    assert ops.best_conv_algo(ops.conv_desc(32, 32, 32, 32, 3, 1, 1, ops.PAD_REFLECT), 32) == ops.ALGO_WINOGRAD_F4
    ref = _pair_oracle()
    s0, s1 = _pair_specs()
    G = T.TwoScaleGenerator(T.TrainableGenerator(s0, ref["sd0"], "cuda:0"), T.TrainableLocalGenerator(s1, ref["sd1"], "cuda:0"))
    Dh = T.TrainableDiscriminator(6, ref["dsd"], 16, 3, 2, "batch", "cuda:0")
    inp = _pair_inputs()
    pz = _nhwc(inp["poses"], 12)
    prev = (_nhwc(inp["prev1"], 8), _nhwc(inp["prev0"], 8))
    fine, coarse = [], []
    for f in range(2):
        fk, rw, fw, fk0, prev = G(pz[f:f + 1], prev, use_raw_only=f == 0)
        assert not fk0.requires_grad and not prev[0].requires_grad and not prev[1].requires_grad
        fine.append(fk)
        coarse.append(fk0)
    hfake = torch.cat(fine, 0)
    for tag, got, want in (("finest", hfake, ref["fake"]), ("coarse", torch.cat(coarse, 0), ref["coarse"])):
        err = (_nchw(got, 3) - want).abs().max().item()
        print(tag, "frames max |delta| %.1e" % err)
        assert err <= 1e-4, (tag, err)
    A8 = _nhwc(inp["poses"][:, 6:9], 3)
    z2 = torch.zeros(2, 64, 64, 2, device="cuda:0")

    def d_in(img4):
        return torch.cat([A8, img4[..., :3], z2], -1).contiguous()

    hp_real = Dh(d_in(_nhwc(inp["real"], 4)))
    hp_fake_d = Dh(d_in(hfake.detach()))
    hloss_D = 0.5 * (T.gan_loss(hp_fake_d, False) + T.gan_loss(hp_real, True))
    hp_fake_g = Dh(d_in(hfake))
    hloss_G = T.gan_loss(hp_fake_g, True) + T.feature_matching_loss(hp_fake_g, hp_real)
    assert abs(hloss_D.item() - ref["loss_D"].item()) <= 1e-4 * max(1, abs(ref["loss_D"].item()))
    assert abs(hloss_G.item() - ref["loss_G"].item()) <= 1e-4 * max(1, abs(ref["loss_G"].item()))
    named = [("G0." + k, p) for k, p in G.G0.named_upstream_parameters().items()] + \
            [("G1." + k, p) for k, p in G.G1.named_upstream_parameters().items()]
    hg = torch.autograd.grad(hloss_G, [p for _, p in named], allow_unused=True)
    got = {k: g for (k, _), g in zip(named, hg)}
    assert sorted(k for k, g in got.items() if g is None) == ref["heads"]
    assert {id(p) for p in G.head_params()} == {id(p) for k, p in named if k in ref["heads"]}
    may_skip = {"G0." + k for k in _zero_gradient_biases(s0)} | {"G1." + k for k in _zero_gradient_biases(s1)}
    _compare_gradients(got, ref["grads"], may_skip, 4e-4, "G0+G1")
    # ---------------- one Adam step on both sides (torch-0.4.1 update rule); G0's heads stay where they were
    trained = [(k, p) for k, p in named if got[k] is not None]
    opt = T.FusedAdam([p for _, p in trained])
    for (k, p) in trained:
        p.grad = got[k]
    opt.step()
    # The first Adam step from zero moments moves an element by lr * g / (|g| + eps / sqrt(1 - beta2)) = lr * g / (|g| + 3.2e-7):
    # by lr = 2e-4 times the gradient's SIGN wherever |g| >> 3e-7, by less below.  Two gradients of one sign therefore leave
    # weights at most lr apart (2.5e-4 with the one-scale test's margin); that is asked of every element whose reference
    # gradient is larger than the error the gradient check above allows (2e-3 of the tensor's max), since there the sign is
    # settled.  Below that an element's sign is not, and the two steps may point apart: 2 lr (+ 1e-6 for fp32 weights) is
    # the most that can happen, and is asked of all of them -- the zero-gradient biases included, nothing is skipped.
    worst_settled = worst_rest = 0.0
    for k, p in named:
        pr = ref["params"][k].clone().double()
        if k not in ref["grads"]:
            assert torch.equal(p.detach().cpu().double(), pr), k        # G0's heads: not touched
            continue
        g = ref["grads"][k].double()
        _adam_041(pr, g, torch.zeros_like(pr), torch.zeros_like(pr), 2e-4, 0.5, 0.999, 1e-8, 1)
        diff = (p.detach().cpu().double() - pr).abs()
        settled = g.abs() > 2e-3 * g.abs().max()
        if settled.any():
            worst_settled = max(worst_settled, diff[settled].max().item())
            assert diff[settled].max().item() <= 2.5e-4, k
        worst_rest = max(worst_rest, diff.max().item())
        assert diff.max().item() <= 2 * 2e-4 + 1e-6, k
    print("weights after one Adam step: max |delta| %.2e where the gradient's sign is settled, %.2e anywhere"
          % (worst_settled, worst_rest))


# ------------------------------------------------------------------------------------------------------------------
# (c), (d): the trainer
# ------------------------------------------------------------------------------------------------------------------
def _train_opt(tmp_path, *extra):
    from text2video_amd.options import TrainOptions
    return TrainOptions().parse(["--name", "two", "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only", "--no_first_img",
                                 "--ngf", "16", "--n_blocks", "2", "--n_downsample_G", "2", "--num_D", "2", "--ndf", "16",
                                 "--no_vgg", "--fineSize", "64", "--loadSize", "64", "--max_frames_per_gpu", "2",
                                 "--n_scales_temporal", "0", "--checkpoints_dir", str(tmp_path), "--synthetic_data",
                                 "--n_scales_spatial", "2", "--n_blocks_local", "1"] + list(extra))


def _clip(frames, seed=0, S=64):
    rng = np.random.default_rng(seed)
    pose = torch.zeros(frames, S, S, 12, device="cuda:0")
    pose[..., :9] = torch.from_numpy(rng.uniform(-1, 1, (frames, S, S, 9)).astype(np.float32)).cuda()
    real = torch.zeros(frames, S, S, 4, device="cuda:0")
    real[..., :3] = torch.tanh(torch.from_numpy(rng.standard_normal((frames, S, S, 3)).astype(np.float32))).cuda()
    real_prev = torch.cat([real[-1:], real[:-1]], 0).contiguous()
    return pose, real, real_prev


def _snapshot(net):
    return {k: v.detach().clone() for k, v in net.named_upstream_parameters().items()}


def test_frozen_phase_leaves_g0_alone_and_the_boundary_starts_it_from_zero_moments(tmp_path):
    from text2video_amd import train as T
    tr = T.Vid2VidTrainer(_train_opt(tmp_path, "--niter_fix_global", "1"), "cuda:0", seed=5)
    assert tr.fix_global and T.global_generator_frozen(1, 1)
    g0_ids = {id(p) for p in tr.G.G0.parameters()}
    head_ids = {id(p) for p in tr.G.head_params()}
    assert not any(p.requires_grad for p in tr.G.G0.parameters())
    assert not any(id(p) in g0_ids for p in tr.optG.params) and not any(id(p) in g0_ids for p in tr.bucketsG.params)
    assert [id(p) for p in tr.optG.params] == [id(p) for p in tr.G.G1.parameters()]
    pose, real, real_prev = _clip(2)
    b0, b1 = _snapshot(tr.G.G0), _snapshot(tr.G.G1)
    losses, prev = tr.train_step(pose, real, None, None, real_prev=real_prev)
    assert all(np.isfinite(v) for v in losses.values())
    assert all(torch.equal(v, b0[k]) for k, v in tr.G.G0.named_upstream_parameters().items()), "frozen G0 moved"
    assert all(p.grad is None for p in tr.G.G0.parameters())
    # (conv biases in front of a norm get an exactly zero gradient delivered: Adam leaves them where they are)
    still = {k for k, v in tr.G.G1.named_upstream_parameters().items() if torch.equal(v, b1[k])}
    assert still == _zero_gradient_biases(tr.G.G1.spec), "every other G1 tensor trains in the frozen phase"
    assert all(s == 1 for s in tr.optG.steps)
    # ---- the boundary: epoch 2 is the first joint one.  G1 keeps its moments, G0's trunk joins with zero ones
    m_before = [m.clone() for m in tr.optG.m]
    tr.set_epoch(1)
    assert tr.fix_global, "the same phase: nothing is rebuilt"
    tr.set_epoch(2)
    assert not tr.fix_global and all(p.requires_grad for p in tr.G.G0.parameters())
    trunk = [p for p in tr.G.G0.parameters() if id(p) not in head_ids]
    n0 = len(trunk)
    assert [id(p) for p in tr.optG.params] == [id(p) for p in trunk] + [id(p) for p in tr.G.G1.parameters()]
    assert [id(p) for p in tr.bucketsG.params] == [id(p) for p in tr.optG.params]
    assert all(s == 0 for s in tr.optG.steps[:n0]) and all(s == 1 for s in tr.optG.steps[n0:])
    assert all(not m.any() and not v.any() for m, v in zip(tr.optG.m[:n0], tr.optG.v[:n0]))
    assert all(torch.equal(a, b) for a, b in zip(m_before, tr.optG.m[n0:]))
    b0 = _snapshot(tr.G.G0)
    losses, _ = tr.train_step(pose, real, None, prev, real_prev=real_prev)
    assert all(np.isfinite(v) for v in losses.values())
    heads = {k for k, p in tr.G.G0.named_upstream_parameters().items() if id(p) in head_ids}
    assert len(heads) == 6
    still = {k for k, v in tr.G.G0.named_upstream_parameters().items() if torch.equal(v, b0[k])}
    assert still == heads | _zero_gradient_biases(tr.G.G0.spec)        # the trunk moves, the heads never do
    assert all(p.grad is None for p in tr.G.head_params())
    assert all(s == 1 for s in tr.optG.steps[:n0]) and all(s == 2 for s in tr.optG.steps[n0:])


def _param_hash(tr):
    h = hashlib.sha256()
    for p in list(tr.G.parameters()) + list(tr.D.parameters()):
        h.update(p.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def test_trainer_two_scale_is_deterministic_saves_the_pair_and_the_pair_serves_the_same_frames(tmp_path):
    from text2video_amd import model as M
    from text2video_amd import train as T
    from text2video_amd.generator import Recurrence
    from text2video_amd.options import TestOptions
    pose, real, real_prev = _clip(2, seed=1)
    runs = []
    for _ in range(2):
        tr = T.Vid2VidTrainer(_train_opt(tmp_path), "cuda:0", seed=5)
        assert tr.two_scale and not tr.fix_global
        l1, prev = tr.train_step(pose, real, None, None, real_prev=real_prev)
        l2, _ = tr.train_step(pose, real, None, prev, real_prev=real_prev)
        for name in ("G_GAN", "G_GAN_Feat", "D", "F_Flow", "F_Warp", "W", "G_Warp"):
            assert name in l1 and np.isfinite(l1[name]) and np.isfinite(l2[name]), name
        runs.append((l1, l2, _param_hash(tr)))
    assert runs[0] == runs[1]
    # ---- the checkpoint pair, as test.py loads it
    tr.save("latest")
    assert sorted(os.listdir(tmp_path / "two")) == ["latest_net_D.pth", "latest_net_G0.pth", "latest_net_G1.pth"]
    sd0, sd1 = (torch.load(tmp_path / "two" / ("latest_net_G%d.pth" % s), map_location="cpu") for s in (0, 1))
    for sd in (sd0, sd1):       # one layout: the parameters and every BatchNorm2d's buffers
        assert any(k.endswith("running_mean") for k in sd) and any(k.endswith("num_batches_tracked") for k in sd)
    assert int(sd1["model_down_seg.2.num_batches_tracked"]) == 4 and int(sd0["model_down_seg.2.num_batches_tracked"]) == 4
    # ---- the trainer's forward on a new sequence with the saved weights (no optimiser step from here on)
    tr.optG.step = tr.optD.step = lambda: None
    p4, r4, rp4 = _clip(4, seed=2)
    _, two = tr.train_step(p4[:2], r4[:2], None, None, real_prev=rp4[:2])      # FIFOs = the frames 1 and 2 of each scale
    _, carried = tr.train_step(p4[2:], r4[2:], None, two, real_prev=rp4[2:])
    # carrying `prev` across two chunks of two frames equals one four-frame chunk's FIFOs
    _, whole = tr.train_step(p4, r4, None, None, real_prev=rp4)
    assert torch.equal(carried[0], whole[0]) and torch.equal(carried[1], whole[1])
    assert not torch.equal(two[0], whole[0])
    topt = TestOptions().parse(["--name", "two", "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only", "--no_first_img",
                                "--ngf", "16", "--n_blocks", "2", "--n_downsample_G", "2", "--checkpoints_dir", str(tmp_path),
                                "--n_scales_spatial", "2", "--n_blocks_local", "1"])
    m = M.create_model(topt)
    assert len(m.nets) == 2 and not m.nets[0].spec.no_flow and m.nets[1].spec.is_local
    st = Recurrence()
    served = [m.inference_nhwc_batch([p4[f].contiguous()], [st])[0].clone() for f in range(2)]
    for f in range(2):
        err = (two[0][0, ..., 3 * f:3 * f + 3] - served[f][..., :3]).abs().max().item()
        print("frame %d: trainer vs Vid2VidModelG max |delta| %.1e" % (f + 1, err))
        assert err <= 1e-4, (f, err)
    # ... and the coarse scale's FIFO behind them
    err = (two[1][0, ..., :6] - st.prev[1][..., :6]).abs().max().item()
    print("coarse FIFO: trainer vs Vid2VidModelG max |delta| %.1e" % err)
    assert err <= 1e-4
