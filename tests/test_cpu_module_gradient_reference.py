"""tests/module_gradient_reference.py checked on the CPU: the masked oracle module against plain autograd, the near-kink cap
of every case, what ONE flipped LeakyReLU element does to D_f's gradient (the conditioning claim of
tests/test_gpu_device_oracle.py::_df_on_hip_frames, tested instead of argued), how the fp32 yardstick moves with and without
shared masks, and the bound of tests/test_gpu_module_gradients.py against faults injected into an fp32 restatement of the
backward pass.  Also the host-side refusal of pt_skip with whole-batch statistics."""
import copy
import functools

import pytest
import torch

import module_gradient_reference as mg

IDS = [c.id for c in mg.CASES]


def _skip(case):
    return case.pt_skip if case.off else 0


@functools.lru_cache(maxsize=None)
def _evaluations(case_id):
    """(float64 with its own masks, fp32 with its own masks, fp32 with the float64 masks): once per case, never written"""
    case = mg.BY_ID[case_id]
    data = mg.build_case(case)
    r64 = mg.reference(case, data, torch.float64, skip=_skip(case))
    r32 = mg.reference(case, data, torch.float32, skip=_skip(case))
    r32s = mg.reference(case, data, torch.float32, masks=mg.own_masks(r64), skip=_skip(case))
    return r64, r32, r32s


def _bounds(case):
    """{tensor: bound} of the GPU test with the float64 masks standing for the HIP masks"""
    r64, _, r32s = _evaluations(case.id)
    g64, g32 = mg.gradient_tensors(case, r64), mg.gradient_tensors(case, r32s)
    return {k: mg.bound(mg.rel_err(g32[k], g64[k])) for k in g64}


@pytest.mark.parametrize("case", mg.CASES, ids=IDS)
def test_masked_module_with_its_own_masks_is_plain_autograd(case):
    """float64, 1e-12 relative per tensor: stage outputs, dx and every parameter gradient; the passes of a grouped or
    two-call case are separate forward calls of the plain module here as well"""
    data = mg.build_case(case)
    r64 = _evaluations(case.id)[0]
    mod = copy.deepcopy(data["ref"]).double().train()
    x = data["x"].double().requires_grad_(True)
    loss, parts = 0.0, []
    for sl in mg.pass_slices(case):
        feats = mod(x[sl])
        parts.append(feats)
        for frow, srow in zip(feats, data["seeds"]):
            for f, R in zip(frow, srow):
                R = R.double().clone()
                R[:_skip(case)] = 0
                loss = loss + (R[sl] * f).sum()
    names = [k for k, _ in mod.named_parameters()]
    g = torch.autograd.grad(loss, [x] + [p for _, p in mod.named_parameters()])
    plain = dict(zip(names, g[1:]))
    shapes = mg.stage_shapes(case)
    for i in range(case.num_D):
        for j in range(mg.N_LAYERS + 2):
            f = torch.cat([p[i][j] for p in parts])
            assert tuple(f.shape[1:]) == shapes[i][j]
            assert mg.rel_err(r64.feats[i][j], f) <= 1e-12, (i, j)
    assert mg.rel_err(r64.dx, g[0]) <= 1e-12
    zero = set(mg.zero_bias_names(case))
    assert set(plain) == set(r64.grads)
    for k in plain:
        if k in zero:
            wk = k.replace(".0.bias", ".0.weight")
            assert plain[k].norm() <= 1e-9 * plain[wk].norm() and r64.grads[k].norm() <= 1e-9 * plain[wk].norm(), k
        else:
            assert mg.rel_err(r64.grads[k], plain[k]) <= 1e-12, k
    # the leading images of a pass-through case get no gradient in the reference either
    if _skip(case):
        assert torch.count_nonzero(r64.dx[:_skip(case)]).item() == 0 and torch.count_nonzero(r64.dx[_skip(case):]).item() > 0


@pytest.mark.parametrize("case", mg.CASES, ids=IDS)
def test_near_kink_cap(case):
    """the float64 reference alone has at most KINK_CAP pre-activations within delta of zero: the condition under which
    the GPU test may cap the mask disagreements at KINK_CAP"""
    r64, r32, _ = _evaluations(case.id)
    deltas = mg.kink_deltas(r32, r64)
    n = mg.near_kink_count(r64, deltas)
    total = sum(z.numel() for row in r64.zs for z in row if z is not None)
    print("MODGRAD-CPU %-16s near-kink %d of %d pre-activations, delta %.2e .. %.2e"
          % (case.id, n, total, min(d for r in deltas for d in r if d), max(d for r in deltas for d in r if d)))
    assert n <= mg.KINK_CAP
    assert all(d is None or 0 < d <= 1e-4 for r in deltas for d in r)


def test_one_flipped_kink_moves_the_norm_bias_gradient_and_everything_upstream():
    """D_f's geometry (face128, norm bias 0 as the trainer draws it): the mask of the normed-layer element nearest the kink
    is flipped.  That layer's norm bias gradient changes by 0.8 |dy| of the element in its channel alone; the layer's conv
    weight gradient and every tensor of the layers below move with it (the norm adjoint's mean(dy) term); the layer's
    d gamma changes by 0.8 dy xhat with xhat = z / gamma ~ 0 -- nothing; the layers above do not change at all."""
    case = mg.BY_ID["face128"]
    data = mg.build_case(case)
    r64 = _evaluations(case.id)[0]
    masks = mg.own_masks(r64)
    j = min(range(1, mg.N_LAYERS + 1), key=lambda l: r64.zs[0][l].abs().min().item())
    z = r64.zs[0][j]
    flat = int(z.abs().argmin().item())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), z.shape))
    ch = idx[1]
    flipped = [[None if m is None else m.clone() for m in row] for row in masks]
    flipped[0][j][idx] = ~flipped[0][j][idx]
    rf = mg.reference(case, data, torch.float64, masks=flipped)
    # dy behind that activation: the seed of the stage plus what the layer above sends down
    mod = copy.deepcopy(data["ref"]).double().train()
    feats, _ = mg.masked_discriminator(mod, masks)(data["x"].double())
    loss = sum((R.double() * f).sum() for f, R in zip(feats[0], data["seeds"][0]))
    dy = torch.autograd.grad(loss, feats[0][j])[0][idx].item()
    pre = "scale0_layer%d" % j
    dbeta = rf.grads[pre + ".1.bias"] - r64.grads[pre + ".1.bias"]
    assert abs(abs(dbeta[ch].item()) - 0.8 * abs(dy)) <= 1e-9 * abs(dy)
    others = dbeta.clone()
    others[ch] = 0
    assert torch.count_nonzero(others).item() == 0
    moved = {k: mg.rel_err(rf.grads[k], r64.grads[k]) for k in r64.grads if k not in mg.zero_bias_names(case)}
    moved["dx"] = mg.rel_err(rf.dx, r64.dx)
    print("MODGRAD-CPU flip in layer %d, |z| = %.2e, dy = %.3e: %s" % (j, abs(z[idx].item()), dy,
                                                                      "  ".join("%s %.1e" % kv for kv in sorted(moved.items()))))
    gamma = data["sd"][pre + ".1.weight"][ch].item()
    dgamma = rf.grads[pre + ".1.weight"] - r64.grads[pre + ".1.weight"]
    assert abs(dgamma[ch].item()) <= 0.8 * abs(dy) * abs(z[idx].item() / gamma) * (1 + 1e-6) + 1e-18
    upstream = [pre + ".1.bias", pre + ".0.weight", "dx"] + \
        [k for k in moved if k != "dx" and int(k.split("layer")[1][0]) < j]
    later = [k for k in moved if k != "dx" and int(k.split("layer")[1][0]) > j]
    assert later and len(upstream) == 3 + 1 + 3 * (j - 1) + 1      # layer 0: weight, bias; normed ones: weight, gamma, beta
    for k in later:
        assert moved[k] == 0.0, (k, moved[k])
    for k in upstream:
        assert moved[k] >= 1e-7, (k, moved[k])
    # the flip is worth more than the whole fp32 bound on the tensors it moves most, and nothing on d gamma
    assert moved[pre + ".1.bias"] >= 1e-4 and moved[pre + ".1.weight"] <= 1e-3 * moved[pre + ".1.bias"]


@pytest.mark.parametrize("case", mg.FACE_SEED_CASES, ids=[c.id for c in mg.FACE_SEED_CASES])
def test_fp32_yardstick_with_and_without_shared_masks(case):
    """D_f's geometry on the seeds of the full-size D_f test: the fp32 torch evaluation with its OWN masks is as far from
    float64 as its kink flips take it (recorded, not bounded: the old yardstick); with the float64 masks every tensor is
    within a few thousand units of fp32 roundoff"""
    r64, r32, r32s = _evaluations(case.id)
    g64, g32, g32s = (mg.gradient_tensors(case, r) for r in (r64, r32, r32s))
    flips = sum(int((a != b).sum().item()) for ra, rb in zip(mg.own_masks(r32), mg.own_masks(r64))
                for a, b in zip(ra, rb) if a is not None)
    print("MODGRAD-CPU %s: fp32 torch, %d of its own masks differ from float64's" % (case.id, flips))
    for k in g64:
        own, shared = mg.rel_err(g32[k], g64[k]), mg.rel_err(g32s[k], g64[k])
        print("MODGRAD-CPU     %-34s own masks %.3e  shared masks %.3e" % (k, own, shared))
        assert shared <= 2000 * mg.U, (k, shared)
        if not flips:
            assert own == shared


# fault -> (case that must see it, layer it sits in)
FAULT_CASES = {"group_stats_whole_batch": ("grouped3", 2), "image_stats_shifted": ("passthrough_in", 2),
               "drop_mean_dy": ("plain_bn", 2), "slope_on_positive": ("plain_bn", 1), "bias_sum_dc": ("plain_bn", 2),
               "skipped_rows_carry": ("passthrough", 2), "pool_div9": ("plain_bn", 2)}


@pytest.mark.parametrize("case", mg.CASES, ids=IDS)
def test_restated_backward_is_within_the_bound(case):
    """the fp32 restatement without a fault is one more correct fp32 implementation: inside the GPU test's bound"""
    data = mg.build_case(case)
    r64 = _evaluations(case.id)[0]
    rs = mg.restated_backward(case, data, mg.own_masks(r64), skip=_skip(case))
    bounds, g64, got = _bounds(case), mg.gradient_tensors(case, r64), mg.gradient_tensors(case, rs)
    for k in g64:
        assert mg.rel_err(got[k], g64[k]) <= bounds[k], k
    for k in mg.zero_bias_names(case):
        assert torch.count_nonzero(rs.grads[k]).item() == 0
    for i in range(case.num_D):
        for j in range(mg.N_LAYERS + 2):
            assert mg.rel_err(rs.feats[i][j], r64.feats[i][j]) <= 1e-5, (i, j)


@pytest.mark.parametrize("fault", mg.FAULTS)
def test_injected_fault_exceeds_the_bound_tenfold(fault):
    cid, layer = FAULT_CASES[fault]
    case = mg.BY_ID[cid]
    data = mg.build_case(case)
    r64 = _evaluations(case.id)[0]
    rs = mg.restated_backward(case, data, mg.own_masks(r64), skip=_skip(case), fault=fault, fault_layer=layer)
    bounds, g64, got = _bounds(case), mg.gradient_tensors(case, r64), mg.gradient_tensors(case, rs)
    over = {k: mg.rel_err(got[k], g64[k]) / bounds[k] for k in g64}
    worst = max(over, key=over.get)
    print("MODGRAD-CPU fault %-24s on %-14s worst %s: %.1e x its bound" % (fault, cid, worst, over[worst]))
    if fault == "bias_sum_dc":
        # this tensor's bound is an exact zero on the HIP side (the GPU test's exact facts): rounding noise is a failure
        k = "scale0_layer%d.0.bias" % layer
        assert torch.count_nonzero(rs.grads[k]).item() > 0
        return
    if fault == "skipped_rows_carry":
        assert torch.count_nonzero(rs.dx[:_skip(case)]).item() > 0
    assert over[worst] >= 10.0, over


def test_pt_skip_with_whole_batch_statistics_is_refused_on_the_host():
    """pt_skip runs the backward on the images [pt_skip:] alone; with norm 'batch' and groups == 1 their statistics are the
    whole batch's, whose adjoint couples them to the skipped images: refused when the node is built, before any launch"""
    from text2video_amd import train as T
    x = torch.zeros(2, 8, 8, 4)
    w = torch.zeros(4, 4, 4, 4, requires_grad=True)
    b = torch.zeros(4)
    with pytest.raises(ValueError, match="pt_skip"):
        T.conv_block(x, w, b, None, torch.ones(4), torch.zeros(4), norm="batch", relu=2, groups=1, pt_skip=1)


def test_data_gradient_geometry_of_a_stride2_layer_on_a_map_of_mixed_parity():
    """the coarse scale of a 45 x 37 input reaches a 7 x 6 map: the adjoint of its stride-2 conv needs output_padding 1 in H
    and 0 in W.  The one output_padding the descriptor has takes the larger; the extra column is cropped (ConvDataGrad.crop)."""
    from text2video_amd import ops
    from text2video_amd.backward import ConvDataGrad
    dg = ConvDataGrad(ops.conv_desc(7, 6, 8, 8, 4, 2, 2, ops.PAD_ZERO))
    assert dg.crop == (7, 6) and tuple(ops.conv_out_dims(dg.desc)) == (7, 7) and dg.desc.algo == ops.ALGO_DIRECT
    for H, W in ((7, 7), (6, 6), (45, 37), (12, 10)):
        dg = ConvDataGrad(ops.conv_desc(H, W, 8, 8, 4, 2, 2, ops.PAD_ZERO))
        assert dg.crop is None and tuple(ops.conv_out_dims(dg.desc)) == (H, W)
