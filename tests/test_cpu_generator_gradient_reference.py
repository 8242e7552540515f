"""tests/generator_gradient_reference.py checked on the CPU: the masked oracle against plain autograd through the stock
oracle, the Winograd restatements against F.conv2d in float64, the three conditions on every case's seeds (near-kink share,
warp kink, bound cap), the restatement levels of the case table against the library's own choice, and the bound of
tests/test_gpu_generator_gradients.py against faults injected into an fp32 evaluation of the masked module."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import generator_gradient_reference as gg

IDS = [c.id for c in gg.CASES]


@functools.lru_cache(maxsize=None)
def _evaluations(case_id):
    """(float64 with its own masks, the fp32 yardstick with its own masks, the yardstick with the float64 masks): once per
    case, never written"""
    case = gg.BY_ID[case_id]
    data = gg.build_case(case)
    r64 = gg.evaluate(case, data, torch.float64)
    y32 = gg.evaluate(case, data, torch.float32, yardstick=True)
    y32s = gg.evaluate(case, data, torch.float32, masks=gg.own_masks(r64), yardstick=True)
    return r64, y32, y32s


def _plain_autograd(case, data):
    """the case through deep copies of the STOCK oracle modules in float64: outputs per frame, gradients by name"""
    nets = [copy.deepcopy(n).double().train() for n in data["nets"]]
    if case.frozen:
        for p in nets[0].parameters():
            p.requires_grad_(False)
    pool = torch.nn.AvgPool2d(3, stride=2, padding=[1, 1], count_include_pad=False)
    loss, outs, coarse = 0.0, [], None
    for fr, (raw_only, need_flow) in zip(data["frames"], case.frames):
        t = {k: v.double() for k, v in fr.items()}
        if case.net == "g0":
            o = nets[0](t["pose"], t["prev"], raw_only)
        elif case.net == "g1":
            coarse = (t["img_c"].requires_grad_(True), t["flow_c"].requires_grad_(True))
            o = nets[0](t["pose"], t["prev"], coarse[0], coarse[1], raw_only)
        else:
            o0 = nets[0](pool(t["pose"]), t["prev0"], raw_only)
            o = nets[1](t["pose"], t["prev"], o0[4], o0[5], raw_only)
        out = {"fake": o[0], "raw": o[3]}
        if not case.no_flow and need_flow:
            out.update(flow=o[1], weight=o[2])
        loss = loss + sum((t["R_" + k] * v).sum() for k, v in out.items()) / float(case.H * case.W)
        outs.append(out)
    named = [(p + k, prm) for p, n in zip(gg.prefixes(case), nets) for k, prm in n.named_parameters() if prm.requires_grad]
    if case.net == "g1":
        named += [("img_feat_coarse", coarse[0])] + ([] if case.no_flow else [("flow_feat_coarse", coarse[1])])
    g = torch.autograd.grad(loss, [p for _, p in named], allow_unused=True)
    return outs, dict(zip([k for k, _ in named], g))


@pytest.mark.parametrize("case", gg.CASES, ids=IDS)
def test_masked_oracle_with_its_own_masks_is_plain_autograd(case):
    """torch.equal in float64: every output and every gradient (G0, G1 and the pair); the sites of a frame are as many and as
    large as site_shapes says, which is what the GPU test attaches the HIP masks by"""
    data = gg.build_case(case)
    r64 = _evaluations(case.id)[0]
    outs, plain = _plain_autograd(case, data)
    for f, out in enumerate(outs):
        assert set(out) == set(r64.outs[f])
        for k, v in out.items():
            assert torch.equal(v, r64.outs[f][k]), (f, k)
        want = [(1,) + s for sp, (H, W) in zip(gg.specs(case), gg.net_sizes(case)) for s in gg.site_shapes(sp, H, W)]
        assert [tuple(z.shape) for z in r64.zs[f]] == want
    assert set(plain) == set(r64.grads)
    for k, g in plain.items():
        if g is None:
            assert r64.grads[k] is None and k.startswith("G0.model_final_"), k
        else:
            assert torch.equal(g, r64.grads[k]), k
    if case.net == "pair":
        heads = sorted(k for k, g in r64.grads.items() if g is None)
        assert (heads == []) if case.frozen else (len(heads) == 6)
        assert case.frozen == (not any(k.startswith("G0.") for k in r64.grads))
    # conv biases in front of a norm: zero to rounding
    for k in gg.zero_bias_names(case):
        if k in r64.grads:
            assert r64.grads[k].norm() <= 1e-9 * r64.grads[k.replace(".bias", ".weight")].norm(), k


def _bottleneck_shapes():
    out = set()
    for case in gg.CASES:
        for s, (H, W), m in zip(gg.specs(case), gg.net_sizes(case), case.wino):
            if m:
                out.add(gg.resblock_shape(s, H, W) + (m,))
    # (the ragged shapes of both tile sizes, whichever the cases take)
    return sorted(out | {(32, 10, 14, 4), (32, 10, 14, 2), (64, 9, 11, 4), (64, 9, 11, 2)})


@pytest.mark.parametrize("C,h,w,m", _bottleneck_shapes())
def test_winograd_restatement_is_the_convolution_in_float64(C, h, w, m):
    """y, dx, dw and db to 1e-12 at the cases' bottleneck shapes (22x26 is ragged for F(4x4)) and at 10x14 / 9x11"""
    g = torch.Generator().manual_seed(C + h)
    x = torch.randn(1, C, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    wt = (torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) * 0.05).requires_grad_(True)
    b = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    R = torch.randn(1, C, h, w, generator=g, dtype=torch.float64)
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect")
    y0, y1 = F.conv2d(xp, wt, b), gg.winograd_conv(F.pad(x, (1, 1, 1, 1), mode="reflect"), wt, b, m)
    assert y1.shape == y0.shape
    g0 = torch.autograd.grad((y0 * R).sum(), [x, wt, b])
    g1 = torch.autograd.grad((y1 * R).sum(), [x, wt, b])
    for name, a, c in zip(("y", "dx", "dw", "db"), (y1,) + g1, (y0,) + g0):
        assert gg.rel_err(a, c) <= 1e-12, (name, gg.rel_err(a, c))
    # ... and in fp32 F(4x4) is noisier than the direct convolution, which is why it is the yardstick (F(2x2), whose matrices
    # hold only 0, 1 and 1/2, is about as good as the direct form: printed, not asserted)
    xs, ws, bs = xp.detach().float(), wt.detach().float(), b.detach().float()
    e_dir, e_win = gg.rel_err(F.conv2d(xs, ws, bs), y0), gg.rel_err(gg.winograd_conv(xs, ws, bs, m), y0)
    print("GENGRAD-CPU winograd F(%dx%d) %3dch %2dx%2d: fp32 error %.2e against the direct convolution's %.2e" % (m, m, C, h, w, e_win, e_dir))
    assert m == 2 or e_win >= 1.5 * e_dir


@pytest.mark.parametrize("case", gg.CASES, ids=IDS)
def test_conditions_on_the_seeds(case):
    """near-kink share <= 1e-4, no warp sample coordinate within delta_w of an integer, every bound <= 2e-4"""
    r64, y32, y32s = _evaluations(case.id)
    deltas = gg.kink_deltas(y32, r64)
    n, total = gg.near_kink_share(r64, deltas)
    warp = gg.warp_condition(case, y32, r64)
    b = gg.bounds(case, y32s, r64)
    worst = max(b, key=lambda k: b[k][1])
    fwd = {"%s[%d]" % (k, f): gg.bound(gg.rel_err(y32.outs[f][k], v)) for f, o in enumerate(r64.outs) for k, v in o.items()}
    print("GENGRAD-CPU %-18s near-kink %d of %d (%.1e), delta %.1e .. %.1e; warp %s; %d gradient tensors, yardstick error "
          "median %.2e, worst bound %.2e (%s); worst forward bound %.2e"
          % (case.id, n, total, n / total, min(min(r) for r in deltas), max(max(r) for r in deltas),
             ["delta_w %.1e px: %d near, |flow| max %.2f mean %.3f" % w for w in warp] or "no composited frame",
             len(b), sorted(v[0] for v in b.values())[len(b) // 2], b[worst][1], worst, max(fwd.values())))
    assert n <= gg.KINK_SHARE * total
    n_comp = sum(1 for raw_only, _ in case.frames if not (raw_only or case.no_flow))
    assert len(warp) == n_comp
    for dw, near, fmax, fmean in warp:
        assert near == 0 and fmax < 8.0 and fmean > 0.05
    for k, (e32, bnd) in b.items():
        assert bnd <= gg.BOUND_CAP, (k, e32, bnd)
    assert max(fwd.values()) <= gg.BOUND_CAP
    # what the comparison covers: every parameter but the zero-gradient biases (and the heads of the pair's G0, G0 when frozen)
    nparam = sum(len(sd) for sd in gg.build_case(case)["sds"])
    absent = sum(1 for v in r64.grads.values() if v is None)
    if case.frozen:
        nparam, zero = len(gg.build_case(case)["sds"][1]), [k for k in gg.zero_bias_names(case) if k.startswith("G1.")]
    else:
        zero = gg.zero_bias_names(case)
    extra = (1 if case.no_flow else 2) if case.net == "g1" else 0
    assert len(b) == nparam - absent - len(zero) + extra


@pytest.mark.parametrize("case", gg.CASES, ids=IDS)
def test_case_table_restatement_levels_are_the_librarys_choice(case, monkeypatch):
    """Case.wino against ops.best_conv_algo / ConvDataGrad; no polyphase layer (asserted inside).  Only this check needs the
    compiled library."""
    try:
        from text2video_amd import ops
        ops.best_conv_algo(ops.conv_desc(8, 8, 16, 16, 3, 1, 1, ops.PAD_REFLECT), 16)
    except (ImportError, OSError) as e:
        pytest.skip("the compiled library does not load here: %s" % e)
    if case.direct:
        monkeypatch.setenv("T2V_CONV_ALGO", "1")
    else:
        monkeypatch.delenv("T2V_CONV_ALGO", raising=False)
    algos = gg.layer_algorithms(case)
    assert tuple(a["level"] for a in algos) == case.wino, [(a["fwd"], a["dgrad"], a["transposed"]) for a in algos]


# fault -> the case that must see it
FAULT_CASES = {"residual_identity_dropped": "g0_direct", "reflect_fold_dropped": "g0_wino", "drop_mean_dy": "g0_direct",
               "ragged_tile_zeroed": "g0_ragged_step", "relu_mask_neighbour": "g0_wino", "weight_adjoint_sign": "g0_direct",
               "flow_weight_halves_swapped": "g1_small", "second_frame_wgrad_dropped": "g0_ragged_step",
               "flow_feat_coarse_dropped": "pair"}


def test_every_fault_has_a_case():
    assert set(FAULT_CASES) == set(gg.FAULTS)


@pytest.mark.parametrize("fault", gg.FAULTS)
def test_injected_fault_exceeds_the_bound_tenfold(fault):
    """each fault in an fp32 evaluation of the masked module (the yardstick itself, under the float64 masks) puts at least one
    gradient tensor 10 x over the bound the GPU test asserts for it"""
    case = gg.BY_ID[FAULT_CASES[fault]]
    data = gg.build_case(case)
    r64, _, y32s = _evaluations(case.id)
    b = gg.bounds(case, y32s, r64)
    bad = gg.evaluate(case, data, torch.float32, masks=gg.own_masks(r64), yardstick=True, fault=fault)
    g64, got = gg.gradient_tensors(case, r64), gg.gradient_tensors(case, bad)
    # (a tensor the fault leaves without any gradient is over every bound)
    over = {k: (gg.rel_err(got[k], g64[k]) / b[k][1] if k in got else float("inf")) for k in g64}
    worst = max(over, key=over.get)
    print("GENGRAD-CPU fault %-28s on %-16s worst %s: %.1e x its bound; %d of %d tensors over"
          % (fault, case.id, worst, over[worst], sum(v > 1 for v in over.values()), len(over)))
    assert over[worst] >= 10.0, over
