"""tests/elementwise_reference.py checked without a GPU:
  * every float64 reference agrees with an independent formulation (torch autograd through batch_norm, F.avg_pool2d with
    count_include_pad=False, oracle.generator_ref.resample and its autograd away from kinks);
  * the fp32 restatement of every GPU case stays inside the case's bound (the worst ratio per case is printed);
  * injected faults in the restatements exceed the bound by at least 10x (the criterion of
    test_cpu_kernel_variants.py::test_bound_sees_injected_faults_at_least_10x);
  * build_case() gives every argument at least extents() floats, and exactly that where ops.py allocates the tensor itself --
    the guard against an out-of-range access through a buffer that is too small."""
import pytest
import torch
import torch.nn.functional as F

import elementwise_reference as er
import kernel_variants as kv

_ids = lambda cases: [c.id for c in cases]


def _side(t, tag):
    return tuple(t[tag + "_" + k] for k in ("y", "mean_rstd", "gamma", "beta", "res"))


# ---- references against independent formulations ------------------------------------------------------------------------------
def test_norm_references_agree_with_batch_norm_autograd():
    g = torch.Generator().manual_seed(1)
    npix, C = 45, 8
    for relu in (0, 1, 2):
        x = torch.randn(npix, C, generator=g)
        dy = torch.randn(npix, C, generator=g)
        ga, be = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        res = torch.randn(npix, C, generator=g)
        xd = x.double().requires_grad_(True)
        gd, bd = ga.double().requires_grad_(True), be.double().requires_grad_(True)
        pre = F.batch_norm(xd.t()[None], None, None, gd, bd, True, 0.0, 1e-5)[0].t()
        # (the references hold the Leaky slope as the kernels do, float32(0.2); it is 7.5e-9 relative from 0.2, inside u)
        y = pre if relu == 0 else F.relu(pre) if relu == 1 else F.leaky_relu(pre, kv.LEAKY32)
        (y * dy.double()).sum().backward()
        # the kernels take (mean, rstd) as given: in float64 here, so that the reference's statistics are batch_norm's
        m = x.double().mean(0)
        mr = torch.stack([m, 1.0 / torch.sqrt(((x.double() - m) ** 2).mean(0) + 1e-5)], 1)
        fwd, _ = kv.lazy_d64(x, mr, ga, be, relu, res)
        assert torch.allclose(fwd, y.detach() + res.double(), rtol=1e-12, atol=1e-12)
        sums, _ = er.bwd_sums64(x, dy, mr, ga, be, relu)
        assert torch.allclose(sums[:, 0], bd.grad, rtol=1e-10, atol=1e-10), relu
        assert torch.allclose(sums[:, 1], gd.grad, rtol=1e-10, atol=1e-10), relu
        dx, _ = kv.dy_front64(dy, x, mr, ga, be, relu, sums, npix)
        assert torch.allclose(dx, xd.grad, rtol=1e-9, atol=1e-10), relu


def test_pool_references_agree_with_avg_pool2d():
    g = torch.Generator().manual_seed(2)
    for (H, W, C) in ((1, 1, 3), (2, 3, 1), (7, 9, 3), (16, 16, 4), (5, 8, 2)):
        x = torch.randn(H, W, C, generator=g)
        xd = x.double().permute(2, 0, 1)[None].requires_grad_(True)
        y = F.avg_pool2d(xd, 3, 2, 1, count_include_pad=False)
        assert er.pool_dims(H, W) == tuple(y.shape[2:])
        dy = torch.randn(y.shape[2], y.shape[3], C, generator=g)
        (y * dy.double().permute(2, 0, 1)[None]).sum().backward()
        assert torch.allclose(er.pool64(x)[0], y[0].permute(1, 2, 0), rtol=1e-12, atol=1e-12)
        assert torch.allclose(er.pool_backward64(dy, H, W)[0], xd.grad[0].permute(1, 2, 0), rtol=1e-12, atol=1e-12)


def test_warp_references_agree_with_the_oracle_and_its_autograd():
    from oracle.generator_ref import resample
    g = torch.Generator().manual_seed(3)
    H, W, cs, c0 = 9, 11, 6, 3
    fw = torch.zeros(H, W, 4)
    fw[..., :2] = torch.randn(H, W, 2, generator=g) * 3          # random: no position on an integer, many outside the image
    fw[..., 2] = torch.rand(H, W, generator=g)
    prev, raw = torch.randn(H, W, cs, generator=g), torch.randn(H, W, 4, generator=g)
    d_out, d_warp = torch.randn(H, W, 4, generator=g), torch.randn(H, W, 4, generator=g)
    img = prev[..., c0:c0 + 3].double().permute(2, 0, 1)[None].requires_grad_(True)
    flow = fw[..., :2].double().permute(2, 0, 1)[None].requires_grad_(True)
    wt = fw[..., 2:3].double().requires_grad_(True)
    warp = resample(img, flow)[0].permute(1, 2, 0)
    out = raw[..., :3].double() * wt + warp * (1 - wt)
    ((out * d_out[..., :3].double()).sum() + (warp * d_warp[..., :3].double()).sum()).backward()
    w64, e = er.warp64(prev, c0, fw)
    assert torch.allclose(w64, warp.detach(), rtol=1e-11, atol=1e-11)
    assert torch.allclose(er.composite64(raw, fw, w64, e)[0], out.detach(), rtol=1e-11, atol=1e-11)
    r = er.warp_backward64(d_out, d_warp, raw, fw, prev, c0)
    assert torch.allclose(r["d_w"], wt.grad[..., 0], rtol=1e-10, atol=1e-10)
    assert torch.allclose(r["d_prev"], img.grad[0].permute(1, 2, 0), rtol=1e-10, atol=1e-10)
    for cands, want in ((r["d_fx"], flow.grad[0, 0]), (r["d_fy"], flow.grad[0, 1])):
        assert torch.allclose(cands[1], want, rtol=1e-10, atol=1e-10)              # the reference position's own cell
        assert er.closest(want, cands).max() < 1e-10


# ---- the restatements inside their bounds, and the faults outside ---------------------------------------------------------------
def _apply_ratio(case, fault=None):
    t = er.build_case(case, "cpu")
    ref, bnd = er.apply64(t["x"], t["mean_rstd"], t["gamma"], t["beta"], case.p["relu"], t["res1"], t["res2"])
    got = er.apply32(t["x"], t["mean_rstd"], t["gamma"], t["beta"], case.p["relu"], t["res1"], t["res2"], fault)
    return (got.double() - ref).abs(), bnd


def _nbwd(case):
    t = er.build_case(case, "cpu")
    a = (t["x"], t["dy"], t["mean_rstd"], t["gamma"], t["beta"], case.p["relu"])
    return t, a


def _warp_ratios(case, fault=None):
    t = er.build_case(case, "cpu")
    c0 = case.p["c0"]
    out = {}
    w64, e = er.warp64(t["prev"], c0, t["fw"])
    o32, w32 = er.warp32(t["raw"], t["fw"], t["prev"], c0, fault)
    o64, eo = er.composite64(t["raw"], t["fw"], w64, e)
    out["warp"] = ((w32.double() - w64).abs(), e)
    out["out"] = ((o32.double() - o64).abs(), eo)
    for mode, (do, dw, raw) in {"composite": (t["d_out"], None, t["raw"]), "warp_only": (None, t["d_warp"], None)}.items():
        r = er.warp_backward64(do, dw, raw, t["fw"], t["prev"], c0)
        d_raw, d_fw, d_prev = er.warp_backward32(do, dw, raw, t["fw"], t["prev"], c0, fault)
        out[mode + " d_fx"] = (er.closest(d_fw[..., 0].double(), r["d_fx"]), r["e_fx"])
        out[mode + " d_fy"] = (er.closest(d_fw[..., 1].double(), r["d_fy"]), r["e_fy"])
        out[mode + " d_prev"] = ((d_prev.double() - r["d_prev"]).abs(), r["e_prev"])
        if do is not None:
            out[mode + " d_w"] = ((d_fw[..., 2].double() - r["d_w"]).abs(), r["e_w"])
            out[mode + " d_raw"] = ((d_raw.double() - r["d_raw"]).abs(), r["e_raw"])
    return out


def restatement_ratios(case):
    """{quantity: worst |restatement - float64| / bound} of one case"""
    p = case.p
    if case.kind == "apply":
        return {"y": er.worst(*_apply_ratio(case))}
    if case.kind == "join":
        t = er.build_case(case, "cpu")
        ref, bnd = er.join64(_side(t, "a"), _side(t, "b"))
        return {"y": er.worst((er.join32(_side(t, "a"), _side(t, "b")).double() - ref).abs(), bnd)}
    if case.kind == "nbwd":
        t, a = _nbwd(case)
        s64, es = er.bwd_sums64(*a)
        s32 = er.bwd_sums32(*a)
        dx64, ed = kv.dy_front64(t["dy"], t["x"], t["mean_rstd"], t["gamma"], t["beta"], p["relu"], s32, t["x"].shape[0])
        dx32 = er.bwd_dx32(*a, s32)
        return {"sums": er.worst((s32.double() - s64).abs(), es), "dx": er.worst((dx32.double() - dx64).abs(), ed)}
    if case.kind == "warp":
        return {k: er.worst(*v) for k, v in _warp_ratios(case).items()}
    if case.kind == "pool":
        t = er.build_case(case, "cpu")
        out = {}
        if p["fwd"]:
            ref, bnd = er.pool64(t["x"])
            out["y"] = er.worst((er.pool32(t["x"]).double() - ref).abs(), bnd)
        if p["bwd"]:
            ref, bnd = er.pool_backward64(t["dy"], p["H"], p["W"])
            out["dx"] = er.worst((er.pool_backward32(t["dy"], p["H"], p["W"]).double() - ref).abs(), bnd)
        return out
    if case.kind == "act":
        t = er.build_case(case, "cpu")
        ref, bnd = er.act64(t["dy"], t["y"], p["mode"], p["slope"])
        return {"dpre": er.worst((er.act32(t["dy"], t["y"], p["mode"], p["slope"]).double() - ref).abs(), bnd)}
    if case.kind == "ml1":
        t = er.build_case(case, "cpu")
        ref, bnd = er.ml1_64(t["a"], t["b"], t["mask"], p["c0"], p["C"])
        return {"sum": er.worst((er.ml1_32(t["a"], t["b"], t["mask"], p["c0"], p["C"]).double() - ref).abs(), bnd)}
    if case.kind == "lossbwd":
        t = er.build_case(case, "cpu")
        ref, bnd = er.loss_backward64(t["a"], t["b"], 0.25, 0.37, p["op"])
        return {"da": er.worst((er.loss_backward32(t["a"], t["b"], 0.25, 0.37, p["op"]).double() - ref).abs(), bnd)}
    raise KeyError(case.kind)


@pytest.mark.parametrize("case", er.ALL_CASES, ids=_ids(er.ALL_CASES))
def test_fp32_restatement_stays_inside_the_bound(case):
    ratios = restatement_ratios(case)
    assert ratios
    for what, r in ratios.items():
        print("%-34s %-22s restatement worst |error| / bound %.3g" % (case.id, what, r))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, "%s: the fp32 restatement leaves the bound: %s" % (case.id, bad)


def _q(err, ref_err, bnd):
    """10th and 25th percentile of |fault - reference| / bound over the outputs the fault moves (cf. _fault_ratio of
    test_cpu_kernel_variants.py); ref_err: the unfaulted restatement's error, to tell what moved"""
    touched = (err - ref_err).abs() > 1e-9 * (err + ref_err + 1e-30)
    assert touched.any(), "the fault touches no output"
    r = (err[touched] / bnd[touched].clamp(min=1e-300)).flatten()
    return r.quantile(0.10).item(), r.quantile(0.25).item(), int(touched.sum())


def test_bounds_see_injected_faults_at_least_10x():
    rows = {}
    by = er.BY_ID
    # norm apply: image 1 normalised with image 0's table; res2 dropped
    case = by["apply_batch3_11x13_c12"]
    base, bnd = _apply_ratio(case)
    for fault in ("table0", "res2"):
        rows["apply: " + fault] = _q(_apply_ratio(case, fault)[0], base, bnd)
    # norm backward: a stride that is no multiple of C4; S1 / N with N - 1; the reduction's tail pixels dropped
    for cid in ("nbwd_12x20_c12_relu2_affine", "nbwd_25x40_c132_relu1_plain"):
        case = by[cid]
        t, a = _nbwd(case)
        assert er.bwd_apply_blocks(t["x"].shape[0], case.p["C"], False) != er.bwd_apply_blocks(t["x"].shape[0], case.p["C"]), cid
        s32 = er.bwd_sums32(*a)
        dx64, ed = kv.dy_front64(t["dy"], t["x"], t["mean_rstd"], t["gamma"], t["beta"], case.p["relu"], s32, t["x"].shape[0])
        base = (er.bwd_dx32(*a, s32).double() - dx64).abs()
        for fault in ("stride", "n-1"):
            rows["nbwd dx: %s (%s)" % (fault, cid)] = _q((er.bwd_dx32(*a, s32, fault).double() - dx64).abs(), base, ed)
        s64, es = er.bwd_sums64(*a)
        rows["nbwd sums: tail (%s)" % cid] = _q((er.bwd_sums32(*a, "tail").double() - s64).abs(), (s32.double() - s64).abs(), es)
    # warp: wy0 / wy1 swapped in d_flow_x; prev_c0 off by one
    case = by["warp_17x23_std12"]
    base = _warp_ratios(case)
    f = _warp_ratios(case, "wy")
    rows["warp d_fx: wy0 / wy1 swapped"] = _q(f["composite d_fx"][0], base["composite d_fx"][0], base["composite d_fx"][1])
    f = _warp_ratios(case, "c0")
    for k in ("warp", "composite d_fx", "warp_only d_fy", "composite d_w"):   # (d_prev's VALUES do not depend on prev: the GPU
        # test sees this fault in the channels outside [c0, c0 + 3), which must stay exactly 0)
        rows["warp %s: prev_c0 off by one" % k] = _q(f[k][0], base[k][0], base[k][1])
    # avgpool: divisor 9 at the border
    case = by["pool_7x9_c3"]
    t = er.build_case(case, "cpu")
    ref, bnd = er.pool64(t["x"])
    rows["pool: divisor 9"] = _q((er.pool32(t["x"], "nine").double() - ref).abs(), (er.pool32(t["x"]).double() - ref).abs(), bnd)
    ref, bnd = er.pool_backward64(t["dy"], 7, 9)
    rows["pool backward: divisor 9"] = _q((er.pool_backward32(t["dy"], 7, 9, "nine").double() - ref).abs(),
                                          (er.pool_backward32(t["dy"], 7, 9).double() - ref).abs(), bnd)
    # masked L1 ignoring c0
    for cid in ("ml1_20x28_cs4_c2_C1_full", "ml1_20x28_cs8_c3_C3_nomask"):
        case = by[cid]
        t = er.build_case(case, "cpu")
        ref, bnd = er.ml1_64(t["a"], t["b"], t["mask"], case.p["c0"], case.p["C"])
        args = (t["a"], t["b"], t["mask"], case.p["c0"], case.p["C"])
        rows["masked L1: c0 ignored (%s)" % cid] = _q((er.ml1_32(*args, "c0").double() - ref).abs().view(1),
                                                      (er.ml1_32(*args).double() - ref).abs().view(1), bnd.view(1))
    lines = ["%-58s |fault| / bound: 10th pct %9.3g, 25th pct %9.3g over %d outputs" % ((k,) + v) for k, v in rows.items()]
    print("\n".join(lines))
    weak = [ln for (k, (p10, p25, n)), ln in zip(rows.items(), lines) if p25 < 10 or p10 < 2]
    assert not weak, "faults too close to the bound:\n" + "\n".join(weak)


# ---- buffers against extents ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", er.ALL_CASES, ids=_ids(er.ALL_CASES))
def test_case_buffers_cover_what_the_kernels_index(case):
    t = er.build_case(case, "cpu")
    ext = er.extents(case)
    for name, tensor in t.items():
        assert name in ext, "%s: extents() does not know argument %s" % (case.id, name)
        if tensor is None:
            assert ext[name] == 0, "%s: %s is None but the kernel indexes %d floats of it" % (case.id, name, ext[name])
            continue
        assert tensor.dtype == torch.float32 and tensor.is_contiguous(), (case.id, name)
        assert tensor.storage_offset() % 4 == 0, (case.id, name)
        assert tensor.numel() >= ext[name], "%s: %s holds %d floats, the kernel indexes %d" % (case.id, name, tensor.numel(), ext[name])
    for name, (n, exact) in er.allocated(case).items():
        assert n >= ext[name], "%s: ops allocates %d floats for %s, the kernel indexes %d" % (case.id, n, name, ext[name])
        assert not exact or n == ext[name], "%s: %s allocated %d != %d" % (case.id, name, n, ext[name])
    # the NaN-margined out= buffers the GPU test builds for this case
    for name in ("out", "dx"):
        if name in ext and case.kind in ("apply", "join", "nbwd"):
            buf, view = er.nan_margin(ext[name], "cpu")
            assert view.numel() == ext[name] and view.is_contiguous() and view.storage_offset() % 4 == 0
            assert buf.numel() == ext[name] + 2 * er.MARGIN


def test_cases_reach_the_edges_they_are_named_for():
    by = er.BY_ID
    p = by["apply_82x100_c256_relu1"].p
    assert p["H"] * p["W"] * p["C"] // 4 == 524800 > er.GRID_CAP                     # a second trip of 512 float4
    assert [er.bwd_slices(c.p["H"] * c.p["W"], c.p["C"]) for c in er.NORM_BWD_CASES[-2:]] == [128, 64]
    assert (82 * 100 + 63) // 64 == 129 and (41 * 100 + 63) // 64 == 65              # ... both caps bind
    for (H, W, C) in ((12, 20, 12), (25, 40, 68), (25, 40, 132)):                     # the lcm_blocks round-up acts
        assert er.bwd_apply_blocks(H * W, C) > er.bwd_apply_blocks(H * W, C, round_up=False), (H, W, C)
    assert er.bwd_apply_blocks(82 * 100, 64) == er.bwd_apply_blocks(82 * 100, 64, round_up=False)
    assert 513 * 1024 == 525312 > er.GRID_CAP
    assert 129 * 129 * 32 == 532512 > er.GRID_CAP and 128 * 129 * 32 == 528384 > er.GRID_CAP
    assert 257 * 512 * 4 == 526336 > er.GRID_CAP and 524292 > er.GRID_CAP and 524292 % 4 == 0 and 524289 > er.GRID_CAP
    assert {(c.p["cs"], c.p["c0"]) for c in er.WARP_CASES} >= {(3, 0), (4, 0), (6, 3), (8, 3), (12, 9)}
    # zero flow, an integer flow and the edge rows put the float64 position exactly on a kink
    for cid in ("warp_64x64_zero", "warp_64x64_const", "warp_19x21_edges"):
        t = er.build_case(by[cid], "cpu")
        px, py, ex, ey = er.warp_pos64(t["fw"])
        assert ((px - px.round()).abs() < ex).sum() >= t["fw"].shape[1], cid
    px, py, _, _ = er.warp_pos64(er.build_case(by["warp_2x2"], "cpu")["fw"])
    assert ((px > 0) & (px < 1) & (py > 0) & (py < 1)).sum() == 3          # the minimum extent still interpolates
    t = er.build_case(by["warp_19x21_edges"], "cpu")
    px, py, _, _ = er.warp_pos64(t["fw"])
    assert (px[5] == 20).all() and (py[:, 8] == 18).all() and (px[9] == 0).all() and (py[:, 3] == 0).all()
    t = er.build_case(by["nbwd_7x5_c4_relu1_affine"], "cpu")
    assert (t["x"][:, er.PIN_CH] == t["mean_rstd"][er.PIN_CH, 0]).all() and t["beta"][er.PIN_CH] == 0
