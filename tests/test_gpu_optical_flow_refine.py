"""ops.optical_flow(..., refine_iters=N) (t2v_optical_flow_refined: Lucas-Kanade plus Horn-Schunck Jacobi steps at every
pyramid level, csrc/optical_flow_refine.hip) against its float64 restatement (tests/flow_refine_reference.py), the bit-identities the
header promises, and the flags that select the refined flow: train.py --flow_ref lkhs and --temporal_flow lkhs.

Kernel bound: max |HIP - f64| <= max(8 * e32, 1.7e-5 px) over EVERY pixel, e32 = the maximum error of the same restatement
run in float32 on the CPU in the same test.  8x allows another legitimate fp32 evaluation (the kernel multiplies by 1/6, 1/12
and by a reciprocal of the denominator formed once; the window sums of the LK part go rows first); the floor is 5x the largest
e32 seen on these cases (3.35e-6 px, on D1; 3.0e-7 .. 3.1e-6 px on the others), set as tests/test_gpu_optical_flow.py sets
its own, so that a lucky CPU run does not set an unreachable bound."""
import numpy as np
import pytest
import torch

import flow_reference as fr
import flow_refine_reference as rr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOOR = 1.7e-5
GEOMETRY = sorted(rr.GEOMETRY_CASES)
TRAIN_ARGS = ["--name", "t", "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only", "--ngf", "16",
              "--n_downsample_G", "2", "--n_blocks", "2", "--num_D", "1", "--ndf", "16", "--no_vgg"]


def _dev4(img3):
    t = torch.zeros(img3.shape[0], img3.shape[1], 4)
    t[..., :3] = img3
    return t.to(DEV)


_frames = {}


def _pair_dev(name):
    """the case's fp32 frames on the device (case_rgb's cur3, prev3 do not depend on the step count)"""
    if name not in _frames:
        c = rr.case_rgb(name, 5 if name in rr.GEOMETRY_CASES else rr.REFINE_ITERS)
        _frames[name] = (_dev4(c["cur3"]), _dev4(c["prev3"]), c["kw"])
    return _frames[name]


def _hip(name, refine_iters=rr.REFINE_ITERS, **over):
    from text2video_amd import ops
    cur, prev, kw = _pair_dev(name)
    return ops.optical_flow(cur, prev, refine_iters=refine_iters, **dict(kw, **over))


def _check_against_float64(name, refine_iters):
    c = rr.case_rgb(name, refine_iters)
    out = _hip(name, refine_iters).cpu()
    assert out.shape == c["u64"].shape + (4,)
    err = max((out[..., 0].double() - c["u64"]).abs().max().item(), (out[..., 1].double() - c["v64"]).abs().max().item())
    bound = max(8 * c["e32"], FLOOR)
    print("case %s, %d steps: max|HIP - f64| = %.3g px, e32 = %.3g px, bound %.3g px" % (name, refine_iters, err, c["e32"], bound))
    assert torch.isfinite(out).all() and (out[..., 2:] == 0).all()
    assert err <= bound, (name, refine_iters, err, c["e32"])
    return c, out


@pytest.mark.parametrize("name", ["A", "B", "C", "D1"])
def test_kernel_matches_the_float64_restatement_at_every_pixel(name):
    c, out = _check_against_float64(name, rr.REFINE_ITERS)
    if name in fr.CASES:      # the definition's functional bounds hold for the kernel's output as well
        epe, ratio = fr.functional_figures(c, out[..., 0], out[..., 1])
        print("case %s: HIP mean endpoint error %.4f px, residual ratio %.4f" % (name, epe, ratio))
        assert epe <= fr.MAX_EPE and ratio <= fr.MAX_RESIDUAL_RATIO, (name, epe, ratio)


@pytest.mark.parametrize("refine_iters", [5, 64])
@pytest.mark.parametrize("name", GEOMETRY)
def test_kernel_matches_the_float64_restatement_on_the_tile_geometries(name, refine_iters):
    """a level smaller than the 16 x 16 tile, tiles hanging over the right and bottom edge, more than one block, odd sizes at
    every level, one level: wherever a cell outside the image could be taken for a cell"""
    _check_against_float64(name, refine_iters)


@pytest.mark.parametrize("name", GEOMETRY)
def test_the_result_does_not_depend_on_the_steps_per_launch(name):
    """5 steps as 1+1+1+1+1, 2+2+1, 5 (of at most MAX_FUSED) and the library's choice: four bit-equal flows"""
    from text2video_amd import _flowlib
    assert _flowlib.MAX_FUSED >= 4 and 5 % _flowlib.MAX_FUSED != 0
    flows = [_hip(name, 5, iters_per_launch=k).clone() for k in (1, 2, _flowlib.MAX_FUSED, 0)]
    for k, f in zip((2, _flowlib.MAX_FUSED, 0), flows[1:]):
        assert torch.equal(flows[0], f), (name, k, (flows[0] - f).abs().max().item())
    assert not torch.equal(flows[0], _hip(name, 4, iters_per_launch=1))         # (the fifth step does something)


def test_no_refinement_steps_is_the_lk_entry_bit_for_bit():
    from text2video_amd import ops
    for name in ("B", "g37x70_l2"):
        cur, prev, kw = _pair_dev(name)
        want = ops.optical_flow(cur, prev, **kw)
        for extra in (dict(refine_iters=0, alpha=0.5), dict(refine_iters=0, iters_per_launch=3)):
            assert torch.equal(want, ops.optical_flow(cur, prev, **dict(kw, **extra))), (name, extra)
        assert not torch.equal(want, ops.optical_flow(cur, prev, refine_iters=1, **kw))
    cur8, prev8 = _bytes("A")
    want = ops.optical_flow_u8(cur8[0], prev8[1])
    assert torch.equal(want, ops.optical_flow_u8(cur8[0], prev8[1], refine_iters=0, alpha=0.5))


def _bytes(name):
    """-> ((cur with stride 3, with stride 4), (prev ...)) uint8 device frames of a case"""
    c = rr.pair(name)
    out = []
    for img in (c["cur"], c["prev"]):
        g = 20.0 + (img.numpy() + 1.0) / 2.0 * 200.0
        b = np.clip(np.round(np.stack([g, 0.8 * g + 10.0, 0.9 * g + 25.0], -1)), 0, 255).astype(np.uint8)
        b4 = np.concatenate([b, np.full(b.shape[:2] + (1,), 77, np.uint8)], -1)
        out.append((torch.from_numpy(b).to(DEV), torch.from_numpy(b4).to(DEV)))
    return out


def test_u8_entry_is_bit_equal_to_the_fp32_entry_on_the_converted_frames():
    from text2video_amd import ops
    cur8, prev8 = _bytes("B")
    H, W = cur8[0].shape[:2]
    f32 = [ops.pose_u8_to_f32(t[0], torch.zeros(H, W, 4, device=DEV), 0) for t in (cur8, prev8)]
    want = ops.optical_flow(f32[0], f32[1], refine_iters=7)
    assert torch.isfinite(want).all() and want[..., :2].abs().max().item() > 0.1
    for ci in (0, 1):
        for pi in (0, 1):
            got = ops.optical_flow_u8(cur8[ci], prev8[pi], refine_iters=7)
            assert torch.isfinite(got).all() and torch.equal(got, want), (ci, pi)
    kw = dict(levels=1, iters=2, radius=2, lam=1e-2, refine_iters=3, alpha=0.1, iters_per_launch=2)
    assert torch.equal(ops.optical_flow_u8(cur8[1], prev8[0], **kw), ops.optical_flow(f32[0], f32[1], **kw))


def test_calls_are_bit_equal_and_an_explicit_workspace_changes_nothing():
    from text2video_amd import ops
    a = _hip("B").clone()
    b = _hip("B").clone()
    assert torch.equal(a, b)
    ws = ops.optical_flow_workspace(85, 64, None, DEV, refined=True)
    assert ws.numel() == 2 * ops.optical_flow_workspace(85, 64, None, DEV).numel()
    ws.fill_(float("inf"))                      # any content
    out = torch.full((85, 64, 4), 7.0, device=DEV)
    got = _hip("B", workspace=ws, out=out)
    assert got is out and torch.equal(a, out)
    with pytest.raises(ValueError, match="workspace"):
        _hip("B", workspace=ops.optical_flow_workspace(85, 64, None, DEV))      # the LK workspace is too small for it


def test_constant_images_give_exact_zeros():
    from text2video_amd import ops
    img = torch.full((40, 56, 4), 0.375, device=DEV)
    out = ops.optical_flow(img, img.clone(), refine_iters=64)
    assert (out == 0).all()


def test_refinement_fills_the_textureless_disc():
    """what the feature is for: inside the flat disc of D1 the LK kernel is 0.56 px off on average, the refined one 0.11 px"""
    c = rr.pair("D1")
    lk, hs = _hip("D1", 0).cpu(), _hip("D1").cpu()
    e_lk, e_hs = rr.inner_epe(c, lk[..., 0], lk[..., 1]), rr.inner_epe(c, hs[..., 0], hs[..., 1])
    print("D1 through the kernel: inner mean EPE lk %.4f -> refined %.4f px (ratio %.3f)" % (e_lk, e_hs, e_hs / e_lk))
    assert e_hs <= rr.MAX_INNER_RATIO * e_lk, (e_lk, e_hs)


def test_refused_arguments_report_through_last_error_and_leave_the_output_alone():
    from text2video_amd import _flowlib, ops
    img = torch.zeros(16, 16, 4, device=DEV)
    small = torch.zeros(7, 16, 4, device=DEV)
    big = _flowlib.MAX_FUSED + 1
    for cur, kw, word in ((small, {}, "must be >= 8"), (img, dict(radius=0), "radius"), (img, dict(radius=8), "radius"),
                          (img, dict(iters=0), "iters"), (img, dict(lam=0.0), "lambda"), (img, dict(levels=9), "level count"),
                          (img, dict(cur_c0=2), "channel"),
                          (img, dict(alpha=0.0), "alpha"), (img, dict(alpha=-0.2), "alpha"), (img, dict(alpha=float("nan")), "alpha"),
                          (img, dict(alpha=float("inf")), "alpha"), (img, dict(refine_iters=-1), "refine_iters"),
                          (img, dict(refine_iters=1025), "refine_iters"), (img, dict(iters_per_launch=-1), "iters_per_launch"),
                          (img, dict(iters_per_launch=big), "iters_per_launch")):
        out = torch.full(cur.shape[:2] + (4,), 3.0, device=DEV)
        with pytest.raises(RuntimeError, match=word):
            ops.optical_flow(cur, cur.clone(), out=out, **dict(dict(refine_iters=4), **kw))
        torch.cuda.synchronize()
        assert (out == 3.0).all(), kw               # nothing ran
    b = torch.zeros(16, 16, 3, dtype=torch.uint8, device=DEV)
    for kw, word in ((dict(alpha=0.0), "alpha"), (dict(refine_iters=2000), "refine_iters"), (dict(iters_per_launch=big), "iters_per_launch")):
        out = torch.full((16, 16, 4), 3.0, device=DEV)
        with pytest.raises(RuntimeError, match=word):
            ops.optical_flow_u8(b, b.clone(), out=out, **dict(dict(refine_iters=4), **kw))
        torch.cuda.synchronize()
        assert (out == 3.0).all(), kw


# ---------------------------------------------------------------------------------------------------------------------
# the train step
# ---------------------------------------------------------------------------------------------------------------------
def _opt(*extra):
    from text2video_amd.options import TrainOptions
    return TrainOptions().parse(TRAIN_ARGS + list(extra))


def test_flow_ref_lkhs_feeds_the_refined_estimate_to_the_flow_losses():
    from text2video_amd import ops
    from text2video_amd import train as T
    H = W = 64
    fs = []
    for k in range(2):      # two real frames of one texture moving by (1.5, -2.25) px, oldest first
        fs.append(_dev4(fr.rgb(fr.affine_pair(H, W, shift=(1.5 * (1 - k), -2.25 * (1 - k)))[1])))
    real_prev, real = fs[0][None].contiguous(), fs[1][None].contiguous()
    rng = np.random.default_rng(3)
    pose = torch.zeros(1, H, W, 12, device=DEV)
    pose[..., :9] = torch.from_numpy(rng.uniform(-1, 1, (1, H, W, 9)).astype(np.float32)).to(DEV)
    prev_in = torch.zeros(1, H, W, 8, device=DEV)
    base = ["--max_frames_per_gpu", "1", "--n_scales_temporal", "0"]

    def step(args, **kw):
        tr = T.Vid2VidTrainer(_opt(*(base + args)), DEV, seed=7)
        return tr.train_step(pose, real, None, prev_in.clone(), real_prev=real_prev, **kw)[0]
    refined = torch.stack([ops.optical_flow(real[0], real_prev[0], refine_iters=64)])
    plain = torch.stack([ops.optical_flow(real[0], real_prev[0])])
    assert not torch.equal(refined, plain)
    lkhs = step(["--flow_ref", "lkhs"])
    assert lkhs == step(["--flow_ref", "zero"], flow_ref=refined)
    lk = step(["--flow_ref", "lk"])
    for k in ("F_Flow", "G_Warp"):
        assert lkhs[k] != lk[k], (k, lk[k])
    # lk and the default are what they were: the LK flow handed in, and the zero flow
    assert lk == step(["--flow_ref", "zero"], flow_ref=plain)
    assert step([]) == step(["--flow_ref", "zero"]) == step([], flow_ref=torch.zeros_like(plain))
    # the flags reach the estimator
    other = step(["--flow_ref", "lkhs", "--flow_refine_iters", "8", "--flow_alpha", "0.5"])
    assert other == step([], flow_ref=torch.stack([ops.optical_flow(real[0], real_prev[0], refine_iters=8, alpha=0.5)]))
    assert other != lkhs
    tr = T.Vid2VidTrainer(_opt("--max_frames_per_gpu", "2", "--n_scales_temporal", "1", "--n_frames_D", "2", "--flow_ref", "lkhs"),
                          DEV, seed=7)
    got = tr._temporal_flows(fs, [1], 1)
    assert torch.equal(got[0], refined[0, ..., :2])


# ---------------------------------------------------------------------------------------------------------------------
# the temporal metrics
# ---------------------------------------------------------------------------------------------------------------------
def test_temporal_flow_lk_is_the_present_report_and_lkhs_changes_it(tmp_path):
    from PIL import Image
    from text2video_amd import evaluate, ops
    from text2video_amd import metrics as M
    H, W = 64, 96
    frames = {}
    for tree, seed in (("a", 3), ("b", 3)):
        for k in range(2):
            img = fr.affine_pair(H, W, shift=(1.5 * (1 - k), -2.25 * (1 - k)), seed=seed)[1].numpy()
            g = 20.0 + (img + 1.0) / 2.0 * (200.0 if tree == "b" else 180.0)
            frames[tree, k] = np.clip(np.round(np.stack([g, 0.8 * g + 10.0, 0.9 * g + 25.0], -1)), 0, 255).astype(np.uint8)
            d = tmp_path / tree / "seq"
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(frames[tree, k]).save(str(d / ("fake_B_%04d.png" % k)))
    a_prev, a_cur, b_prev, b_cur = (torch.from_numpy(frames[k]).to(DEV) for k in (("a", 0), ("a", 1), ("b", 0), ("b", 1)))

    def rows(**kw):
        return ops.temporal_metrics(a_cur, a_prev, b_cur, b_prev, ops.optical_flow_u8(b_cur, b_prev, **kw),
                                    ops.optical_flow_u8(b_prev, b_cur, **kw), ops.optical_flow_u8(a_cur, a_prev, **kw)).cpu().numpy()
    present, refined = rows(), rows(refine_iters=64, alpha=0.2)
    assert present[0][0] != refined[0][0] or present[0][2] != refined[0][2]          # n_valid or warp_sse_b
    dirs = (str(tmp_path / "a"), str(tmp_path / "b"))
    default = evaluate.compare_trees(*dirs, pattern="fake_B_*", device=DEV, temporal=True)
    lk = evaluate.compare_trees(*dirs, pattern="fake_B_*", device=DEV, temporal=True, temporal_flow="lk")
    lkhs = evaluate.compare_trees(*dirs, pattern="fake_B_*", device=DEV, temporal=True, temporal_flow="lkhs")
    assert default == lk and lk["temporal_flow"] == "lk" and lk["temporal_definition"] == ops.TEMPORAL_DEFINITION
    assert lk["overall"]["temporal"] == M.pool_temporal([(present[0], H * W)]) == lk["sequences"]["seq"]["temporal"]
    assert lkhs["overall"]["temporal"] == M.pool_temporal([(refined[0], H * W)]) != lk["overall"]["temporal"]
    assert lkhs["temporal_flow"] == "lkhs" and "lkhs" in lkhs["temporal_definition"]
    assert {k: v for k, v in lkhs.items() if not k.startswith("temporal") and k not in ("overall", "sequences")} == \
        {k: v for k, v in lk.items() if not k.startswith("temporal") and k not in ("overall", "sequences")}
    # test.py --metrics_temporal keeps a sequence's rows in metrics.SequenceRows
    docs = {}
    for choice in ("lk", "lkhs"):
        sr = M.SequenceRows(torch, "seq", 2, DEV, True, choice) if choice != "lk" else M.SequenceRows(torch, "seq", 2, DEV, True)
        sr.compare(a_prev, b_prev, "0.jpg", None)
        sr.compare(a_cur, b_cur, "1.jpg", None)
        docs[choice] = M.summarise(sr.frames, *sr.split_host(sr.buf.cpu().numpy()), temporal_flow=sr.temporal_flow)
    want = ops.temporal_summary(present[0], H * W)
    want["face"] = None
    assert docs["lk"]["frames"][1]["temporal"] == want and docs["lk"]["temporal_definition"] == ops.TEMPORAL_DEFINITION
    want = ops.temporal_summary(refined[0], H * W)
    want["face"] = None
    assert docs["lkhs"]["frames"][1]["temporal"] == want and "lkhs" in docs["lkhs"]["temporal_definition"]
    assert docs["lkhs"]["frames"][0] == docs["lk"]["frames"][0]
    with pytest.raises(ValueError):
        M.SequenceRows(torch, "seq", 2, DEV, True, "farneback")
