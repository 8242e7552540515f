"""ops.optical_flow (t2v_optical_flow: dense coarse-to-fine Lucas-Kanade, csrc/optical_flow.hip) against its float64
restatement (tests/flow_reference.py), and the train step's --flow_ref lk that feeds it to the flow / warp losses and the
temporal discriminators' flow channels.

Kernel bound: max |HIP - f64| <= max(8 * e32, 2e-5 px) over EVERY pixel, e32 = the maximum error of the same restatement
run in float32 on the CPU in the same test (1e-6 .. 4e-6 px on these cases).  8x allows another legitimate fp32 summation
order in the window sums (the kernel sums rows, then columns); the floor is 5x the largest e32 seen, so that a lucky CPU
run does not set an unreachable bound."""
import numpy as np
import pytest
import torch

import flow_reference as fr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TRAIN_ARGS = ["--name", "t", "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only", "--ngf", "16",
              "--n_downsample_G", "2", "--n_blocks", "2", "--num_D", "1", "--ndf", "16", "--no_vgg"]


def _place(img3, cs, c0):
    """fp32 [H,W,3] -> device [H,W,cs] with the image at channels c0..c0+2 and noise everywhere else"""
    g = torch.Generator().manual_seed(cs * 16 + c0)
    t = torch.randn(img3.shape[0], img3.shape[1], cs, generator=g)
    t[..., c0:c0 + 3] = img3
    return t.to(DEV).contiguous()


def _hip_flow(name, **over):
    from text2video_amd import ops
    c = fr.case_rgb(name)
    # case C: the images inside wider tensors, cur and prev with different strides and offsets
    (ccs, cc0), (pcs, pc0) = ((8, 3), (12, 5)) if name == "C" else ((4, 0), (4, 0))
    kw = dict(c["kw"], **over)
    return ops.optical_flow(_place(c["cur3"], ccs, cc0), _place(c["prev3"], pcs, pc0), cur_c0=cc0, prev_c0=pc0, **kw)


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_kernel_matches_the_float64_restatement_at_every_pixel(name):
    c = fr.case_rgb(name)
    out = _hip_flow(name).cpu()
    assert out.shape == c["u64"].shape + (4,)
    err = max((out[..., 0].double() - c["u64"]).abs().max().item(), (out[..., 1].double() - c["v64"]).abs().max().item())
    bound = max(8 * c["e32"], 2e-5)
    print("case %s: max|HIP - f64| = %.3g px, e32 = %.3g px, bound %.3g px" % (name, err, c["e32"], bound))
    assert err <= bound, (name, err, c["e32"])
    assert (out[..., 2:] == 0).all()
    # the definition's functional bounds hold for the kernel's output as well
    epe, ratio = fr.functional_figures(c, out[..., 0], out[..., 1])
    print("case %s: HIP mean endpoint error %.4f px, residual ratio %.4f" % (name, epe, ratio))
    assert epe <= fr.MAX_EPE and ratio <= fr.MAX_RESIDUAL_RATIO, (name, epe, ratio)


@pytest.mark.parametrize("name", sorted(fr.EDGE_CASES))
def test_kernel_matches_the_float64_restatement_at_the_edges_of_its_geometry(name):
    """radius 7 (the LDS staging at its full extent, a window wider than the smallest frame), radius 1, a single level"""
    c = fr.case_rgb(name)
    out = _hip_flow(name).cpu()
    err = max((out[..., 0].double() - c["u64"]).abs().max().item(), (out[..., 1].double() - c["v64"]).abs().max().item())
    print("case %s: max|HIP - f64| = %.3g px, e32 = %.3g px" % (name, err, c["e32"]))
    assert torch.isfinite(out).all() and (out[..., 2:] == 0).all()
    assert err <= max(8 * c["e32"], 2e-5), (name, err, c["e32"])


def test_calls_are_bit_equal_and_an_explicit_workspace_changes_nothing():
    from text2video_amd import ops
    a = _hip_flow("B").clone()
    b = _hip_flow("B").clone()
    assert torch.equal(a, b)
    ws = ops.optical_flow_workspace(85, 64, None, DEV)
    ws.fill_(float("inf"))                      # any content
    out = torch.full((85, 64, 4), 7.0, device=DEV)
    got = _hip_flow("B", workspace=ws, out=out)
    assert got is out and torch.equal(a, out)
    # explicit level count = what the default rule picks
    assert torch.equal(a, _hip_flow("B", levels=3))
    assert not torch.equal(a, _hip_flow("B", levels=1))


def test_constant_images_give_exact_zeros():
    from text2video_amd import ops
    img = torch.full((40, 56, 4), 0.375, device=DEV)
    out = ops.optical_flow(img, img.clone())
    assert (out == 0).all()


def test_refused_arguments_report_through_last_error_and_leave_the_output_alone():
    from text2video_amd import ops
    img = torch.zeros(16, 16, 4, device=DEV)
    small = torch.zeros(7, 16, 4, device=DEV)
    narrow = torch.zeros(16, 6, 4, device=DEV)
    for cur, kw, word in ((small, {}, "must be >= 8"), (narrow, {}, "must be >= 8"), (img, dict(radius=0), "radius"),
                          (img, dict(radius=8), "radius"), (img, dict(iters=0), "iters"), (img, dict(cur_c0=2), "channel")):
        out = torch.full(cur.shape[:2] + (4,), 3.0, device=DEV)
        with pytest.raises(RuntimeError, match=word):
            ops.optical_flow(cur, cur.clone(), out=out, **kw)
        torch.cuda.synchronize()
        assert (out == 3.0).all()               # nothing ran


# ---------------------------------------------------------------------------------------------------------------------
# the train step
# ---------------------------------------------------------------------------------------------------------------------
def _frames(n, H=64, W=64):
    """n + 1 real frames [H,W,4] of one analytic texture moving by (1.5, -2.25) px per frame (case A's motion), oldest first"""
    out = []
    for k in range(n + 1):
        img = fr.affine_pair(H, W, shift=(1.5 * (n - k), -2.25 * (n - k)))[1]       # frame n = the texture itself
        t = torch.zeros(H, W, 4)
        t[..., :3] = fr.rgb(img)
        out.append(t.to(DEV))
    return out


def _pose(F_, H=64, W=64, seed=3):
    rng = np.random.default_rng(seed)
    pose = torch.zeros(F_, H, W, 12, device=DEV)
    pose[..., :9] = torch.from_numpy(rng.uniform(-1, 1, (F_, H, W, 9)).astype(np.float32)).to(DEV)
    return pose


def _opt(*extra):
    from text2video_amd.options import TrainOptions
    return TrainOptions().parse(TRAIN_ARGS + list(extra))


def test_flow_ref_lk_feeds_the_estimate_to_the_flow_losses():
    from text2video_amd import ops
    from text2video_amd import train as T
    fs = _frames(1)
    real_prev, real = fs[0][None].contiguous(), fs[1][None].contiguous()
    pose = _pose(1)
    prev_in = torch.zeros(1, 64, 64, 8, device=DEV)
    base = ["--max_frames_per_gpu", "1", "--n_scales_temporal", "0"]

    def step(args, **kw):
        tr = T.Vid2VidTrainer(_opt(*(base + args)), DEV, seed=7)
        return tr.train_step(pose, real, None, prev_in.clone(), real_prev=real_prev, **kw)[0]
    flow = torch.stack([ops.optical_flow(real[0], real_prev[0])])
    assert flow[..., :2].abs().mean().item() > 1.0           # there is a motion to find: (1.5, -2.25) px
    lk = step(["--flow_ref", "lk"])
    handed = step(["--flow_ref", "zero"], flow_ref=flow)
    today = step([])                                          # the option absent from the command line
    zero = step(["--flow_ref", "zero"])
    assert lk == handed, (lk, handed)
    assert zero == today, (zero, today)
    for k in ("F_Flow", "G_Warp"):
        assert lk[k] != zero[k], (k, lk[k])
    # an explicit flow_ref still wins under lk
    assert step(["--flow_ref", "lk"], flow_ref=torch.zeros_like(flow)) == step([], flow_ref=torch.zeros_like(flow))


def test_temporal_flows_are_the_flows_between_consecutive_real_frames():
    from text2video_amd import ops
    from text2video_amd import train as T
    fs = _frames(2)
    tr = T.Vid2VidTrainer(_opt("--max_frames_per_gpu", "3", "--n_scales_temporal", "1", "--flow_ref", "lk"), DEV, seed=7)
    got = tr._temporal_flows(fs, [2], 1)
    assert got.shape == (1, 64, 64, 4)
    assert torch.equal(got[0, ..., 0:2], ops.optical_flow(fs[1], fs[0])[..., :2])
    assert torch.equal(got[0, ..., 2:4], ops.optical_flow(fs[2], fs[1])[..., :2])
    stacked = tr._temporal_stack(fs, [2], 1, tr.DT[0], got)
    assert stacked.shape == (1, 64, 64, 16)
    assert torch.equal(stacked[0, ..., 9:13], got[0]) and (stacked[0, ..., 13:] == 0).all()
    assert all(torch.equal(stacked[0, ..., 3 * k:3 * k + 3], fs[k][..., :3]) for k in range(3))
    tr0 = T.Vid2VidTrainer(_opt("--max_frames_per_gpu", "3", "--n_scales_temporal", "1"), DEV, seed=7)
    assert tr0._temporal_flows(fs, [2], 1) is None
    assert (tr0._temporal_stack(fs, [2], 1, tr0.DT[0])[0, ..., 9:] == 0).all()


@pytest.mark.parametrize("batched", ["1", "0"])
def test_three_frame_sequence_with_a_temporal_discriminator(batched, t2v_env):
    """both step bodies (the batched default and its one-pass-per-launch twin) take the window's flows from the shared helper"""
    from text2video_amd import train as T
    t2v_env("T2V_D_BATCHED", batched)
    fs = _frames(3)
    real = torch.stack(fs[1:]).contiguous()
    real_prev = torch.stack(fs[:3]).contiguous()
    pose = _pose(3)
    base = ["--max_frames_per_gpu", "3", "--n_scales_temporal", "1"]

    def step(args):
        tr = T.Vid2VidTrainer(_opt(*(base + args)), DEV, seed=7)
        return tr.train_step(pose, real, None, None, real_prev=real_prev)[0]
    lk, zero, today = step(["--flow_ref", "lk"]), step(["--flow_ref", "zero"]), step([])
    assert zero == today, (zero, today)
    for k in ("D_T0", "G_T_GAN0"):
        assert np.isfinite(lk[k]), (k, lk[k])
        assert lk[k] != zero[k], (k, lk[k])       # the discriminator saw the flows
