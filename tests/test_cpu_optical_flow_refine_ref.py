"""The definition of the refined estimator (tests/flow_refine_reference.py, the float64 restatement of
t2v_optical_flow_refined: Lucas-Kanade plus Horn-Schunck Jacobi steps at every level) on pairs whose true flow is exact, and
the command-line refusals of the flags that select it.  These bounds test the algorithm, not the kernel:
tests/test_gpu_optical_flow_refine.py holds the HIP kernels to this restatement pixel by pixel."""
import pytest
import torch

import flow_reference as fr
import flow_refine_reference as rr

TRAIN_ARGS = ["--name", "t", "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only"]


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_no_refinement_steps_is_the_lk_estimate_exactly(name):
    c = fr.case(name)
    u, v = rr.lkhs_flow(c["cur"], c["prev"], refine_iters=0, **c["kw"])
    assert torch.equal(u, c["u64"]) and torch.equal(v, c["v64"])


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_refinement_does_not_hurt_the_textured_cases(name):
    c = fr.case(name)
    lk = fr.functional_figures(c, c["u64"], c["v64"])
    hs = fr.functional_figures(c, *rr.flows64(name))
    print("case %s: mean EPE lk %.4f -> refined %.4f px, residual ratio %.4f -> %.4f" % (name, lk[0], hs[0], lk[1], hs[1]))
    assert hs[0] <= lk[0], (name, lk, hs)
    for epe, ratio in (lk, hs):
        assert epe <= fr.MAX_EPE and ratio <= fr.MAX_RESIDUAL_RATIO, (name, lk, hs)


@pytest.mark.parametrize("name", sorted(rr.DISC_CASES))
def test_refinement_fills_the_textureless_disc(name):
    c = rr.pair(name)
    lk, hs = rr.inner_epe(c, *rr.flows64(name, 0)), rr.inner_epe(c, *rr.flows64(name))
    print("case %s: inner mean EPE lk %.4f -> refined %.4f px (ratio %.3f)" % (name, lk, hs, hs / lk))
    assert hs <= rr.MAX_INNER_RATIO * lk, (name, lk, hs)


def test_constant_images_give_exactly_zero_flow():
    img = torch.full((40, 56), 0.375, dtype=torch.float64)
    for dtype in (torch.float64, torch.float32):
        u, v = rr.lkhs_flow(img, img.clone(), dtype=dtype)
        assert (u == 0).all() and (v == 0).all()


def _refused(cls, args, capsys):
    with pytest.raises(SystemExit):
        cls().parse(args)
    return capsys.readouterr().err


def test_train_options_refuse_the_refinement_flags_without_lkhs(capsys):
    from text2video_amd.options import TrainOptions
    opt = TrainOptions().parse(TRAIN_ARGS)
    assert (opt.flow_ref, opt.flow_refine_iters, opt.flow_alpha) == ("zero", 64, 0.2)
    opt = TrainOptions().parse(TRAIN_ARGS + ["--flow_ref", "lkhs"])
    assert (opt.flow_ref, opt.flow_refine_iters, opt.flow_alpha) == ("lkhs", 64, 0.2)
    opt = TrainOptions().parse(TRAIN_ARGS + ["--flow_ref", "lkhs", "--flow_refine_iters", "16", "--flow_alpha", "0.5"])
    assert (opt.flow_refine_iters, opt.flow_alpha) == (16, 0.5)
    for ref in ([], ["--flow_ref", "zero"], ["--flow_ref", "lk"]):
        err = _refused(TrainOptions, TRAIN_ARGS + ref + ["--flow_refine_iters", "64"], capsys)
        assert "--flow_refine_iters 64" in err and "--flow_ref lkhs, which is not given" in err
        err = _refused(TrainOptions, TRAIN_ARGS + ref + ["--flow_alpha", "0.2"], capsys)
        assert "--flow_alpha 0.2" in err and "--flow_ref lkhs, which is not given" in err
    for bad in (["--flow_refine_iters", "0"], ["--flow_refine_iters", "1025"], ["--flow_alpha", "0"], ["--flow_alpha", "-1"],
                ["--flow_alpha", "inf"], ["--flow_alpha", "nan"]):
        assert "is not" in _refused(TrainOptions, TRAIN_ARGS + ["--flow_ref", "lkhs"] + bad, capsys)


def test_test_options_refuse_temporal_flow_without_metrics_temporal(capsys):
    from text2video_amd.options import TestOptions
    assert TestOptions().parse(TRAIN_ARGS + ["--metrics_temporal"]).temporal_flow == "lk"
    assert TestOptions().parse(TRAIN_ARGS).temporal_flow == "lk"
    assert TestOptions().parse(TRAIN_ARGS + ["--metrics_temporal", "--temporal_flow", "lkhs"]).temporal_flow == "lkhs"
    for extra in ([], ["--metrics"]):
        err = _refused(TestOptions, TRAIN_ARGS + extra + ["--temporal_flow", "lkhs"], capsys)
        assert "--temporal_flow lkhs" in err and "--metrics_temporal, which is not given" in err


def test_evaluate_refuses_temporal_flow_without_temporal(tmp_path, capsys):
    from text2video_amd import evaluate
    with pytest.raises(SystemExit):
        evaluate.main([str(tmp_path), str(tmp_path), "--temporal_flow", "lkhs"])
    assert "--temporal, which is not given" in capsys.readouterr().err
