"""The definition of the dense Lucas-Kanade estimator (tests/flow_reference.py, the float64 restatement of
t2v_optical_flow) on analytic image pairs whose true flow is exact.  These bounds test the algorithm, not the kernel:
tests/test_gpu_optical_flow.py holds the HIP kernels to this restatement pixel by pixel."""
import pytest
import torch

import flow_reference as fr


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_estimate_recovers_the_known_motion(name):
    c = fr.case(name)
    epe, ratio = fr.functional_figures(c, c["u64"], c["v64"])
    print("case %s: mean endpoint error %.4f px, residual ratio %.4f" % (name, epe, ratio))
    assert epe <= fr.MAX_EPE, (name, epe)
    assert ratio <= fr.MAX_RESIDUAL_RATIO, (name, ratio)


def test_constant_images_give_exactly_zero_flow():
    img = torch.full((40, 56), 0.375, dtype=torch.float64)
    for dtype in (torch.float64, torch.float32):
        u, v = fr.lk_flow(img, img.clone(), dtype=dtype)
        assert torch.isfinite(u).all() and torch.isfinite(v).all()
        assert (u == 0).all() and (v == 0).all()


def test_default_level_rule():
    assert fr.default_levels(512, 512) == 6
    assert fr.default_levels(64, 96) == 3
    assert fr.default_levels(48, 40) == 2
    assert fr.default_levels(85, 64) == 3          # 85 -> 43 -> 22 (the next would be 11 x 8)
    assert fr.default_levels(8, 8) == 1
    assert fr.default_levels(1024, 1024) == 6      # capped


def test_true_flow_warps_prev_onto_cur():
    """the sign convention: cur(x) = prev(x + flow).  With the exact flow only the bilinear interpolation error is left (a
    fraction of the frame difference); with the flow negated the warp moves the image the wrong way and the residual grows
    past the unwarped difference."""
    c = fr.case("B")

    def residual(sign):
        return (fr.warp(c["prev"], sign * c["u_true"], sign * c["v_true"]) - c["cur"]).abs()[8:-8, 8:-8].mean().item()
    base = (c["prev"] - c["cur"]).abs()[8:-8, 8:-8].mean().item()
    assert residual(1.0) <= 0.25 * base, (residual(1.0), base)
    assert residual(-1.0) > base, (residual(-1.0), base)
