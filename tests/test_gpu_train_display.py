"""train.py --display_web on the GPU: ops.train_visuals (t2v_train_visuals_u8) against the numpy definition of
tests/visuals_reference.py -- IMAGE and UNIT bytes equal, FLOW bytes equal wherever the value before rounding is not within
1e-6 of a rounding boundary and within 1 there --, its refusals, and the train loop: the files a displayed run writes, the
bytes it shows against the reference on the trainer's own tensors, and that a displayed run trains bit-identically to one
without the display."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visuals_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 7      # (chosen on the CPU: tests/test_cpu_train_display.py holds the fragile-byte cap on it)


def _device_panels(panels):
    return [(kind, torch.from_numpy(x).cuda().contiguous(), c0) for kind, x, c0 in panels]


def _check(panels, scale, got):
    want, frag = R.render(panels, scale)
    flow_rows = [i for i, p in enumerate(panels) if p[0] == R.FLOW]
    other = [i for i, p in enumerate(panels) if p[0] != R.FLOW]
    # (a condition on the inputs, stated on the reference alone)
    share = frag[flow_rows].mean() if flow_rows else 0.0
    print("fragile share of the FLOW bytes: %.3g" % share)
    assert share <= 1e-3
    assert got.shape == want.shape and got.dtype == np.uint8
    assert not frag[other].any()
    for i in other:
        assert np.array_equal(got[i], want[i]), "panel %d (kind %d)" % (i, panels[i][0])
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("FLOW bytes that differ: %d of %d, all fragile: %s" % ((diff[flow_rows] != 0).sum(), diff[flow_rows].size,
                                                                 bool(frag[diff != 0].all())))
    assert not diff[~frag].any(), "bytes differ at %s" % np.argwhere((diff != 0) & ~frag)[:8].tolist()
    assert diff.max() <= 1


# 24x40 and the ragged 17x23: the shapes the definition was written for; 72x60 at scale 2: five min/max slices per panel
@pytest.mark.parametrize("shape,scale", [((24, 40), 1), ((24, 40), 2), ((24, 40), 4), ((17, 23), 1), ((72, 60), 2)],
                         ids=["24x40", "24x40_s2", "24x40_s4", "17x23", "72x60_s2"])
def test_eight_panels_against_the_reference(lib_built, shape, scale):
    from text2video_amd import ops
    panels = R.make_panels(shape[0], shape[1], SEED)
    assert [p[0] for p in panels] == [R.IMAGE, R.IMAGE, R.UNIT, R.UNIT, R.FLOW, R.FLOW, R.FLOW, R.FLOW]
    small = np.hypot(panels[4][1][..., 0], panels[4][1][..., 1]).max()
    large = np.hypot(panels[5][1][..., 0], panels[5][1][..., 1]).max()
    assert small <= 0.5 < 20.0 <= large <= 40.0               # two ranges: a lo / hi shared between panels would show
    assert np.abs(panels[0][1]).max() > 1.0 and panels[2][1].min() < 0.0 and panels[3][1].max() > 1.0
    assert all(np.isfinite(p[1]).all() for p in panels[:4]) and not np.isfinite(panels[7][1][..., :2]).all()
    got = ops.train_visuals(_device_panels(panels), scale)
    assert tuple(got.shape) == (8, shape[0] // scale, shape[1] // scale, 3)
    got = got.cpu().numpy()
    _check(panels, scale, got)
    assert not got[6].any()                                     # the constant panel: black
    if scale == 1:
        assert got[4].max() == 255 and got[5].max() == 255      # each normalised to its own range


def test_image_panel_is_tensor2im(lib_built):
    from text2video_amd import ops
    g = torch.Generator().manual_seed(SEED)
    for shape in ((24, 40, 4), (17, 23, 3)):
        x = (torch.randn(shape, generator=g) * 0.8).cuda()
        got = ops.train_visuals([(ops.VISUALS_IMAGE, x, 0)])
        assert torch.equal(got[0], ops.tensor2im_u8(x)[..., :3].contiguous())


def test_two_calls_give_the_same_bytes(lib_built):
    from text2video_amd import ops
    dev = _device_panels(R.make_panels(24, 40, SEED))
    first = ops.train_visuals(dev, 2).clone()
    assert torch.equal(first, ops.train_visuals(dev, 2))
    scratch = torch.full((ops.train_visuals_scratch_doubles(24, 40, 8),), float("nan"), dtype=torch.float64, device="cuda")
    assert torch.equal(first, ops.train_visuals(dev, 2, scratch=scratch))      # (a scratch of any content, of the exact size)


def test_refusals_launch_nothing(lib_built):
    from text2video_amd import ops
    dev = _device_panels(R.make_panels(24, 40, SEED))
    out = torch.full((9, 24, 40, 3), 0xA5, dtype=torch.uint8, device="cuda")

    def refused(panels, **kw):
        with pytest.raises((RuntimeError, ValueError)):
            ops.train_visuals(panels, out=out, **kw)
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all())

    refused(dev, scale=3)
    odd = [(k, t[:23].contiguous(), c0) for k, t, c0 in dev]
    refused(odd, scale=2)                                        # H = 23 is no multiple of the scale
    refused(dev + dev[:1])                                       # 9 panels
    refused([])
    refused([(ops.VISUALS_IMAGE, dev[1][1], 2)])                 # channels [2, 5) of 4
    refused([(ops.VISUALS_FLOW, dev[3][1], 0)])                  # channels [0, 2) of 1
    refused([(ops.VISUALS_UNIT, dev[1][1], 4)])
    need = ops.train_visuals_scratch_doubles(24, 40, 8)
    refused(dev, scratch=torch.zeros(need - 1, dtype=torch.float64, device="cuda"))
    refused([(ops.VISUALS_IMAGE, dev[1][1].double(), 0)])        # not fp32
    refused(dev[:1] + [(ops.VISUALS_IMAGE, dev[1][1][:, :39].contiguous(), 0)])      # another W
    assert bool((ops.train_visuals(dev, out=out)[:8] != 0xA5).any())      # and the same `out` is written by a good call


# ---- the train loop -------------------------------------------------------------------------------------------------

def _train(ckpt, extra):
    """3 steps of the tiny synthetic recipe with the flow branch -> (losses of every step, {file: {tensor name: tensor}}
    of the saved nets, watch = {"trainer", "display"})"""
    from text2video_amd import train as T
    from text2video_amd.options import TrainOptions
    opt = TrainOptions().parse(["--name", "disp", "--checkpoints_dir", str(ckpt), "--synthetic_data", "--ngf", "16",
                                "--n_blocks", "2", "--n_downsample_G", "2", "--fineSize", "64", "--max_frames_per_gpu", "2",
                                "--no_vgg", "--display_freq", "1"] + extra)
    steps, inner, mp = [], T.Vid2VidTrainer.train_step, pytest.MonkeyPatch()

    def recording(self, *a, **k):
        losses, prev = inner(self, *a, **k)
        steps.append({name: float(v) for name, v in losses.items()})
        return losses, prev

    watch = {}
    try:
        mp.setattr(T.Vid2VidTrainer, "train_step", recording)
        torch.manual_seed(0)
        stats = T.run_train(opt, steps=3, watch=watch)
    finally:
        mp.undo()
    assert stats["steps"] == 3 and len(steps) == 3 and all("F_Flow" in s for s in steps)
    d = os.path.join(str(ckpt), "disp")
    nets = {f: torch.load(os.path.join(d, f), map_location="cpu") for f in sorted(os.listdir(d)) if f.endswith(".pth")}
    return steps, nets, watch


@pytest.fixture(scope="module")
def plain_run(lib_built, tmp_path_factory):
    ckpt = tmp_path_factory.mktemp("plain")
    return (ckpt,) + _train(ckpt, [])


@pytest.fixture(scope="module")
def shown_run(lib_built, tmp_path_factory):
    ckpt = tmp_path_factory.mktemp("shown")
    return (ckpt,) + _train(ckpt, ["--display_web"])


def _check_files(ckpt, watch, labels, side):
    web = os.path.join(str(ckpt), "disp", "web")
    want = ["epoch%03d_iter%07d_%s.jpg" % (e, e, l) for e in (3, 2, 1) for l in labels]      # (synthetic: one sample an epoch)
    assert sorted(os.listdir(os.path.join(web, "images"))) == sorted(want)
    for f in want:
        im = Image.open(os.path.join(web, "images", f))
        assert im.size == (side, side) and im.mode == "RGB"
    page = open(os.path.join(web, "index.html")).read()
    assert re.findall(r'<img src="images/([^"]+)"', page) == want
    log = open(os.path.join(str(ckpt), "disp", "loss_log.txt")).read().splitlines()
    assert log[0].startswith("================ Training Loss (")
    assert [l.split(",")[0] for l in log[1:]] == ["(iter 0", "(iter 1", "(iter 2"] and all("F_Flow: " in l for l in log[1:])
    # what the last display showed = the reference on the tensors the trainer still holds
    from text2video_amd.train_display import panels_of
    disp, vis = watch["display"], watch["trainer"].visuals
    named = panels_of(vis)
    assert [n[0] for n in named] == list(labels) == list(disp.last_panels)
    assert tuple(vis["pose"].shape) == (64, 64, 12) and tuple(vis["fw"].shape) == (64, 64, 4)
    assert tuple(vis["conf_ref"].shape) == (64, 64)
    panels = [(kind, t.detach().cpu().numpy(), c0) for _, kind, t, c0 in named]
    _check(panels, disp.scale, np.stack([disp.last_panels[l] for l in labels]))
    return named


def test_displayed_run_writes_pictures_page_and_log(shown_run):
    from text2video_amd.train_display import LABELS
    ckpt, _, _, watch = shown_run
    _check_files(ckpt, watch, LABELS, 64)
    assert watch["trainer"].keep_visuals is True


def test_displayed_run_at_half_size_with_an_estimated_reference_flow(lib_built, tmp_path):
    from text2video_amd.train_display import LABELS
    _, _, watch = _train(tmp_path, ["--display_web", "--display_scale", "2", "--flow_ref", "lk"])
    named = _check_files(tmp_path, watch, LABELS, 32)
    assert bool(named[6][2][..., :2].any())                     # (the Lucas-Kanade reference is not the zero flow)


def test_display_does_not_perturb_training(plain_run, shown_run):
    plain_ckpt, want_steps, want_nets, watch = plain_run
    _, got_steps, got_nets, _ = shown_run
    assert watch["display"] is None and watch["trainer"].keep_visuals is False and watch["trainer"].visuals is None
    assert sorted(f for f in os.listdir(os.path.join(str(plain_ckpt), "disp")) if not f.endswith(".pth")) == ["iter.txt"]
    assert got_steps == want_steps, [(g, w) for g, w in zip(got_steps, want_steps) if g != w]
    assert list(got_nets) == list(want_nets) and any("net_G" in f for f in want_nets) and any("net_D" in f for f in want_nets)
    for f in want_nets:
        assert got_nets[f].keys() == want_nets[f].keys()
        for k in want_nets[f]:
            assert torch.equal(got_nets[f][k], want_nets[f][k]), (f, k)
