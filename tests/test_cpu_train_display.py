"""CPU side of train.py --display_web: the library exports and binds the training-visuals entry points, the options parse,
the numpy definition the kernel is held to (tests/visuals_reference.py) gives the colours it states, and TrainDisplay's
page and log writers lay the files out as documented.  The kernel and the train loop: tests/test_gpu_train_display.py."""
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visuals_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_binding(lib_built):
    from text2video_amd import _lib, ops
    assert lib_built.t2v_abi_version() == 22 == _lib.ABI_VERSION
    for name in ("t2v_train_visuals_scratch_doubles", "t2v_train_visuals_u8"):
        assert name in _lib.SIGNATURES and getattr(lib_built, name).argtypes == _lib.SIGNATURES[name][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T t2v_train_visuals_u8" in out and " T t2v_train_visuals_scratch_doubles" in out
    assert (ops.VISUALS_IMAGE, ops.VISUALS_UNIT, ops.VISUALS_FLOW) == (R.IMAGE, R.UNIT, R.FLOW) == (0, 1, 2)
    # a (lo, hi) pair per panel and slice of 1024 pixels, at most 64 slices; 0 for a shape the call refuses
    f = lib_built.t2v_train_visuals_scratch_doubles
    assert f(24, 40, 8) == 8 * 2 and f(64, 64, 3) == 3 * 4 * 2 and f(512, 512, 8) == 8 * 64 * 2 and f(1, 1, 1) == 2
    assert f(0, 5, 1) == 0 and f(5, 8193, 1) == 0 and f(5, 5, 0) == 0 and f(5, 5, 9) == 0


def test_header_keeps_the_abi_and_marks_the_entries_additive():
    header = open(os.path.join(ROOT, "include", "t2v.h")).read()
    assert "#define T2V_ABI_VERSION 22" in header
    i = header.index("t2v_train_visuals_u8(")
    block = header[header.rindex("/* ----", 0, i):i]
    assert "Training visuals (additive to ABI 22)" in block
    assert "size_t t2v_train_visuals_scratch_doubles(int H, int W, int npanels);" in header
    assert "enum { T2V_VISUALS_IMAGE = 0, T2V_VISUALS_UNIT = 1, T2V_VISUALS_FLOW = 2 };" in header
    makefile = open(os.path.join(ROOT, "text2video_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\btrain_visuals\.hip\b", makefile, re.M)


def test_display_web_is_off_by_default():
    from text2video_amd.options import TrainOptions
    opt = TrainOptions().parse([])
    assert opt.display_web is False and opt.display_scale == 1 and opt.display_freq == 100


def test_display_options_parse():
    from text2video_amd.options import TrainOptions
    opt = TrainOptions().parse(["--display_web", "--display_scale", "4", "--display_freq", "7"])
    assert opt.display_web is True and opt.display_scale == 4 and opt.display_freq == 7


def _flow(pixels):
    x = np.zeros((1, len(pixels), 2), np.float32)
    x[0, :, :] = pixels
    return x


def test_reference_flow_colours():
    b, fr = R.flow_bytes(_flow([(1.0, 0.0), (0.0, 0.0)]))
    assert b[0, 0].tolist() == [255, 0, 0] and b[0, 1].tolist() == [0, 0, 0]            # +x beside a zero pixel: pure red
    b, _ = R.flow_bytes(_flow([(0.0, 1.0), (0.0, 0.0)]))
    assert b[0, 0].tolist() == [128, 255, 0]                                             # +y: hue 90 degrees
    b, _ = R.flow_bytes(_flow([(-2.0, 0.0), (0.0, 0.0), (1.0, 0.0)]))
    assert b[0, 0].tolist() == [0, 255, 255] and b[0, 2].tolist() == [128, 0, 0]        # 180 degrees: cyan; half the magnitude
    b, _ = R.flow_bytes(_flow([(0.0, -1.0), (0.0, 0.0)]))
    assert b[0, 0].tolist() == [128, 0, 255]                                             # 270 degrees
    const = np.empty((5, 7, 2), np.float32)
    const[...] = (1.5, -2.25)
    b, fr = R.flow_bytes(const)
    assert not b.any() and not fr.any()                                                  # hi == lo: black


def test_reference_flow_ignores_non_finite_pixels():
    clean = _flow([(3.0, 4.0), (0.0, 1.0), (1.0, 1.0), (0.5, 0.0)])
    holed = clean.copy()
    holed[0, 2] = (np.nan, 1.0)
    b0, _ = R.flow_bytes(clean)
    b1, _ = R.flow_bytes(holed)
    assert b1[0, 2].tolist() == [0, 0, 0]
    assert np.array_equal(b1[0, [0, 1, 3]], b0[0, [0, 1, 3]])      # lo = 0.5, hi = 5 either way
    holed[0, 2] = (1e30, -np.inf)
    assert np.array_equal(R.flow_bytes(holed)[0], b1)
    none = np.full((2, 3, 2), np.nan, np.float32)
    assert not R.flow_bytes(none)[0].any()                          # no finite pixel: black


def test_reference_image_unit_and_downscale():
    x = np.array([[[-1.5, -1.0, 0.0], [0.999, 1.0, 7.0]]], np.float32)
    assert R.image_bytes(x)[0].tolist() == [[[0, 0, 127], [254, 255, 255]]]
    u = np.array([[-0.5, 0.0, 0.5, 0.999, 1.0, 3.0, np.nan]], np.float32)
    assert R.unit_bytes(u)[0][0, :, 0].tolist() == [0, 0, 127, 254, 255, 255, 0]
    assert np.array_equal(R.unit_bytes(u)[0][..., 0], R.unit_bytes(u)[0][..., 2])
    b = np.zeros((2, 4, 3), np.uint8)
    b[:, :2, 0] = [[1, 2], [3, 4]]          # (10 + 2) // 4 = 3
    b[:, 2:, 0] = [[0, 0], [0, 1]]          # (1 + 2) // 4 = 0
    b[:, 2:, 1] = [[0, 0], [1, 1]]          # (2 + 2) // 4 = 1: halves round up
    fr = np.zeros(b.shape, bool)
    fr[1, 3, 2] = True
    d, dfr = R.downscale(b, fr, 2)
    assert d.tolist() == [[[3, 0, 0], [0, 1, 0]]] and dfr.tolist() == [[[False] * 3, [False, False, True]]]
    # the test panels keep the cap on fragile bytes the GPU test states, on every shape it uses
    for (H, W), s in (((24, 40), 1), ((24, 40), 2), ((24, 40), 4), ((17, 23), 1)):
        panels = R.make_panels(H, W, seed=7)
        _, frag = R.render(panels, s)
        flow_rows = [i for i, p in enumerate(panels) if p[0] == R.FLOW]
        assert frag[flow_rows].mean() <= 1e-3


class _Opt:
    def __init__(self, root):
        self.checkpoints_dir, self.name, self.display_scale = str(root), "run", 1


def test_display_writes_pages_and_log(tmp_path):
    from PIL import Image
    from text2video_amd.train_display import LABELS, TrainDisplay
    assert LABELS == ("input_image", "fake_image", "fake_raw_image", "real_image", "flow", "weight", "flow_ref", "conf_ref")
    rng = np.random.default_rng(0)
    disp = TrainDisplay(_Opt(tmp_path))
    shown = [(1, 8, LABELS[:4]), (1, 16, LABELS), (2, 24, LABELS[:6])]
    for k, (epoch, total, labels) in enumerate(shown):
        panels = {label: rng.integers(0, 256, (12, 20, 3)).astype(np.uint8) for label in labels}
        paths = disp.write_panels(panels, epoch, total)
        assert [os.path.basename(p) for p in paths] == ["epoch%03d_iter%07d_%s.jpg" % (epoch, total, l) for l in labels]
        assert all(os.path.dirname(p) == str(tmp_path / "run" / "web" / "images") for p in paths)
        assert all(Image.open(p).size == (20, 12) for p in paths)
        assert list(disp.last_panels) == list(labels) and all(disp.last_panels[l] is panels[l] for l in labels)
        disp.log("(iter %d, epoch %d, 84 ms, all-reduce 0.0 MB) G_GAN: 1.000 D: 0.500" % (k, epoch))
    disp.close()
    page = open(tmp_path / "run" / "web" / "index.html").read()
    assert '<meta http-equiv="refresh"' in page
    want = ["images/epoch%03d_iter%07d_%s.jpg" % (e, t, l) for e, t, labels in reversed(shown) for l in labels]
    assert re.findall(r'<img src="([^"]+)"', page) == want                     # every written file, newest first
    assert sorted(os.listdir(tmp_path / "run" / "web" / "images")) == sorted(os.path.basename(w) for w in want)
    assert all(os.path.exists(tmp_path / "run" / "web" / w) for w in want)      # the page's paths are relative to it
    for label in LABELS:
        assert "<p>%s</p>" % label in page
    assert page.index("epoch [2], iter [24]") < page.index("epoch [1], iter [16]") < page.index("epoch [1], iter [8]")
    log = open(tmp_path / "run" / "loss_log.txt").read().splitlines()
    assert len(log) == 1 + len(shown) and log[0].startswith("================ Training Loss (") and log[0].endswith("================")
    assert [l.split(",")[0] for l in log[1:]] == ["(iter 0", "(iter 1", "(iter 2"]
    # a resumed run appends: a second header, the earlier lines stay
    disp = TrainDisplay(_Opt(tmp_path))
    disp.log("(iter 3, epoch 2) D: 0.250")
    disp.close()
    log = open(tmp_path / "run" / "loss_log.txt").read().splitlines()
    assert len(log) == 6 and log[4].startswith("================ Training Loss (") and log[5] == "(iter 3, epoch 2) D: 0.250"
