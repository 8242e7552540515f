"""t2v_image_metrics_u8 / ops.image_metrics against the float64 reference of tests/metrics_reference.py, and
`test.py --metrics` / `python -m text2video_amd.evaluate` end to end.

Bounds: sse, sad and ssim_n are integers and must be equal.  The SSIM mean must be within 1e-10 of the reference: two
float64 evaluations of the definition in different orders differ by 3.7e-14 at most (measured on the CPU, direct 2-D window
against separable), a float32 window sum by 8e-6 on the `smooth` inputs -- so the bound also proves the arithmetic."""
import functools
import glob
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SSIM_TOL = 1e-10
SENTINEL = -12345.5


@functools.lru_cache(maxsize=None)
def _case(kind, H, W):
    a, b = R.make_pair(kind, H, W)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, tuple(R.reference_row(a, b))


def _dev(img, cs=3):
    return torch.from_numpy(R.with_stride(img, cs)).cuda()


def _check_row(got, want, what):
    print("%s: got %r want %r" % (what, list(got), list(want)))
    assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3], what
    if want[3]:
        assert abs(got[2] / got[3] - want[2] / want[3]) <= SSIM_TOL, (what, got[2] / got[3] - want[2] / want[3])
    else:
        assert got[2] == 0.0, what


@pytest.mark.parametrize("kind", ["noise", "smooth", "same"])
@pytest.mark.parametrize("shape", [(11, 11), (12, 27), (43, 70), (64, 64), (75, 133)])
def test_whole_frame_against_reference(lib_built, shape, kind):
    from text2video_amd import ops
    a, b, want = _case(kind, *shape)
    rows = []
    for a_cs in (3, 4):
        for b_cs in (3, 4):
            got = ops.image_metrics(_dev(a, a_cs), _dev(b, b_cs)).cpu().numpy()
            assert got.shape == (1, 4)
            _check_row(got[0], want, "%s %dx%d strides %d/%d" % ((kind,) + shape + (a_cs, b_cs)))
            rows.append(got.tobytes())
    assert len(set(rows)) == 1          # the pad channel is never read into a sum
    if kind == "same":
        assert got[0][0] == 0 and got[0][2] == got[0][3]     # every window's index is exactly 1


BOXES = [(7, 40, 13, 60),        # interior, odd offsets
         (0, 31, 100, 133),      # touches the top and the right edge
         (33, 44, 65, 76),       # 11 x 11: one window position
         (50, 60, 3, 43)]        # 10 x 40: narrower than the window


def test_boxes_equal_the_cropped_pair(lib_built):
    from text2video_amd import ops
    for kind in ("noise", "smooth"):
        a, b, want0 = _case(kind, 75, 133)
        da, db = _dev(a, 4), _dev(b, 3)
        alone = ops.image_metrics(da, db).cpu().numpy()
        for boxes in (BOXES[:3], BOXES[3:], BOXES[1:]):
            got = ops.image_metrics(da, db, boxes).cpu().numpy()
            assert got.shape == (1 + len(boxes), 4)
            assert got[0].tobytes() == alone[0].tobytes()       # row 0: same bits with and without boxes
            _check_row(got[0], want0, kind + " frame")
            for r, box in enumerate(boxes, 1):
                _check_row(got[r], R.reference_row(a, b, box), "%s box %r" % (kind, box))
        eleven = ops.image_metrics(da, db, [BOXES[2]]).cpu().numpy()[1]
        narrow = ops.image_metrics(da, db, [BOXES[3]]).cpu().numpy()[1]
        assert eleven[3] == 3 and narrow[3] == 0 and narrow[2] == 0 and narrow[0] == R.integer_sums(a[50:60, 3:43], b[50:60, 3:43])[0]


def test_two_calls_same_bits_and_rows_past_the_last_keep_their_values(lib_built):
    from text2video_amd import ops
    a, b, _ = _case("smooth", 75, 133)
    da, db = _dev(a, 4), _dev(b, 3)
    outs = []
    for _ in range(2):
        out = torch.full((6, 4), SENTINEL, dtype=torch.float64, device="cuda")
        assert ops.image_metrics(da, db, BOXES[:2], out=out, out_row=1) is out
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    assert (outs[0][0] == SENTINEL).all() and (outs[0][4:] == SENTINEL).all() and (outs[0][1:4] != SENTINEL).all()
    assert outs[0][1:4].tobytes() == ops.image_metrics(da, db, BOXES[:2]).cpu().numpy().tobytes()
    # a scratch of exactly the stated size, holding anything, gives the same bits
    need = ops.image_metrics_scratch_doubles(75, 133, 2)
    scratch = torch.full((need,), float("nan"), dtype=torch.float64, device="cuda")
    assert ops.image_metrics(da, db, BOXES[:2], scratch=scratch).cpu().numpy().tobytes() == outs[0][1:4].tobytes()


def test_refusals_raise_and_leave_out_untouched(lib_built):
    from text2video_amd import ops
    a, b, _ = _case("noise", 43, 70)
    da, db = _dev(a), _dev(b)
    out = torch.full((4, 4), SENTINEL, dtype=torch.float64, device="cuda")

    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8, device="cuda")
    bad = [
        dict(a=u8(43, 70, 2), b=db),                              # channel stride outside {3, 4}
        dict(a=da, b=u8(43, 70, 5)),
        dict(a=u8(1, 8193, 3), b=u8(1, 8193, 3)),                  # W > 8192
        dict(a=u8(8193, 1, 3), b=u8(8193, 1, 3)),                  # H > 8192
        dict(a=u8(0, 70, 3), b=u8(0, 70, 3)),                      # H < 1
        dict(a=u8(43, 0, 3), b=u8(43, 0, 3)),                      # W < 1
        dict(a=da, b=db, boxes=[(0, 11, 0, 11)] * 4),              # nbox > 3
        dict(a=da, b=db, boxes=[(5, 5, 0, 11)]),                   # empty box
        dict(a=da, b=db, boxes=[(0, 11, 20, 10)]),
        dict(a=da, b=db, boxes=[(0, 44, 0, 11)]),                  # outside the frame
        dict(a=da, b=db, boxes=[(0, 11, -1, 11)]),
        dict(a=da, b=db, boxes=[(0, 11, 60, 71)]),
        dict(a=da, b=db, scratch=torch.zeros(ops.image_metrics_scratch_doubles(43, 70, 0) - 1, dtype=torch.float64, device="cuda")),
        dict(a=da, b=db, boxes=[(0, 11, 0, 11)],                   # (large enough for no box, too small for one)
             scratch=torch.zeros(ops.image_metrics_scratch_doubles(43, 70, 0), dtype=torch.float64, device="cuda")),
    ]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises((RuntimeError, ValueError)):
            ops.image_metrics(kw.pop("a"), kw.pop("b"), kw.pop("boxes", ()), out=out, **kw)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert ops.image_metrics(da, db, out=out) is out and (out.cpu().numpy()[0] != SENTINEL).all()      # and a good call works


def test_512x512_pair_with_a_128_box(lib_built):
    from text2video_amd import ops
    for kind in ("noise", "smooth"):
        a, b, want = _case(kind, 512, 512)
        box = (190, 318, 201, 329)
        got = ops.image_metrics(_dev(a, 4), _dev(b, 3), [box]).cpu().numpy()
        _check_row(got[0], want, kind + " 512x512")
        _check_row(got[1], R.reference_row(a, b, box), kind + " 512x512 box")
        assert got[0][3] == 3 * 502 * 502 and got[1][3] == 3 * 118 * 118


# ------------------------------------------------------------------------------------------------
# test.py --metrics and evaluate, end to end
# ------------------------------------------------------------------------------------------------
ARGS = ["--name", "fadg0", "--dataroot", "datasets/fadg0", "--dataset_mode", "pose", "--input_nc", "3", "--resize_or_crop",
        "scaleHeight", "--loadSize", "512", "--openpose_only", "--how_many", "1200", "--no_first_img", "--random_drop_prob", "0",
        "--synthetic_weights", "1", "--ngf", "32", "--n_blocks", "3"]


def _make_dataset(tmp):
    """the pose JSONs of the reference's L2 driver + seeded noise JPEGs of 512x384 standing in for the real frames"""
    root = os.path.join(tmp, "vid2vid", "datasets", "fadg0")
    rng = np.random.default_rng(11)
    for seq, pat in (("tmp", "%04d.jpg"), ("tmp_smooth", "smooth_%04d.jpg")):
        src = os.path.join(GOLD, "dataset_fadg0_l2", "test_openpose", seq)
        os.makedirs(os.path.join(root, "test_openpose", seq))
        os.makedirs(os.path.join(root, "test_img", seq))
        for i, f in enumerate(sorted(os.listdir(src))):
            shutil.copyfile(os.path.join(src, f), os.path.join(root, "test_openpose", seq, f))
            Image.fromarray(rng.integers(0, 256, (384, 512, 3), dtype=np.uint8)).save(os.path.join(root, "test_img", seq, pat % i))
    return os.path.join(tmp, "vid2vid")


def _real(path):
    """the test's own resize and crop of a real frame: BICUBIC to 680x512, the central 320 columns"""
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB").resize((680, 512), Image.BICUBIC).crop((180, 0, 500, 512)))


def test_run_test_metrics_json_equals_the_reference(lib_built, tmp_path, monkeypatch):
    from text2video_amd import model, ops
    from text2video_amd.keypoints import get_face_region
    from text2video_amd.options import TestOptions
    from text2video_amd.pose_dataset import PoseDataset
    from text2video_amd.visualizer import Visualizer
    work = _make_dataset(str(tmp_path))
    monkeypatch.chdir(work)
    captured = {}
    save = Visualizer.save_images

    def capture(self, visuals, a_path):
        captured[a_path] = visuals["fake_B"].copy()
        return save(self, visuals, a_path)
    monkeypatch.setattr(Visualizer, "save_images", capture)
    opt = TestOptions().parse(ARGS + ["--metrics", "--timing_json", "timing.json"])
    stats = model.run_test(opt)
    assert stats["frames"] == 8 and len(captured) == 8
    ds = PoseDataset(opt)
    timing = json.load(open("timing.json"))
    for seq in ("tmp", "tmp_smooth"):
        doc = json.load(open(os.path.join(stats["results_dir"], seq, "metrics.json")))
        assert timing["metrics"][seq] == doc["summary"] and isinstance(doc["definition"], str)
        paths = sorted(p for p in captured if os.path.basename(os.path.dirname(p)) == seq)
        assert [f["name"] for f in doc["frames"]] == [os.path.basename(p) for p in paths] and len(paths) == 4
        sse = n = 0.0
        ssims, maes, f_ssims, f_sse, f_n = [], [], [], 0.0, 0.0
        for p, got in zip(paths, doc["frames"]):
            fake, real = captured[p], _real(p)
            assert fake.shape == real.shape == (512, 320, 3)
            want = ops.metrics_summary(R.reference_row(fake, real), fake.size)
            print(p, got, want)
            assert got["psnr"] == want["psnr"] and got["mae"] == want["mae"]          # from the exact integer sums
            assert abs(got["ssim"] - want["ssim"]) <= SSIM_TOL
            sse, n = sse + want["mse"] * fake.size, n + fake.size
            ssims.append(want["ssim"])
            maes.append(want["mae"])
            i = ds.img[seq].index(p)
            box = get_face_region(ds._pose_map(seq, i), 512)
            assert box is not None and got["face"]["box"] == list(box) and box[1] - box[0] == box[3] - box[2] == 128
            fwant = ops.metrics_summary(R.reference_row(fake, real, box), 3 * 128 * 128)
            assert got["face"]["psnr"] == fwant["psnr"] and got["face"]["mae"] == fwant["mae"]
            assert abs(got["face"]["ssim"] - fwant["ssim"]) <= SSIM_TOL
            f_ssims.append(fwant["ssim"])
            f_sse, f_n = f_sse + fwant["mse"] * 3 * 128 * 128, f_n + 3 * 128 * 128
        s = doc["summary"]
        assert s["frames"] == 4 and s["face"]["frames"] == 4
        assert abs(s["psnr"] - 10 * math.log10(65025.0 * n / sse)) <= 1e-9
        assert abs(s["ssim"] - sum(ssims) / 4) <= SSIM_TOL and abs(s["mae"] - sum(maes) / 4) <= 1e-12
        assert abs(s["face"]["psnr"] - 10 * math.log10(65025.0 * f_n / f_sse)) <= 1e-9
        assert abs(s["face"]["ssim"] - sum(f_ssims) / 4) <= SSIM_TOL


def test_metrics_start_up_errors(lib_built, tmp_path, monkeypatch):
    from text2video_amd import model
    from text2video_amd.options import TestOptions
    work = _make_dataset(str(tmp_path))
    monkeypatch.chdir(work)
    shutil.rmtree(os.path.join("datasets", "fadg0", "test_img", "tmp_smooth"))
    with pytest.raises(ValueError, match="no real frames for sequence.*tmp_smooth"):
        model.run_test(TestOptions().parse(ARGS + ["--metrics"]))


def test_command_lean_and_torch_write_the_same_metrics_and_the_same_jpegs(lib_built, tmp_path):
    work = _make_dataset(str(tmp_path))
    res = os.path.join(work, "results", "fadg0", "test_latest")
    cmd = [sys.executable, os.path.join(ROOT, "vid2vid", "test.py")] + ARGS + ["--timing_json", "timing.json"]

    def run(lean, metrics):
        shutil.rmtree(os.path.join(work, "results"), ignore_errors=True)
        env = dict(os.environ, CUDA_VISIBLE_DEVICES="0", T2V_LEAN="1" if lean else "0")
        r = subprocess.run(cmd + (["--metrics"] if metrics else []), cwd=work, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        timing = json.load(open(os.path.join(work, "timing.json")))
        assert timing["cold_start"]["torch_imported"] is (not lean) and ("metrics" in timing) is metrics
        return ({os.path.relpath(f, res): open(f, "rb").read() for f in sorted(glob.glob(os.path.join(res, "*", "*.jpg")))},
                {os.path.relpath(f, res): open(f, "rb").read() for f in sorted(glob.glob(os.path.join(res, "*", "metrics.json")))})

    jpg_torch, met_torch = run(False, True)
    jpg_plain, met_plain = run(True, False)
    jpg_lean, met_lean = run(True, True)
    assert sorted(met_lean) == ["tmp/metrics.json", "tmp_smooth/metrics.json"] and met_lean == met_torch
    assert met_plain == {} and len(jpg_plain) == 16 and jpg_plain == jpg_lean == jpg_torch
    doc = json.loads(met_lean["tmp/metrics.json"])
    assert doc["summary"]["frames"] == 4 and doc["summary"]["face"]["frames"] == 4 and doc["summary"]["psnr"] is not None

    # evaluate on the tree against itself (lean tree still on disk): identical pictures
    from text2video_amd import evaluate
    out = os.path.join(work, "eval.json")
    assert evaluate.main([res, res, "--json", out]) == 0
    rep = json.load(open(out))
    assert rep["overall"] == {"frames": 8, "psnr": None, "ssim": 1.0, "mae": 0.0}
    assert sorted(rep["sequences"]) == ["tmp", "tmp_smooth"] and rep["sequences"]["tmp"]["frames"] == 4
    # an unpaired file and a size mismatch are listed and fail the command
    other = os.path.join(work, "other")
    shutil.copytree(res, other)
    os.remove(os.path.join(other, "tmp", "fake_B_0002.jpg"))
    Image.new("RGB", (64, 48)).save(os.path.join(other, "tmp", "fake_B_0003.jpg"))
    assert evaluate.main([res, other, "--json", out]) == 1
    rep = json.load(open(out))
    assert rep["unpaired_a"] == ["tmp/fake_B_0002.jpg"] and rep["unpaired_b"] == []
    assert [m["file"] for m in rep["size_mismatch"]] == ["tmp/fake_B_0003.jpg"] and rep["overall"]["frames"] == 6
