"""CPU side of test.py --metrics / ops.image_metrics: the float64 reference stated two ways agrees with itself and with
closed forms, the library exports and binds the entry points, and the host logic (options, summaries, the face box's new
home, evaluate's pairing) does what the documents say.  The kernel itself: tests/test_gpu_image_metrics.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("shape", [(11, 11), (12, 27), (43, 70)])
def test_direct_and_separable_references_agree(kind, shape):
    a, b = R.make_pair(kind, *shape)
    (sd, nd), (ss, ns) = R.ssim_direct(a, b), R.ssim_separable(a, b)
    assert nd == ns == 3 * (shape[0] - 10) * (shape[1] - 10)
    assert abs(sd / nd - ss / ns) <= 1e-12


def test_closed_forms():
    a, _ = R.make_pair("noise", 20, 31)
    row = R.reference_row(a, a, ssim=R.ssim_direct)
    assert row[0] == 0 and row[1] == 0 and abs(row[2] / row[3] - 1.0) <= 1e-12
    zero, full = np.zeros((20, 20, 3), np.uint8), np.full((20, 20, 3), 255, np.uint8)
    for ssim in (R.ssim_direct, R.ssim_separable):
        row = R.reference_row(zero, full, ssim=ssim)
        assert row[0] == 78030000 and row[1] == 20 * 20 * 3 * 255 and row[3] == 300
        assert abs(row[2] / row[3] - R.C1 / (255.0 ** 2 + R.C1)) <= 1e-15
        assert abs(row[2] / row[3] - 9.99900009999e-5) <= 1e-15
    # narrower than the window: no SSIM position, the integer sums still count
    row = R.reference_row(zero[:10, :], full[:10, :])
    assert row[2:] == [0.0, 0.0] and row[0] == 10 * 20 * 3 * 65025


def test_library_exports_and_binding(lib_built):
    from text2video_amd import _lib
    assert lib_built.t2v_abi_version() == 22 == _lib.ABI_VERSION
    for name in ("t2v_image_metrics_scratch_doubles", "t2v_image_metrics_u8"):
        assert name in _lib.SIGNATURES and getattr(lib_built, name).argtypes == _lib.SIGNATURES[name][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T t2v_image_metrics_u8" in out and " T t2v_image_metrics_scratch_doubles" in out
    # one partial per 32x32 tile, region and sum; 0 for a shape the call refuses
    f = lib_built.t2v_image_metrics_scratch_doubles
    assert f(512, 512, 0) == 16 * 16 * 3 and f(75, 133, 3) == 3 * 5 * 4 * 3 and f(1, 1, 0) == 3
    assert f(0, 5, 0) == 0 and f(8193, 5, 0) == 0 and f(5, 5, 4) == 0 and f(5, 5, -1) == 0
    header = open(os.path.join(ROOT, "include", "t2v.h")).read()
    assert "t2v_image_metrics_u8" in header and "#define T2V_ABI_VERSION 22" in header


def test_metrics_option_parses_and_refuses_shard_chunks(capsys):
    from text2video_amd.options import TestOptions
    assert TestOptions().parse([]).metrics is False
    assert TestOptions().parse(["--metrics"]).metrics is True
    with pytest.raises(SystemExit):
        TestOptions().parse(["--metrics", "--shard_chunks"])
    assert "--metrics with --shard_chunks" in capsys.readouterr().err


def test_metrics_summary_and_pooling():
    from text2video_amd import metrics as M
    from text2video_amd import ops
    s = ops.metrics_summary([300.0, 30.0, 45.0, 50.0], 100)
    assert s["mse"] == 3.0 and s["mae"] == 0.3 and s["ssim"] == 0.9
    assert abs(s["psnr"] - 10.0 * np.log10(65025.0 / 3.0)) <= 1e-12
    same = ops.metrics_summary([0.0, 0.0, 50.0, 50.0], 100)
    assert same["psnr"] is None and same["ssim"] == 1.0 and same["mse"] == 0.0
    narrow = ops.metrics_summary([10.0, 10.0, 0.0, 0.0], 100)
    assert narrow["ssim"] is None and narrow["psnr"] is not None
    # the summary's PSNR is that of the pooled MSE, not the mean of the frames' PSNRs; ssim and mae are means
    doc = M.summarise([("a.jpg", (10, 10), None), ("b.jpg", (10, 10), (0, 5, 0, 4))],
                      np.array([[300.0, 30.0, 45.0, 50.0], [9, 9, 9, 9],       # (row 1: no face, not read)
                                [900.0, 90.0, 25.0, 50.0], [60.0, 6.0, 0.0, 0.0]]))
    assert abs(doc["summary"]["psnr"] - 10.0 * np.log10(65025.0 / (1200.0 / 600.0))) <= 1e-12
    assert abs(doc["summary"]["ssim"] - 0.7) <= 1e-15 and abs(doc["summary"]["mae"] - 0.2) <= 1e-15
    assert doc["summary"]["frames"] == 2 and doc["summary"]["face"]["frames"] == 1
    assert doc["frames"][0]["face"] is None and doc["frames"][1]["face"]["ssim"] is None
    assert abs(doc["frames"][1]["face"]["mae"] - 0.1) <= 1e-15 and doc["summary"]["face"]["ssim"] is None
    assert isinstance(doc["definition"], str) and "\n" not in doc["definition"]
    empty = M.summarise([], np.zeros((0, 4)))
    assert empty["summary"]["frames"] == 0 and empty["summary"]["psnr"] is None


def test_get_face_region_lives_in_keypoints_without_torch():
    code = ("import sys, numpy as np\n"
            "from text2video_amd.keypoints import get_face_region, NOSE_NECK_RGB\n"
            "m = np.zeros((512, 320, 3), np.uint8); m[100:140, 150:153] = NOSE_NECK_RGB\n"
            "assert get_face_region(m, 512) == (55, 183, 87, 215), get_face_region(m, 512)\n"
            "assert get_face_region(np.zeros((64, 64, 3), np.uint8), 64) is None\n"
            "assert 'torch' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    from text2video_amd import keypoints, train
    assert train.get_face_region is keypoints.get_face_region


def test_metrics_and_evaluate_import_without_torch_on_the_lean_provider():
    """what a plain `test.py --metrics` run and `python -m text2video_amd.evaluate` import"""
    code = ("import sys\nfrom text2video_amd import _xp\n_xp.use_lean()\nimport text2video_amd.metrics, text2video_amd.evaluate\n"
            "assert 'torch' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]


def test_evaluate_pairs_files_by_relative_path(tmp_path):
    from text2video_amd.evaluate import pair_files
    a, b = tmp_path / "a", tmp_path / "b"
    for root, files in ((a, ["tmp/fake_B_0002.jpg", "tmp/fake_B_0003.jpg", "tmp/real_A_0002.jpg", "s2/fake_B_0002.jpg",
                             "tmp/fake_B_notes.txt", "tmp/metrics.json"]),
                        (b, ["tmp/fake_B_0002.jpg", "tmp/fake_B_0004.jpg", "tmp/real_A_0002.jpg", "s2/fake_B_0002.jpg",
                             "fake_B_top.png"])):
        for f in files:
            (root / f).parent.mkdir(parents=True, exist_ok=True)
            (root / f).write_bytes(b"x")
    pairs, only_a, only_b = pair_files(str(a), str(b))
    assert pairs == ["s2/fake_B_0002.jpg", "tmp/fake_B_0002.jpg"]
    assert only_a == ["tmp/fake_B_0003.jpg"] and only_b == ["fake_B_top.png", "tmp/fake_B_0004.jpg"]
    assert pair_files(str(a), str(b), "real_A_*") == (["tmp/real_A_0002.jpg"], [], [])


def test_real_frame_geometry_is_the_pose_maps():
    from text2video_amd.metrics import face_box, real_frame_geometry
    from text2video_amd.options import TestOptions
    opt = TestOptions().parse(["--resize_or_crop", "scaleHeight", "--loadSize", "512"])
    assert real_frame_geometry(opt, (512, 384)) == ((680, 512), (180, 0, 500, 512), (512, 320))
    opt.no_pose_crop = True
    assert real_frame_geometry(opt, (512, 384)) == ((680, 512), (0, 0, 680, 512), (512, 680))
    # a frame too small to hold the face box has none
    from text2video_amd.keypoints import NOSE_NECK_RGB
    m = np.zeros((64, 12, 3), np.uint8)
    m[30, 5] = NOSE_NECK_RGB
    assert face_box(m) is None
    m = np.zeros((64, 64, 3), np.uint8)
    m[30, 5] = NOSE_NECK_RGB
    assert face_box(m) == (22, 38, 0, 16)
