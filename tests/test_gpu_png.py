"""GPU tests of the PNG writer (libt2v_png.so, ops.png_encode_u8, test.py --frame_format png): the kernels' file against the
numpy restatement (tests/png_reference.py), byte for byte, on the cases tests/test_cpu_png.py shows to be valid PNG files
of their input; batching, storage, repeatability, the capacity guard, the refusal of an unsupported geometry, the frame
loop's window / second-copy rule, and the frames and metrics of `test.py --frame_format png` against the plain command's."""
import glob
import io
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def dev(lib_built):
    import torch
    from text2video_amd import ops
    ops.context(0)
    return torch.device("cuda:0")


_reference = {}


def reference(case):
    """the restatement's file of a case: computed once, shared, never modified"""
    if case not in _reference:
        _reference[case] = R.encode(R.make_image(*case)).file
    return _reference[case]


def gpu_files(images_np, dev, **kw):
    """[N,H,W,cs] or [H,W,cs] uint8 -> the N files"""
    import torch
    from text2video_amd import ops
    x = torch.from_numpy(images_np).to(dev)
    out, lengths = ops.png_encode_u8(x, **kw)
    torch.cuda.synchronize()
    n = lengths.cpu().numpy()
    assert (n <= out.shape[1]).all()
    host = out.cpu().numpy()
    return [host[i, :n[i]].tobytes() for i in range(len(n))]


def first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


@pytest.mark.parametrize("cs", [3, 4])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_file_equals_the_restatement(dev, case, cs):
    """cs 4: the fourth channel holds random bytes, which the writer ignores"""
    want = reference(case)
    (got,) = gpu_files(R.make_image(*case, cs), dev)
    assert got == want, "%s: %d bytes, the restatement %d, first difference at %d" % (
        R.case_id(case), len(got), len(want), first_difference(got, want))


def test_frame_sized_image_equals_the_restatement_and_decodes_to_the_input(dev):
    """512 x 512, the crop tiled, its lower half with noise: 64 bands, rows of 1537 bytes (several bytes per thread of a band's
    workgroup, several 4096-byte chunks of the IDAT)"""
    img = R.make_image(*R.BIG_CASE)
    (got,) = gpu_files(img, dev)
    want = reference(R.BIG_CASE)
    assert got == want, "%d bytes, the restatement %d, first difference at %d" % (len(got), len(want), first_difference(got, want))
    im = Image.open(io.BytesIO(got))
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)


@pytest.mark.parametrize("cs", [3, 4])
def test_a_batch_equals_the_single_calls_and_two_runs_agree(dev, cs):
    from text2video_amd import ops
    cases = [("noise", 33, 65), ("colour", 33, 65), ("mixed", 33, 65)]
    images = [R.make_image(*c, cs) for c in cases]
    batch = gpu_files(np.stack(images), dev)
    assert batch == [gpu_files(im, dev)[0] for im in images]
    assert len(set(batch)) == 3
    assert batch == gpu_files(np.stack(images), dev)
    assert batch == [R.encode(im).file for im in images]
    # the capacity of the rows does not change the files
    import torch
    cap = max(len(f) for f in batch) + 13
    out = torch.empty(3, cap, dtype=torch.uint8, device=dev)
    assert gpu_files(np.stack(images), dev, out=out) == batch and cap < ops.png_file_capacity(33, 65)


def test_capacity_guard(dev):
    """out_capacity below the file's length: lengths reports the true length, the bytes up to the capacity are the file's and
    the guard bytes behind every slot, inside the same allocation, keep their value -- at a capacity inside the IDAT, and at
    one inside the header the closing kernel writes"""
    import torch
    from text2video_amd import ops
    case = ("noise", 33, 65)
    want = reference(case)
    x = torch.from_numpy(np.stack([R.make_image(*case)] * 2)).to(dev)
    for cap in (len(want) // 2 + 3, 20, len(want) - 5):
        buf = torch.full((2 * (cap + 64),), 0x5A, dtype=torch.uint8, device=dev)
        # two slots of `cap` bytes, each followed by 64 guard bytes: rows of a [2, cap + 64] view, capacity passed as cap
        view = buf.view(2, cap + 64)
        lengths = torch.zeros(2, dtype=torch.int32, device=dev)
        from text2video_amd import _pnglib
        ws = torch.empty(ops.png_workspace_bytes(33, 65, 1), dtype=torch.uint8, device=dev)
        for i in range(2):
            st = _pnglib.load().t2v_png_encode_u8(None, x[i].data_ptr(), 3, 33, 65, 1, ws.data_ptr(), view[i].data_ptr(), cap,
                                                  lengths[i:].data_ptr())
            assert st == 0
        torch.cuda.synchronize()
        host = view.cpu().numpy()
        assert lengths.cpu().tolist() == [len(want)] * 2 and len(want) > cap
        for i in range(2):
            assert host[i, :cap].tobytes() == want[:cap]
            assert (host[i, cap:] == 0x5A).all()
    # a batch: the slots follow each other at out_capacity, guard bytes behind the last
    cap = len(want) // 2 + 3
    buf = torch.full((2 * cap + 64,), 0x5A, dtype=torch.uint8, device=dev)
    out, lengths = ops.png_encode_u8(x, out=buf[:2 * cap].view(2, cap))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert lengths.cpu().tolist() == [len(want)] * 2
    assert host[:cap].tobytes() == want[:cap] and host[cap:2 * cap].tobytes() == want[:cap]
    assert (host[2 * cap:] == 0x5A).all()


def test_unsupported_geometry_is_refused_with_nothing_launched(dev):
    import torch
    from text2video_amd import _pnglib, ops
    assert not ops.png_supported(0, 64) and not ops.png_supported(64, 2049) and ops.png_supported(1, 2048) and ops.png_supported(1, 1)
    assert ops.png_file_capacity(0, 64) == 0 and ops.png_workspace_bytes(64, 4096, 1) == 0
    x = torch.zeros(64, 2049, 3, dtype=torch.uint8, device=dev)
    out = torch.full((1, 256), 7, dtype=torch.uint8, device=dev)
    lengths = torch.full((1,), -5, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="64x2049"):
        ops.png_encode_u8(x, out=out, lengths=lengths)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    st = _pnglib.load().t2v_png_encode_u8(None, x.data_ptr(), 3, 64, 2049, 1, ws.data_ptr(), out.data_ptr(), 256, lengths.data_ptr())
    assert st == -1 and b"64x2049" in _pnglib.load().t2v_png_last_error()
    torch.cuda.synchronize()
    assert (out.cpu() == 7).all() and lengths.cpu().tolist() == [-5]
    with pytest.raises(ValueError, match="uint8"):
        ops.png_encode_u8(torch.zeros(16, 16, 3, device=dev))


def test_window_rule_second_copy_yields_the_same_file(dev):
    """png_frames.StepEncoder (the frame loop's --frame_format png path): a file longer than the window that travels with the
    lengths is completed by a second copy and is the same file; the slot's window then grows, so that the steps encoded
    afterwards take such a file whole.  Four steps: every slot of the ring and its reuse are seen."""
    import torch
    from text2video_amd.png_frames import StepEncoder
    H, W = 33, 65
    long_file = reference(("noise", H, W))
    small = R.make_image("colour", H, W, 4)
    small_file = R.encode(small).file
    enc = StepEncoder(H, W, 2, dev, window=1024)
    assert enc.windows == (1024, 1024) and 1024 < len(long_file) and len(small_file) < 1024
    frames = torch.from_numpy(np.stack([R.make_image("noise", H, W, 4), small])).to(dev)
    steps = []
    for n in range(4):
        enc.image(0).copy_(frames[n % 2])
        enc.image(1).copy_(frames[1 - n % 2])
        steps.append(enc.encode())
        if n >= 1:
            files = enc.files(steps[n - 1])
            assert files == ([long_file, small_file] if (n - 1) % 2 == 0 else [small_file, long_file])
    assert enc.files(steps[3]) == [small_file, long_file]
    grown = (len(long_file) * 5 // 4 + 255) // 256 * 256
    assert enc.second_copies == 2 and enc.windows == (grown, grown)
    assert [st.windows for st in steps] == [(1024, 1024), (1024, 1024), (grown, 1024), (grown, grown)]
    enc = StepEncoder(H, W, 1, dev, window=len(long_file))
    enc.image(0).copy_(frames[0])
    assert enc.files(enc.encode()) == [long_file] and enc.second_copies == 0


def test_evaluate_pairs_a_png_tree_with_a_jpeg_tree(dev, tmp_path):
    """compare_trees(pair_by_stem=True): the writer's .png files against Pillow's .jpg files of the same pictures are paired,
    nothing is left over, and the figures are those of the JPEG loss; without the flag nothing pairs"""
    from text2video_amd.evaluate import compare_trees
    images = [R.make_image("crop", 128, 128), R.make_image("crop", 128, 128)[::-1].copy()]
    for root, ext in ((tmp_path / "a" / "s", ".png"), (tmp_path / "b" / "s", ".jpg")):
        os.makedirs(root)
        for i, img in enumerate(images):
            if ext == ".png":
                (root / ("fake_B_%04d.png" % i)).write_bytes(gpu_files(img, dev)[0])
            else:
                Image.fromarray(img).save(root / ("fake_B_%04d.jpg" % i))
    rep = compare_trees(str(tmp_path / "a"), str(tmp_path / "b"), device="cuda:0", pair_by_stem=True)
    assert rep["overall"]["frames"] == 2 and not (rep["unpaired_a"] or rep["unpaired_b"] or rep["size_mismatch"])
    assert 25.0 < rep["overall"]["psnr"] < 60.0
    same = compare_trees(str(tmp_path / "a"), str(tmp_path / "a"), device="cuda:0", pair_by_stem=True)
    assert same["overall"]["frames"] == 2 and same["overall"]["psnr"] is None and same["overall"]["mae"] == 0
    rep = compare_trees(str(tmp_path / "a"), str(tmp_path / "b"), device="cuda:0")
    assert rep["overall"]["frames"] == 0 and len(rep["unpaired_a"]) == len(rep["unpaired_b"]) == 2


def _make_dataset(tmp):
    """datasets/fadg0 as the L2 driver leaves it (tests/test_gpu_jpeg.py uses the same): pose JSONs + the skeleton jpgs"""
    from text2video_amd.keypoints import read_keypoints
    root = os.path.join(tmp, "vid2vid", "datasets", "fadg0")
    for seq, pat in (("tmp", "%04d.jpg"), ("tmp_smooth", "smooth_%04d.jpg")):
        src = os.path.join(GOLD, "dataset_fadg0_l2", "test_openpose", seq)
        os.makedirs(os.path.join(root, "test_openpose", seq))
        os.makedirs(os.path.join(root, "test_img", seq))
        for i, f in enumerate(sorted(os.listdir(src))):
            shutil.copyfile(os.path.join(src, f), os.path.join(root, "test_openpose", seq, f))
            Image.fromarray(read_keypoints(os.path.join(src, f), (512, 384))).save(
                os.path.join(root, "test_img", seq, pat % i))
    return os.path.join(tmp, "vid2vid")


def test_png_command_writes_the_frames_of_the_plain_command(tmp_path):
    """test.py --frame_format png on the tiny dataset of the JPEG command test: .png files named like the plain command's
    .jpg files; their decoded pixels, saved by Pillow as JPEG at its default quality, are the plain command's files byte for
    byte -- the frames are the same uint8 arrays; metrics.json of --metrics is identical; --timing_json carries png_s"""
    work = _make_dataset(str(tmp_path))
    cmd = [sys.executable, os.path.join(ROOT, "vid2vid", "test.py"), "--name", "fadg0", "--dataroot", "datasets/fadg0",
           "--dataset_mode", "pose", "--input_nc", "3", "--resize_or_crop", "scaleHeight", "--loadSize", "128",
           "--openpose_only", "--how_many", "1200", "--no_first_img", "--random_drop_prob", "0", "--synthetic_weights", "1",
           "--ngf", "16", "--n_blocks", "2", "--n_downsample_G", "2", "--timing_json", "timing.json", "--metrics"]
    res = os.path.join(work, "results", "fadg0", "test_latest")

    def run(extra):
        shutil.rmtree(os.path.join(work, "results"), ignore_errors=True)
        env = dict(os.environ, CUDA_VISIBLE_DEVICES="0", T2V_LEAN="1")
        r = subprocess.run(cmd + extra, cwd=work, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        files = sorted(glob.glob(os.path.join(res, "*", "*.jpg")) + glob.glob(os.path.join(res, "*", "*.png")))
        metrics = {seq: json.load(open(os.path.join(res, seq, "metrics.json"))) for seq in ("tmp", "tmp_smooth")}
        return ({os.path.relpath(f, res): open(f, "rb").read() for f in files}, metrics,
                json.load(open(os.path.join(work, "timing.json")))["cold_start"])
    plain, m_plain, t_plain = run([])
    assert len(plain) == 16 and all(k.endswith(".jpg") for k in plain)
    got, m_got, t = run(["--frame_format", "png"])
    assert sorted(os.path.splitext(k)[0] for k in got) == sorted(os.path.splitext(k)[0] for k in plain)
    assert all(k.endswith(".png") for k in got)
    for k, blob in got.items():
        im = Image.open(io.BytesIO(blob))
        assert im.mode == "RGB"
        buf = io.BytesIO()
        Image.fromarray(np.asarray(im)).save(buf, format="JPEG")
        assert buf.getvalue() == plain[os.path.splitext(k)[0] + ".jpg"], k
    assert m_got == m_plain
    assert t["loop_split"]["png_s"] > 0 and t["loop_split"]["png_second_copies"] >= 0 and "jpeg_s" not in t["loop_split"]
    assert "png_s" not in t_plain["loop_split"] and t["d2h_bytes_per_frame"] > 0
