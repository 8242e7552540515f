"""GPU tests of the JPEG writer (libt2v_jpeg.so, ops.jpeg_encode_u8, test.py --gpu_jpeg): the kernels' file against the
numpy restatement (tests/jpeg_reference.py) and against Pillow, byte for byte, on the cases tests/test_cpu_jpeg.py shows to
reach every rule of the format; batching, repeatability, the capacity guard, the refusal of an unsupported geometry, the
frame loop's window / second-copy rule, and the files of `test.py --gpu_jpeg` against those of the plain command."""
import glob
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_reference as R  # noqa: E402

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
    """(the restatement's file, Pillow's file) of a case: computed once, shared, never modified"""
    if case not in _reference:
        kind, H, W, q = case
        buf = io.BytesIO()
        Image.fromarray(R.make_image(kind, H, W)).save(buf, format="JPEG", quality=q)
        _reference[case] = (R.encode(R.make_image(kind, H, W), q), buf.getvalue())
    return _reference[case]


def gpu_files(images_np, quality, dev, **kw):
    """[N,H,W,cs] or [H,W,cs] uint8 -> the N finished files"""
    import torch
    from text2video_amd import jpeg, ops
    x = torch.from_numpy(images_np).to(dev)
    out, lengths = ops.jpeg_encode_u8(x, quality, **kw)
    torch.cuda.synchronize()
    n = lengths.cpu().numpy()
    assert (n <= out.shape[1]).all()
    H, W = images_np.shape[-3:-1]
    host = out.cpu().numpy()
    return [jpeg.file_bytes(jpeg.header(H, W, quality), host[i, :n[i]].tobytes()) for i in range(len(n))]


@pytest.mark.parametrize("cs", [3, 4])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_file_equals_the_restatement_and_pillow(dev, case, cs):
    kind, H, W, q = case
    ref, pil = reference(case)
    (got,) = gpu_files(R.make_image(kind, H, W, cs), q, dev)
    assert got == ref.file, "%s: %d bytes, the restatement %d, first difference at %d" % (
        R.case_id(case), len(got), len(ref.file), next((i for i, (a, b) in enumerate(zip(got, ref.file)) if a != b), -1))
    assert got == pil
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got))), np.asarray(Image.open(io.BytesIO(pil))))


@pytest.mark.parametrize("case", [("noise", 250, 130, 90), ("smooth", 512, 512, 75), ("noise", 512, 320, 100)], ids=R.case_id)
def test_frame_sized_images_equal_pillow(dev, case):
    """more blocks than one workgroup of the prefix sum has threads (864 / 6144 / 3840: several per thread), scans of many
    4096-byte chunks (the 0xFF offsets cross chunks), odd MCU counts; at these sizes the reference is Pillow alone"""
    kind, H, W, q = case
    img = R.make_image(kind, H, W)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=q)
    (got,) = gpu_files(np.stack([img, img[::-1].copy()]), q, dev)[:1]
    assert len(got) == len(buf.getvalue()) and got == buf.getvalue()
    if kind == "noise":
        assert got.count(b"\xff\x00") > 8 and len(got) > 3 * 4096


def test_a_batch_equals_the_single_calls_and_two_runs_agree(dev):
    a, b = R.make_image("noise", 40, 56), R.make_image("smooth", 40, 56)
    both = gpu_files(np.stack([a, b]), 90, dev)
    assert both == gpu_files(a, 90, dev) + gpu_files(b, 90, dev)
    assert both[0] != both[1]
    assert both == gpu_files(np.stack([a, b]), 90, dev)
    assert both == [R.encode(a, 90).file, R.encode(b, 90).file]


def test_capacity_guard(dev):
    """out_capacity below the scan length: lengths reports the true length, the bytes up to the capacity are the scan's and
    the 64 guard bytes behind the capacity, inside the same allocation, keep their value"""
    import torch
    from text2video_amd import ops
    case = ("noise", 40, 56, 100)
    kind, H, W, q = case
    scan = reference(case)[0].scan
    cap = len(scan) // 2 + 3
    x = torch.from_numpy(np.stack([R.make_image(kind, H, W)] * 2)).to(dev)
    buf = torch.full((2 * cap + 64,), 0x5A, dtype=torch.uint8, device=dev)
    out, lengths = ops.jpeg_encode_u8(x, q, out=buf[:2 * cap].view(2, cap))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert lengths.cpu().tolist() == [len(scan)] * 2 and len(scan) > cap
    assert host[:cap].tobytes() == scan[:cap] and host[cap:2 * cap].tobytes() == scan[:cap]
    assert (host[2 * cap:] == 0x5A).all()


def test_unsupported_geometry_is_refused_with_nothing_launched(dev):
    import torch
    from text2video_amd import _jpeglib, ops
    assert not ops.jpeg_supported(7, 64) and not ops.jpeg_supported(64, 2049) and ops.jpeg_supported(8, 2048)
    assert ops.jpeg_scan_capacity(7, 64) == 0 and ops.jpeg_workspace_bytes(64, 4096, 1) == 0
    x = torch.zeros(7, 64, 3, dtype=torch.uint8, device=dev)
    out = torch.full((1, 256), 7, dtype=torch.uint8, device=dev)
    lengths = torch.full((1,), -5, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="7x64"):
        ops.jpeg_encode_u8(x, 75, out=out, lengths=lengths)
    # the library itself refuses as well (status T2V_JPEG_ERR_INVALID), before any launch
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    st = _jpeglib.load().t2v_jpeg_encode_u8(None, x.data_ptr(), 3, 7, 64, 1, 75, ws.data_ptr(), out.data_ptr(), 256,
                                            lengths.data_ptr())
    assert st == -1 and b"7x64" in _jpeglib.load().t2v_jpeg_last_error()
    torch.cuda.synchronize()
    assert (out.cpu() == 7).all() and lengths.cpu().tolist() == [-5]
    with pytest.raises(ValueError, match="quality"):
        ops.jpeg_encode_u8(torch.zeros(16, 16, 3, dtype=torch.uint8, device=dev), 0)
    with pytest.raises(ValueError, match="uint8"):
        ops.jpeg_encode_u8(torch.zeros(16, 16, 3, device=dev))


def test_stage_copies_through_the_byte_map(dev):
    """t2v_jpeg_stage_u8: 3 -> 4 and 4 -> 3 channel strides, with and without a byte map, odd pixel counts and more pixels
    than one pass of the grid"""
    import torch
    from text2video_amd import ops
    rng = np.random.default_rng(5)
    lut = rng.permutation(256).astype(np.uint8)
    for (H, W), scs, dcs, use_lut in (((21, 37), 3, 4, True), ((21, 37), 4, 3, False), ((768, 700), 3, 4, True)):
        src = rng.integers(0, 256, (H, W, scs), dtype=np.uint8)
        dst = torch.full((H, W, dcs), 9, dtype=torch.uint8, device=dev)
        ops.jpeg_stage_u8(torch.from_numpy(src).to(dev), dst, lut if use_lut else None)
        want = np.zeros((H, W, dcs), np.uint8)
        want[..., :3] = lut[src[..., :3]] if use_lut else src[..., :3]
        assert np.array_equal(dst.cpu().numpy(), want)


def test_window_rule_second_copy_yields_the_same_file(dev):
    """jpeg_frames.StepEncoder (the frame loop's --gpu_jpeg path): a scan longer than the window that travels with the
    lengths is completed by a second copy and yields the same file; the slot's window then grows, so that the steps encoded
    afterwards take such a scan whole.  Four steps: every slot of the ring and its reuse are seen."""
    import torch
    from text2video_amd.jpeg_frames import StepEncoder
    case = ("noise", 40, 56, 100)
    kind, H, W, q = case
    ref = reference(case)[0]
    small = R.make_image("constant", H, W, 4)
    small_file = R.encode(small, q).file
    enc = StepEncoder(H, W, 2, q, dev, window=1024)
    assert enc.windows == (1024, 1024) and 1024 < len(ref.scan) and len(small_file) - 625 < 1024
    frames = torch.from_numpy(np.stack([R.make_image(kind, H, W, 4), small])).to(dev)
    steps = []
    for n in range(4):
        enc.image(0).copy_(frames[n % 2])
        enc.image(1).copy_(frames[1 - n % 2])
        steps.append(enc.encode())
        if n >= 1:
            files = enc.files(steps[n - 1])
            assert files == ([ref.file, small_file] if (n - 1) % 2 == 0 else [small_file, ref.file])
    assert enc.files(steps[3]) == [small_file, ref.file]
    # steps 0 and 1 were encoded with the small windows (one long scan each); steps 2 and 3 with the grown ones
    grown = (len(ref.scan) * 5 // 4 + 255) // 256 * 256
    assert enc.second_copies == 2 and enc.windows == (grown, grown)
    assert [st.windows for st in steps] == [(1024, 1024), (1024, 1024), (grown, 1024), (grown, grown)]
    # a window of exactly the scan's length takes it whole
    enc = StepEncoder(H, W, 1, q, dev, window=len(ref.scan))
    enc.image(0).copy_(frames[0])
    assert enc.files(enc.encode()) == [ref.file] and enc.second_copies == 0


def _make_dataset(tmp):
    """datasets/fadg0 as the L2 driver leaves it (tests/test_gpu_e2e.py): pose JSONs + the skeleton jpgs it renders"""
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


def _command(work):
    """(run, results directory): run(extra flags, lean) -> ({relative path: file bytes}, timing["cold_start"]) of test.py on
    the dataset of _make_dataset at --loadSize 128 (the smallest an existing end-to-end test uses), small net, seeded weights"""
    import json
    cmd = [sys.executable, os.path.join(ROOT, "vid2vid", "test.py"), "--name", "fadg0", "--dataroot", "datasets/fadg0",
           "--dataset_mode", "pose", "--input_nc", "3", "--resize_or_crop", "scaleHeight", "--loadSize", "128",
           "--openpose_only", "--how_many", "1200", "--no_first_img", "--random_drop_prob", "0", "--synthetic_weights", "1",
           "--ngf", "16", "--n_blocks", "2", "--n_downsample_G", "2", "--timing_json", "timing.json"]
    res = os.path.join(work, "results", "fadg0", "test_latest")

    def run(extra, lean, ok=True):
        shutil.rmtree(os.path.join(work, "results"), ignore_errors=True)
        env = dict(os.environ, CUDA_VISIBLE_DEVICES="0", T2V_LEAN="1" if lean else "0")
        r = subprocess.run(cmd + extra, cwd=work, env=env, capture_output=True, text=True, timeout=600)
        if not ok:
            return r
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        timing = json.load(open(os.path.join(work, "timing.json")))
        assert timing["cold_start"]["torch_imported"] is (not lean)
        files = sorted(glob.glob(os.path.join(res, "*", "*.jpg")))
        return {os.path.relpath(f, res): open(f, "rb").read() for f in files}, timing["cold_start"]
    return run, res


def test_gpu_jpeg_command_writes_the_files_of_the_plain_command(tmp_path):
    """test.py on tests/golden/dataset_fadg0_l2 with --synthetic_weights: every fake_B_*.jpg and real_A_*.jpg of the
    --gpu_jpeg run is the plain run's file, byte for byte -- on torch and through the lean (torch-free) entry;
    --timing_json carries jpeg_s and the D2H bytes per frame; --jpeg_quality alone is refused."""
    run, _ = _command(_make_dataset(str(tmp_path)))
    plain, t_plain = run([], False)
    assert len(plain) == 16 and sum(k.split(os.sep)[1].startswith("real_A_") for k in plain) == 8
    H, W = Image.open(io.BytesIO(plain[sorted(plain)[0]])).size[::-1]
    assert t_plain["d2h_bytes_per_frame"] == H * W * 4 and "jpeg_s" not in t_plain["loop_split"]
    for lean in (False, True):
        got, t = run(["--gpu_jpeg"], lean)
        assert got.keys() == plain.keys()
        assert [k for k in plain if got[k] != plain[k]] == []
        assert t["loop_split"]["jpeg_s"] > 0 and t["loop_split"]["jpeg_second_copies"] >= 0
        assert 0 < t["d2h_bytes_per_frame"] < t_plain["d2h_bytes_per_frame"]
    r = run(["--jpeg_quality", "90"], True, ok=False)
    assert r.returncode != 0 and "--gpu_jpeg" in r.stderr


def test_gpu_jpeg_leaves_the_metrics_as_they_are(tmp_path):
    """--metrics_temporal under --gpu_jpeg keeps comparing the bytes before JPEG, the previous frame's included (the batch
    slot a frame was rendered into is rewritten by the next step): the same figures and the same files as without the flag"""
    import json
    run, res = _command(_make_dataset(str(tmp_path)))

    def metrics():
        return {seq: json.load(open(os.path.join(res, seq, "metrics.json"))) for seq in ("tmp", "tmp_smooth")}
    plain, _ = run(["--metrics_temporal"], True)
    want = metrics()
    got, _ = run(["--gpu_jpeg", "--metrics_temporal"], True)
    assert len(plain) == 16 and got == plain and metrics() == want and "temporal" in want["tmp"]["summary"]
