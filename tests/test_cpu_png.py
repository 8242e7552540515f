"""CPU tests of the PNG writer's contract (include/t2v_png.h):

* the numpy restatement (tests/png_reference.py) writes, for every case tests/test_gpu_png.py compares the kernels against,
  a file Pillow opens as RGB with exactly the input pixels, whose IDAT zlib inflates to the filtered bytes, with zlib's
  CRC-32 on every chunk and zlib's Adler-32;
* its size against zlib's Z_RLE strategy over the same filtered bytes in one stream, on the committed crop and a pose map;
* the length-limit case needs, by the restatement's own check, a 16-bit code before limiting;
* libt2v_png.so builds, exports every symbol of t2v_png.h, bounds every case's file; refused calls launch nothing and say
  why; the library's kernels are each claimed by a GPU test;
* --frame_format parses and refuses the JPEG writer's options; evaluate's --pair_by_stem pairs and counts.
"""
import io
import os
import re
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every kernel of libt2v_png.so -> the test of tests/test_gpu_png.py that checks its output (all seven run in every encode
# call; the test named is the one whose cases single the kernel out)
KERNELS = {
    "png_filter_kernel": "test_file_equals_the_restatement",            # all five filter types, W below one wave
    "png_hist_kernel": "test_file_equals_the_restatement",              # runs across rows and the 258-byte chunking
    "png_code_kernel": "test_file_equals_the_restatement",              # the length-limit case, two-symbol codes
    "png_prepare_kernel": "test_a_batch_equals_the_single_calls_and_two_runs_agree",
    "png_pack_kernel": "test_frame_sized_image_equals_the_restatement_and_decodes_to_the_input",
    "png_crc_copy_kernel": "test_capacity_guard",
    "png_close_kernel": "test_capacity_guard",
}
ALL_CASES = R.CASES + [R.BIG_CASE]

_encoded = {}


def _reference(case):
    if case not in _encoded:
        _encoded[case] = R.encode(R.make_image(*case))
    return _encoded[case]


def _rle_size(filtered):
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(co.compress(filtered) + co.flush())


@pytest.fixture(scope="module")
def png_lib():
    from text2video_amd import _pnglib
    if not os.path.exists(_pnglib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _pnglib.load()


@pytest.mark.parametrize("case", ALL_CASES, ids=R.case_id)
def test_restatement_writes_a_valid_file_of_the_input(case):
    img = R.make_image(*case)
    e = _reference(case)
    im = Image.open(io.BytesIO(e.file))
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)
    chunks = R.chunks_of(e.file)
    assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    _, H, W = case
    assert chunks[0][1] == W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, 2, 0, 0, 0]) and chunks[2][1] == b""
    payload = chunks[1][1]
    assert payload[:2] == b"\x78\x01" and payload == e.payload
    assert zlib.decompress(payload) == e.filtered and len(e.filtered) == H * (1 + 3 * W)
    d = zlib.decompressobj(-15)      # the raw stream alone ends exactly where the Adler value starts
    assert d.decompress(payload[2:]) == e.filtered and d.eof and d.unused_data == payload[-4:]
    for kind, body, crc in chunks:
        assert crc == zlib.crc32(kind + body)
    assert int.from_bytes(payload[-4:], "big") == zlib.adler32(e.filtered)
    assert len(e.file) <= R.file_capacity(H, W)
    # a fourth channel is ignored, whatever it holds
    assert R.encode(R.make_image(*case, 4)).file == e.file


def test_cases_reach_the_rules():
    """from the restatement's own record: what the GPU test's byte equality is evidence of"""
    stats = {c: _reference(c).stats for c in ALL_CASES}
    filters = {c: set(_reference(c).filters.tolist()) for c in ALL_CASES}
    assert set().union(*filters.values()) == {0, 1, 2, 3, 4}
    assert stats[("zero", 24, 90)]["max_match"] == 258 and stats[("zero", 24, 90)]["matches"] == 27      # 8 x 258 + 103 per band
    assert stats[("colour", 16, 100)]["max_match"] == 258 and filters[("colour", 16, 100)] == {1, 2}
    assert stats[("noise", 33, 65)]["matches"] == 0 and stats[("noise", 33, 65)]["no_match_bands"] == 5
    assert stats[("mixed", 1, 1)]["no_match_bands"] == 1 and stats[("crop", 128, 128)]["no_match_bands"] == 0
    assert stats[("pose", 64, 64)]["max_match"] > 150 and stats[("pose", 64, 64)]["literals"] > 1000
    assert any(H % 8 == 1 for _, H, _ in R.CASES) and any(H < 8 for _, H, _ in R.CASES)
    # the repeat symbols of the code-length alphabet: 18 and 17 in a sparse table, 16 in a flat one
    rle = R.rle_code_lengths([0] * 150 + [8] * 9 + [0, 0] + [7] * 4 + [0] * 5)
    assert [s for s, _, _ in rle] == [18, 18, 8, 16, 8, 8, 0, 0, 7, 16, 17]
    assert rle[0][2] == 138 - 11 and rle[1][2] == 12 - 11 and rle[3][2] == 6 - 3 and rle[9][2] == 0 and rle[10][2] == 5 - 3


def test_length_limit_case_needs_a_longer_code_before_limiting():
    case = ("fibonacci", 8, 175)
    assert case in R.CASES
    e = _reference(case)
    assert e.stats["unlimited_max"] > 15 and (1 + 3 * 175) * 8 == 4208
    hist = np.bincount(np.frombuffer(e.filtered, np.uint8), minlength=R.NSYM)
    hist[256] = 1
    lengths, unlimited = R.code_lengths(hist, 15)
    assert unlimited == e.stats["unlimited_max"] == 16 and max(lengths) == 15
    assert sum(2.0 ** -n for n in lengths if n) == 1.0          # still a complete code
    # the unlimited lengths are those of a Huffman code: the same cost as heapq's
    import heapq
    heap = sorted(int(c) for c in hist if c)
    cost = 0
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, a + b)
    free, _ = R.code_lengths(hist, 32)
    assert sum(int(c) * n for c, n in zip(hist, free)) == cost < sum(int(c) * n for c, n in zip(hist, lengths))


SIZE_RATIO_CROP = 1.02       # measured 1.0109 (20713 / 20490 bytes, profiles/png_encode.txt), rounded up to the next 0.01
SIZE_RATIO_POSE = 1.06       # measured 1.0533 (8376 / 7952): a pose map is nearly empty, its 48 block headers weigh more


def test_size_against_zlib_rle():
    """the IDAT payload against zlib.compressobj(6, strategy=Z_RLE) over the same filtered bytes in one stream"""
    crop = _reference(("crop", 128, 128))
    ratio = len(crop.payload) / _rle_size(crop.filtered)
    print("crop 128x128: %d / %d = %.4f" % (len(crop.payload), _rle_size(crop.filtered), ratio))
    assert ratio <= SIZE_RATIO_CROP
    pose = R.encode(np.load(os.path.join(R.GOLD, "pose_maps_fadg0.npz"))["maps"][0])
    ratio = len(pose.payload) / _rle_size(pose.filtered)
    print("pose map 384x512: %d / %d = %.4f" % (len(pose.payload), _rle_size(pose.filtered), ratio))
    assert ratio <= SIZE_RATIO_POSE


def test_library_exports_every_declared_symbol(png_lib):
    from text2video_amd import _pnglib
    header = open(os.path.join(ROOT, "include", "t2v_png.h")).read()
    declared = set(re.findall(r"\b(t2v_png_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_pnglib.SIGNATURES) and len(declared) == 6
    nm = shutil.which("nm")
    assert nm, "`nm` (binutils) is needed to list the symbols of %s" % _pnglib.LIB_PATH
    out = subprocess.run([nm, "-D", "--defined-only", _pnglib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert declared <= exported, declared - exported
    assert png_lib.t2v_png_abi_version() == _pnglib.ABI_VERSION == int(re.search(r"T2V_PNG_ABI_VERSION (\d+)", header).group(1))
    assert (_pnglib.MIN_DIM, _pnglib.MAX_DIM, _pnglib.MAX_IMAGES, _pnglib.BAND_ROWS, _pnglib.OK, _pnglib.ERR_INVALID) == (1, 2048, 1024, 8, 0, -1)
    # the other libraries' headers are as they were
    for other in ("t2v.h", "t2v_jpeg.h"):
        assert "png" not in open(os.path.join(ROOT, "include", other)).read().lower()


def test_geometry_queries_and_capacity_bound(png_lib):
    for H, W in ((1, 1), (2048, 2048), (1, 2048), (512, 320), (9, 5)):
        assert png_lib.t2v_png_supported(H, W) == 1
        assert png_lib.t2v_png_file_capacity(H, W) == R.file_capacity(H, W)
        one, four = png_lib.t2v_png_workspace_bytes(H, W, 1), png_lib.t2v_png_workspace_bytes(H, W, 4)
        assert one >= H * (1 + 3 * W) + R.file_capacity(H, W) - 63 and one % 256 == 0 and one < four <= 4 * one
    for H, W in ((0, 8), (8, 0), (2049, 8), (8, 2049), (0, 0), (-1, 64)):
        assert png_lib.t2v_png_supported(H, W) == 0
        assert png_lib.t2v_png_file_capacity(H, W) == 0 and png_lib.t2v_png_workspace_bytes(H, W, 1) == 0
    assert png_lib.t2v_png_workspace_bytes(64, 64, 0) == 0 and png_lib.t2v_png_workspace_bytes(64, 64, 1025) == 0
    for case in ALL_CASES:
        e = _reference(case)
        assert png_lib.t2v_png_file_capacity(*case[1:]) >= len(e.file)
        assert e.stats["header_bits_max"] <= 2083
    # what the bound is derived from: no literal/length code above 15 bits, no code-length code above 7
    rng = np.random.default_rng(1)
    for _ in range(20):
        counts = (rng.integers(0, 2, 286) * rng.integers(1, 50000, 286) ** rng.integers(0, 2, 286))
        counts[256] = 1
        assert max(R.code_lengths(counts, 15)[0]) <= 15
        small = rng.integers(0, 300, 19) * rng.integers(0, 2, 19)
        small[0] += 1
        assert max(R.code_lengths(small, 7)[0]) <= 7


def test_refused_calls_launch_nothing_and_say_why(png_lib):
    """argument checks come before the first launch, so they can be seen without a GPU"""
    #                    src  cs  H   W  nimg  ws  out  cap  lengths
    for args, word in (((256, 3, 0, 64, 1, 256, 256, 16, 256), b"0x64"), ((256, 3, 64, 0, 1, 256, 256, 16, 256), b"64x0"),
                       ((256, 3, 2049, 64, 1, 256, 256, 16, 256), b"2049x64"), ((256, 3, 64, 2049, 1, 256, 256, 16, 256), b"64x2049"),
                       ((256, 3, 64, 64, 0, 256, 256, 16, 256), b"images"), ((256, 2, 64, 64, 1, 256, 256, 16, 256), b"src_cs"),
                       ((256, 3, 64, 64, 1, None, 256, 16, 256), b"null"), ((256, 3, 64, 64, 1, 257, 256, 16, 256), b"aligned"),
                       ((256, 3, 64, 64, 1, 256, 256, 0, 256), b"out_capacity"), ((None, 3, 64, 64, 1, 256, 256, 16, 256), b"null")):
        assert png_lib.t2v_png_encode_u8(None, *args) == -1 and word in png_lib.t2v_png_last_error(), args


def test_every_kernel_of_the_library_is_claimed(png_lib):
    from text2video_amd import _pnglib
    nm = shutil.which("nm")
    assert nm, "`nm` (binutils) is needed to list the kernels of %s" % _pnglib.LIB_PATH
    out = subprocess.run([nm, "-C", _pnglib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    stubs = [line for line in out.splitlines() if "__device_stub__" in line]
    names = [m.group(1) for m in (re.search(r"__device_stub__(\w+)", line) for line in stubs) if m]
    assert len(names) == len(stubs) > 0, stubs
    assert set(names) == set(KERNELS), (sorted(set(names) - set(KERNELS)), sorted(set(KERNELS) - set(names)))
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_png.py")).read()
    for kernel, test in KERNELS.items():
        assert "def %s(" % test in gpu_tests, (kernel, test)


def test_options():
    from text2video_amd.options import TestOptions
    base = ["--name", "p"]
    assert TestOptions().parse(base).frame_format == "jpg"
    assert TestOptions().parse(base + ["--gpu_jpeg", "--jpeg_quality", "90"]).frame_format == "jpg"
    assert TestOptions().parse(base + ["--frame_format", "png"]).frame_format == "png"
    for bad in (["--frame_format", "png", "--gpu_jpeg"], ["--frame_format", "png", "--jpeg_quality", "90"],
                ["--frame_format", "png", "--gpu_jpeg", "--jpeg_quality", "90"], ["--frame_format", "bmp"],
                ["--frame_format", "png", "--write_video"]):
        with pytest.raises(SystemExit):
            TestOptions().parse(base + bad)


def test_pair_by_stem(tmp_path):
    from text2video_amd.evaluate import pair_files
    a, b = tmp_path / "a", tmp_path / "b"
    for root, names in ((a, ["s/fake_B_0001.png", "s/fake_B_0002.png", "s/fake_B_0003.png", "t/fake_B_0001.png", "s/real_A_0001.png"]),
                        (b, ["s/fake_B_0001.jpg", "s/fake_B_0002.jpg", "s/fake_B_0002.png", "t/fake_B_0009.jpg", "s/fake_B_0003.png"])):
        for n in names:
            os.makedirs(os.path.dirname(root / n), exist_ok=True)
            (root / n).write_bytes(b"")
    # without the flag: by relative path, as always
    assert pair_files(str(a), str(b)) == (["s/fake_B_0002.png", "s/fake_B_0003.png"], ["s/fake_B_0001.png", "t/fake_B_0001.png"],
                                           ["s/fake_B_0001.jpg", "s/fake_B_0002.jpg", "t/fake_B_0009.jpg"])
    pairs, only_a, only_b = pair_files(str(a), str(b), by_stem=True)
    assert pairs == [("s/fake_B_0001.png", "s/fake_B_0001.jpg"), ("s/fake_B_0002.png", "s/fake_B_0002.jpg"),
                     ("s/fake_B_0003.png", "s/fake_B_0003.png")]
    assert only_a == ["t/fake_B_0001.png"] and only_b == ["s/fake_B_0002.png", "t/fake_B_0009.jpg"]
    assert pair_files(str(a), str(b), "real_A_*", by_stem=True) == ([], ["s/real_A_0001.png"], [])


def test_evaluate_takes_the_flag(tmp_path, monkeypatch):
    """main() hands --pair_by_stem to compare_trees; without it the call is the one it always was"""
    from text2video_amd import evaluate
    seen = []

    def fake(*args, **kw):
        seen.append(kw)
        return {"sequences": {}, "overall": {"frames": 1, "psnr": None, "ssim": None, "mae": None}, "unpaired_a": [], "unpaired_b": [],
                "size_mismatch": []}
    monkeypatch.setattr(evaluate, "compare_trees", fake)
    monkeypatch.setenv("T2V_LEAN", "0")
    assert evaluate.main([str(tmp_path), str(tmp_path)]) == 0 and evaluate.main([str(tmp_path), str(tmp_path), "--pair_by_stem"]) == 0
    assert seen == [{}, {"pair_by_stem": True}]


def test_visualizer_names_files_by_the_format(tmp_path):
    """save_bytes takes the extension (default .jpg, as before); a Visualizer built for PNG writes Pillow PNGs from
    save_images (the fallback of --frame_format png for a geometry the encoder refuses)"""
    import types
    from text2video_amd.visualizer import Visualizer
    opt = types.SimpleNamespace(results_dir=str(tmp_path), name="p", phase="test", which_epoch="latest")
    img = R.make_image("mixed", 9, 5)
    blob = R.encode(img).file
    vis = Visualizer(opt, ext=".png")
    a, = vis.save_images({"fake_B": img}, "/x/seq/0001.jpg")
    b, = vis.save_bytes({"real_A": blob}, "/x/seq/0001.jpg", ".png")
    c, = vis.save_bytes({"real_A": b"jpeg bytes"}, "/x/seq/0002.jpg")
    vis.close()
    assert [os.path.basename(p) for p in (a, b, c)] == ["fake_B_0001.png", "real_A_0001.png", "real_A_0002.jpg"]
    assert open(b, "rb").read() == blob and open(c, "rb").read() == b"jpeg bytes"
    im = Image.open(a)
    assert im.format == "PNG" and np.array_equal(np.asarray(im), img)
