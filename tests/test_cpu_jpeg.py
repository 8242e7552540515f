"""CPU tests of the JPEG writer's contract (include/t2v_jpeg.h):

* the numpy restatement (tests/jpeg_reference.py) and jpeg.header() against the bytes the installed Pillow writes, on the
  cases both test files share -- a Pillow that writes other bytes is reported as such, with its version;
* the Annex K tables of text2video_amd/jpeg.py against the DQT / DHT segments of a Pillow file;
* the coverage condition: the cases make the reference emit every rule of the format, asserted from its symbol stream;
* libt2v_jpeg.so builds, exports every symbol of t2v_jpeg.h, bounds every case's scan; the two options parse;
* the library's own kernel ledger: every kernel stub `nm -C` lists is named here next to the GPU test that checks it.
"""
import io
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import PIL
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_reference as R  # noqa: E402

from text2video_amd import jpeg as J  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every kernel of libt2v_jpeg.so -> the test of tests/test_gpu_jpeg.py that checks its output (all six encode kernels run in
# every encode call; the test named is the one whose cases single the kernel out)
KERNELS = {
    "jpeg_mcu_kernel": "test_file_equals_the_restatement_and_pillow",           # edges, dummy blocks, every quality
    "jpeg_block_bits_kernel": "test_file_equals_the_restatement_and_pillow",    # ZRL, EOB, no EOB, categories 10 / 9
    "jpeg_scan_kernel": "test_a_batch_equals_the_single_calls_and_two_runs_agree",
    "jpeg_block_pack_kernel": "test_file_equals_the_restatement_and_pillow",
    "jpeg_ff_count_kernel": "test_file_equals_the_restatement_and_pillow",      # 114 stuffed bytes in one scan
    "jpeg_stuff_kernel": "test_capacity_guard",
    "jpeg_stage_u8_kernel": "test_stage_copies_through_the_byte_map",
}


def _pillow_file(case):
    kind, H, W, q = case
    buf = io.BytesIO()
    Image.fromarray(R.make_image(kind, H, W)).save(buf, format="JPEG", quality=q)
    return buf.getvalue()


_encoded = {}


def _reference(case):
    if case not in _encoded:
        kind, H, W, q = case
        _encoded[case] = R.encode(R.make_image(kind, H, W), q)
    return _encoded[case]


def _segments(blob):
    """[(marker, payload)] up to and including SOS; + the offset of the scan"""
    out, i = [], 2
    assert blob[:2] == J.SOI
    while True:
        assert blob[i] == 0xFF
        marker, length = blob[i + 1], int.from_bytes(blob[i + 2:i + 4], "big")
        out.append((marker, blob[i + 4:i + 2 + length]))
        i += 2 + length
        if marker == 0xDA:
            return out, i


@pytest.fixture(scope="module")
def jpeg_lib():
    from text2video_amd import _jpeglib
    if not os.path.exists(_jpeglib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _jpeglib.load()


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_and_header_equal_pillow(case):
    kind, H, W, q = case
    want = _pillow_file(case)
    got = _reference(case)
    _, scan_at = _segments(want)
    note = "Pillow %s writes other bytes than the contract of DESIGN.md section 4.10 for %s" % (PIL.__version__, R.case_id(case))
    assert scan_at == 623 and J.header(H, W, q) == want[:scan_at], note + " (before the scan)"
    assert got.file == want, note + " (%d bytes, the restatement %d)" % (len(want), len(got.file))
    assert got.file == J.file_bytes(J.header(H, W, q), got.scan) and want[-2:] == J.EOI
    # a fourth channel is ignored
    assert R.encode(R.make_image(kind, H, W, 4), q).file == got.file


def test_tables_are_the_ones_pillow_writes():
    for q in (30, 75, 100):
        segs, _ = _segments(_pillow_file(("noise", 16, 16, q)))
        assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
        dqt = [p for m, p in segs if m == 0xDB]
        for i, table in enumerate(J.quant_tables(q)):
            assert dqt[i][0] == i and list(dqt[i][1:]) == [int(v) for v in table[J.ZIGZAG]]
        dht = [p for m, p in segs if m == 0xC4]
        for (tc_th, (bits, vals)), p in zip(J.HUFFMAN_TABLES, dht):
            assert p[0] == tc_th and tuple(p[1:17]) == tuple(bits) and p[17:] == vals and sum(bits) == len(vals)
    assert sorted(J.ZIGZAG.tolist()) == list(range(64))
    with pytest.raises(ValueError):
        J.quant_tables(0)
    with pytest.raises(ValueError):
        J.quant_tables(101)


def test_cases_reach_every_rule():
    """from the reference's symbol stream: what the GPU test's byte equality is evidence of"""
    stats = {c: _reference(c).stats for c in R.CASES}

    def some(key, least=1):
        return [c for c in R.CASES if stats[c][key] >= least]
    assert some("zrl") and some("eob") and some("no_eob") and some("stuffed")
    assert some("dummy_right") and some("dummy_bottom") and some("dummy_corner")
    assert some("ac_category_max", 10) and some("dc_category_max", 9)
    assert any(W % 2 for _, H, W, _ in R.CASES) and any(H % 2 for _, H, W, _ in R.CASES)
    assert any(2 <= H % 16 <= 8 for _, H, W, _ in R.CASES)
    # the figures of the feasibility run, at their cases
    assert stats[("smooth", 64, 88, 90)]["zrl"] and stats[("noise", 32, 48, 30)]["zrl"]
    assert stats[("checker", 48, 32, 100)]["ac_category_max"] == 10 and stats[("checker", 48, 32, 100)]["stuffed"] > 100
    assert stats[("edges", 33, 31, 90)]["dc_category_max"] >= 9
    assert stats[("noise", 40, 56, 100)]["no_eob"] > 50
    # down-sampled rows are replicated, not full-resolution rows: at H % 16 in 2..8 the other rule gives other bytes
    kind, H, W, q = ("smooth", 24, 40, 75)
    img = R.make_image(kind, H, W)
    padded = np.pad(img, ((0, 32 - H), (0, 0), (0, 0)), mode="edge")
    assert R.encode(padded, q).scan != _reference((kind, H, W, q)).scan


def test_library_exports_every_declared_symbol(jpeg_lib):
    from text2video_amd import _jpeglib
    header = open(os.path.join(ROOT, "include", "t2v_jpeg.h")).read()
    declared = set(re.findall(r"\b(t2v_jpeg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_jpeglib.SIGNATURES) and len(declared) >= 6
    nm = shutil.which("nm")
    assert nm, "`nm` (binutils) is needed to list the symbols of %s" % _jpeglib.LIB_PATH
    out = subprocess.run([nm, "-D", "--defined-only", _jpeglib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert declared <= exported, declared - exported
    assert jpeg_lib.t2v_jpeg_abi_version() == _jpeglib.ABI_VERSION == int(re.search(r"T2V_JPEG_ABI_VERSION (\d+)", header).group(1))
    # the generator library and its header are as they were
    assert "jpeg" not in open(os.path.join(ROOT, "include", "t2v.h")).read().lower()


def test_geometry_queries_and_capacity_bound(jpeg_lib):
    for H, W in ((8, 8), (2048, 2048), (8, 2048), (512, 320)):
        assert jpeg_lib.t2v_jpeg_supported(H, W) == 1
        mcus = ((H + 15) // 16) * ((W + 15) // 16)
        assert jpeg_lib.t2v_jpeg_scan_capacity(H, W) == 6 * mcus * 416
        one, four = jpeg_lib.t2v_jpeg_workspace_bytes(H, W, 1), jpeg_lib.t2v_jpeg_workspace_bytes(H, W, 4)
        assert one >= 6 * mcus * (128 + 8 + 208) and one % 256 == 0 and one < four <= 4 * one
    for H, W in ((7, 8), (8, 7), (2049, 8), (8, 2049), (0, 0), (-1, 64)):
        assert jpeg_lib.t2v_jpeg_supported(H, W) == 0
        assert jpeg_lib.t2v_jpeg_scan_capacity(H, W) == 0 and jpeg_lib.t2v_jpeg_workspace_bytes(H, W, 1) == 0
    assert jpeg_lib.t2v_jpeg_workspace_bytes(64, 64, 0) == 0 and jpeg_lib.t2v_jpeg_workspace_bytes(64, 64, 1025) == 0
    for case in R.CASES:
        _, H, W, _ = case
        assert jpeg_lib.t2v_jpeg_scan_capacity(H, W) >= len(_reference(case).scan)
    # the longest code words the bound is derived from (include/t2v_jpeg.h)
    assert max(R.DC_TABLES[1][c][1] + c for c in range(12)) == 22 and max(R.DC_TABLES[0][c][1] + c for c in range(12)) <= 22
    assert max(length + (sym & 15) for t in R.AC_TABLES for sym, (_, length) in t.items()) == 26


def test_refused_calls_launch_nothing_and_say_why(jpeg_lib):
    """argument checks come before the first launch, so they can be seen without a GPU"""
    st = jpeg_lib.t2v_jpeg_encode_u8(None, 256, 3, 7, 64, 1, 75, 256, 256, 16, 256)
    assert st == -1 and b"7x64" in jpeg_lib.t2v_jpeg_last_error()
    for args, word in (((256, 5, 64, 64, 1, 75, 256, 256, 16, 256), b"src_cs"), ((256, 3, 64, 64, 0, 75, 256, 256, 16, 256), b"images"),
                       ((256, 3, 64, 64, 1, 101, 256, 256, 16, 256), b"quality"), ((256, 3, 64, 64, 1, 75, 257, 256, 16, 256), b"aligned"),
                       ((256, 3, 64, 64, 1, 75, 256, 256, 0, 256), b"out_capacity"), ((None, 3, 64, 64, 1, 75, 256, 256, 16, 256), b"null")):
        assert jpeg_lib.t2v_jpeg_encode_u8(None, *args) == -1 and word in jpeg_lib.t2v_jpeg_last_error(), args
    assert jpeg_lib.t2v_jpeg_stage_u8(None, 256, 2, 256, 4, 10, None) == -1 and b"channel" in jpeg_lib.t2v_jpeg_last_error()


def test_options():
    from text2video_amd.options import TestOptions
    base = ["--name", "p"]
    opt = TestOptions().parse(base)
    assert opt.gpu_jpeg is False and opt.jpeg_quality is None
    opt = TestOptions().parse(base + ["--gpu_jpeg"])
    assert opt.gpu_jpeg is True and opt.jpeg_quality is None          # run_test takes 75, Pillow's default
    assert TestOptions().parse(base + ["--gpu_jpeg", "--jpeg_quality", "90"]).jpeg_quality == 90
    for bad in (["--jpeg_quality", "90"], ["--gpu_jpeg", "--jpeg_quality", "0"], ["--gpu_jpeg", "--jpeg_quality", "101"]):
        with pytest.raises(SystemExit):
            TestOptions().parse(base + bad)


def test_every_kernel_of_the_library_is_claimed(jpeg_lib):
    from text2video_amd import _jpeglib
    nm = shutil.which("nm")
    assert nm, "`nm` (binutils) is needed to list the kernels of %s" % _jpeglib.LIB_PATH
    out = subprocess.run([nm, "-C", _jpeglib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    stubs = [line for line in out.splitlines() if "__device_stub__" in line]
    names = [m.group(1) for m in (re.search(r"__device_stub__(\w+)", line) for line in stubs) if m]
    assert len(names) == len(stubs) > 0, stubs
    assert not set(names) - set(KERNELS), "kernels of libt2v_jpeg.so no entry of KERNELS claims: %s" % sorted(set(names) - set(KERNELS))
    assert not set(KERNELS) - set(names), "KERNELS entries with no such kernel: %s" % sorted(set(KERNELS) - set(names))
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_jpeg.py")).read()
    for kernel, test in KERNELS.items():
        assert "def %s(" % test in gpu_tests, (kernel, test)


def test_visualizer_writes_encoded_files_as_they_are_and_pillow_files_as_before(tmp_path):
    """save_bytes: the writer threads only write; save_images without a quality is the call it always was, with one it is
    Pillow at that quality (the fallback of --gpu_jpeg for a geometry the encoder refuses)"""
    import types
    from text2video_amd.visualizer import Visualizer
    opt = types.SimpleNamespace(results_dir=str(tmp_path), name="p", phase="test", which_epoch="latest")
    img = R.make_image("smooth", 24, 40)
    blob = R.encode(img, 75).file

    def pillow(**kw):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", **kw)
        return buf.getvalue()
    for quality, want in ((None, pillow()), (75, pillow()), (90, pillow(quality=90))):
        vis = Visualizer(opt, quality=quality)
        a, = vis.save_images({"fake_B": img}, "/x/seq/0001.jpg")
        b, = vis.save_bytes({"real_A": blob}, "/x/seq/0001.jpg")
        vis.close()
        assert (os.path.basename(a), os.path.basename(b)) == ("fake_B_0001.jpg", "real_A_0001.jpg")
        assert open(a, "rb").read() == want and open(b, "rb").read() == blob
    assert pillow() == blob != pillow(quality=90)
