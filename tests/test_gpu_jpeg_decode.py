"""GPU tests of the JPEG decoder (libt2v_jpegdec.so, ops.jpeg_decode_u8, jpeg_decode.decode_files): the kernels' pixels against
Pillow's Image.open(...).convert("RGB"), byte for byte, at the smallest shapes at which each stage can go wrong (the cases of
tests/jpeg_decode_reference.py, which tests/test_cpu_jpeg_decode.py shows to converge within the library's rounds, so that
nothing here hides behind the Pillow fallback); batches with their own tables, the two status bits with exact neighbours,
and repeatability."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_reference as D  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(lib_built):
    import torch
    from text2video_amd import _jpegdeclib, ops
    if not os.path.exists(_jpegdeclib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _jpegdeclib.load()
    ops.context(0)
    return torch.device("cuda:0")


def gpu_decode(blobs, dev, cs=3, cut=None, poison=0x5A):
    """the files of ONE geometry through one ops.jpeg_decode_u8 call -> (uint8 [n,H,W,cs], [status]); no fallback.
    cut = (j, length): file j's scan length as the call sees it (the bytes stay in the buffer)"""
    import torch
    from text2video_amd import jpeg_decode
    groups, refused = jpeg_decode.pack(blobs)
    assert not refused and len(groups) == 1, (refused, len(groups))
    g, = groups
    assert g.index == list(range(len(blobs)))
    if cut is not None:
        g.lengths()[cut[0]] = cut[1]
    dst = torch.full((g.n, g.H, g.W, cs), poison, dtype=torch.uint8, device=dev)
    dst, status = jpeg_decode.upload_and_decode(g, dev, cs, dst=dst)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), status.cpu().tolist()


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_pixels_equal_pillow(dev, case):
    blob = D.pillow_file(case)
    got, status = gpu_decode([blob], dev)
    want = D.pillow_rgb(blob)
    assert status == [0]
    assert got.shape[1:] == want.shape
    assert int((got[0] != want).sum()) == 0, "%s: %d of %d bytes differ, first at %s" % (
        D.case_id(case), (got[0] != want).sum(), want.size, np.argwhere(got[0] != want)[0].tolist())


@pytest.mark.parametrize("cs", [3, 4])
def test_a_batch_with_its_own_tables_and_lengths(dev, cs):
    """three files of one geometry, different quality and optimize: three table blobs, three lengths, one call"""
    blobs = [D.pillow_file(c) for c in D.BATCH]
    assert len({len(b) for b in blobs}) == 3
    got, status = gpu_decode(blobs, dev, cs)
    assert status == [0, 0, 0]
    for j, blob in enumerate(blobs):
        assert np.array_equal(got[j, ..., :3], D.pillow_rgb(blob)), j
    if cs == 4:
        assert (got[..., 3] == 0).all()


def test_a_member_that_does_not_synchronise_reports_it_and_the_neighbours_are_exact(dev):
    from text2video_amd import _jpegdeclib, jpeg_decode
    blobs = [D.pillow_file(c) for c in D.BATCH_FALLBACK]
    got, status = gpu_decode(blobs, dev)
    assert status[0] == 0 and status[2] == 0 and status[1] & _jpegdeclib.NOT_CONVERGED
    for j in (0, 2):
        assert np.array_equal(got[j], D.pillow_rgb(blobs[j])), j
    tensors, fallback = jpeg_decode.decode_files(blobs, dev)
    assert [i for i, _ in fallback] == [1] and "synchronise" in fallback[0][1]
    for j, blob in enumerate(blobs):
        assert np.array_equal(tensors[j].cpu().numpy(), D.pillow_rgb(blob)), j


def test_decode_files_groups_geometries_and_hands_refused_files_to_pillow(dev):
    """two geometries, a progressive file and a grey one between them: the order of the result is the order of the files"""
    import io
    from PIL import Image
    from text2video_amd import jpeg_decode
    prog, grey = io.BytesIO(), io.BytesIO()
    img = D.make_image("smooth", 24, 40)
    Image.fromarray(img).save(prog, format="JPEG", progressive=True)
    Image.fromarray(img).convert("L").save(grey, format="JPEG")
    blobs = [D.pillow_file(D.BATCH[0]), prog.getvalue(), D.pillow_file(D.CASES[6]), grey.getvalue(), D.pillow_file(D.BATCH[1])]
    for cs in (3, 4):
        tensors, fallback = jpeg_decode.decode_files(blobs, dev, out_cs=cs)
        assert [i for i, _ in fallback] == [1, 3] and "progressive" in fallback[0][1]
        for j, blob in enumerate(blobs):
            got = tensors[j].cpu().numpy()
            assert np.array_equal(got[..., :3], D.pillow_rgb(blob)) and (cs == 3 or (got[..., 3] == 0).all()), j


def test_a_scan_cut_in_half_reports_corrupt_and_the_neighbours_are_exact(dev):
    """the length is halved, the buffer keeps its capacity and its bytes: the decoder must stop at the length"""
    from text2video_amd import _jpegdeclib, jpeg
    blobs = [D.pillow_file(c) for c in D.BATCH]
    half = jpeg.parse(blobs[1]).scan_length // 2
    got, status = gpu_decode(blobs, dev, cut=(1, half))
    assert status[0] == 0 and status[2] == 0 and status[1] & _jpegdeclib.CORRUPT
    for j in (0, 2):
        assert np.array_equal(got[j], D.pillow_rgb(blobs[j])), j
    # a length beyond the capacity is taken as the capacity and reported
    got, status = gpu_decode(blobs, dev, cut=(2, 1 << 30))
    assert status[0] == 0 and status[1] == 0 and status[2] & _jpegdeclib.CORRUPT
    for j in (0, 1):
        assert np.array_equal(got[j], D.pillow_rgb(blobs[j])), j


def test_a_second_identical_call_gives_identical_bytes(dev):
    blobs = [D.pillow_file(("pose", 160, 96, 75, 2, False)), D.pillow_file(("smooth", 160, 96, 95, 2, False))]
    a, sa = gpu_decode(blobs, dev, poison=0x00)
    b, sb = gpu_decode(blobs, dev, poison=0xFF)
    assert sa == sb == [0, 0] and np.array_equal(a, b)
