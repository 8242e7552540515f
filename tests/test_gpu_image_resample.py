"""t2v_resample_crop_normalize_u8 (ops.resample_crop_normalize_u8) against Pillow: Image.resize(..., BICUBIC) of every
frame, the crop, and the trainer's torch expression (u8.float()/255.0 - 0.5)/0.5 -- bit-equal float32, for every geometry
of tests/resample_reference.py, crops at odd offsets that are no whole tiles and the full frame, both channel layouts,
with the channels the call does not own left alone."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import resample_reference as rr

pytestmark = pytest.mark.gpu
T = 3
SENTINEL = -7.25


@functools.lru_cache(maxsize=None)
def _case(geom):
    """(frames uint8 [T,h,w,3], Pillow's resized frames uint8 [T,h',w',3]): noise, the checkerboard, noise"""
    size, new_size = geom
    a = rr.images(size, new_size, seed=11)
    b = rr.images(size, new_size, seed=12)
    frames = np.stack([a["noise"], a["checker"], b["noise"]])
    want = np.stack([np.asarray(Image.fromarray(f).resize(new_size, Image.BICUBIC)) for f in frames])
    frames.setflags(write=False)
    want.setflags(write=False)
    return frames, want


def _crops(new_size):
    nw, nh = new_size
    small = (min(29, nw - 3), min(19, nh - 5))
    out = [((3, 5), small), ((0, 0), (nw, nh))]
    if nw > 70 and nh > 40:      # more than one block in both directions, ragged last tiles, odd offset
        out.append(((1, 7), (67, 27)))
    return out


@pytest.mark.parametrize("geom", rr.GEOMETRIES, ids=rr.geometry_id)
def test_kernel_equals_pillow_crop_normalize_bitwise(geom, lib_built):
    from text2video_amd import ops
    frames, resized = _case(geom)
    new_size = geom[1]
    src = torch.from_numpy(frames.copy()).cuda()
    for (cx, cy), (cw, ch) in _crops(new_size):
        u8 = torch.from_numpy(resized[:, cy:cy + ch, cx:cx + cw].copy()).cuda()
        want = (u8.float() / 255.0 - 0.5) / 0.5
        for cs, c0 in ((4, 0), (8, 3)):
            out = torch.full((T, ch, cw, cs), SENTINEL, device="cuda")
            got = ops.resample_crop_normalize_u8(src, new_size, (cx, cy), (cw, ch), out=out, c0=c0)
            assert got is out
            what = "crop %dx%d at (%d,%d), cs %d c0 %d" % (cw, ch, cx, cy, cs, c0)
            assert torch.equal(out[..., c0:c0 + 3], want), "%s: %d values differ" % (
                what, int((out[..., c0:c0 + 3] != want).sum()))
            rest = torch.cat([out[..., :c0], out[..., c0 + 3:]], -1)
            assert (rest == SENTINEL).all(), what + ": a channel outside [c0, c0+3) was written"
            again = torch.full((T, ch, cw, cs), SENTINEL, device="cuda")
            ops.resample_crop_normalize_u8(src, new_size, (cx, cy), (cw, ch), out=again, c0=c0)
            assert torch.equal(again, out), what + ": two calls differ"


def test_default_output_has_a_zero_pad_channel(lib_built):
    from text2video_amd import ops
    frames, resized = _case(rr.GEOMETRIES[0])
    nw, nh = rr.GEOMETRIES[0][1]
    out = ops.resample_crop_normalize_u8(torch.from_numpy(frames.copy()).cuda(), (nw, nh), (0, 0), (nw, nh))
    assert out.shape == (T, nh, nw, 4) and (out[..., 3] == 0).all()
    assert torch.equal(out[..., :3], (torch.from_numpy(resized.copy()).cuda().float() / 255.0 - 0.5) / 0.5)


def test_over_limit_downscale_is_refused_and_launches_nothing(lib_built):
    """400 -> 40 columns is 41 taps, over T2V_RESAMPLE_MAX_TAPS = 33: status T2V_ERR_INVALID (-1), the output untouched; 33
    taps (8x) is inside the limit and equals Pillow."""
    from text2video_amd import ops
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (2, 24, 400, 3), dtype=np.uint8)
    src = torch.from_numpy(frames).cuda()
    assert ops.pillow_bicubic_tables(400, 40)[2].shape[1] == 41 > ops.RESAMPLE_MAX_TAPS
    out = torch.full((2, 24, 40, 4), SENTINEL, device="cuda")
    with pytest.raises(RuntimeError, match=r"status -1\).*taps"):
        ops.resample_crop_normalize_u8(src, (40, 24), (0, 0), (40, 24), out=out)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    # both axes at the limit: 400x264 -> 50x33
    frames = rng.integers(0, 256, (1, 264, 400, 3), dtype=np.uint8)
    assert ops.pillow_bicubic_tables(400, 50)[2].shape[1] == ops.pillow_bicubic_tables(264, 33)[2].shape[1] == 33
    want = torch.from_numpy(np.asarray(Image.fromarray(frames[0]).resize((50, 33), Image.BICUBIC)).copy()).cuda()
    got = ops.resample_crop_normalize_u8(torch.from_numpy(frames).cuda(), (50, 33), (0, 0), (50, 33))
    assert torch.equal(got[0, ..., :3], (want.float() / 255.0 - 0.5) / 0.5)


def test_bad_arguments_are_refused(lib_built):
    from text2video_amd import ops
    src = torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="outside"):
        ops.resample_crop_normalize_u8(src, (20, 20), (5, 0), (16, 20), out=torch.zeros(1, 20, 16, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="channel stride"):
        ops.resample_crop_normalize_u8(src, (20, 20), (0, 0), (20, 20), out=torch.zeros(1, 20, 20, 4, device="cuda"), c0=2)
