"""ops.pillow_bicubic_tables against the installed Pillow: the two-pass integer rule of t2v_resample_crop_normalize_u8,
restated in numpy (tests/resample_reference.py) and driven by the host tables, gives Image.resize(..., BICUBIC)'s bytes."""
import numpy as np
import pytest
from PIL import Image

import resample_reference as rr


@pytest.mark.parametrize("geom", rr.GEOMETRIES, ids=rr.geometry_id)
def test_tables_reproduce_pillow_bicubic_bytes(geom):
    from text2video_amd import ops
    size, new_size = geom
    for name, img in rr.images(size, new_size, seed=size[0] * 1000 + new_size[0]).items():
        want = np.asarray(Image.fromarray(img).resize(new_size, Image.BICUBIC))
        got = rr.resize_u8(img, new_size, ops.pillow_bicubic_tables)
        assert got.shape == want.shape == (new_size[1], new_size[0], 3)
        assert np.array_equal(got, want), "%s: %d bytes differ, max |delta| %d" % (
            name, int((got != want).sum()), int(np.abs(got.astype(int) - want.astype(int)).max()))
        if name == "checker":
            assert want.min() == 0 and want.max() == 255        # the saturation was exercised at both ends


def test_table_shapes_and_identity():
    from text2video_amd import ops
    first, count, coef = ops.pillow_bicubic_tables(40, 40)
    assert coef.shape == (40, 1) and (coef == 1 << 22).all() and (count == 1).all() and (first == np.arange(40)).all()
    for n_in, n_out, ksize in ((61, 24, 13), (47, 20, 11),(130, 33, 17), (90, 23, 17), (19, 76, 5)):
        first, count, coef = ops.pillow_bicubic_tables(n_in, n_out)
        assert coef.shape == (n_out, ksize) and coef.dtype == first.dtype == count.dtype == np.int32
        assert (first >= 0).all() and (first + count <= n_in).all() and (count >= 1).all() and (count <= ksize).all()
        assert (np.diff(first) >= 0).all()
        assert (np.abs(coef.sum(1) - (1 << 22)) <= ksize).all()       # normalised weights, each rounded once
        assert all((coef[i, count[i]:] == 0).all() for i in range(n_out))
