"""tests/finalize_reference.py on the CPU: its pooled-moment formula is the mean and biased variance of the map, and the
checks of tests/test_gpu_norm_finalize_grouped.py can see the faults the grouped finalize can have.

In float64, on the data the GPU test feeds (a component that is constant inside each finalize group and steps by one
standard deviation between groups), each fault moves mean or rstd of some channel by >= 10x the tolerance (measured: 2.9e3x
for the pixel count, 1.5e5x .. 4.3e5x for the others).

On plain random data a dropped or doubled group moves the tables by the sampling error of a group mean only, sigma /
sqrt(pixels per group) = sigma / 256 on a 512 x 512 map: about 200 times less than on the striped data, and less the larger
the map.  That is the reason for the stripes.  It is NOT inside this tolerance, though (rtol 2e-5, atol 2e-6 is tight: 700x
.. 1400x of it, measured), so the test asserts the ratio between the two kinds of data, not that random data hides the
fault; the figures of all faults are printed."""
import numpy as np
import pytest

import finalize_reference as fr

C = 20           # two channel blocks of 16, the second ragged; groups() gives G = 4 at 2048 partials as for 32 channels


def _map(H, W, striped, batch=1, seed=1):
    part, npi = fr.partial_map(H, W)
    gmap, G = fr.group_map(part, npi, batch, C)
    y = np.random.default_rng(seed).standard_normal((batch, H, W, C))
    if striped:
        y = y + fr.stripes(gmap, G, C)
    return y, part, npi, G


def _worst(y, part, npi, G, fault):
    """max over channels of |fault - ref| / tolerance, for mean and rstd"""
    mean, m2, n = fr.partials64(y, part, npi)
    ref = fr.pooled64(mean, m2, n, G)
    bad = fr.pooled64(mean, m2, n, G, fault)
    return max(float((np.abs(b - r) / fr.tolerance(r)).max()) for r, b in zip(ref, bad))


def test_groups_rule_and_partial_geometry():
    assert fr.groups(2047, 32) == 1 and fr.groups(2048, 32) == 4 and fr.groups(2080, 36) == 4 and fr.groups(4096, 32) == 8
    assert fr.groups(1 << 20, 16) == 64 and fr.groups(1 << 20, 1024) == 8
    for (H, W), want in (((512, 512), 2048), ((512, 520), 2080), ((510, 509), 2048), ((256, 512), 1024)):
        part, npi = fr.partial_map(H, W)
        assert npi == want and part.max() < npi, (H, W, npi)
    part, npi = fr.partial_map(512, 512, BM=128)
    assert npi == 2048 and (np.bincount(part.reshape(-1)) == 128).all()
    # at W = 512 with F(4x4), 64 partials are 16 pixel rows: the groups are stripes of 16 rows
    gmap, G = fr.group_map(fr.partial_map(512, 512)[0], 2048, 1, 32)
    assert G == 4 and (gmap[0] == ((np.arange(512) // 16) % 4)[:, None]).all()
    # ragged: partials of fewer than 128 pixels
    part, npi = fr.partial_map(510, 509)
    counts = np.bincount(part.reshape(-1), minlength=npi)
    assert counts.min() < 128 and counts.max() == 128 and counts.sum() == 510 * 509


@pytest.mark.parametrize("H,W,batch", [(512, 512, 1), (510, 509, 1), (256, 512, 4)])
def test_pooled_formula_is_the_mean_and_biased_variance(H, W, batch):
    y, part, npi, G = _map(H, W, True, batch)
    mean, rstd = fr.pooled64(*fr.partials64(y, part, npi), G)
    flat = y.reshape(-1, C)
    assert np.allclose(mean, flat.mean(0), rtol=0, atol=1e-12)
    assert np.allclose(rstd, 1.0 / np.sqrt(flat.var(0) + fr.EPS), rtol=1e-12, atol=0)


def test_faults_move_the_tables_on_striped_data_far_more_than_on_random_data():
    lines, seen = [], {}
    for H, W in ((512, 512), (510, 509)):
        for fault in fr.FAULTS:
            if fault == "pixel count taken as uniform" and H % 4 == 0:
                continue                                      # whole tiles: every partial does hold 128 pixels
            y, part, npi, G = _map(H, W, True)
            striped = _worst(y, part, npi, G, fault)
            y, part, npi, G = _map(H, W, False)
            plain = _worst(y, part, npi, G, fault)
            lines.append("%dx%d %-32s |fault - ref| / tolerance: striped %9.3g, plain random %9.3g" % (H, W, fault, striped, plain))
            seen[(H, fault)] = (striped, plain)
    print("\n".join(lines))
    for key, (striped, plain) in seen.items():
        assert striped >= 10.0, (key, striped)
        if "group" in key[1]:
            # a step of sigma between groups against a sampling error of sigma / sqrt(512 * 512 / 4) = sigma / 256
            assert striped >= 50.0 * plain, (key, striped, plain)
    assert len(seen) == 7
