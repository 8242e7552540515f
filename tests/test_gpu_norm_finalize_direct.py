"""The norm finalize's direct form (launches that pool at most 64 partials per channel: one thread per channel, no LDS)
against the pooled form (T2V_FINALIZE_DIRECT=0), each in a fresh child process, and against float64.

The direct form adds the partials in index order, which is the order the pooled form's 64 slices are added in when every
slice holds at most one partial: the (mean, rstd) tables -- and BatchNorm2d's running statistics where the launch moves
them -- must be the same bits under both settings.  Launches of more than 64 partials stay on the pooled form under both
settings (the 64x132 map: 80 partials; the batch of three 64x64 maps: 96) and are equal trivially; they pin the threshold.
In the parent every table is checked against the float64 mean and biased variance of the conv output it belongs to, within
the tolerance tests/test_gpu_ops.py sets for a finalize (rtol 2e-5, atol 2e-6); a constant map must give mean == the
constant and M2 == 0 exactly.

Partials come from the real producers: the Winograd F(4x4) / F(2x2) output transforms, the direct implicit-GEMM kernel
(partials of BM GEMM rows) and the 7x7 stem kernel (16x16 pixel tiles)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5

CHILD = r'''
import os, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
out_dir = sys.argv[2]
from text2video_amd import ops

dev = torch.device("cuda:0")
results = {}


def rand(*shape, seed, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift).to(dev)


def conv_case(name, H, W, Cin, Cout, k, pad, algo, batch=1, finalize="instance", constant=None, x_cs=None):
    """`batch` images through the producer with stats=, then one finalize launch over all of them"""
    desc = ops.conv_desc(H, W, Cin, Cout, k, 1, pad, ops.PAD_REFLECT, algo=algo)
    x_cs = Cin if x_cs is None else x_cs
    if algo:
        assert ops.winograd_supported(desc, x_cs), name
    w = rand(Cout, Cin, k, k, seed=7, scale=0.1)
    b = rand(Cout, seed=8, scale=0.5)
    if constant is not None:
        w.zero_()
        b.fill_(constant)
    pw = ops.pack_conv_weight(w, desc, x_cs)
    n = ops.conv_stats_buffer(desc, dev).numel()
    stats = torch.full((batch * n,), float("nan"), device=dev)   # what no partial covers is never read
    ys = []
    for i in range(batch):
        x = torch.zeros(H, W, x_cs, device=dev)
        x[..., :Cin] = rand(H, W, Cin, seed=20 + i, shift=0.3 * (i + 1))
        st = stats[i * n:(i + 1) * n]
        ys.append(ops.conv2d_winograd(x, pw, b, desc, stats=st) if algo else ops.conv2d(x, pw, b, desc, y_cs=Cout, stats=st))
    results[name + ".y"] = torch.stack(ys).cpu().numpy()
    if finalize == "instance":
        mr = ops.instance_norm_finalize(stats, desc, EPS)
    elif finalize == "batch":
        mr = ops.batch_norm_finalize(stats, desc, batch, EPS)
    else:   # the running= form: BatchNorm2d's running statistics moved twice in the same launch
        rm, rv = rand(Cout, seed=9, scale=0.2), rand(Cout, seed=10, scale=0.1).abs() + 0.5
        mr = ops.batch_norm_finalize(stats, desc, batch, EPS, running=(rm, rv, 0.1, 2)) if batch > 1 else \
            ops.instance_norm_finalize(stats, desc, EPS, running=(rm, rv, 0.1, 2))
        results[name + ".running"] = torch.stack([rm, rv]).cpu().numpy()
    results[name + ".mr"] = mr.view(-1, 2).cpu().numpy()


EPS = 1e-5
F2, F4 = ops.ALGO_WINOGRAD, ops.ALGO_WINOGRAD_F4
conv_case("f4_padded_8x8", 8, 8, 32, 32, 3, 1, F4)                     # 4 real tiles padded to 128: trailing empty partials
conv_case("f4_ragged_9x7", 9, 7, 32, 32, 3, 1, F4)                     # per-partial pixel counts
conv_case("f4_64x128_64_partials", 64, 128, 32, 32, 3, 1, F4)          # exactly 64: the last size of the direct form
conv_case("f4_64x132_80_partials", 64, 132, 32, 32, 3, 1, F4)          # pooled under both settings
conv_case("f2_16x16", 16, 16, 32, 32, 3, 1, F2)
conv_case("direct3x3_32x32", 32, 32, 32, 32, 3, 1, 0)                  # whole partials of BM rows
conv_case("direct3x3_30x30", 30, 30, 32, 32, 3, 1, 0)                  # 900 rows: a short last partial
conv_case("stem7x7_40x24", 40, 24, 6, 64, 7, 3, 0, x_cs=8)             # 16x16 pixel tiles, ragged right and bottom
conv_case("f4_64x64_batch2", 64, 64, 32, 32, 3, 1, F4, batch=2, finalize="batch")     # 2 x 32 partials: direct
conv_case("f4_64x64_batch3", 64, 64, 32, 32, 3, 1, F4, batch=3, finalize="batch")     # 96 partials: pooled
conv_case("f4_64x64_running", 64, 64, 32, 32, 3, 1, F4, finalize="running")
conv_case("f4_9x7_batch2_running", 9, 7, 32, 32, 3, 1, F4, batch=2, finalize="running")
conv_case("f4_16x16_cout36", 16, 16, 32, 36, 3, 1, F4)                 # channels: no multiple of 16 or 64
conv_case("direct3x3_30x30_cout36", 30, 30, 32, 36, 3, 1, 0)
conv_case("f4_constant_9x7", 9, 7, 32, 32, 3, 1, F4, constant=0.7)
conv_case("direct3x3_constant_30x30", 30, 30, 32, 32, 3, 1, 0, constant=-1.3)
torch.cuda.synchronize()
ops.check_async_errors()
np.savez(os.path.join(out_dir, "outputs.npz"), **results)
print("child ok: %d arrays" % len(results))
'''


def _run_child(tmp_path, name, direct_env):
    out = tmp_path / name
    out.mkdir()
    script = tmp_path / (name + "_child.py")
    script.write_text(CHILD)
    env = {k: v for k, v in os.environ.items() if k != "T2V_FINALIZE_DIRECT"}
    if direct_env is not None:
        env["T2V_FINALIZE_DIRECT"] = direct_env
    p = subprocess.run([sys.executable, str(script), ROOT, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "child %s failed (%d):\n%s\n%s" % (name, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return dict(np.load(str(out / "outputs.npz")))


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("finalize_direct")
    return _run_child(tmp, "direct", None), _run_child(tmp, "pooled", "0")


def test_direct_form_is_bit_identical_to_the_pooled_form(twins):
    direct, pooled = twins
    assert sorted(direct) == sorted(pooled)
    tables = [k for k in sorted(direct) if k.endswith(".mr") or k.endswith(".running")]
    assert len([k for k in tables if k.endswith(".mr")]) == 16 and len([k for k in tables if k.endswith(".running")]) == 2
    for k in tables:
        a, b = direct[k], pooled[k]
        assert a.shape == b.shape and a.dtype == np.float32 and np.isfinite(a).all(), k
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "%s: %d values differ, max |d| %.3g" % (
            k, (a.view(np.int32) != b.view(np.int32)).sum(), np.abs(a - b).max())
    for k in sorted(direct):
        if k.endswith(".y"):   # the producers do not depend on the switch
            assert np.array_equal(direct[k].view(np.int32), pooled[k].view(np.int32)), k


def test_tables_against_float64_of_the_conv_output(twins):
    for tables in twins:
        for k in sorted(tables):
            if not k.endswith(".mr"):
                continue
            y = tables[k[:-3] + ".y"].astype(np.float64)   # [batch, H, W, C]
            mr = tables[k]
            assert mr.shape == (y.shape[-1], 2), k
            mean = y.mean(axis=(0, 1, 2))
            var = ((y - mean) ** 2).mean(axis=(0, 1, 2))
            want = np.stack([mean, 1.0 / np.sqrt(var + EPS)], 1)
            err = np.abs(mr - want)
            print("%s: max |mean - f64| %.3g, max |rstd - f64| / rstd %.3g" % (k, err[:, 0].max(), (err[:, 1] / want[:, 1]).max()))
            assert np.allclose(mr, want, rtol=2e-5, atol=2e-6), (k, err.max())


def test_constant_map_gives_its_value_and_zero_variance(twins):
    for tables in twins:
        for name, value in (("f4_constant_9x7", 0.7), ("direct3x3_constant_30x30", -1.3)):
            y, mr = tables[name + ".y"], tables[name + ".mr"]
            assert (y == np.float32(value)).all(), name
            assert (mr[:, 0] == np.float32(value)).all(), (name, mr[:, 0])                               # mean == ref exactly
            assert (mr[:, 1] == np.float32(1.0) / np.sqrt(np.float32(EPS), dtype=np.float32)).all(), (name, mr[:, 1])   # M2 == 0
