"""The norm finalize's grouped form: a launch that pools >= 2048 partials and is given a scratch buffer runs
inorm_finalize_kernel with one block row per group and then inorm_finalize_merge_kernel (csrc/elementwise.hip).  Reached
through the scratch= argument of ops.instance_norm_finalize / ops.batch_norm_finalize (t2v_batch_norm_finalize_scratch).

Partials come from the real producers (the F(4x4) output transform, the direct implicit-GEMM kernel).  Per case: the
profiler shows the merge kernel; the tables are the float64 mean and biased variance of the conv output actually
produced, within tests/test_gpu_norm_finalize_direct.py's tolerance (rtol 2e-5, atol 2e-6); the same partials finalized
without a scratch buffer give tables within 2 fp32 ulp (mean) / 3 ulp (rstd: one more fp32 step) -- both are fp64 sums in
different orders, rounded once; a constant map gives mean == the constant and rstd == 1 / sqrtf(eps) exactly.

The input carries a component that is constant inside each finalize group and steps by one standard deviation between
groups (tests/finalize_reference.py derives the groups from the geometry): a group that is dropped, counted twice or read
from the wrong scratch row then moves the tables by >= 1e3 x the tolerance (tests/test_cpu_norm_finalize_grouped.py)."""
import numpy as np
import pytest
import torch

import finalize_reference as fr
import kernel_variants as kv

pytestmark = pytest.mark.gpu
EPS = fr.EPS

# name: H, W, Cout, algo ("F4" | "direct"), batch, running statistics moved in the launch, pooled partials, groups
CASES = {
    "f4_512x512": (512, 512, 32, "F4", 1, False, 2048, 4),                  # whole groups
    "f4_512x520_cout36": (512, 520, 36, "F4", 1, False, 2080, 4),           # ragged groups, ragged channel blocks
    "f4_510x509": (510, 509, 32, "F4", 1, False, 2048, 4),                  # per-partial pixel counts inside groups
    "f4_256x512_batch4_running": (256, 512, 32, "F4", 4, True, 4096, 8),    # G = 8; running_update by the merge kernel
    "direct3x3_512x512": (512, 512, 32, "direct", 1, False, None, None),    # conv-kernel partials of BM rows
}
CIN = 32


def _dev():
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return torch.device("cuda:0")


def _profiled(fn):
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, {kv.normalise(e.name) for e in prof.events() if "t2v::" in e.name}


def _geometry(ops, desc, H, W, Cout, algo, dev):
    """(partial of every output pixel, partials per image) of this producer"""
    per_image = ops.conv_stats_buffer(desc, dev).numel() // (2 * Cout)
    if algo == "F4":
        part, npi = fr.partial_map(H, W)
    else:
        bms = [bm for bm in (64, 128, 256) if -(-H * W // bm) == per_image]
        assert len(bms) == 1, (per_image, bms)
        part, npi = fr.partial_map(H, W, BM=bms[0])
    assert npi == per_image, (npi, per_image)
    return part, npi


def _run_case(name):
    from text2video_amd import ops
    dev = _dev()
    H, W, Cout, algo, batch, running, nparts_want, G_want = CASES[name]
    mk = lambda h: ops.conv_desc(h, W, CIN, Cout, 3, 1, 1, ops.PAD_REFLECT, algo=ops.ALGO_WINOGRAD_F4 if algo == "F4" else 0)
    desc = mk(H)
    if algo == "direct":
        # 2048 partials if the plan's BM is 128; otherwise the smallest map (whole rows) that gives >= 2048
        per = ops.conv_stats_buffer(desc, dev).numel() // (2 * Cout)
        if per < 2048:
            H = -(-2048 * (H * W // per) // W)
            desc = mk(H)
    else:
        assert ops.winograd_supported(desc, CIN), name
    part, npi = _geometry(ops, desc, H, W, Cout, algo, dev)
    gmap, G = fr.group_map(part, npi, batch, Cout)
    assert batch * npi >= 2048 and G > 1
    if nparts_want is not None:
        assert (batch * npi, G) == (nparts_want, G_want), (name, batch * npi, G)
    g = torch.Generator().manual_seed(11)
    # identity-like weights: the centre tap of input channel co % CIN is 1, small noise everywhere
    w = torch.randn(Cout, CIN, 3, 3, generator=g) * 0.01
    for co in range(Cout):
        w[co, co % CIN, 1, 1] += 1.0
    b = torch.randn(Cout, generator=g) * 0.5
    stripe = torch.from_numpy(fr.stripes(gmap, G, Cout)[..., :CIN]).float()             # [batch, H, W, CIN]
    x = (torch.randn(batch, H, W, CIN, generator=g) + stripe + 0.3).to(dev).contiguous()
    res = {"G": G, "nparts": batch * npi, "H": H}

    def produce(wt, bt):
        pw = ops.pack_conv_weight(wt.to(dev), desc, CIN)
        n = ops.conv_stats_buffer(desc, dev).numel()
        stats = torch.full((batch * n,), float("nan"), device=dev)
        ys = []
        for i in range(batch):
            st = stats[i * n:(i + 1) * n]
            ys.append(ops.conv2d_winograd(x[i], pw, bt.to(dev), desc, stats=st) if algo == "F4"
                      else ops.conv2d(x[i], pw, bt.to(dev), desc, y_cs=Cout, stats=st))
        return torch.stack(ys), stats

    def finalize(stats, scratch, run=None):
        if batch > 1:
            return ops.batch_norm_finalize(stats, desc, batch, EPS, running=run, scratch=scratch)
        return ops.instance_norm_finalize(stats, desc, EPS, running=run, scratch=scratch)

    y, stats = produce(w, b)
    scratch = ops.norm_finalize_scratch(desc, dev)
    assert scratch.dtype == torch.float64 and scratch.numel() == 64 * Cout * 4
    scratch.fill_(float("nan"))                           # whatever the merge kernel reads, a group has written
    rm0, rv0 = torch.randn(Cout, generator=g) * 0.2, torch.randn(Cout, generator=g).abs() * 0.1 + 0.5
    runs = [(rm0.clone().to(dev), rv0.clone().to(dev), 0.1, 2) if running else None for _ in range(2)]
    mr_grouped, ran = _profiled(lambda: finalize(stats, scratch, runs[0]))
    mr_plain, ran_plain = _profiled(lambda: finalize(stats, None, runs[1]))
    res["ran"], res["ran_plain"] = ran, ran_plain
    # the float64 statistics of the conv output actually produced, on the device
    yd = y.double().reshape(-1, Cout)
    mean = yd.mean(0)
    var = ((yd - mean) ** 2).mean(0)
    res["want"] = torch.stack([mean, 1.0 / torch.sqrt(var + EPS)], 1).cpu().numpy()
    res["var"], res["n"] = var.cpu().numpy(), yd.shape[0]
    res["grouped"], res["plain"] = mr_grouped.view(-1, 2).cpu().numpy(), mr_plain.view(-1, 2).cpu().numpy()
    if running:
        res["running"] = [torch.stack([r[0], r[1]]).cpu().numpy() for r in runs]
        res["running0"] = torch.stack([rm0, rv0]).numpy()
    # a constant map
    const = -1.3
    yc, stats_c = produce(torch.zeros_like(w), torch.full((Cout,), const))
    scratch.fill_(float("nan"))
    res["const_y_ok"] = bool((yc == const).all())
    res["const"] = finalize(stats_c, scratch).view(-1, 2).cpu().numpy()
    # a scratch buffer that is too short: refused, nothing launched (a valid pointer, a small length)
    short = torch.zeros(8, dtype=torch.float64, device=dev)
    out = torch.full((Cout, 2), float("nan"), device=dev)
    with pytest.raises((RuntimeError, ValueError)):
        if batch > 1:
            ops.batch_norm_finalize(stats, desc, batch, EPS, scratch=short)
        else:
            ops.instance_norm_finalize(stats, desc, EPS, out=out, scratch=short)
    torch.cuda.synchronize()
    ops.check_async_errors()
    res["short_untouched"] = bool(torch.isnan(out).all()) and not bool(short.any())
    return res


@pytest.fixture(scope="module")
def results():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run_case(name)
        return cache[name]
    return get


def _ulps(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_grouped_tables_against_float64_and_the_single_kernel_form(results, name):
    r = results(name)
    assert "t2v::inorm_finalize_merge_kernel" in r["ran"] and "t2v::inorm_finalize_kernel" in r["ran"], r["ran"]
    assert "t2v::inorm_finalize_merge_kernel" not in r["ran_plain"] and "t2v::inorm_finalize_kernel" in r["ran_plain"], r["ran_plain"]
    got, want = r["grouped"], r["want"]
    assert got.shape == want.shape and np.isfinite(got).all()
    ratio = np.abs(got - want) / fr.tolerance(want)
    print("finalize grouped %-28s G=%d, %d partials: worst |mean - f64| / tol %.3g, |rstd - f64| / tol %.3g" % (
        name, r["G"], r["nparts"], ratio[:, 0].max(), ratio[:, 1].max()))
    assert ratio.max() <= 1.0, (name, ratio.max())
    # the stripes are in the data: the groups' means differ by about a standard deviation
    assert (r["var"] > 1.5).all(), r["var"].min()
    u = _ulps(got, r["plain"])
    print("finalize grouped %-28s against the single-kernel form: mean %.1f ulp, rstd %.1f ulp" % (name, u[:, 0].max(), u[:, 1].max()))
    assert u[:, 0].max() <= 2 and u[:, 1].max() <= 3, (name, u.max(0))
    if "running" in r:
        # BatchNorm2d's running statistics after `times` = 2 moves by these statistics (momentum 0.1, unbiased variance)
        keep = 0.9 ** 2
        n = r["n"]
        stat = np.stack([want[:, 0], r["var"] * n / (n - 1)])
        ref = keep * r["running0"] + (1 - keep) * stat
        for which in r["running"]:
            assert np.allclose(which, ref, rtol=2e-5, atol=2e-6), (name, np.abs(which - ref).max())
        assert _ulps(r["running"][0], r["running"][1]).max() <= 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_constant_map_and_the_short_scratch_refusal(results, name):
    r = results(name)
    assert r["const_y_ok"]
    mr = r["const"]
    assert (mr[:, 0] == np.float32(-1.3)).all(), mr[:, 0]
    assert (mr[:, 1] == np.float32(1.0) / np.sqrt(np.float32(EPS), dtype=np.float32)).all(), mr[:, 1]
    assert r["short_untouched"]
