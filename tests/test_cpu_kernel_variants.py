"""tests/kernel_variants.py's table against the library as built, and its float64 bound against injected faults.

* Every `t2v::` kernel instantiation in libt2v_hip.so (its `__device_stub__` symbols, `nm -C`; kernels of
  `t2v::(anonymous namespace)::` included) has exactly one table entry, and every entry names an instantiation that
  exists: a new instantiation nobody claims fails, as does a stale entry, as does a stub spelled in a way the listing does
  not understand (the names kept are counted against the `__device_stub__` lines of `nm`).
* Case ids, existing-test node ids and unreachability reasons in the table are well formed.
* The bound can see the bugs it is meant to catch: in float64 on the CPU, at small H and W with the channel storage, taps
  and K stage count of every GPU case family, plausible kernel faults move 3/4 of the outputs they touch by >= 10x the bound, and 9/10 by >= 2x."""
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import kernel_variants as kv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiled_instantiations(lib_path):
    nm = shutil.which("nm")
    if nm is None:
        pytest.fail("`nm` (binutils) is needed to list the kernel instantiations of %s and is not on PATH" % lib_path)
    out = subprocess.run([nm, "-C", lib_path], check=True, capture_output=True, text=True).stdout
    names, stubs, strange = [], 0, []
    for line in out.splitlines():
        if "__device_stub__" not in line:
            continue
        stubs += 1
        sym = line.split(None, 2)[-1]
        if sym.startswith("void "):                                    # (templates demangle with their return type)
            sym = sym[5:]
        if sym.startswith(("t2v::__device_stub__", "t2v::(anonymous namespace)::__device_stub__")):
            names.append(kv.normalise(sym))
        else:
            strange.append(line)
    # a stub in some third spelling must fail here, not vanish; so must two stubs that normalise to one name
    assert len(names) == stubs and not strange, "%d of %d __device_stub__ symbols kept; not understood:\n  %s" % (
        len(names), stubs, "\n  ".join(strange))
    assert len(set(names)) == len(names), "stubs that normalise to the same name: %s" % sorted(
        n for n in set(names) if names.count(n) > 1)
    return set(names)


def test_normalise_gives_one_name_whether_nm_or_the_profiler_spells_it():
    nm_t = "void t2v::(anonymous namespace)::__device_stub__flow_lk_kernel<1>(t2v::(anonymous namespace)::LkArgs)"
    prof_t = "void t2v::(anonymous namespace)::flow_lk_kernel<1>(t2v::(anonymous namespace)::LkArgs)"
    assert kv.normalise(nm_t) == kv.normalise(prof_t) == "t2v::flow_lk_kernel<1>"
    nm_p = "t2v::(anonymous namespace)::__device_stub__flow_out_kernel(HIP_vector_type<float, 2u> const*, HIP_vector_type<float, 4u>*, int, int)"
    prof_p = "t2v::(anonymous namespace)::flow_out_kernel(HIP_vector_type<float, 2u> const*, HIP_vector_type<float, 4u>*, int, int)"
    assert kv.normalise(nm_p) == kv.normalise(prof_p) == "t2v::flow_out_kernel"
    assert kv.normalise("void t2v::(anonymous namespace)::__device_stub__polyphase_input_split_kernel<false, true>(HIP_vector_type<float, 2u> const*, unsigned int*)") \
        == "t2v::polyphase_input_split_kernel<false,true>"
    assert kv.family(nm_t) == "flow_lk_kernel"
    # the named namespace keeps working, nested template arguments and all
    assert kv.normalise("void t2v::__device_stub__f<t2v::T<1, 2>, 3>(t2v::P)") == kv.normalise("void t2v::f<t2v::T<1, 2>, 3>(t2v::P)") \
        == "t2v::f<t2v::T<1,2>,3>"


def test_table_claims_exactly_the_compiled_instantiations(lib_built):
    from text2video_amd import _lib
    compiled = _compiled_instantiations(_lib.LIB_PATH)
    assert len(compiled) > 100, "nm found only %d kernel stubs in %s" % (len(compiled), _lib.LIB_PATH)
    table = set(kv.TABLE)
    assert not compiled - table, "instantiations no table entry claims:\n  " + "\n  ".join(sorted(compiled - table))
    assert not table - compiled, "table entries with no such instantiation:\n  " + "\n  ".join(sorted(table - compiled))


def test_table_entries_are_well_formed():
    claimed = {}
    for name, entry in kv.TABLE.items():
        assert isinstance(entry, (kv.Cases, kv.Existing, kv.Uncovered, kv.Unreachable)), name
        if isinstance(entry, kv.Cases):
            assert entry.ids, "%s: no case" % name
            for cid in entry.ids:
                if cid in kv.PIPE_BY_ID:          # a pipeline case expects one or more instantiations
                    assert name in kv.PIPE_BY_ID[cid].expect, "%s: case %s expects %s" % (name, cid, kv.PIPE_BY_ID[cid].expect)
                else:
                    assert cid in kv.CASE_BY_ID, "%s: unknown case id %s" % (name, cid)
                    assert kv.CASE_BY_ID[cid].expect == name, "%s: case %s expects %s" % (name, cid, kv.CASE_BY_ID[cid].expect)
                claimed[cid] = name
        elif isinstance(entry, (kv.Unreachable, kv.Uncovered)):
            assert len(entry.reason) > 20, name
        else:
            assert entry.nodeids, name
    assert len(kv.CASE_BY_ID) == len(kv.CONV_CASES), "duplicate case ids"
    assert len(kv.PIPE_BY_ID) == len(kv.PIPE_CASES) and not set(kv.PIPE_BY_ID) & set(kv.CASE_BY_ID), "duplicate case ids"
    unclaimed = [c.id for c in kv.CONV_CASES + kv.PIPE_CASES if c.id not in claimed]
    assert not unclaimed, "cases whose kernel has no table entry listing them: %s" % unclaimed
    for c in kv.PIPE_CASES:
        for name in c.expect:
            assert name in kv.TABLE, "%s expects %s, which is no compiled instantiation the table knows" % (c.id, name)
            assert kv.family(name) in kv.PIPE_FAMILIES, (c.id, name)
    # what stays Uncovered has nothing to pin: a self-test without numerical output (add_kernel has an entry point, ops.add)
    uncovered = sorted(n for n, e in kv.TABLE.items() if isinstance(e, kv.Uncovered))
    assert uncovered == ["t2v::dispatch_order_kernel"], uncovered


def test_existing_node_ids_name_tests_that_exist():
    for name, entry in kv.TABLE.items():
        if not isinstance(entry, kv.Existing):
            continue
        for nodeid in entry.nodeids:
            path, _, test = nodeid.partition("::")
            full = os.path.join(ROOT, path)
            assert os.path.isfile(full), "%s: no file %s" % (name, path)
            with open(full) as f:
                src = f.read()
            assert re.search(r"^def %s\(" % re.escape(test), src, re.M), "%s: no test %s in %s" % (name, test, path)


# ---- sensitivity of the bound ---------------------------------------------------------------------------------------------
def _small(case):
    """the case's family (channels, storage, taps, stride, padding, K stages) on a small map, one image"""
    lo = case.pad + 1 if case.reflect else 1
    H, W = max(min(case.H, 9), lo, case.k - 2 * case.pad), max(min(case.W, 10), lo, case.k - 2 * case.pad)
    return case._replace(H=H, W=W, batch=1)


def _families():
    seen, out = set(), []
    for c in kv.CONV_CASES:
        key = (c.Cin, kv.x_cs(c), c.Cout > 16, c.k, c.stride, c.pad, c.reflect, c.transposed, c.offset)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def _border_tap(case):
    """the tap output row 0 reads the image's first row through: kernel row `pad`, last kernel column"""
    return min(case.pad, case.k - 1) * case.k + case.k - 1


def _im2col_conv(case, x, w, b, k_keep=None, pad_mode=None, drop_border_tap=False):
    """conv2d in float64 as the implicit GEMM sees it: K index = tap * x_cs + c over the padded channel storage, packed
    to a multiple of 32.  k_keep: 0/1 per packed K index; drop_border_tap: output row 0 loses _border_tap()."""
    cs, kk, taps = kv.x_cs(case), case.k, case.k * case.k
    reflect = case.reflect if pad_mode is None else pad_mode == "reflect"
    xd = torch.zeros(1, cs, case.H, case.W, dtype=torch.float64)
    xd[:, :case.Cin] = x.double()
    xp = F.pad(xd, (case.pad,) * 4, mode="reflect" if reflect else "constant") if case.pad else xd
    cols = F.unfold(xp, kk, stride=case.stride)                        # [1, cs * taps, L], index c * taps + tap
    L = cols.shape[-1]
    cols = cols.view(cs, taps, L).permute(1, 0, 2).reshape(taps * cs, L)
    wd = torch.zeros(case.Cout, cs, kk, kk, dtype=torch.float64)
    wd[:, :case.Cin] = w.double()
    wm = wd.view(case.Cout, cs, taps).permute(0, 2, 1).reshape(case.Cout, taps * cs)
    Kp = -(-taps * cs // 32) * 32
    if k_keep is not None:
        cols = cols * k_keep[:taps * cs, None]
    y = wm @ cols + b.double()[:, None]
    Ho = (case.H + 2 * case.pad - kk) // case.stride + 1
    Wo = L // Ho
    y = y.view(1, case.Cout, Ho, Wo)
    if drop_border_tap:
        t = _border_tap(case)
        y[0, :, 0, :] -= (wm[:, t * cs:(t + 1) * cs] @ cols[t * cs:(t + 1) * cs]).view(case.Cout, Ho, Wo)[:, 0, :]
    assert Kp % 32 == 0
    return y


def _fault_ratio(case, ref, faulty, bnd):
    """|fault - ref| / bound over the outputs the fault touches (those it moves at all): its 10th and 25th percentiles.
    Percentiles, not the minimum: a dropped term is a signed sum, and on a few outputs of random data it cancels to
    nearly nothing."""
    d = (faulty - ref).abs()
    touched = d > 1e-12 * (ref.abs() + 1)
    assert touched.any(), "%s: the fault touches no output" % case.id
    r = d[touched] / bnd[touched]
    return r.quantile(0.10).item(), r.quantile(0.25).item(), int(touched.sum())


def test_bound_sees_injected_faults_at_least_10x():
    worst = {}
    for fam in _families():
        case = _small(fam)
        x, w, b = kv.case_tensors(case, seed=5)
        ref = kv.conv64(case, x, w, b)
        bnd = kv.bound(case, x, w, b)
        faults = {}
        if case.transposed:
            # one sub-pixel phase's last output row computed without the input's last row (a masked tap instead of a
            # masked store): phase (1, 1), rows 1, 3, ...
            xz = x.clone()
            xz[:, :, -1, :] = 0
            f = ref.clone()
            last = ref.shape[2] - 1 if (ref.shape[2] - 1) % 2 == 1 else ref.shape[2] - 2
            f[:, :, last, 1::2] = kv.conv64(case, xz, w, b)[:, :, last, 1::2]
            faults["phase (1,1) last row"] = f
        else:
            assert torch.allclose(_im2col_conv(case, x, w, b), ref, rtol=1e-12, atol=1e-12), case.id
            K = case.k * case.k * kv.x_cs(case)
            Kp = -(-K // 32) * 32
            keep = torch.ones(Kp, dtype=torch.float64)
            if kv.family(case.expect) == "conv_head7x7_strip_kernel":
                # the head kernel's K loop runs over 16-channel passes of all 49 taps: its last pass dropped
                keep.view(-1)[:K].view(case.k * case.k, -1)[:, -16:] = 0
            else:
                keep[Kp - 32:] = 0
            faults["last K stage dropped"] = _im2col_conv(case, x, w, b, k_keep=keep)
            faults["border tap dropped"] = _im2col_conv(case, x, w, b, drop_border_tap=True)
            if case.pad > 0:
                faults["reflect / zero padding swapped"] = _im2col_conv(
                    case, x, w, b, pad_mode="zero" if case.reflect else "reflect")
        for what, f in faults.items():
            worst[(what, fam.id)] = _fault_ratio(case, ref, f, bnd)
    rows = sorted(worst.items(), key=lambda t: t[1][1])
    lines = ["%-32s %-36s |fault| / bound: 10th pct %8.3g, 25th pct %8.3g over %d outputs" % (w, c, p10, p25, n)
             for (w, c), (p10, p25, n) in rows]
    print("\n".join(lines))
    # at least 3/4 of the outputs a fault touches move by >= 10x the bound, and 9/10 by >= 2x
    weak = [ln for ((w, c), (p10, p25, n)), ln in zip(rows, lines) if p25 < 10 or p10 < 2]
    assert not weak, "faults too close to the bound:\n" + "\n".join(weak)
    kinds = {w for w, _ in worst}
    assert kinds == {"last K stage dropped", "border tap dropped", "reflect / zero padding swapped",
                     "phase (1,1) last row"}, kinds


# ---- the Winograd / polyphase pipelines ---------------------------------------------------------------------------------
def _pipe_conv(algo, x, w, b, pad=1, reflect=True):
    """the stage references composed into one conv, in float64: x [H, W, C] -> y [Ho, Wo, Cout]"""
    H, W, _ = x.shape
    if algo in ("down", "up"):
        up = algo == "up"
        V, TH, TW = kv.polyphase_input64(x.double(), H, W, up)
        Ub = kv.weight64(w, kv.PP["kGU" if up else "kGD"], transposed_layout=up)
        Ho, Wo = (2 * H, 2 * W) if up else (H // 2, W // 2)
        A = kv.PP["kAU" if up else "kAD"]
    else:
        mats, m = (kv.F4, 4) if algo == "F4" else (kv.F2, 2)
        V, TH, TW = kv.wino_input64(x.double(), H, W, pad, reflect, m=m, BT=mats["kBT"])
        Ub = kv.weight64(w, mats["kG"])
        Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
        A = mats["kAT"]
    return kv.output64(kv.gemm64(V, Ub), A, TH, TW, Ho, Wo, b)[0]


def _torch_conv(algo, x, w, b, pad=1, reflect=True):
    xd = x.double().permute(2, 0, 1)[None]
    if algo == "up":
        y = F.conv_transpose2d(xd, w.double(), b.double(), stride=2, padding=1, output_padding=1)
    elif algo == "down":
        y = F.conv2d(xd, w.double(), b.double(), stride=2, padding=1)
    elif reflect:
        y = F.conv2d(F.pad(xd, (pad,) * 4, mode="reflect"), w.double(), b.double())
    else:
        y = F.conv2d(xd, w.double(), b.double(), padding=pad)
    return y[0].permute(1, 2, 0)


@pytest.mark.parametrize("algo,H,W,pad,reflect", [("F4", 9, 14, 1, True), ("F4", 7, 5, 2, False), ("F4", 6, 9, 0, False),
                                                  ("F2", 7, 10, 1, True), ("down", 14, 10, 1, False), ("up", 7, 9, 1, False)])
def test_transform_matrices_reproduce_a_plain_correlation(algo, H, W, pad, reflect):
    """The generated headers' matrices, assembled as A^T[(G g G^T) . (B^T d B)]A (F(4x4), F(2x2)) and as the polyphase down
    (stride 2) and up (ConvTranspose2d(3, 2, 1, output_padding=1)) forms, reproduce a plain 3x3 correlation in float64 to
    1e-12 relative error, ragged tiles and the reflected / zero borders included."""
    g = torch.Generator().manual_seed(21)
    Cin, Cout = 3, 5
    x = torch.randn(H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(*((Cin, Cout, 3, 3) if algo == "up" else (Cout, Cin, 3, 3)), generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    ref = _torch_conv(algo, x, w, b, pad, reflect)
    got = _pipe_conv(algo, x, w, b, pad, reflect)
    assert got.shape == ref.shape
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    assert rel <= 1e-12, "%s: relative error %.3g" % (algo, rel)


def _pipe_faults():
    """{(family, fault): (ref, faulty, bound)} over the pipeline references at small shapes, fp32 data"""
    g = torch.Generator().manual_seed(22)
    out = {}
    r32 = lambda *s: torch.randn(*s, generator=g).float().double()
    H, W, C, N = 10, 14, 8, 6
    BT4, n4 = kv.F4["kBT"], kv.nnz_rows(kv.F4["kBT"])
    x = r32(H, W, C)
    # F(4x4) input transform, reflect pad 1, ragged (10 x 14: 3 x 4 tiles)
    ref, TH, TW = kv.wino_input64(x, H, W, 1, True)
    aab = kv.wino_input64(x.abs(), H, W, 1, True, BT=BT4.abs())[0]
    bnd = kv.input_bound(aab, n4)
    bad = BT4.clone()
    bad[1, 2] += 2.0 ** -6
    out[("winograd4_input", "B^T coefficient off by 2^-6")] = (ref, kv.wino_input64(x, H, W, 1, True, BT=bad)[0], bnd)
    # reflect taken as symmetric (edge repeated) at the border
    xs = F.pad(x.permute(2, 0, 1)[None], (1, 1, 1, 1), mode="replicate")[0].permute(1, 2, 0)
    f = kv.wino_input64(xs, H + 2, W + 2, 0, False)[0]
    out[("winograd4_input", "reflect taken as symmetric")] = (ref, f, bnd)
    # the last ragged tile column dropped (zeros)
    f = ref.clone().view(36, TH, TW, C)
    f[:, :, -1] = 0
    out[("winograd4_input", "last ragged tile column dropped")] = (ref, f.view(36, -1, C), bnd)
    # lazy modes: beta applied to the zero padding (pad 1, zero)
    mr = torch.stack([r32(C) * 0.5 + 0.3, torch.rand(C, generator=g).double() + 0.5], -1)
    gm, bt = r32(C) * 0.5 + 1.0, r32(C) * 0.5 + 0.2
    d, e_d = kv.lazy_d64(x, mr, gm, bt, relu=True)
    refz = kv.wino_input64(x, H, W, 1, False, d=d)[0]
    bz = kv.input_bound(kv.wino_input64(x, H, W, 1, False, BT=BT4.abs(), d=d.abs())[0], n4,
                        kv.wino_input64(e_d, H, W, 1, False, BT=BT4.abs())[0])
    dpad = F.pad(d.permute(2, 0, 1)[None], (1, 1, 1, 1))[0].permute(1, 2, 0)
    dpad[0, :] = dpad[-1, :] = dpad[:, 0] = dpad[:, -1] = bt.clamp(min=0)       # norm(0-padding) = relu(beta)
    out[("winograd4_input lazy", "beta applied to zero padding")] = (refz, kv.wino_input64(dpad, H + 2, W + 2, 0, False)[0], bz)
    # mode 2: the xout pixel taken from the neighbouring tile (4 columns to the right)
    res = r32(H, W, C)
    d2, e2 = kv.lazy_d64(x, mr, gm, bt, res=res)
    xo = d2.clone()
    xo[:, :-4] = d2[:, 4:]
    out[("winograd4_input mode 2 xout", "pixel from the neighbouring tile")] = (d2, xo, e2)
    # output transform (F(4x4)): a coefficient off
    M = r32(36, TH * TW, N)
    bias = r32(N) * 0.1
    y, ay = kv.output64(M, kv.F4["kAT"], TH, TW, H, W, bias)
    badA = kv.F4["kAT"].clone()
    badA[2, 3] += 2.0 ** -6
    out[("winograd4_output", "A^T coefficient off by 2^-6")] = (
        y, kv.output64(M, badA, TH, TW, H, W, bias)[0], kv.output_bound(ay, kv.nnz_rows(kv.F4["kAT"])))
    # polyphase up: even and odd output phases swapped (rows)
    xu = r32(7, 9, C)
    wu = r32(C, N, 3, 3) * (9 * C) ** -0.5
    Vu, THu, TWu = kv.polyphase_input64(xu, 7, 9, True)
    Mu = kv.gemm64(Vu, kv.weight64(wu, kv.PP["kGU"], transposed_layout=True))
    yu, au = kv.output64(Mu, kv.PP["kAU"], THu, TWu, 14, 18, bias)
    perm = torch.arange(8).view(4, 2).flip(1).reshape(-1)
    yf = kv.output64(Mu, kv.PP["kAU"][perm], THu, TWu, 14, 18, bias)[0]
    out[("polyphase_output_up", "even and odd phases swapped")] = (yu, yf, kv.output_bound(au, kv.nnz_rows(kv.PP["kAU"])))
    # GEMM: one stream-K hand-over partial counted twice (the second half of K of one 128-row tile added again)
    K = 256
    Vg, Ug = r32(4, 160, K), r32(4, N, K) * K ** -0.5
    Mg = kv.gemm64(Vg, Ug)
    f = Mg.clone()
    f[1, :128] += kv.gemm64(Vg[1:2, :128, K // 2:], Ug[1:2, :, K // 2:])[0]
    out[("wino_gemm_sk", "hand-over partial counted twice")] = (Mg, f, kv.gemm_bound(Vg, Ug, K))
    # weight-gradient reduction: one image slot dropped (rows [Tp, 2 Tp) of a batch of 2)
    Tp = 64
    Vw, Mw = r32(36, 2 * Tp, C), r32(36, 2 * Tp, N)
    dU = kv.gemm64(Mw.transpose(1, 2), Vw.transpose(1, 2))
    f = kv.gemm64(Mw[:, :Tp].transpose(1, 2), Vw[:, :Tp].transpose(1, 2))
    out[("wino_wgrad_sk", "one image slot dropped")] = (dU, f, kv.gemm_bound(Mw.transpose(1, 2), Vw.transpose(1, 2), 2 * Tp))
    # data gradient: one of the four overlapping dgrad_output contributions dropped (the top-left neighbour's)
    THd, TWd = 3, 4
    dV = r32(36, THd * TWd, C)
    dxp, adx = kv.dgrad_output64(dV, THd, TWd)
    v = dV.view(6, 6, THd, TWd, C)
    dd = torch.einsum("ai,bj,abyxc->yixjc", kv.F4["kBT"], kv.F4["kBT"], v)
    f = dxp.clone()
    for ty in range(1, THd):
        for tx in range(1, TWd):
            f[4 * ty:4 * ty + 2, 4 * tx:4 * tx + 2] -= dd[ty - 1, 4:, tx - 1, 4:]
    out[("winograd4_dgrad_output", "top-left contribution dropped")] = (dxp, f, kv.dgrad_output_bound(adx))
    # dy<NORM>: the sign of the S1 term flipped
    Ho, Wo = 12, 9
    dy, xo_ = r32(Ho, Wo, N), r32(Ho, Wo, N) + 0.3
    mrn = torch.stack([r32(N) * 0.2 + 0.3, torch.rand(N, generator=g).double() + 0.5], -1).float()
    gmn, btn = (r32(N) * 0.5 + 1.0).float(), (r32(N) * 0.5 + 0.2).float()
    sums = (r32(N, 2) * (Ho * Wo) ** 0.5).float()
    front, ef = kv.dy_front64(dy.float(), xo_.float(), mrn, gmn, btn, 1, sums, Ho * Wo)
    neg = sums.clone()
    neg[:, 1] = -neg[:, 1]
    frontf, _ = kv.dy_front64(dy.float(), xo_.float(), mrn, gmn, btn, 1, neg, Ho * Wo)
    r1, a1 = kv.dy64(front, Ho, Wo)
    out[("winograd4_dy<NORM>", "sign of the S1 term flipped")] = (r1, kv.dy64(frontf, Ho, Wo)[0],
                                                                 kv.dy_bound(a1, kv.dy64(ef, Ho, Wo)[1]))
    # weight transform: a G coefficient off
    wg = r32(N, C, 3, 3)
    U64 = kv.weight64(wg, kv.F4["kG"])
    badG = kv.F4["kG"].clone()
    badG[1, 1] += 2.0 ** -6
    out[("winograd4_weight", "G coefficient off by 2^-6")] = (U64, kv.weight64(wg, badG),
                                                             kv.weight_bound(U64, kv.weight64(wg.abs(), kv.F4["kG"].abs())))
    return out


def test_pipeline_bounds_see_injected_faults_at_least_10x():
    """The pipeline references and bounds against plausible kernel faults, in float64 on the CPU: as for the direct kernels,
    3/4 of the outputs a fault touches move by >= 10x the bound, and 9/10 by >= 2x."""
    rows = []
    for (fam, what), (ref, faulty, bnd) in _pipe_faults().items():
        d = (faulty - ref).abs()
        touched = d > 1e-12 * (ref.abs() + 1)
        assert touched.any(), "%s / %s: the fault touches nothing" % (fam, what)
        r = d[touched] / bnd[touched]
        rows.append((fam, what, r.quantile(0.10).item(), r.quantile(0.25).item(), int(touched.sum())))
    lines = ["%-30s %-36s 10th pct %9.3g, 25th pct %9.3g over %d outputs" % t for t in rows]
    print("\n".join(lines))
    weak = [ln for t, ln in zip(rows, lines) if t[3] < 10 or t[2] < 2]
    assert not weak, "faults too close to the bound:\n" + "\n".join(weak)
    assert len(rows) == 12, len(rows)


def test_backward_compositions_reproduce_autograd():
    """The adjoint algebra the backward stage references encode (dy64: A dy A^T; dgrad_output64: the scatter of B dV B^T;
    dw64: G^T dU G; reflect_fold), composed as the library composes the kernels, reproduces autograd's input and weight
    gradients of a ReflectionPad(1) 3x3 conv in float64 to 1e-12 -- a transposition shared by a reference and its kernel
    would not."""
    g = torch.Generator().manual_seed(23)
    H, W, Cin, Cout = 8, 12, 3, 5
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(H, W, Cout, generator=g, dtype=torch.float64)
    x0 = torch.zeros(1, Cin, H, W, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(F.conv2d(F.pad(x0, (1,) * 4, mode="reflect"), w), x0, dy.permute(2, 0, 1)[None])
    got = kv.dgrad64(dy, w)
    ref = ref[0].permute(1, 2, 0)
    assert ((got - ref).abs().max() / ref.abs().max()).item() <= 1e-12
    # the weight gradient over two images, one of them ragged (7 x 10: the tiles reach past the map)
    for Hx, Wx in ((8, 12), (7, 10)):
        x = torch.randn(2, Hx, Wx, Cin, generator=g, dtype=torch.float64)
        dyb = torch.randn(2, Hx, Wx, Cout, generator=g, dtype=torch.float64)
        w0 = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (1,) * 4, mode="reflect"), w0)
        (rw,) = torch.autograd.grad(y, w0, dyb.permute(0, 3, 1, 2))
        gw = kv.wgrad64(x, dyb)
        assert ((gw - rw).abs().max() / rw.abs().max()).item() <= 1e-12, (Hx, Wx)


def test_tile_padding_rule_matches_the_library(lib_built):
    """kernel_variants.pad_tiles (the GEMM row padding the tests use to find rows in a workspace) is the library's rule"""
    import ctypes
    from text2video_amd import _lib
    for H in range(2, 140, 7):
        for W in range(2, 140, 11):
            d = _lib.ConvDesc(H, W, 32, 32, 3, 3, 1, 1, _lib.PAD_REFLECT, 0, 0, 1.0, 0, _lib.ALGO_WINOGRAD_F4)
            assert lib_built.t2v_conv_winograd_tile_rows(ctypes.byref(d)) == kv.pad_tiles(-(-H // 4) * -(-W // 4)), (H, W)
            for nimg in (1, 2, 3):
                n = lib_built.t2v_conv_winograd_batch_workspace_floats(ctypes.byref(d), 32, nimg)
                one = lib_built.t2v_conv_winograd_workspace_floats(ctypes.byref(d), 32)
                Tt = kv.pad_tiles(nimg * -(-H // 4) * -(-W // 4))
                assert n - one == 36 * 64 * (Tt - kv.pad_tiles(-(-H // 4) * -(-W // 4))), (H, W, nimg)
