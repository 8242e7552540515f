"""tests/kernel_variants.py's table against the library as built, and its float64 bound against injected faults.

* Every `t2v::` kernel instantiation in libt2v_hip.so (its `__device_stub__` symbols, `nm -C`) has exactly one table
  entry, and every entry names an instantiation that exists: a new instantiation nobody claims fails, as does a stale
  entry.
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
    names = set()
    for line in out.splitlines():
        if "__device_stub__" not in line:
            continue
        sym = line.split(None, 2)[-1]
        if sym.startswith("void "):                                    # (templates demangle with their return type)
            sym = sym[5:]
        if sym.startswith("t2v::__device_stub__"):
            names.add(kv.normalise(sym))
    return names


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
                assert cid in kv.CASE_BY_ID, "%s: unknown case id %s" % (name, cid)
                assert kv.CASE_BY_ID[cid].expect == name, "%s: case %s expects %s" % (name, cid, kv.CASE_BY_ID[cid].expect)
                claimed[cid] = name
        elif isinstance(entry, (kv.Unreachable, kv.Uncovered)):
            assert len(entry.reason) > 20, name
        else:
            assert entry.nodeids, name
    assert len(kv.CASE_BY_ID) == len(kv.CONV_CASES), "duplicate case ids"
    unclaimed = [c.id for c in kv.CONV_CASES if c.id not in claimed]
    assert not unclaimed, "cases whose kernel has no table entry listing them: %s" % unclaimed


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
