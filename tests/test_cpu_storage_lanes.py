"""tests/storage_lanes.py's table against the headers as written, and its twin-run method against injected faults.

* Every parameter named cs, *_cs, c0 or *_c0 of every entry point of t2v.h, t2v_flow_refine.h, t2v_bf16x2.h and
  t2v_grad_fold.h (read through text2video_amd/_cabi.py, the reader the bindings use) has exactly one LANES entry; every
  LANES entry names a parameter that exists; every Existing node id names a test that exists; every Case id has a twin run in
  tests/test_gpu_storage_lanes.py and every twin run is claimed.  A new entry point with a cs argument and no entry fails
  here, as tests/test_cpu_kernel_variants.py fails for a kernel instantiation nobody claims.
* Each of those assertions was seen to fail when its condition is broken: the checks are functions of the table, and
  test_header_coverage_sees_a_broken_table runs them on a table with an entry removed, a bogus parameter and a node id of a
  test that does not exist.
* The twin run sees the faults it is for, in float64 on the CPU: a pad weight slot of 2^-20, a K loop over cs with the
  neighbouring tap's weight, a channel sum over cs, a flat sum |a - b| over [npix, cs] -- each makes the junk twin differ
  from the zero twin under both patterns, and the unfaulted forms give equal twins."""
import os
import re

import pytest
import torch

import storage_lanes as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_PARAMETER = re.compile(r"(\w+_)?(cs|c0)")


def _headers():
    from text2video_amd import _cabi
    base = _cabi.read_header("t2v.h")
    return {name: (base if name == "t2v.h" else _cabi.read_header(name, base if name == "t2v_bf16x2.h" else None))
            for name in sl.HEADERS}


def _lane_parameters(headers):
    return {(h, fn, p) for h, hd in headers.items() for fn, names in hd.parameters.items() for p in names
            if LANE_PARAMETER.fullmatch(p)}


def coverage_problems(table, headers, runners):
    """every way `table` fails to claim the headers' lane parameters exactly, as a list of sentences"""
    out = []
    want = _lane_parameters(headers)
    out += ["no LANES entry for %s: %s(%s)" % k for k in sorted(want - set(table))]
    for (h, fn, p), entry in table.items():
        if h not in headers or fn not in headers[h].parameters:
            out.append("LANES names %s: %s, which the header does not declare" % (h, fn))
        elif p not in headers[h].parameters[fn]:
            out.append("LANES names parameter %s of %s: %s, which it does not have" % (p, h, fn))
        if isinstance(entry, sl.Existing):
            for nodeid in entry.nodeids:
                path, _, test = nodeid.partition("::")
                full = os.path.join(ROOT, path)
                if not os.path.isfile(full):
                    out.append("%s: no file %s" % (fn, path))
                elif not re.search(r"^def %s\(" % re.escape(test), open(full).read(), re.M):
                    out.append("%s: no test %s in %s" % (fn, test, path))
        elif isinstance(entry, sl.Case):
            out += ["%s: case %s has no twin run" % (fn, i) for i in entry.ids if i not in runners]
            if not entry.ids:
                out.append("%s(%s): a Case without a case" % (fn, p))
        elif isinstance(entry, sl.NotApplicable):
            if not re.search(r'"[^"]*(==|!=)[^"]*"', entry.reason):
                out.append("%s(%s): NotApplicable must quote the cs == C condition it rests on" % (fn, p))
        elif isinstance(entry, sl.Query):
            if h in headers and fn in headers[h].functions and any(
                    t.replace("const ", "") in ("float*", "uint8_t*", "double*") for t in headers[h].functions[fn][1]):
                out.append("%s: a Query is handed no tensor, this entry takes one" % fn)
        else:
            out.append("%s(%s): %r is none of Case, Existing, NotApplicable, Query" % (fn, p, entry))
    return out


def _runners():
    import test_gpu_storage_lanes
    return test_gpu_storage_lanes.RUNNERS


def test_every_lane_parameter_of_the_headers_is_claimed_exactly_once():
    headers = _headers()
    assert len(_lane_parameters(headers)) > 80          # (the reader found the declarations)
    problems = coverage_problems(sl.LANES, headers, _runners())
    assert not problems, "\n".join(problems)
    # (a dict holds each key once: "exactly one entry" is "an entry")
    unclaimed = set(_runners()) - set(sl.case_ids())
    assert not unclaimed, "twin runs no LANES / PYTHON_CASES entry lists: %s" % sorted(unclaimed)
    missing = [i for ids in sl.PYTHON_CASES.values() for i in ids if i not in _runners()]
    assert not missing, missing
    for (path, _), ids in sl.PYTHON_CASES.items():
        assert os.path.isfile(os.path.join(ROOT, path)) and ids, path


def test_conv_geometries_are_float64_pinned_cases_with_lanes():
    import kernel_variants as kv
    for cid, geom in sl.CONV_GEOMETRY.items():
        case = kv.CASE_BY_ID[geom]
        assert kv.x_cs(case) > case.Cin or case.Cout % 4 != 0, (cid, geom)
        assert cid in sl.case_ids(), cid
    cins = {kv.CASE_BY_ID[g].Cin for g in sl.CONV_GEOMETRY.values()}
    assert {3, 5, 6, 7, 9, 11} <= cins, cins


def test_header_coverage_sees_a_broken_table():
    headers, runners = _headers(), _runners()
    key = ("t2v.h", "t2v_channel_sum", "cs")
    removed = {k: v for k, v in sl.LANES.items() if k != key}
    assert coverage_problems(removed, headers, runners) == ["no LANES entry for t2v.h: t2v_channel_sum(cs)"]
    bogus = dict(sl.LANES)
    bogus[("t2v.h", "t2v_channel_sum", "channel_stride")] = sl.Case(("channel_sum_c6_cs8",))
    assert coverage_problems(bogus, headers, runners) == [
        "LANES names parameter channel_stride of t2v.h: t2v_channel_sum, which it does not have"]
    bogus = dict(sl.LANES)
    bogus[("t2v.h", "t2v_channel_total", "cs")] = sl.Case(("channel_sum_c6_cs8",))
    assert coverage_problems(bogus, headers, runners) == ["LANES names t2v.h: t2v_channel_total, which the header does not declare"]
    stale = dict(sl.LANES)
    stale[key] = sl.Existing(("tests/test_gpu_backward.py::test_channel_sum_ignores_its_lanes",))
    assert coverage_problems(stale, headers, runners) == [
        "t2v_channel_sum: no test test_channel_sum_ignores_its_lanes in tests/test_gpu_backward.py"]
    stale[key] = sl.Existing(("tests/test_gpu_nowhere.py::test_x",))
    assert coverage_problems(stale, headers, runners) == ["t2v_channel_sum: no file tests/test_gpu_nowhere.py"]
    stale[key] = sl.Case(("channel_sum_without_a_run",))
    assert coverage_problems(stale, headers, runners) == ["t2v_channel_sum: case channel_sum_without_a_run has no twin run"]
    stale[key] = sl.NotApplicable("the entry needs whole quads")
    assert coverage_problems(stale, headers, runners) == [
        "t2v_channel_sum(cs): NotApplicable must quote the cs == C condition it rests on"]
    stale[key] = sl.Query("computes a size")
    assert coverage_problems(stale, headers, runners) == ["t2v_channel_sum: a Query is handed no tensor, this entry takes one"]
    # a new entry point with a cs argument and no case
    from text2video_amd import _cabi
    grown = dict(headers)
    with open(os.path.join(_cabi.INCLUDE_DIR, "t2v_grad_fold.h")) as f:
        text = f.read().replace("int t2v_grad_fold_abi_version(void);",
                                "int t2v_grad_fold_abi_version(void);\nint t2v_grad_fold_nhwc(t2v_ctx* ctx, float* grad, long npix, int C, int grad_cs);")
    grown["t2v_grad_fold.h"] = _cabi.Header(text, "t2v_grad_fold.h")
    assert coverage_problems(sl.LANES, grown, runners) == ["no LANES entry for t2v_grad_fold.h: t2v_grad_fold_nhwc(grad_cs)"]


# ---- the patterns -------------------------------------------------------------------------------------------------------------
def test_patterns_are_finite_seeded_and_fill_only_the_lanes():
    t = torch.randn(5, 7, 12, generator=torch.Generator().manual_seed(1))
    for pattern in sl.PATTERNS:
        a, b = sl.with_lanes(t, 9, pattern), sl.with_lanes(t, 9, pattern)
        assert torch.equal(a, b) and torch.isfinite(a).all() and a.dtype == torch.float32
        assert torch.equal(a[..., :9], t[..., :9]) and (a[..., 9:] != 0).any()
        assert not torch.equal(sl.with_lanes(t, 9, pattern, seed=1)[..., 9:], a[..., 9:])
        o = sl.with_lanes_outside(t, 3, 5, pattern)
        assert torch.equal(o[..., 3:8], t[..., 3:8]) and (o[..., :3] != t[..., :3]).any() and (o[..., 8:] != t[..., 8:]).any()
    assert torch.equal(sl.with_lanes(t, 9, "zero")[..., 9:], torch.zeros(5, 7, 3))
    big = sl.junk((4096,), "extreme")
    for v in sl.EXTREMES:
        assert (big == v).any(), v
    assert (big.abs() < 10).any() and torch.signbit(big[big == 0]).all()          # randn entries; the zeros are -0.0
    assert sl.junk((4096,), "moderate").abs().max() > 1e3
    with pytest.raises(ValueError):
        sl.junk((4,), "nan")


# ---- fault sensitivity ----------------------------------------------------------------------------------------------------------
def _twins(pattern, Cin, cs, H=6, W=7, k=3):
    g = torch.Generator().manual_seed(7)
    x = torch.zeros(H, W, cs)
    x[..., :Cin] = torch.randn(H, W, Cin, generator=g)
    w, b = torch.randn(5, Cin, k, k, generator=g), torch.randn(5, generator=g)
    chw = lambda t: t.permute(2, 0, 1).double()
    return chw(sl.with_lanes(x, Cin, "zero")), chw(sl.with_lanes(x, Cin, pattern)), w, b


@pytest.mark.parametrize("pattern", sl.PATTERNS)
@pytest.mark.parametrize("Cin,cs", [(3, 4), (6, 8), (9, 12), (5, 8)])
def test_twin_run_sees_each_injected_fault_and_passes_the_unfaulted_form(pattern, Cin, cs):
    xa, xb, w, b = _twins(pattern, Cin, cs)
    conv = lambda x, fault=None: sl.im2col_conv(x, w, b, cs, 3, 1, fault)
    ref = torch.nn.functional.conv2d(xa[None, :Cin], w.double(), b.double(), padding=1)[0]
    assert torch.allclose(conv(xa), ref, rtol=1e-12, atol=1e-12)
    assert torch.equal(conv(xa), conv(xb)), "the unfaulted conv must give equal twins"
    for fault in sl.FAULTS[:2]:
        ya, yb = conv(xa, fault), conv(xb, fault)
        assert torch.isfinite(ya).all()
        assert not torch.equal(ya, yb), "%s: the twins are equal under %s" % (fault, pattern)
        assert (ya != yb).float().mean() > 0.5, fault                 # and not at a stray output: most of them move
    pa, pb = xa.flatten(1).t(), xb.flatten(1).t()                      # [npix, cs]
    assert torch.equal(sl.channel_sum(pa, Cin), sl.channel_sum(pb, Cin))
    assert not torch.equal(sl.channel_sum(pa, Cin, sl.FAULTS[2]), sl.channel_sum(pb, Cin, sl.FAULTS[2]))
    qa, qb = pa.flip(0), sl.with_lanes(pb.flip(0).float(), Cin, pattern, seed=3).double()
    assert torch.equal(sl.sum_abs_diff(pa, qa, Cin), sl.sum_abs_diff(pb, qb, Cin))
    assert not torch.equal(sl.sum_abs_diff(pa, qa, Cin, sl.FAULTS[3]), sl.sum_abs_diff(pb, qb, Cin, sl.FAULTS[3]))
