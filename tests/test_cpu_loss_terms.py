"""tests/loss_terms_reference.py against itself, on the CPU: the reference is the definition (weight * mean, and its gradient),
the kernel's summation order emulated in fp32 stays inside the bound, and the checks tests/test_gpu_loss_terms.py makes can
see the faults they are meant to catch -- each fault moves a checked value by >= 10x its bound or flips seed bits."""
import math

import numpy as np
import torch

import loss_terms_reference as lr

CHUNK = 1 << 11       # the structure (chunk edges, tails, several partials) at a size the CPU emulation walks quickly


def _cases():
    return lr.build_terms(CHUNK)


def test_cases_cover_the_paths_the_issue_names():
    terms = _cases()
    kinds = {t.kind for t in terms}
    assert kinds == {"mse", "l1", "zero"}
    l1 = [t for t in terms if t.kind == "l1"]
    assert {t.shifted for t in l1} == {None, "a", "b", "seed"}
    assert {t.n for t in l1 if t.name == "GAN_Feat"} == {1, 3, 4, 5, 1023, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 7, 3 * CHUNK + 7}
    mse = [t for t in terms if t.kind == "mse"]
    assert {(t.n, t.cs, t.target, t.seeded) for t in mse} == {
        (n, cs, tg, sd) for n in (1, 255, CHUNK, CHUNK + 1, 2 * CHUNK + 5) for cs in (1, 4) for tg in (0.0, 1.0) for sd in (True, False)}
    assert {t.n for t in terms if t.kind == "zero"} == {1, CHUNK + 3}
    # valued terms with zero terms between them, names shared by several terms
    order = [t.kind for t in terms]
    assert any(order[i] == "zero" and order[i - 1] != "zero" and order[i + 1] != "zero" for i in range(1, len(order) - 1))
    names = [t.name for t in terms if t.name]
    assert max(names.count(n) for n in set(names)) >= 2
    # the large elements: the last one, the first after each chunk edge, the scalar tail
    for t in l1:
        if "ties" in t.label:
            continue
        for i in lr._edges(t.n, CHUNK):
            assert abs(t.a[i]) == lr.BIG, (t.label, i)
    assert lr._edges(CHUNK + 7, CHUNK) == [CHUNK, CHUNK + 4, CHUNK + 5, CHUNK + 6]
    assert lr._edges(2 * CHUNK, CHUNK) == [CHUNK, 2 * CHUNK - 1]


def test_reference_is_the_weighted_mean_and_its_gradient():
    for t in _cases():
        if t.kind == "zero":
            assert not lr.bits(lr.seeds32(t, CHUNK)).any()
            continue
        a = torch.from_numpy(t.a.astype(np.float64)).requires_grad_()
        if t.kind == "mse":
            loss = t.weight * ((a[:, 0] - t.target) ** 2).mean()
        else:
            loss = t.weight * (a - torch.from_numpy(t.b.astype(np.float64))).abs().mean()
        value, scale = lr.value64(t, CHUNK)
        assert abs(value - loss.item()) <= 1e-12 * scale, t.label
        if t.seeded:
            (g,) = torch.autograd.grad(loss, a)
            s = lr.seeds32(t, CHUNK).astype(np.float64).reshape(g.shape)
            # the weight's conversion, the difference (relative to the difference: exact ties stay 0) and the product
            assert np.all(np.abs(s - g.numpy()) <= 3 * 2.0 ** -23 * np.abs(g.numpy()) + 1e-30), t.label
            if t.kind == "mse" and t.cs > 1:
                assert not lr.bits(s.astype(np.float32)[:, 1:]).any()


def test_chain_lengths_at_the_library_chunk():
    mk = lambda kind, n, shifted=None: lr.Term("x", kind, "x", n, 1, 0.0, 1.0, True, shifted, None, None)
    C = 1 << 14
    assert lr.chain_length(mk("mse", 2 * C + 5), C) == 89
    assert lr.chain_length(mk("l1", C + 7, "a"), C) == 88
    assert lr.chain_length(mk("l1", 3 * C + 7), C) == 43
    assert lr.chain_length(mk("l1", 1), C) == 28 and lr.chain_length(mk("l1", 300 * C), C) == 44


def _block_sum32(per_thread):
    """block_sum of csrc/elementwise.hip in fp32: six xor-shuffle levels inside each wave of 64, then the wave sums in order"""
    v = per_thread.astype(np.float32).reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, np.arange(64) ^ o]
    tot = np.float32(0.0)
    for w in range(4):
        tot = np.float32(tot + v[w, 0])
    return tot


def _emulate32(term, chunk):
    """the value the two kernels give, in their own order and fp32 arithmetic"""
    n, f32 = term.n, np.float32
    parts = []
    for off in range(0, n, chunk):
        end = min(n, off + chunk)
        s = np.zeros(lr.BLOCK, f32)
        if term.kind == "mse":
            d = term.a[off:end, 0] - f32(term.target)
            e, body = d * d, 0
        else:
            d = np.abs(term.a[off:end] - term.b[off:end])
            body = (end - off) // 4 * 4 if lr.vector_path(term) else 0
            q = d[:body].reshape(-1, 4)
            q = (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])
            for i0 in range(0, len(q), lr.BLOCK):
                row = q[i0:i0 + lr.BLOCK]
                s[:len(row)] += row
            e = d
        for i0 in range(body, end - off, lr.BLOCK):
            row = e[i0:i0 + lr.BLOCK]
            s[:len(row)] += row
        parts.append(_block_sum32(s))
    parts = np.array(parts, f32)
    s = np.zeros(lr.BLOCK, f32)
    for i0 in range(0, len(parts), lr.BLOCK):
        row = parts[i0:i0 + lr.BLOCK]
        s[:len(row)] += row
    return float(f32(_block_sum32(s) * f32(term.weight / n)))


def test_the_kernels_own_summation_order_stays_well_inside_the_bound():
    worst = {}
    for t in _cases():
        if t.kind == "zero":
            continue
        r = abs(_emulate32(t, CHUNK) - lr.value64(t, CHUNK)[0]) / lr.value_bound(t, CHUNK)
        key = "float4" if lr.vector_path(t) else "scalar"
        worst[key] = max(worst.get(key, 0.0), r)
        assert r <= 0.25, (t.label, r)
    print("emulated fp32 order, worst |value - f64| / bound: %s" % worst)


def test_value_bound_and_seed_bits_see_injected_faults():
    terms = _cases()
    lines = []
    for fault in lr.VALUE_FAULTS:
        ratios = {}
        for t in terms:
            if t.kind == "zero":
                continue
            ref, faulty = lr.value64(t, CHUNK)[0], lr.value64(t, CHUNK, fault)[0]
            if faulty != ref:
                ratios[t.label] = abs(faulty - ref) / lr.value_bound(t, CHUNK)
        assert ratios, "%s: touches no term" % fault
        lo = min(ratios, key=ratios.get)
        lines.append("value | %-40s touches %2d terms, |fault - ref| / bound >= %.3g (%s)" % (fault, len(ratios), ratios[lo], lo))
        # every term the fault touches, not just one: the large elements sit where each fault bites
        assert ratios[lo] >= 10.0, lines[-1]
    for fault in lr.SEED_FAULTS:
        flipped = {}
        for t in terms:
            if not t.seeded:
                continue
            k = lr.seed_mismatches(lr.seeds32(t, CHUNK), lr.seeds32(t, CHUNK, fault))
            if k:
                flipped[t.label] = k
        lines.append("seeds | %-40s flips bits in %2d terms" % (fault, len(flipped)))
        assert flipped, lines[-1]
    print("\n".join(lines))
    # which terms each fault must reach
    assert lr.value64(terms[0], CHUNK, "last element dropped")[0] == 0.0                      # n = 1: the only element
    tail = [t for t in terms if lr.vector_path(t) and t.n % 4]
    assert all(lr.value64(t, CHUNK, "scalar tail dropped")[0] != lr.value64(t, CHUNK)[0] for t in tail) and len(tail) >= 6
    ties = [t for t in terms if "ties" in t.label]
    assert all(lr.seed_mismatches(lr.seeds32(t, CHUNK), lr.seeds32(t, CHUNK, "tie seeded as +s")) >= 2 for t in ties) and len(ties) == 2


def test_seed_comparison_is_bitwise():
    z = np.zeros(3, np.float32)
    assert lr.seed_mismatches(z, -z) == 3 and lr.seed_mismatches(z, z) == 0
    nan = np.full(2, np.nan, np.float32)
    assert (lr.bits(nan) == lr.NAN_BITS).all() and lr.seed_mismatches(nan, np.zeros(2, np.float32)) == 2
    assert math.isclose(lr.gamma(89), 89 * lr.U, rel_tol=1e-5)
