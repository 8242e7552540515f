"""loss_terms_kernel and loss_terms_final_kernel (csrc/elementwise.hip) through train.LossBook, against float64 values and
bit-exact seeds (tests/loss_terms_reference.py; tests/test_cpu_loss_terms.py shows what these checks can see).

All terms go into ONE LossBook.run(), so the chunk tables span terms: mse rows of 1 .. 2 CHUNK + 5 logits with 1 and 4
channels, targets 0 and 1, seeded and not; l1 terms of 1 .. 3 CHUNK + 7 elements on the float4 path, the same term with a,
b or the seed at an address that is 4 mod 16 (the scalar fallback), exact ties, l1 without a seed, rows of zeros between the
valued terms, several terms under one name.  An element 50x the others sits wherever an off-by-one would lose it.

Every seed is a slice of a larger NaN-filled buffer: after the run the slice holds the expected bits and the margins on
both sides still hold the NaN they were filled with -- an overrun shows there, inside the allocation.  The profiler must
show both kernels, and a second run over the same operands must give the same bits."""
import numpy as np
import pytest
import torch

import kernel_variants as kv
import loss_terms_reference as lr

pytestmark = pytest.mark.gpu
MARGIN = 64           # fp32 elements (256 bytes: a slice behind it keeps the allocation's alignment)


def _dev():
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return torch.device("cuda:0")


def _profiled(fn):
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {kv.normalise(e.name) for e in prof.events() if "t2v::" in e.name}


def _operand(arr, shifted, dev):
    """(keep-alive buffer, device tensor of arr's shape); shifted: the tensor is base[1:1 + n], 4 bytes past 16-byte alignment"""
    n = arr.size
    base = torch.full((n + 2 if shifted else n,), 0.25, device=dev)
    view = (base[1:1 + n] if shifted else base).view(arr.shape)
    view.copy_(torch.from_numpy(arr))
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 if shifted else 0)
    return base, view


def _seed_buffer(shape, shifted, dev):
    """(NaN-filled base, the seed slice inside it, the slice's first element in base)"""
    n = int(np.prod(shape))
    lo = 1 if shifted else MARGIN
    base = torch.full((lo + n + MARGIN,), float("nan"), device=dev)
    seed = base[lo:lo + n].view(shape)
    assert seed.is_contiguous() and seed.data_ptr() % 16 == (4 if shifted else 0)
    return base, seed, lo


def _enqueue(book, terms, ops_):
    for t, (a, b, seed) in zip(terms, ops_):
        if t.kind == "mse":
            book.mse(t.name, a, t.target, t.weight, seed=seed)
        elif t.kind == "l1":
            book.l1(t.name, a, b, t.weight, seed=seed)
        else:
            book.zero(seed)


def test_values_against_float64_and_seeds_bit_for_bit_in_one_run():
    from text2video_amd import ops
    from text2video_amd import train as T
    dev = _dev()
    chunk = T.LossBook.CHUNK
    terms = lr.build_terms(chunk)
    # every operand, seed and base buffer stays referenced from these lists until the last synchronize below
    keep, operands, seeds = [], [], []
    for t in terms:
        a = b = None
        if t.kind != "zero":
            base, a = _operand(t.a, t.shifted == "a", dev)
            keep.append(base)
        if t.kind == "l1":
            base, b = _operand(t.b, t.shifted == "b", dev)
            keep.append(base)
        entry = None
        if t.seeded:
            shape = (t.n, t.cs) if t.kind == "mse" else (t.n,)
            entry = _seed_buffer(shape, t.shifted == "seed", dev)
        seeds.append(entry)
        operands.append((a, b, entry[1] if entry else None))

    runs = []
    for rep in range(2):
        for entry in seeds:
            if entry:
                entry[0].fill_(float("nan"))
        book = T.LossBook(dev)
        _enqueue(book, terms, operands)
        assert len(book.terms) == len(terms)
        if rep == 0:
            ran = _profiled(book.run)
        else:
            book.run()
        torch.cuda.synchronize()
        ops.check_async_errors()
        runs.append((book.out.cpu().numpy().copy(), book.read(), [e[0].cpu().numpy().copy() if e else None for e in seeds]))
    assert {"t2v::loss_terms_kernel", "t2v::loss_terms_final_kernel"} <= ran, ran
    out, named, bases = runs[0]
    assert out.shape == (len(terms),) and out.dtype == np.float32

    # values, term by term
    worst = {}
    by_name = {}
    for i, t in enumerate(terms):
        if t.kind == "zero":
            assert lr.bits(out[i:i + 1])[0] == 0, (t.label, out[i])
            continue
        ref, bound = lr.value64(t, chunk)[0], lr.value_bound(t, chunk)
        r = abs(float(out[i]) - ref) / bound
        key = "%s %s" % (t.kind, "float4" if lr.vector_path(t) else "scalar")
        if r > worst.get(key, (-1.0, ""))[0]:
            worst[key] = (r, t.label)
        assert np.isfinite(out[i]) and r <= 1.0, "%s: got %.9g, float64 %.9g, |d| / bound %.3g (k = %d)" % (
            t.label, out[i], ref, r, lr.chain_length(t, chunk))
        s = by_name.setdefault(t.name, [0.0, 0.0])
        s[0] += ref
        s[1] += bound
    for key in sorted(worst):
        print("loss_terms %-10s worst |got - ref| / bound %.3g (%s)" % (key, worst[key][0], worst[key][1]))
    # read(): the by-name sums (fp32 values added in double on the host)
    assert sorted(named) == sorted(by_name)
    for name, (ref, bound) in by_name.items():
        r = abs(named[name] - ref) / bound
        print("loss_terms read() %-16s |got - ref| / bound %.3g" % (name, r))
        assert r <= 1.0, (name, named[name], ref)

    # seeds: the expected bits inside, the fill's NaN on both sides
    checked = 0
    for t, entry, base in zip(terms, seeds, bases):
        if entry is None:
            continue
        lo, n = entry[2], t.n * t.cs
        want = lr.seeds32(t, chunk).reshape(-1)
        bad = lr.seed_mismatches(want, base[lo:lo + n])
        assert bad == 0, "%s: %d of %d seed elements differ, first at %d" % (
            t.label, bad, n, int(np.nonzero(lr.bits(want) != lr.bits(base[lo:lo + n]))[0][0]))
        assert (lr.bits(base[:lo]) == lr.NAN_BITS).all() and (lr.bits(base[lo + n:]) == lr.NAN_BITS).all(), \
            "%s: the margin around the seed slice was written" % t.label
        checked += n
    print("loss_terms seeds: %d elements of %d terms bit-equal, margins untouched" % (checked, sum(e is not None for e in seeds)))

    # the second run: the same bits everywhere
    out2, named2, bases2 = runs[1]
    assert np.array_equal(lr.bits(out), lr.bits(out2)) and named == named2
    for b1, b2 in zip(bases, bases2):
        assert (b1 is None) == (b2 is None) and (b1 is None or np.array_equal(lr.bits(b1), lr.bits(b2)))
    del keep, operands, seeds
