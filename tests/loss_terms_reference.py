"""loss_terms_kernel / loss_terms_final_kernel (csrc/elementwise.hip; train.LossBook builds their tables): the terms the tests
feed them, their float64 values, their gradient seeds restated in fp32, and the bound the values are held to.

A plain helper module (no fixtures, no pytest hooks; numpy only), imported by tests/test_cpu_loss_terms.py and
tests/test_gpu_loss_terms.py.

Values.  A term's value is v * sum(t_i) with v = weight / n and t_i = (a[i, 0] - c)^2 (op 0, "mse") or |a_i - b_i| (op 1,
"l1"); a "zero" term (op 2) has no value.  The reference takes t_i in float64 from the fp32 operands.

Seeds are not approximate: they are one or two fp32 operations per element and are compared bit for bit.
  op 0: fl(fl(2 s) * fl(a - c)) in channel 0 (2 s is exact), +0.0 in channels 1 .. cs-1       (s = fl32(weight / n))
  op 1: +s, -s or +0.0 by the sign of fl(a - b); a tie -- +0.0 against -0.0 included -- gives +0.0
  op 2: +0.0

Bound: |got - v sum t_i| <= gamma(k) |v| sum|t_i|, gamma(k) = k u / (1 - k u), u = 2^-24, with k the longest chain of fp32
roundings one t_i goes through on its way into the value (the library is built with -ffp-contract=off: no fused
multiply-add shortens it).  Read off the kernels, for a block of 256 threads and chunks of `chunk` elements:
    per element      op 0: the difference and the square (2); op 1: the difference (1; fabsf is exact)
    chunk kernel     scalar loop (op 0 always; op 1 when an operand or the seed is not 16-byte aligned): thread j adds
                     elements j, j + 256, ...: ceil(L / 256) adds for the first one, L = min(n, chunk)
                     float4 body (op 1, aligned): ceil(L / 1024) adds of a 4-wide sum, whose tree is 2 adds deep, + 1 add
                     where the same thread then takes a scalar-tail element
    block_sum        6 __shfl_xor levels + 4 wave sums (10)
    final kernel     thread j adds partials j, j + 256, ...: ceil(chunks / 256) adds, then block_sum again (10)
    value scale      the product with v (1) and v's own conversion to fp32 (1: LossBook stores weight / n as a float)
k does not grow with n except through ceil(chunks / 256).  With chunk = 16384 and one final-pass add: 89 for op 0, 88 for
the scalar op 1, 43 for the float4 op 1."""
import collections
import math

import numpy as np

U = 2.0 ** -24
BLOCK = 256
BIG = 50.0          # against operands of unit variance
NAN_BITS = 0x7FC00000

# label: unique; kind: "mse" | "l1" | "zero"; name: LossBook's (several terms may share one) or None; a: fp32 [n, cs] (mse) or
# [n] (l1); b: fp32 [n] (l1); seeded: the term writes a seed; shifted: None, or which of "a" / "b" / "seed" is taken as
# base[1:1 + n] of a larger buffer, so that its address is 4 mod 16 and the kernel must leave the float4 path
Term = collections.namedtuple("Term", "label kind name n cs target weight seeded shifted a b")


def gamma(k):
    return k * U / (1.0 - k * U)


def vector_path(term):
    """the float4 body runs: op 1 with every operand (and the seed) 16-byte aligned"""
    return term.kind == "l1" and term.shifted is None


def chain_length(term, chunk):
    """k of the module docstring"""
    L = min(term.n, chunk)
    chunks = max(1, -(-term.n // chunk))
    per_element = 2 if term.kind == "mse" else 1
    loop = (-(-L // (4 * BLOCK)) + 2 + 1) if vector_path(term) else -(-L // BLOCK)
    return per_element + loop + 10 + -(-chunks // BLOCK) + 10 + 2


def _edges(n, chunk):
    """the positions an off-by-one would lose: the last element, the first element after each chunk edge, and the elements
    of the last chunk's scalar tail (those past its last whole group of 4)"""
    idx = {n - 1}
    idx.update(range(chunk, n, chunk))
    last0 = (n - 1) // chunk * chunk
    idx.update(range(last0 + (n - last0) // 4 * 4, n))
    return sorted(idx)


def _operands(rng, n, chunk):
    a = rng.standard_normal(n).astype(np.float32)
    for j, i in enumerate(_edges(n, chunk)):
        a[i] = BIG if j % 2 == 0 else -BIG
    return a


def build_terms(chunk):
    """Every term of the one LossBook.run() the GPU test makes, in order.  Sizes come from `chunk` (LossBook.CHUNK)."""
    rng = np.random.default_rng(20)
    terms = []

    def mse(n, cs, target, seeded):
        a = (rng.standard_normal((n, cs)) * 7.0).astype(np.float32)      # the pad channels hold junk the kernel must not read
        a[:, 0] = _operands(rng, n, chunk)
        terms.append(Term("mse_n%d_cs%d_t%g_%s" % (n, cs, target, "seed" if seeded else "noseed"), "mse",
                          "GAN_real" if target else "GAN_fake", n, cs, target, 0.5 if target else 1.0, seeded, None, a, None))

    def l1(label, n, name, weight=2.5, seeded=True, shifted=None, ties=None):
        a, b = _operands(rng, n, chunk), rng.standard_normal(n).astype(np.float32)
        if ties is not None:
            lo, hi = ties
            b[lo:hi] = a[lo:hi]
            a[lo], b[lo] = 0.0, -0.0                 # +0.0 against -0.0 and the other way round: fl(a - b) is +0.0 / -0.0
            a[lo + 1], b[lo + 1] = -0.0, 0.0
            assert np.signbit(b[lo]) and np.signbit(a[lo + 1])
        terms.append(Term(label, "l1", name, n, 1, 0.0, weight, seeded, shifted, a, b))

    def zero(n):
        terms.append(Term("zero_n%d_%d" % (n, len(terms)), "zero", None, n, 1, 0.0, 0.0, True, None, None, None))

    sizes = (1, 255, chunk, chunk + 1, 2 * chunk + 5)
    for n in sizes:
        for cs in (1, 4):
            mse(n, cs, 1.0, True)
            mse(n, cs, 0.0, True)
        zero(1)                                       # valued terms with rows of zeros between them
    for n in (1, 3, 4, 5, 1023, chunk - 1, chunk, chunk + 1, chunk + 7, 3 * chunk + 7):
        l1("l1_n%d" % n, n, "GAN_Feat")               # ten terms under one name: read() sums them
    zero(chunk + 3)
    for which in ("a", "b", "seed"):
        l1("l1_shifted_%s" % which, chunk + 7, "Feat_shifted_" + which, weight=10.0 / 3.0, shifted=which)
    l1("l1_ties", 2 * chunk + 3, "Feat_ties", ties=(chunk - 40, chunk - 8))
    l1("l1_ties_tail", 7, "Feat_ties", ties=(4, 6))   # ties in a scalar tail (a[6], the last element, stays large)
    zero(1)
    l1("l1_noseed_n5", 5, "Feat_noseed", seeded=False)
    l1("l1_noseed", chunk + 7, "Feat_noseed", seeded=False)
    for n in sizes:
        for cs in (1, 4):
            mse(n, cs, 1.0, False)
            mse(n, cs, 0.0, False)
    assert len({t.label for t in terms}) == len(terms)
    return terms


# ---- the float64 value; `fault` restates one way the kernels could be wrong -------------------------------------------------
VALUE_FAULTS = ("last element dropped", "first element of a chunk counted twice", "scalar tail dropped",
                "one chunk's partial left out", "value scale 1/(n*cs)")
SEED_FAULTS = ("last element dropped", "scalar tail dropped", "pad channels left unwritten", "tie seeded as +s")


def terms64(term):
    if term.kind == "mse":
        return (term.a[:, 0].astype(np.float64) - float(np.float32(term.target))) ** 2
    return np.abs(term.a.astype(np.float64) - term.b.astype(np.float64))


def value64(term, chunk, fault=None):
    """(value, sum |v t_i|) of a valued term in float64, summed chunk by chunk as the two kernels do"""
    assert term.kind != "zero"
    t, n = terms64(term), term.n
    v = term.weight / (n * term.cs if fault == "value scale 1/(n*cs)" else n)
    parts = []
    for off in range(0, n, chunk):
        seg = t[off:min(n, off + chunk)]
        s = math.fsum(seg)
        if fault == "last element dropped" and off + chunk >= n:
            s -= seg[-1]
        if fault == "first element of a chunk counted twice" and off > 0:
            s += seg[0]
        if fault == "scalar tail dropped" and vector_path(term):
            s = math.fsum(seg[:len(seg) // 4 * 4])
        parts.append(s)
    if fault == "one chunk's partial left out" and len(parts) > 1:
        parts = parts[:-1]
    return v * math.fsum(parts), abs(term.weight / n) * math.fsum(t)


def value_bound(term, chunk):
    return gamma(chain_length(term, chunk)) * value64(term, chunk)[1]


# ---- the seeds, in the kernel's own fp32 arithmetic -----------------------------------------------------------------------
def seeds32(term, chunk, fault=None):
    """the fp32 seed block (mse: [n, cs]; l1, zero: [n]) a seeded term must leave, bit for bit; with `fault`, what a kernel
    with that fault would leave in a NaN-filled buffer"""
    assert term.seeded
    nan = np.float32(np.nan)
    if term.kind == "zero":
        return np.zeros(term.n, np.float32)
    s = np.float32(term.weight / term.n)
    if term.kind == "mse":
        d = term.a[:, 0] - np.float32(term.target)                          # fl(a - c)
        out = np.full((term.n, term.cs), nan if fault == "pad channels left unwritten" else 0.0, np.float32)
        out[:, 0] = (np.float32(2.0) * s) * d                               # fl(fl(2 s) * d)
    else:
        d = term.a - term.b                                                 # fl(a - b)
        tie = s if fault == "tie seeded as +s" else np.float32(0.0)
        out = np.where(d > 0, s, np.where(d < 0, -s, tie)).astype(np.float32)
        if fault == "scalar tail dropped" and vector_path(term):
            last0 = (term.n - 1) // chunk * chunk
            out[last0 + (term.n - last0) // 4 * 4:] = nan
    assert out.dtype == np.float32
    if fault == "last element dropped":
        out.reshape(term.n, -1)[-1, :] = nan
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def seed_mismatches(want, got):
    """elements whose bits differ (-0.0 for +0.0 and any NaN included)"""
    want, got = bits(want), bits(got)
    assert want.shape == got.shape, (want.shape, got.shape)
    return int((want != got).sum())
