"""ops.grad_fold (libt2v_gradfold.so) against numpy in fp32, bit for bit: the three modes, sizes around the 16-byte body and
the block, every pairing of the two pointers' alignments, the scales a mean over clips uses, and nothing written outside
[0, n) of the buffer the mode writes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8           # elements on each side of a view (a multiple of 4: a view's offset alone decides its alignment modulo 16)
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 4099, (1 << 20) + 3]
SCALES = [1.0, 0.5, float(np.float32(1.0) / np.float32(3.0)), 0.125]


def _buffers(n, seed):
    """two host buffers of n + 2 GUARD + 3 floats of mixed magnitudes (sums that round)"""
    rng = np.random.default_rng(seed)
    size = n + 2 * GUARD + 3
    return [(rng.standard_normal(size) * 10.0 ** rng.integers(-3, 4, size)).astype(np.float32) for _ in range(2)]


@pytest.mark.parametrize("n", SIZES)
def test_grad_fold_matches_numpy_bit_for_bit(n):
    from text2video_amd import ops
    assert float(np.float32(SCALES[2])) == SCALES[2]
    g_host, a_host = _buffers(n, n)
    cases = [(ops.GRAD_FOLD_OPEN, 1.0), (ops.GRAD_FOLD_ADD, 1.0)] + [(ops.GRAD_FOLD_CLOSE, s) for s in SCALES]
    for go in range(4):
        for ao in range(4):     # equal alignment (the 16-byte body with a scalar head and tail) and unequal (scalar throughout)
            gs, as_ = slice(GUARD + go, GUARD + go + n), slice(GUARD + ao, GUARD + ao + n)
            for mode, scale in cases:
                g_dev, a_dev = torch.from_numpy(g_host).to(DEV), torch.from_numpy(a_host).to(DEV)
                assert g_dev[gs].data_ptr() % 16 == 4 * go and a_dev[as_].data_ptr() % 16 == 4 * ao
                want_g, want_a = g_host.copy(), a_host.copy()
                if mode == ops.GRAD_FOLD_OPEN:
                    want_a[as_] = g_host[gs]
                elif mode == ops.GRAD_FOLD_ADD:
                    want_a[as_] = a_host[as_] + g_host[gs]
                else:
                    want_g[gs] = (a_host[as_] + g_host[gs]) * np.float32(scale)
                ops.grad_fold(g_dev[gs], a_dev[as_], mode, scale)
                # whole buffers: the result, the guards on both sides, and the operand the mode only reads
                got_g, got_a = g_dev.cpu().numpy(), a_dev.cpu().numpy()
                assert np.array_equal(got_g.view(np.uint32), want_g.view(np.uint32)), (n, go, ao, mode, scale)
                assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32)), (n, go, ao, mode, scale)


def test_grad_fold_at_a_production_bucket_size_runs_every_loop_of_the_kernel():
    """The sizes above fit one trip of the kernel's plain loops.  A bucket of the 512 x 512 trainer (9,440,256 floats, here with
    an odd tail) is longer than three grid strides of 16-byte elements: the four-way unrolled loop runs, the plain loop behind
    it starts from where that one stopped, and with unequal alignments the one-float loop makes many trips."""
    from text2video_amd import ops
    n = 9440256 + 3
    # the library's grid: 8 blocks of 256 lanes per compute unit; one lane's stride in 16-byte (one-float) elements
    stride = 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256
    nvec = (n - 3) // 4
    assert nvec > 3 * stride and nvec % (4 * stride) > 0, "the size no longer reaches the unrolled loop and the loop behind it"
    assert n > 4 * stride
    g_host, a_host = _buffers(n, 7)
    third = SCALES[2]
    for go, ao in ((0, 0), (3, 3), (1, 2)):       # the 16-byte body without and with a scalar head; one float at a time
        gs, as_ = slice(GUARD + go, GUARD + go + n), slice(GUARD + ao, GUARD + ao + n)
        for mode in (ops.GRAD_FOLD_OPEN, ops.GRAD_FOLD_ADD, ops.GRAD_FOLD_CLOSE):
            g_dev, a_dev = torch.from_numpy(g_host).to(DEV), torch.from_numpy(a_host).to(DEV)
            want_g, want_a = g_host.copy(), a_host.copy()
            if mode == ops.GRAD_FOLD_OPEN:
                want_a[as_] = g_host[gs]
            elif mode == ops.GRAD_FOLD_ADD:
                want_a[as_] = a_host[as_] + g_host[gs]
            else:
                want_g[gs] = (a_host[as_] + g_host[gs]) * np.float32(third)
            ops.grad_fold(g_dev[gs], a_dev[as_], mode, third)
            assert np.array_equal(g_dev.cpu().numpy().view(np.uint32), want_g.view(np.uint32)), (go, ao, mode)
            assert np.array_equal(a_dev.cpu().numpy().view(np.uint32), want_a.view(np.uint32)), (go, ao, mode)


def test_three_clips_fold_to_the_fp32_mean():
    """OPEN, ADD, CLOSE over three gradients in one buffer pair, as GradBuckets issues them"""
    from text2video_amd import ops
    n = 70001
    rng = np.random.default_rng(3)
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    third = np.float32(1.0 / 3)
    grad, acc = torch.empty(n, device=DEV), torch.full((n,), float("nan"), device=DEV)      # (OPEN never reads acc)
    for j, g in enumerate(gs):
        grad.copy_(torch.from_numpy(g))
        ops.grad_fold(grad, acc, (ops.GRAD_FOLD_OPEN, ops.GRAD_FOLD_ADD, ops.GRAD_FOLD_CLOSE)[j], float(third))
    assert np.array_equal(grad.cpu().numpy(), ((gs[0] + gs[1]) + gs[2]) * third)
    assert np.array_equal(acc.cpu().numpy(), gs[0] + gs[1])


def test_refusals_reach_python_with_the_library_s_message():
    from text2video_amd import ops
    x, y = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    with pytest.raises(ValueError, match="elements"):
        ops.grad_fold(x, y[:32], ops.GRAD_FOLD_ADD)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.grad_fold(x[:40], x[24:], ops.GRAD_FOLD_ADD)
    with pytest.raises(RuntimeError, match="scale"):
        ops.grad_fold(x, y, ops.GRAD_FOLD_CLOSE, 0.0)
    with pytest.raises(RuntimeError, match="mode"):
        ops.grad_fold(x, y, 7)
    assert float(x.abs().sum()) == 0.0 and float(y.abs().sum()) == 0.0
