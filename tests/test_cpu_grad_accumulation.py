"""CPU tests (no GPU) of --batchSize above the number of ranks: the batch rule, the global clip slots, and GradBuckets summing
the gradients of K clips (micro-steps) on host tensors -- alone and between two gloo ranks -- bit for bit
((g_0 + g_1) + ... + g_{K-1}) * fp32(1 / K), then the mean over the ranks."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_the_batch_rule():
    from text2video_amd.gradients import clips_per_rank
    assert clips_per_rank(1, 1) == (1, None)
    assert clips_per_rank(8, 8) == (1, None)
    assert clips_per_rank(1, 8) == (1, None)
    k, warn = clips_per_rank(2, 8)      # below the ranks: one clip per rank as before, with the warning as before
    assert k == 1 and warn == "warning: --batchSize 2, but the batch is one clip per rank = 8 (list 2 devices in --gpu_ids)"
    assert clips_per_rank(8, 1) == (8, None)
    assert clips_per_rank(8, 2) == (4, None)
    assert clips_per_rank(8, 4) == (2, None)
    with pytest.raises(ValueError, match=r"--batchSize 8 .* 3 ranks"):
        clips_per_rank(8, 3)


def test_the_slot_schedule_does_not_depend_on_the_layout():
    from text2video_amd.gradients import clip_slots
    for it in (0, 1, 7, 1000):
        want = list(range(it * 8, it * 8 + 8))
        for world, K in ((8, 1), (2, 4), (1, 8)):
            per_rank = [clip_slots(it, r, world, K) for r in range(world)]
            assert all(len(p) == K for p in per_rank)
            flat = [sc for p in per_rank for sc in p]      # in rank order
            assert [s for s, _ in flat] == list(range(8)) and [c for _, c in flat] == want, (it, world, K)
    # K = 1: the clip every rank read before there were slots
    for world in (1, 2, 8):
        for it in (0, 3):
            for rank in range(world):
                assert clip_slots(it, rank, world, 1) == [(rank, it * world + rank)]


# ---- GradBuckets over K = 3 micro-steps -----------------------------------------------------------------------------------
SIZES = (6, 70000, 3, 1 << 18, 17, 40)      # the parameter sizes of test_cpu_distributed._buckets_worker
# backward nodes per parameter in each micro-step: parameter 2 is delivered in micro-step 1 only, parameter 5 never
USES = ([1, 2, 0, 3, 1, 0], [2, 1, 1, 1, 1, 0], [1, 3, 0, 2, 1, 0])
K = len(USES)


def _node(rank, step, j, i, k):
    g = torch.Generator().manual_seed(((rank * 7 + step) * 5 + j) * 1000 + i * 10 + k)
    return torch.randn(SIZES[i], generator=g)


def _want(rank, step, i):
    """the fp32 fold of parameter i's micro-step gradients on `rank`, each the sum of its nodes in arrival order"""
    total = None
    for j in range(K):
        gj = np.zeros(SIZES[i], np.float32)
        for k in range(USES[j][i]):
            n = _node(rank, step, j, i, k).numpy()
            gj = n.copy() if k == 0 else gj + n
        total = gj if total is None else total + gj
    assert total.dtype == np.float32
    return total * np.float32(1.0 / K)


def _accumulate(world, rank):
    from text2video_amd import train as T
    params = [torch.nn.Parameter(torch.zeros(n)) for n in SIZES]
    gb = T.GradBuckets(params, bucket_mb=0.5)
    assert len(gb.bounds) >= 3 and gb.acc is None
    issued, inner = [], gb._issue
    gb._issue = lambda b: (issued.append(b), inner(b))[1]
    payload = 4 * sum(SIZES) if world > 1 else 0
    for step in range(2):          # the accumulator persists across optimiser steps and starts over in each
        for j in range(K):
            gb.begin_step(micro=(j, K))
            for p, u in zip(params, USES[j]):
                for _ in range(u):
                    T.expect_gradient(p)
            gb.seal()
            for i in reversed(range(len(params))):
                for k in range(USES[j][i]):
                    T.deliver(T.grad_slot(params[i]), _node(rank, step, j, i, k))
            assert gb._launched >= 1          # buckets complete (and fold) from inside the "backward pass"
            gb.absorb([None] * len(params))
            if j < K - 1:
                assert not issued and not gb._works and gb.finish() == 0      # no collective before the last micro-step
            else:
                assert issued == (list(range(len(gb.bounds))) if world > 1 else [])
                assert gb.finish() == payload == gb.nbytes                    # counted once per optimiser step
        del issued[:]
        assert gb.acc is not None and gb.acc.shape == gb.flat.shape
        for i, p in enumerate(params):
            if i == 5:
                assert p.grad is None
                continue
            assert p.grad is not None and p.grad.data_ptr() == gb.slots[i].view.data_ptr()
            want = _want(0, step, i)
            if world > 1:       # gloo sums, finish() scales by fp32(1 / 2)
                want = (want + _want(1, step, i)) * np.float32(0.5)
            assert np.array_equal(p.grad.numpy(), want), (step, i, float(np.abs(p.grad.numpy() - want).max()))
        T.check_presence_across_ranks([gb], "cpu")
    # a micro-step out of order is an error, not a wrong sum
    gb.begin_step(micro=(0, K))
    with pytest.raises(RuntimeError, match="micro-step"):
        gb.begin_step(micro=(2, K))
    # begin_step() without an argument: one clip per step as before, no accumulator
    gb1 = T.GradBuckets([torch.nn.Parameter(torch.zeros(n)) for n in SIZES], bucket_mb=0.5)
    for step in range(2):
        gb1.begin_step()
        for p, u in zip(gb1.params, USES[0]):
            for _ in range(u):
                T.expect_gradient(p)
        gb1.seal()
        for i in reversed(range(len(SIZES))):
            for k in range(USES[0][i]):
                T.deliver(T.grad_slot(gb1.params[i]), _node(rank, step, 0, i, k))
        gb1.absorb([None] * len(SIZES))
        assert gb1.finish() == payload and gb1.acc is None
        for i, p in enumerate(gb1.params):
            if USES[0][i] == 0:
                assert p.grad is None
                continue
            sums = []
            for r in range(world):
                t = None
                for k in range(USES[0][i]):
                    n = _node(r, step, 0, i, k).numpy()
                    t = n.copy() if t is None else t + n
                sums.append(t)
            want = sums[0] if world == 1 else (sums[0] + sums[1]) * np.float32(0.5)
            assert np.array_equal(p.grad.numpy(), want), (step, i)


def test_a_slot_written_in_one_micro_step_loses_its_record_of_zeros():
    """deliver(zero=True) records that a slot's memory holds zeros and later steps skip the memset.  The last micro-step's
    fold rewrites the whole bucket with the mean: a slot a kernel wrote in an earlier micro-step is not zero afterwards, whatever
    its last micro-step delivered, so the next step's zero delivery must write zeros again."""
    from text2video_amd import train as T
    params = [torch.nn.Parameter(torch.zeros(n)) for n in (5, 300)]
    gb = T.GradBuckets(params, bucket_mb=0.5)
    sl = gb.slots[0]
    for step, real_first in enumerate((True, False, False)):
        for j in range(2):
            gb.begin_step(micro=(j, 2))
            for p in params:
                T.expect_gradient(p)
            gb.seal()
            T.deliver(T.grad_slot(params[1]), torch.ones(300))
            if real_first and j == 0:
                T.deliver(T.grad_slot(params[0]), torch.full((5,), 3.0))
            else:
                T.deliver(T.grad_slot(params[0]), zero=True)
            gb.absorb([None, None])
            gb.finish()
        want = 1.5 if real_first else 0.0
        assert torch.equal(params[0].grad, torch.full((5,), want)), (step, params[0].grad)
        assert sl.zero_valid is (not real_first)        # zeros on record only where zeros are what the slot holds
        assert torch.equal(params[1].grad, torch.ones(300))


def test_grad_buckets_fold_three_micro_steps_without_a_process_group():
    assert not dist.is_initialized()
    _accumulate(1, 0)


def _worker(rank, world, port):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), T2V_GRAD_RS_AG="0")
    from text2video_amd import distributed as D
    D.init_from_env("gloo")
    _accumulate(world, rank)
    dist.barrier()
    dist.destroy_process_group()


def test_grad_buckets_fold_three_micro_steps_between_two_gloo_ranks():
    mp.spawn(_worker, args=(2, _free_port()), nprocs=2, join=True)
