"""--batchSize above the number of ranks on the GPU: K clips per rank and optimiser step (train_step(micro=(j, K))).

Trainer level: with both learning rates at 0 the weights stay put, so the gradient an optimiser step leaves in p.grad can be
compared with the gradients of the same clips stepped one at a time: bit for bit ((g_0 + g_1) + ...) * fp32(1 / K), the
parameters without gradient those no clip delivered to, over two chunks per clip (the carried FIFO and the temporal
discriminators' frame history are each clip's own).  End to end: vid2vid/train.py --batchSize 2 on two ranks and on one
writes the same checkpoint; with a dataset both loaders feed the same batch."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "keypoints_fadg0")
DEV = "cuda:0"
NARROW = ["--ngf", "16", "--n_blocks", "2", "--n_downsample_G", "2", "--ndf", "16", "--num_D", "2", "--fineSize", "64",
          "--max_frames_per_gpu", "2", "--no_vgg", "--add_face_disc"]
S, F_, CHUNKS = 64, 2, 2


def _trainer(seed=5):
    from text2video_amd import train as T
    from text2video_amd.options import TrainOptions
    opt = TrainOptions().parse(["--name", "t", "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only", "--no_first_img"]
                               + NARROW)
    assert not opt.no_flow and opt.n_scales_temporal == 2
    tr = T.Vid2VidTrainer(opt, DEV, seed=seed)
    tr.optG.lr = tr.optD.lr = 0.0
    return tr


def _clip(c):
    """clip c: CHUNKS chunks of F_ frames (pose, real, real_prev, face boxes); clip 1 shows no face"""
    rng = np.random.default_rng(40 + c)
    n = CHUNKS * F_
    pose = torch.zeros(n, S, S, 12, device=DEV)
    pose[..., :9] = torch.from_numpy(np.where(rng.random((n, S, S, 1)) < 0.05, rng.uniform(-1, 1, (n, S, S, 9)), -1.0)
                                     .astype(np.float32)).to(DEV)
    frames = torch.zeros(n + 1, S, S, 4, device=DEV)
    frames[..., :3] = torch.tanh(torch.from_numpy(rng.standard_normal((n + 1, S, S, 3)).astype(np.float32))).to(DEV)
    boxes = None if c == 1 else [(8, 40, 16, 48)] * F_
    return [(pose[k * F_:(k + 1) * F_], frames[1 + k * F_:1 + (k + 1) * F_], frames[k * F_:(k + 1) * F_], boxes)
            for k in range(CHUNKS)]


def _grads(tr):
    return [None if p.grad is None else p.grad.detach().cpu().numpy().copy() for p in tr.optG.params + tr.optD.params]


def _one_at_a_time(clips, folds):
    """the clips in lock-step, every chunk of every clip an optimiser step of its own (K = 1): -> [chunk][clip] gradients.
    The trainer's frame history is handed from a clip's chunk to its next by hand."""
    tr = _trainer()
    prev, hist = [None] * len(clips), [([], [])] * len(clips)
    out = []
    for k in range(CHUNKS):
        out.append([])
        for c, clip in enumerate(clips):
            pose, real, real_prev, boxes = clip[k]
            tr._hist_real, tr._hist_fake = hist[c]
            _, prev[c] = tr.train_step(pose, real, boxes, prev[c], real_prev=real_prev)
            hist[c] = (tr._hist_real, tr._hist_fake)
            out[-1].append(_grads(tr))
    assert not folds, "a step of one clip per rank launched the fold"
    return out, tr


def _accumulated(clips):
    """-> [chunk] gradients after the optimiser step over the K clips' chunk, the trainer"""
    tr, K = _trainer(), len(clips)
    prev, out = [None] * K, []
    for k in range(CHUNKS):
        for j, clip in enumerate(clips):
            pose, real, real_prev, boxes = clip[k]
            _, prev[j] = tr.train_step(pose, real, boxes, prev[j], real_prev=real_prev, micro=(j, K))
        out.append(_grads(tr))
    return out, tr


@pytest.fixture(scope="module")
def fold_calls():
    """every ops.grad_fold call of this module's trainers is counted here"""
    from text2video_amd import ops
    mp = pytest.MonkeyPatch()
    calls, inner = [], ops.grad_fold
    mp.setattr(ops, "grad_fold", lambda *a, **k: (calls.append(a[2]), inner(*a, **k))[1])
    yield calls
    mp.undo()


def test_a_single_clip_step_repeats_its_gradient_bits(fold_calls):
    """the precondition of everything below"""
    pose, real, real_prev, boxes = _clip(0)[0]
    tr = _trainer()
    runs = []
    for _ in range(2):
        tr.train_step(pose, real, boxes, None, real_prev=real_prev)
        runs.append(_grads(tr))
    assert any(g is not None for g in runs[0])
    for i, (a, b) in enumerate(zip(*runs)):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), i
    assert not fold_calls


@pytest.mark.parametrize("K", [2, 3])
def test_accumulated_gradients_are_the_fp32_fold_of_the_clips_gradients(K, fold_calls):
    from text2video_amd import ops
    from text2video_amd.train import running_stats
    clips = [_clip(c) for c in range(K)]
    del fold_calls[:]
    single, tr1 = _one_at_a_time(clips, fold_calls)
    got, tr = _accumulated(clips)
    # OPEN, ADD ..., CLOSE per bucket and optimiser step
    nb = len(tr.bucketsG.bounds) + len(tr.bucketsD.bounds)
    assert sorted(fold_calls) == sorted(CHUNKS * nb * ([ops.GRAD_FOLD_OPEN] + [ops.GRAD_FOLD_ADD] * (K - 2) + [ops.GRAD_FOLD_CLOSE]))
    params = tr.optG.params + tr.optD.params
    present = []
    for k in range(CHUNKS):         # the second chunk: every clip came back to its own FIFO and frame history
        present.append([])
        for i, p in enumerate(params):
            parts = [single[k][c][i] for c in range(K)]
            present[-1].append(any(g is not None for g in parts))
            if not present[-1][-1]:
                assert got[k][i] is None, (k, i)
                continue
            total = None
            for g in parts:
                g = np.zeros(p.numel(), np.float32).reshape(tuple(p.shape)) if g is None else g
                total = g if total is None else total + g
            want = total * np.float32(1.0 / K)
            assert want.dtype == np.float32 and got[k][i] is not None
            assert np.array_equal(got[k][i], want), (k, i, float(np.abs(got[k][i] - want).max()))
    # the union differs from every single clip's set (clip 1 has no face terms) and between the chunks (the temporal
    # discriminators have their first full window in the second)
    assert [g is not None for g in single[0][1]] != present[0] and present[0] != present[1]
    # Adam: one step per optimiser step and parameter with a gradient
    steps = tr.optG.steps + tr.optD.steps
    assert steps == [int(present[0][i]) + int(present[1][i]) for i in range(len(params))] and max(steps) == CHUNKS
    # BatchNorm running statistics moved with clip 0 only: 1 / K of the updates the K single-clip steps made
    counted = 0
    for p, p1 in zip(tr.D.parameters(), tr1.D.parameters()):
        rs, rs1 = running_stats(p, create=False), running_stats(p1, create=False)
        if rs1 is not None and rs1[2]:
            counted += 1
            assert rs is not None and rs[2] * K == rs1[2], (rs and rs[2], rs1[2])
    assert counted > 0


def _checkpoint(directory):
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "latest_net_*.pth"))):
        for k, v in torch.load(path, map_location="cpu").items():
            out[os.path.basename(path) + ":" + k] = v
    return out


def test_train_py_batch_of_two_on_two_ranks_and_on_one_write_the_same_checkpoint(tmp_path):
    """--batchSize 2 as two ranks of one clip (gloo transport, both on this GPU) and as one rank of two clips: the global
    clip slots see the same data, the gradient is (g_0 + g_1) * 0.5 either way, BatchNorm running statistics follow slot 0."""
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="0", T2V_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    args = [os.path.join(ROOT, "vid2vid", "train.py"), "--name", "dp", "--dataset_mode", "pose", "--input_nc", "3",
            "--openpose_only", "--no_first_img"] + NARROW + ["--batchSize", "2", "--niter", "2", "--niter_decay", "0",
                                                              "--synthetic_data"]
    two = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29571"] + args + ["--checkpoints_dir", str(tmp_path / "two")]
    one = [sys.executable] + args + ["--gpu_ids", "0", "--checkpoints_dir", str(tmp_path / "one")]
    outs = []
    for cmd in (two, one):
        r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        outs.append(r.stdout)
    assert "replicas in sync after 2 steps" in outs[0] and "done: 2 steps" in outs[1]
    assert "warning: --batchSize" not in outs[0] and "warning: --batchSize" not in outs[1]
    a, b = _checkpoint(str(tmp_path / "two" / "dp")), _checkpoint(str(tmp_path / "one" / "dp"))
    assert a.keys() == b.keys() and any(k.endswith("running_mean") for k in a) and len({k.split(":")[0] for k in a}) >= 3
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert (tmp_path / "one" / "dp" / "iter.txt").read_text() == (tmp_path / "two" / "dp" / "iter.txt").read_text()


@pytest.fixture(scope="module")
def dataroot(tmp_path_factory):
    """the dataset of tests/test_gpu_train_loader.py: two sequences in the reference's layout"""
    import shutil
    from PIL import Image
    from text2video_amd.keypoints import read_keypoints
    root = tmp_path_factory.mktemp("accumulation_loader") / "fadg0"
    files = sorted(f for f in os.listdir(GOLD) if f.startswith("sa1_"))
    for seq in ("clipA", "clipB"):
        os.makedirs(root / "train_openpose" / seq)
        os.makedirs(root / "train_img" / seq)
        for i, f in enumerate(files + files[::-1]):
            shutil.copyfile(os.path.join(GOLD, f), root / "train_openpose" / seq / ("%04d_keypoints.json" % i))
            Image.fromarray(read_keypoints(os.path.join(GOLD, f), (256, 192))).save(root / "train_img" / seq / ("%04d.jpg" % i))
    return root


def test_both_loaders_feed_a_batch_of_two_clips_identically(dataroot, tmp_path, capsys):
    """one rank, --batchSize 2 on a dataset: --train_loader sync and prefetch --gpu_resize print the same losses and write
    the same checkpoint (two clips held while the next two are staged)"""
    from text2video_amd import train as T
    from text2video_amd.options import TrainOptions
    runs = []
    for name, extra in (("sync", ["--train_loader", "sync"]), ("prefetch", ["--train_loader", "prefetch", "--gpu_resize"])):
        opt = TrainOptions().parse(
            ["--name", "fadg0", "--dataroot", str(dataroot), "--checkpoints_dir", str(tmp_path / name), "--dataset_mode", "pose",
             "--input_nc", "3", "--openpose_only", "--num_D", "2", "--resize_or_crop", "randomScaleHeight_and_scaledCrop",
             "--loadSize", "136", "--fineSize", "128", "--batchSize", "2", "--max_frames_per_gpu", "2", "--no_first_img",
             "--n_frames_total", "3", "--max_t_step", "2", "--add_face_disc", "--random_drop_prob", "0", "--ngf", "16",
             "--n_blocks", "2", "--niter", "3", "--niter_decay", "0", "--nThreads", "2", "--gpu_ids", "0"] + extra)
        capsys.readouterr()
        torch.manual_seed(0)
        stats = T.run_train(opt, steps=3)
        assert stats["steps"] == 3
        out = capsys.readouterr().out
        assert "warning: --batchSize" not in out
        lines = [ln.split(") ", 1)[1] for ln in out.splitlines() if ln.startswith("(iter")]
        runs.append((lines, _checkpoint(str(tmp_path / name / "fadg0"))))
    (lines_s, ck_s), (lines_p, ck_p) = runs
    assert len(lines_s) == 3 and all("G_GAN" in ln and "F_Flow" in ln for ln in lines_s)
    assert lines_s == lines_p
    assert ck_s.keys() == ck_p.keys() and len(ck_s) > 10
    for k in ck_s:
        assert torch.equal(ck_s[k], ck_p[k]), k
