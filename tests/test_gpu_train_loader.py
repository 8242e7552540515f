"""train.py --train_loader {sync, prefetch, prefetch --gpu_resize} on a real-layout dataset: the three loaders feed the
trainer the same numbers, so every loss of every optimiser step and every saved generator tensor is identical.

The tiny recipe of test_train_py_on_a_real_layout_dataset (ngf 16, 2 blocks, 128 px), in-process through
run_train(opt, steps=3): two 3-frame clips in epoch 1, then --niter_step 1 doubles the clip length, so the third clip is
drawn ahead of the boundary it lies behind."""
import os
import shutil

import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keypoints_fadg0")


@pytest.fixture(scope="module")
def dataroot(tmp_path_factory):
    from text2video_amd.keypoints import read_keypoints
    root = tmp_path_factory.mktemp("train_loader") / "fadg0"
    files = sorted(f for f in os.listdir(GOLD) if f.startswith("sa1_"))
    for seq in ("clipA", "clipB"):
        os.makedirs(root / "train_openpose" / seq)
        os.makedirs(root / "train_img" / seq)
        for i, f in enumerate(files + files[::-1]):
            shutil.copyfile(os.path.join(GOLD, f), root / "train_openpose" / seq / ("%04d_keypoints.json" % i))
            Image.fromarray(read_keypoints(os.path.join(GOLD, f), (256, 192))).save(root / "train_img" / seq / ("%04d.jpg" % i))
    return root


def _run(dataroot, ckpt, extra, monkeypatch):
    """-> ([losses dict of every optimiser step], {generator tensor name: tensor}, [clip geometry lines])"""
    from text2video_amd import train as T
    from text2video_amd.options import TrainOptions
    opt = TrainOptions().parse(
        ["--name", "fadg0", "--dataroot", str(dataroot), "--checkpoints_dir", str(ckpt), "--dataset_mode", "pose",
         "--input_nc", "3", "--openpose_only", "--num_D", "2", "--resize_or_crop", "randomScaleHeight_and_scaledCrop",
         "--loadSize", "136", "--fineSize", "128", "--batchSize", "1", "--max_frames_per_gpu", "2", "--no_first_img",
         "--n_frames_total", "3", "--max_t_step", "2", "--niter_step", "1", "--add_face_disc", "--random_drop_prob", "0",
         "--ngf", "16", "--n_blocks", "2", "--niter", "2", "--niter_decay", "1", "--nThreads", "2"] + extra)
    steps = []
    inner = T.Vid2VidTrainer.train_step

    def recording(self, *a, **k):
        losses, prev = inner(self, *a, **k)
        steps.append({name: float(v) for name, v in losses.items()})
        return losses, prev

    monkeypatch.setattr(T.Vid2VidTrainer, "train_step", recording)
    torch.manual_seed(0)
    stats = T.run_train(opt, steps=3)
    assert stats["steps"] == 3
    sd = torch.load(os.path.join(str(ckpt), "fadg0", "latest_net_G0.pth"), map_location="cpu")
    return steps, sd


@pytest.fixture(scope="module")
def sync_run(dataroot, tmp_path_factory):
    mp = pytest.MonkeyPatch()
    try:
        return _run(dataroot, tmp_path_factory.mktemp("ck_sync"), [], mp)
    finally:
        mp.undo()


@pytest.mark.parametrize("extra", [["--train_loader", "prefetch"], ["--train_loader", "prefetch", "--gpu_resize"]],
                         ids=["prefetch", "prefetch_gpu_resize"])
def test_loaders_train_identically(dataroot, sync_run, tmp_path, monkeypatch, extra):
    want_steps, want_sd = sync_run
    # 2 clips of 3 frames (2 chunks each), then one of 6 frames (3 chunks) behind the epoch boundary
    assert len(want_steps) == 7 and all("G_GAN" in s and "F_Flow" in s for s in want_steps)
    if "--gpu_resize" in extra:      # the kernel is what ran: count its launches, one per clip
        from text2video_amd import ops
        calls, inner = [], ops.resample_crop_normalize_u8
        monkeypatch.setattr(ops, "resample_crop_normalize_u8", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    got_steps, got_sd = _run(dataroot, tmp_path / "ck", extra, monkeypatch)
    if "--gpu_resize" in extra:
        assert len(calls) == 3
    assert len(got_steps) == len(want_steps)
    for i, (g, w) in enumerate(zip(got_steps, want_steps)):
        assert g == w, "optimiser step %d: %s" % (i, {k: (g.get(k), w.get(k)) for k in set(g) | set(w) if g.get(k) != w.get(k)})
    assert got_sd.keys() == want_sd.keys()
    for k in want_sd:
        assert torch.equal(got_sd[k], want_sd[k]), k
