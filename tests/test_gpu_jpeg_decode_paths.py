"""The two callers of the GPU JPEG decoder give what they gave without it:

* `python -m text2video_amd.evaluate --gpu_decode` (evaluate.compare_trees): the same report, value for value, on two small
  trees with a PNG pair among the JPEG ones;
* `train.py --train_loader prefetch --gpu_resize --gpu_decode`: the check of tests/test_gpu_train_loader.py restated on the
  same tiny dataset geometry -- every loss of every optimiser step and every saved generator tensor is identical to the
  `--gpu_resize` run.  One source file is progressive, so that one whole clip takes the "raw" route."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_reference as D  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keypoints_fadg0")


@pytest.fixture(scope="module")
def dec_built(lib_built):
    from text2video_amd import _jpegdeclib
    if not os.path.exists(_jpegdeclib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _jpegdeclib.load()


def test_evaluate_gives_the_same_report_with_gpu_decode(dec_built, tmp_path):
    from text2video_amd import evaluate
    a, b = tmp_path / "a", tmp_path / "b"
    for root, quality in ((a, 75), (b, 90)):
        for seq in ("s1", "s2"):
            os.makedirs(root / seq)
        for i in range(6):
            img = D.make_image("smooth" if i % 2 else "pose", 48, 64)
            img = np.roll(img, 3 * i, axis=1)
            Image.fromarray(img).save(root / ("s1" if i < 4 else "s2") / ("fake_B_%04d.jpg" % i), quality=quality,
                                      optimize=bool(i == 2))
        Image.fromarray(D.make_image("edges", 48, 64) // (1 if quality == 75 else 2)).save(root / "s2" / "fake_B_0009.png")
    want = evaluate.compare_trees(str(a), str(b), temporal=True)
    fallback = []
    got = evaluate.compare_trees(str(a), str(b), temporal=True, gpu_decode=True, fallback=fallback)
    assert want["overall"]["frames"] == 7 and want["overall"]["temporal"]["pairs"] == 5 and not want["size_mismatch"]
    assert got == want
    assert sorted(os.path.basename(f) for f, _ in fallback) == ["fake_B_0009.png"] * 2 and "not a JPEG" in fallback[0][1]
    # the command itself, on the torch-free provider it runs on by default: the same report in its --json file
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "T2V_LEAN"}
    r = subprocess.run([sys.executable, "-m", "text2video_amd.evaluate", str(a), str(b), "--temporal", "--gpu_decode", "--json",
                        str(tmp_path / "report.json")], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert "Pillow decoded 2 file(s)" in r.stderr
    assert json.load(open(tmp_path / "report.json")) == json.loads(json.dumps(want))


TRAIN_ARGS = ["--name", "fadg0", "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only", "--num_D", "2",
              "--resize_or_crop", "randomScaleHeight_and_scaledCrop", "--loadSize", "136", "--fineSize", "128", "--batchSize", "1",
              "--max_frames_per_gpu", "2", "--no_first_img", "--n_frames_total", "3", "--max_t_step", "2", "--niter_step", "1",
              "--add_face_disc", "--random_drop_prob", "0", "--ngf", "16", "--n_blocks", "2", "--niter", "2", "--niter_decay", "1",
              "--nThreads", "2", "--train_loader", "prefetch", "--gpu_resize"]


def _options(dataroot, ckpt, extra):
    from text2video_amd.options import TrainOptions
    return TrainOptions().parse(TRAIN_ARGS + ["--dataroot", str(dataroot), "--checkpoints_dir", str(ckpt)] + extra)


@pytest.fixture(scope="module")
def dataroot(tmp_path_factory):
    """the dataset of tests/test_gpu_train_loader.py; the first frame the run's second clip reads is a progressive file.
    (The clips' frames follow from the options, the sequence lengths and the image size alone: drawn here the way
    TrainPoseDataset.iter_clips draws them, rank 0's generator, clips 0 and 1 of 3 frames.)"""
    from text2video_amd.keypoints import read_keypoints
    from text2video_amd.pose_dataset import TrainPoseDataset, get_train_img_params, get_video_params
    root = tmp_path_factory.mktemp("train_decode") / "fadg0"
    files = sorted(f for f in os.listdir(GOLD) if f.startswith("sa1_"))
    for seq in ("clipA", "clipB"):
        os.makedirs(root / "train_openpose" / seq)
        os.makedirs(root / "train_img" / seq)
        for i, f in enumerate(files + files[::-1]):
            shutil.copyfile(os.path.join(GOLD, f), root / "train_openpose" / seq / ("%04d_keypoints.json" % i))
            Image.fromarray(read_keypoints(os.path.join(GOLD, f), (256, 192))).save(root / "train_img" / seq / ("%04d.jpg" % i))
    opt = _options(root, tmp_path_factory.mktemp("unused"), [])
    ds = TrainPoseDataset(opt, seed=1000)
    for index in (0, 1):
        seq = ds.seqs[index % len(ds.seqs)]
        n, start, step = get_video_params(opt, 3, len(ds.op[seq]), ds.rng)
        get_train_img_params(opt, (256, 192), ds.rng)
    victim = ds.img[seq][start]
    with Image.open(victim) as im:
        assert im.size == (256, 192)
    json_of = os.path.join(str(root), "train_openpose", seq, "%04d_keypoints.json" % start)
    Image.fromarray(read_keypoints(json_of, (256, 192))).save(victim, progressive=True)
    return root


def _run(dataroot, ckpt, extra):
    """-> ([losses dict of every optimiser step], {generator tensor name: tensor}, {"jpeg": clips decoded on the GPU,
    "raw": clips that went the raw way})"""
    from text2video_amd import pose_dataset as P
    from text2video_amd import train as T
    opt = _options(dataroot, ckpt, extra)
    steps, routes = [], {"jpeg": 0, "raw": 0, "calls": 0}
    inner = T.Vid2VidTrainer.train_step

    def recording(self, *a, **k):
        losses, prev = inner(self, *a, **k)
        steps.append({name: float(v) for name, v in losses.items()})
        return losses, prev

    assemble = P._assemble_jpeg_clip

    def routed(*a, **k):
        out = assemble(*a, **k)
        routes[out[0]] += 1
        return out

    decode = T._ClipFeeder._decode

    def counted(self, clip, slot):
        routes["calls"] += 1
        return decode(self, clip, slot)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(T.Vid2VidTrainer, "train_step", recording)
        mp.setattr(P, "_assemble_jpeg_clip", routed)
        mp.setattr(T._ClipFeeder, "_decode", counted)
        torch.manual_seed(0)
        stats = T.run_train(opt, steps=3)
    assert stats["steps"] == 3
    sd = torch.load(os.path.join(str(ckpt), "fadg0", "latest_net_G0.pth"), map_location="cpu")
    return steps, sd, routes


def test_gpu_decode_trains_identically(dec_built, dataroot, tmp_path):
    want_steps, want_sd, routes = _run(dataroot, tmp_path / "ck_resize", [])
    assert len(want_steps) == 7 and routes == {"jpeg": 0, "raw": 0, "calls": 0}
    got_steps, got_sd, routes = _run(dataroot, tmp_path / "ck_decode", ["--gpu_decode"])
    # three clips consumed: the second holds the progressive file and goes the raw way whole, the other two are decoded on
    # the GPU (the loader works ahead: it may have assembled and staged clips the three steps never took)
    assert routes["calls"] >= 2 and routes["raw"] >= 1 and routes["jpeg"] >= 2, routes
    assert len(got_steps) == len(want_steps)
    for i, (g, w) in enumerate(zip(got_steps, want_steps)):
        assert g == w, "optimiser step %d: %s" % (i, {k: (g.get(k), w.get(k)) for k in set(g) | set(w) if g.get(k) != w.get(k)})
    assert got_sd.keys() == want_sd.keys()
    for k in want_sd:
        assert torch.equal(got_sd[k], want_sd[k]), k
