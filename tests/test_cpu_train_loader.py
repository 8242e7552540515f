"""TrainPoseDataset.iter_clips: the prefetching loader yields the clips sample() returns for the same seed and index
order -- across an epoch boundary at which the clip length changes, with and without --random_drop_prob's draws inside
the rasteriser, with the resize on the CPU or left to the GPU -- and names the file that ends a run."""
import os
import shutil

import numpy as np
import pytest
from PIL import Image

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keypoints_fadg0")


def _dataset(root):
    """the scratch dataset of test_train_dataset_sampling: two sequences of 18 / 12 frames, 256x192 images"""
    from text2video_amd.keypoints import read_keypoints
    files = sorted(f for f in os.listdir(GOLD) if f.startswith("sa1_"))
    for seq, reps in (("a", 3), ("b", 2)):
        os.makedirs(root / "train_openpose" / seq)
        os.makedirs(root / "train_img" / seq)
        for i, f in enumerate(files * reps):
            shutil.copyfile(os.path.join(GOLD, f), root / "train_openpose" / seq / ("%04d.json" % i))
            Image.fromarray(read_keypoints(os.path.join(GOLD, f), (256, 192))).save(root / "train_img" / seq / ("%04d.jpg" % i))
    return root


@pytest.fixture(scope="module")
def dataroot(tmp_path_factory):
    return _dataset(tmp_path_factory.mktemp("loader") / "ds")


def _opt(root, *extra):
    from text2video_amd.options import TrainOptions
    return TrainOptions().parse(["--name", "x", "--dataroot", str(root), "--dataset_mode", "pose", "--input_nc", "3",
                                 "--resize_or_crop", "randomScaleHeight_and_scaledCrop", "--loadSize", "136", "--fineSize",
                                 "128", "--n_frames_total", "3", "--max_t_step", "3", "--fast_pose", "--nThreads", "2"]
                                + list(extra))


def _same(got, want):
    assert set(want) <= set(got)
    for k in ("seq", "start", "t_step", "params"):
        assert got[k] == want[k], k
    for k in ("A", "B"):
        assert got[k].dtype == np.uint8 and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("drop", ["0", "0.3"])
def test_iter_clips_yields_the_clips_of_sample(dataroot, drop):
    """Two epochs of two clips with update_training_batch in between: one iter_clips call per epoch, and one call drawn
    across the boundary with the clip length stated per index."""
    from text2video_amd.pose_dataset import TrainPoseDataset
    extra = ["--random_drop_prob", drop] + (["--remove_face_labels"] if drop != "0" else [])
    opt = _opt(dataroot, *extra)
    twin = TrainPoseDataset(opt, seed=7)
    want = [twin.sample(i) for i in (0, 1)]
    twin.update_training_batch(1)
    want += [twin.sample(i) for i in (2, 3)]
    assert want[0]["A"].shape[0] == 3 + 2 and want[2]["A"].shape[0] == 6 + 2       # the length did change
    if drop != "0":       # the draws inside the rasteriser matter: another seed gives other maps for the same frames
        other = TrainPoseDataset(opt, seed=8)
        assert any(not np.array_equal(o["A"], w["A"]) for o, w in zip([other.sample(i) for i in (0, 1)], want))

    ds = TrainPoseDataset(opt, seed=7)
    got = list(ds.iter_clips(range(0, 2), ahead=2))
    ds.update_training_batch(1)
    got += list(ds.iter_clips(range(2, 4), ahead=1))
    assert len(got) == 4
    for g, w in zip(got, want):
        _same(g, w)
    # the generator is where sample() left its twin's: the next clip agrees too
    _same(ds.sample(4), twin.sample(4))

    ds = TrainPoseDataset(opt, seed=7)
    got = list(ds.iter_clips([(0, 3), (1, 3), (2, 6), (3, 6)], ahead=3))
    for g, w in zip(got, want):
        _same(g, w)


def test_iter_clips_in_the_pump_thread_and_raw_frames(dataroot):
    """workers=0 rasterises in the pump thread; gpu_resize hands out the decoded frames in one buffer from `alloc`, and
    resizing them as sample() does gives sample()'s B."""
    from text2video_amd.pose_dataset import TrainPoseDataset
    opt = _opt(dataroot, "--random_drop_prob", "0.3")
    want = [TrainPoseDataset(opt, seed=3).sample(0)]
    made = []

    def alloc(shape):
        made.append(np.zeros(shape, np.uint8))
        return made[-1]

    (got,) = list(TrainPoseDataset(opt, seed=3).iter_clips([0], workers=0, gpu_resize=True, alloc=alloc))
    assert "B" not in got and got["size"] == (256, 192) and got["raw"].shape == (5, 192, 256, 3)
    assert any(got["raw"] is m for m in made) and any(got["A"] is m for m in made)
    assert np.array_equal(got["A"], want[0]["A"]) and got["params"] == want[0]["params"]
    (cx, cy), (cw, ch) = got["params"]["crop_pos"], got["params"]["crop_size"]
    B = np.stack([np.asarray(Image.fromarray(f).resize(got["params"]["new_size"], Image.BICUBIC)
                             .crop((cx, cy, cx + cw, cy + ch))) for f in got["raw"]])
    assert np.array_equal(B, want[0]["B"])


def test_a_missing_file_ends_the_iteration_with_its_name(tmp_path):
    from text2video_amd.pose_dataset import TrainPoseDataset
    root = _dataset(tmp_path / "ds")
    opt = _opt(root, "--random_drop_prob", "0", "--max_t_step", "1", "--n_frames_total", "30")
    ds, ds2 = TrainPoseDataset(opt, seed=1), TrainPoseDataset(opt, seed=1)      # (the file lists are read here)
    # 30 frames asked: a clip is its whole sequence
    victim = root / "train_img" / "b" / "0007.jpg"
    os.remove(victim)
    with pytest.raises(RuntimeError, match="0007.jpg"):
        list(ds.iter_clips([1]))
    victim = root / "train_openpose" / "a" / "0009.json"
    os.remove(victim)
    with pytest.raises(RuntimeError, match="0009.json"):
        list(ds2.iter_clips([0]))
