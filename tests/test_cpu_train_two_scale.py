"""Two-scale training (--n_scales_spatial 2, --niter_fix_global) without a GPU: the local generator's parameter set, the
freeze schedule, and the trainer's flag guard."""
import pytest
import torch


@pytest.mark.parametrize("no_flow", [False, True], ids=["flow", "noflow"])
@pytest.mark.parametrize("norm", ["batch", "instance"])
def test_local_generator_has_the_oracles_parameter_names_and_shapes(no_flow, norm):
    from oracle.generator_ref import CompositeLocalGenerator
    from text2video_amd import train as T
    from text2video_amd.generator import GeneratorSpec, layer_keys, synthetic_state_dict
    ngf_global, blocks = 16, 2
    ref = CompositeLocalGenerator(9, 3, 6, ngf_global=ngf_global, n_blocks_local=blocks, scale=1, no_flow=no_flow, norm=norm)
    want = {k: tuple(v.shape) for k, v in ref.named_parameters()}
    assert set(want) == {k for k in ref.state_dict() if "running_" not in k and "num_batches" not in k}
    spec = GeneratorSpec(ngf=ngf_global // 2, n_blocks=blocks, no_flow=no_flow, norm=norm, is_local=True, scale=1)
    net = T.TrainableLocalGenerator(spec, synthetic_state_dict(spec, 2, "vid2vid"), "cpu")
    got = {k: tuple(v.shape) for k, v in net.named_upstream_parameters().items()}
    assert got == want
    assert all(p.device.type == "cpu" and p.requires_grad for p in net.parameters())
    # ... which is layer_keys(local spec): the modules of upstream's CompositeLocalGenerator and no other
    convs = [c for ck, _, _ in layer_keys(spec) for c in ((ck,) if isinstance(ck, str) else ck)]
    assert {c + ".weight" for c in convs} == {k for k, s in want.items() if len(s) == 4}
    assert {k.split(".")[0] for k in got} =={"model_down_seg", "model_down_img", "model_up_img", "model_final_img"} | \
        (set() if no_flow else {"model_up_flow", "model_final_flow", "model_final_w"})


def test_each_generator_class_refuses_the_other_ones_spec():
    from text2video_amd import train as T
    from text2video_amd.generator import GeneratorSpec, synthetic_state_dict
    local = GeneratorSpec(ngf=8, n_blocks=1, is_local=True, scale=1)
    with pytest.raises(ValueError, match="TrainableLocalGenerator"):
        T.TrainableGenerator(local, synthetic_state_dict(local, 1), "cpu")
    glob = GeneratorSpec(ngf=8, n_downsample=1, n_blocks=1)
    with pytest.raises(ValueError, match="TrainableGenerator"):
        T.TrainableLocalGenerator(glob, synthetic_state_dict(glob, 1), "cpu")


@pytest.mark.parametrize("n,frozen_epochs", [(0, []), (1, [1]), (3, [1, 2, 3])])
def test_freeze_schedule_around_the_boundary(n, frozen_epochs):
    from text2video_amd.train import global_generator_frozen
    assert [e for e in range(1, n + 4) if global_generator_frozen(e, n)] == frozen_epochs
    assert not global_generator_frozen(n + 1, n)          # the first joint epoch
    assert global_generator_frozen(n, n) == (n >= 1)      # the last frozen one


def _opt(*extra):
    from text2video_amd.options import TrainOptions
    return TrainOptions().parse(["--name", "t", "--dataset_mode", "pose", "--input_nc", "3", "--openpose_only", "--ngf", "16",
                                 "--n_downsample_G", "2", "--n_blocks", "2", "--num_D", "2", "--ndf", "16", "--no_vgg",
                                 "--max_frames_per_gpu", "2", "--n_scales_temporal", "0", "--no_first_img"] + list(extra))


def test_flag_guard_refuses_three_scales_and_lets_two_pass_before_any_device_work():
    from text2video_amd import train as T
    with pytest.raises(NotImplementedError, match="--n_scales_spatial: two spatial scales are built"):
        T.Vid2VidTrainer(_opt("--n_scales_spatial", "3"), "cuda:0")
    # two scales pass the guard: the constructor goes on to build the nets.  Nothing before that touches a device, so a
    # net constructor that raises is reached (and a guard that still refused the flag would raise its own error instead)
    reached = []

    class Reached(Exception):
        pass

    def stop(*a, **k):
        reached.append(a[0])
        raise Reached()

    orig = T.TrainableGenerator.__init__
    T.TrainableGenerator.__init__ = stop
    try:
        with pytest.raises(Reached):
            T.Vid2VidTrainer(_opt("--n_scales_spatial", "2", "--niter_fix_global", "1"), "cuda:0")
    finally:
        T.TrainableGenerator.__init__ = orig
    assert len(reached) == 1


def test_two_scale_generator_refuses_a_frame_the_pyramid_cannot_halve():
    from text2video_amd import train as T
    from text2video_amd.generator import GeneratorSpec, synthetic_state_dict
    s0 = GeneratorSpec(ngf=8, n_downsample=2, n_blocks=1)
    s1 = GeneratorSpec(ngf=4, n_downsample=2, n_blocks=1, is_local=True, scale=1)
    G = T.TwoScaleGenerator(T.TrainableGenerator(s0, synthetic_state_dict(s0, 1), "cpu"),
                            T.TrainableLocalGenerator(s1, synthetic_state_dict(s1, 2), "cpu"))
    G.check_geometry(64, 48)
    with pytest.raises(ValueError, match=r"36 x 64 .* multiple of 8 = 2\^\(n_downsample_G 2 \+ 1\)"):
        G.check_geometry(36, 64)
    # G0's three head convolutions (weight and bias each) are the ones the trainer keeps out of the optimiser
    assert len(G.head_params()) == 6 and all(p.dim() in (1, 4) for p in G.head_params())
