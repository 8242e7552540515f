"""Option surface of vid2vid's test.py / test_fifo.py / train.py as the reference drives it.

Flag names used by the reference (must parse and behave): text2video_audio.sh:42, README.md:171-176,
212-214.  The remaining upstream names and their defaults follow SURVEY.md Appendix B [RECALL];
unknown flags are ignored with a warning so that a fork-specific flag does not abort a run.
"""
import argparse
import os
import sys


def _common(p):
    g = p.add_argument
    g("--name", type=str, default="label2city")
    g("--gpu_ids", type=str, default="0")
    g("--checkpoints_dir", type=str, default="./checkpoints")
    g("--model", type=str, default="vid2vid")
    g("--norm", type=str, default="batch", choices=["batch", "instance"])
    g("--fp16", action="store_true", help="accepted, ignored: the reduced-precision mode of the MI355X path is --arith bf16x2")
    g("--arith", type=str, default="fp32", choices=["fp32", "bf16x2"], help="fp32: every kernel in exact fp32; bf16x2 "
      "(inference only): the ResnetBlock trunk's Winograd GEMMs on the bf16 matrix cores with fp32 operands split into two "
      "bf16 terms (~16 mantissa bits per product, fp32 accumulation; everything else stays fp32).  Measured: 512x512 frames "
      "1.30x faster; 2.2e-5 of a conv's output rms against 1.8e-7 in fp32, frames 1.8e-4 from float64 against 2.7e-5 "
      "(DESIGN.md section 0)")
    g("--arith_layers", type=str, default=None, choices=["trunk", "trunk+stride2"], help="with --arith bf16x2, the layers "
      "that run in split-bf16 arithmetic: trunk (what --arith bf16x2 alone selects): the ResnetBlock convs; trunk+stride2: "
      "also the polyphase stride-2 and transposed layers (the 81 GEMMs of each on the same kernel; the float64 emulation of "
      "one such conv is 1.7e-5 of its output's rms from the exact one)")
    g("--arith_outer", action="store_true", help="with --arith bf16x2 --arith_layers trunk+stride2: also the stride-2 and "
      "transposed layers that run as direct convolutions (128 <-> 256 channels), their contraction in the same split-bf16 "
      "arithmetic where that measured faster; the norm apply pass in front of such a layer stores the two bf16 terms of each "
      "value in place of it")
    g("--batchSize", type=int, default=1,
      help="train.py: clips per optimiser step over all ranks (devices in --gpu_ids).  Up to the number of ranks the batch "
      "is one clip per rank; above it, it must be a multiple of the ranks and every rank walks batchSize / ranks clips per "
      "step, summing their gradients before the one exchange and optimiser step (--gpu_ids 0 --batchSize 8 trains the "
      "batch --gpu_ids 0,...,7 --batchSize 8 trains)")
    g("--loadSize", type=int, default=512)
    g("--fineSize", type=int, default=512)
    g("--input_nc", type=int, default=3)
    g("--label_nc", type=int, default=0)
    g("--output_nc", type=int, default=3)
    g("--dataroot", type=str, default="datasets/Cityscapes/")
    g("--dataset_mode", type=str, default="temporal")
    g("--resize_or_crop", type=str, default="scaleWidth")
    g("--serial_batches", action="store_true")
    g("--no_flip", action="store_true")
    g("--nThreads", type=int, default=2)
    g("--netG", type=str, default="composite")
    g("--ngf", type=int, default=128)
    g("--n_blocks", type=int, default=9)
    g("--n_downsample_G", type=int, default=3)
    g("--n_blocks_local", type=int, default=3)
    g("--n_frames_G", type=int, default=3)
    g("--n_scales_spatial", type=int, default=1)
    g("--no_first_img", action="store_true")
    g("--use_single_G", action="store_true")
    g("--fg", action="store_true")
    g("--no_flow", action="store_true")
    g("--use_instance", action="store_true")
    g("--densepose_only", action="store_true")
    g("--openpose_only", action="store_true")
    g("--remove_face_labels", action="store_true")
    g("--basic_point_only", action="store_true")
    g("--random_drop_prob", type=float, default=0.2)
    g("--n_gpus_gen", type=int, default=-1)
    g("--debug", action="store_true")
    # extensions of this implementation (not upstream)
    g("--synthetic_weights", type=int, default=None, metavar="SEED",
      help="no checkpoint: run with seeded random-init weights (plumbing / benchmarks only)")
    g("--no_pose_crop", action="store_true", help="keep the full width instead of upstream's central-width crop")
    g("--fast_pose", action="store_true", help="closed-form segment fit in the rasteriser (not bit-identical)")
    g("--no_hand_discs", action="store_true", help="do not draw the two radius-8 hand discs")
    g("--pose_workers", type=int, default=None, help="processes rasterising pose maps ahead of the GPU")
    g("--timing_json", type=str, default=None, help="write fps / per-stage timing to this file")
    g("--resident", action="store_true", help="test.py: run through the resident server (weights stay on the GPU between "
      "calls; started on first use, text2video_amd/resident.py); T2V_RESIDENT=1 does the same")
    g("--resident_idle_s", type=float, default=600.0, help="the resident server leaves after this long without a request")
    g("--resident_stop", action="store_true", help="test.py: stop the resident server of this device selection")
    g("--write_video", action="store_true", help="after the frame loop, mux every sequence's frames into "
      "results/<name>/<name>_<seq>.mp4 at 25 fps (the reference's image2video*.py stage; text2video_amd/mux.py)")
    g("--video_audio", type=str, default=None, help="--write_video: .wav / .mp3 sound track")
    g("--batch_sequences", type=int, default=2, metavar="N", help="advance up to N independent sequences (or chunks) of this "
      "rank in lock-step, one batched generator call per frame; frames are identical to N=1")
    g("--shard_chunks", action="store_true", help="multi-GPU test.py: also cut sequences into chunks so that every rank "
      "has work (each chunk restarts the recurrence; default: whole sequences only, frames identical to 1 GPU)")
    g("--chunks_per_rank", type=int, default=1, metavar="C", help="with --shard_chunks: cut as for C x the number of ranks "
      "and give every rank C chunks (BASELINE configs[2]'s 8 x 64 plan on fewer than 8 GPUs); a rank advances its chunks in "
      "lock-step (--batch_sequences)")
    g("--stitch_frames", type=int, default=0, metavar="K", help="with --shard_chunks: re-generate the first K frames of "
      "every continuation chunk from its predecessor's last frames (all-gathered over RCCL)")
    g("--stitch_rounds", type=int, default=1, help="repetitions of the stitch pass")


class BaseOptions:
    is_train = False

    def __init__(self):
        self.parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
        _common(self.parser)
        self.extra()

    def extra(self):
        pass

    def parse(self, argv=None, save=False):
        opt, unknown = self.parser.parse_known_args(argv)
        if opt.arith_layers is not None and opt.arith != "bf16x2":
            self.parser.error("--arith_layers %s: the scope of --arith bf16x2, which is not given" % opt.arith_layers)
        opt.arith_layers = opt.arith_layers or "trunk"
        if opt.arith_outer and not (opt.arith == "bf16x2" and opt.arith_layers == "trunk+stride2"):
            self.parser.error("--arith_outer: on top of --arith bf16x2 --arith_layers trunk+stride2, which %s not given"
                              % ("are" if opt.arith != "bf16x2" else "is"))
        if opt.arith_outer and self.is_train:
            self.parser.error("--arith_outer: a forward-only form of --arith bf16x2; training computes in fp32")
        if unknown:
            print("warning: ignoring unknown options %s" % unknown, file=sys.stderr)
        opt.isTrain = self.is_train
        opt.gpu_ids = [int(i) for i in str(opt.gpu_ids).split(",") if i.strip() != "" and int(i) >= 0]
        # CUDA_VISIBLE_DEVICES from the reference's shell is honoured by the ROCm runtime as well
        # (HIP reads CUDA_VISIBLE_DEVICES when HIP_VISIBLE_DEVICES is unset): nothing to translate.
        # Inference: whether --openpose_only implies no_flow upstream is a recollection; it is the default
        # here, and a checkpoint that carries a flow branch overrides it (create_model).  Training follows the
        # explicit flag only: the reference's recipe (README.md:171-176) passes --openpose_only without --no_flow,
        # and north_star names the flow-warp compositor as part of the generator.
        opt.no_flow_explicit = bool(opt.no_flow)
        if opt.openpose_only and not self.is_train:
            opt.no_flow = True
        if save:
            d = os.path.join(opt.checkpoints_dir, opt.name)
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "opt.txt"), "w") as fh:
                for k, v in sorted(vars(opt).items()):
                    fh.write("%s: %s\n" % (k, v))
        return opt


class TestOptions(BaseOptions):
    def extra(self):
        g = self.parser.add_argument
        g("--ntest", type=int, default=float("inf"))
        g("--results_dir", type=str, default="./results/")
        g("--phase", type=str, default="test")
        g("--which_epoch", type=str, default="latest")
        g("--how_many", type=int, default=300)
        g("--use_real_img", action="store_true")
        g("--start_frame", type=int, default=0)
        g("--fifo", type=str, default=None, help="test_fifo.py: named pipe to read requests from")
        g("--metrics", action="store_true", help="compare every generated frame (before JPEG) with the real frame "
          "<dataroot>/<phase>_img/<seq>/<same index> on the GPU (ops.image_metrics): PSNR, SSIM and MAE of the frame and of "
          "its face region, written to <results>/<seq>/metrics.json and under \"metrics\" in --timing_json")

        g("--metrics_temporal", action="store_true", help="--metrics plus, for every frame after a sequence's first, the "
          "temporal-consistency figures of the pair (t-1, t) against the real pair (ops.optical_flow_u8 + ops.temporal_metrics): "
          "warping error under the real flow's forward-backward mask, tOF, and the flow-free flicker term, under "
          "\"temporal\" in metrics.json and --timing_json")
        g("--temporal_flow", type=str, default=None, choices=["lk", "lkhs"], help="with --metrics_temporal: the flow estimator, "
          "lk (default) = ops.optical_flow_u8 as it is, lkhs = with the Horn-Schunck refinement (64 steps per level, alpha 0.2); "
          "the choice is named in the reports")

        g("--gpu_jpeg", action="store_true", help="encode fake_B_*.jpg / real_A_*.jpg on the GPU (ops.jpeg_encode_u8: the "
          "bytes Pillow writes) instead of copying every frame to the host and encoding it on threads there")
        g("--jpeg_quality", type=int, default=None, help="with --gpu_jpeg: the JPEG quality, 1..100 (default 75, Pillow's)")
        g("--frame_format", type=str, default="jpg", choices=["jpg", "png"], help="jpg (default): fake_B_*.jpg / real_A_*.jpg as "
          "always.  png: the same frames as lossless fake_B_*.png / real_A_*.png, encoded on the GPU (ops.png_encode_u8; a "
          "geometry it refuses is written by Pillow); not with --gpu_jpeg / --jpeg_quality.  vid2vid/image2video*.py and the "
          "mux of --write_video / the pipeline take JPEG frames only: a PNG tree is for evaluation "
          "(python -m text2video_amd.evaluate --pair_by_stem), a later re-encode or a regression diff")

    def parse(self, argv=None, save=False):
        opt = super().parse(argv, save)
        if opt.frame_format == "png" and (opt.gpu_jpeg or opt.jpeg_quality is not None):
            self.parser.error("--frame_format png with --gpu_jpeg / --jpeg_quality: those are the JPEG writer's; PNG frames are "
                              "lossless and always encoded on the GPU")
        if opt.frame_format == "png" and getattr(opt, "write_video", False):
            self.parser.error("--frame_format png with --write_video: the mux (like vid2vid/image2video*.py) takes JPEG frames only")
        if opt.jpeg_quality is not None and not opt.gpu_jpeg:
            self.parser.error("--jpeg_quality %d: the quality of --gpu_jpeg, which is not given" % opt.jpeg_quality)
        if opt.jpeg_quality is not None and not 1 <= opt.jpeg_quality <= 100:
            self.parser.error("--jpeg_quality %d is not in 1..100" % opt.jpeg_quality)
        if opt.temporal_flow is not None and not opt.metrics_temporal:
            self.parser.error("--temporal_flow %s: the estimator of --metrics_temporal, which is not given" % opt.temporal_flow)
        if opt.temporal_flow is None:
            opt.temporal_flow = "lk"
        if opt.metrics_temporal:
            opt.metrics = True
        if opt.metrics and opt.shard_chunks:
            self.parser.error("--metrics with --shard_chunks: a sequence's frames are then spread over the ranks; "
                              "evaluate whole sequences (drop --shard_chunks)")
        # test.py forces these upstream
        opt.nThreads = 1
        opt.batchSize = 1
        opt.serial_batches = True
        opt.no_flip = True
        return opt


class TrainOptions(BaseOptions):
    is_train = True

    def parse(self, argv=None, save=False):
        opt = super().parse(argv, save)
        if opt.gpu_decode and not (opt.train_loader == "prefetch" and opt.gpu_resize):
            self.parser.error("--gpu_decode: the decoder in front of --train_loader prefetch --gpu_resize, which %s not given"
                              % ("are" if opt.train_loader != "prefetch" and not opt.gpu_resize else "is"))
        if opt.flow_refine_iters is not None and opt.flow_ref != "lkhs":
            self.parser.error("--flow_refine_iters %d: the Jacobi steps of --flow_ref lkhs, which is not given"
                              % opt.flow_refine_iters)
        if opt.flow_alpha is not None and opt.flow_ref != "lkhs":
            self.parser.error("--flow_alpha %g: the smoothness weight of --flow_ref lkhs, which is not given" % opt.flow_alpha)
        if opt.flow_refine_iters is not None and not 1 <= opt.flow_refine_iters <= 1024:
            self.parser.error("--flow_refine_iters %d is not in 1..1024" % opt.flow_refine_iters)
        if opt.flow_alpha is not None and not 0 < opt.flow_alpha < float("inf"):
            self.parser.error("--flow_alpha %g is not a positive finite number" % opt.flow_alpha)
        if opt.flow_refine_iters is None:
            opt.flow_refine_iters = 64
        if opt.flow_alpha is None:
            opt.flow_alpha = 0.2
        return opt

    def extra(self):
        g = self.parser.add_argument
        g("--display_freq", type=int, default=100)
        g("--print_freq", type=int, default=100)
        g("--display_web", action="store_true", help="rank 0 writes checkpoints/<name>/web/index.html with sample pictures of "
          "the step that completes every --display_freq samples (pose, generated frame, raw frame, real frame and, with the "
          "flow branch, predicted flow, weight map, reference flow and its confidence; rendered on the GPU by "
          "ops.train_visuals) and appends every printed loss line to checkpoints/<name>/loss_log.txt; without it "
          "--display_freq has no effect (upstream: on unless --no_html)")
        g("--display_scale", type=int, default=1, choices=[1, 2, 4], help="--display_web: the pictures at 1/N of the frame's "
          "size (N x N blocks of bytes averaged)")
        g("--save_latest_freq", type=int, default=1000)
        g("--save_epoch_freq", type=int, default=1)
        g("--continue_train", action="store_true")
        g("--load_pretrain", type=str, default="")
        g("--which_epoch", type=str, default="latest")
        g("--phase", type=str, default="train")
        g("--niter", type=int, default=10)
        g("--niter_decay", type=int, default=10)
        g("--beta1", type=float, default=0.5)
        g("--lr", type=float, default=0.0002)
        g("--TTUR", action="store_true")
        g("--pool_size", type=int, default=1)
        g("--num_D", type=int, default=1)
        g("--n_layers_D", type=int, default=3)
        g("--ndf", type=int, default=64)
        g("--lambda_feat", type=float, default=10.0)
        g("--lambda_F", type=float, default=10.0)
        g("--lambda_T", type=float, default=10.0)
        g("--no_ganFeat", action="store_true")
        g("--no_vgg", action="store_true")
        g("--flow_ref", type=str, default="zero", choices=["zero", "lk", "lkhs"], help="reference flow of the flow / warp losses "
          "and the temporal discriminators' flow channels when the caller passes none (upstream: FlowNet2, not available): "
          "zero flow, lk = the dense Lucas-Kanade estimate between the real frames (ops.optical_flow), or lkhs = that "
          "estimate with a Horn-Schunck refinement at every pyramid level, which fills textureless regions "
          "(ops.optical_flow(..., refine_iters=N))")
        g("--flow_refine_iters", type=int, default=None, help="with --flow_ref lkhs: Jacobi steps per pyramid level, 1..1024 "
          "(default 64)")
        g("--flow_alpha", type=float, default=None, help="with --flow_ref lkhs: the smoothness weight alpha, grey values in "
          "[-1, 1] (default 0.2)")
        g("--train_loader", type=str, default="sync", choices=["sync", "prefetch"], help="sync: every clip is read, "
          "rasterised and resized on the main thread between optimiser steps; prefetch: the same clips prepared ahead by "
          "--nThreads rasteriser processes and decoder threads (TrainPoseDataset.iter_clips) and uploaded from pinned "
          "memory on a copy stream")
        g("--gpu_resize", action="store_true", help="with --train_loader prefetch: the frames' BICUBIC resize, crop and "
          "normalisation run on the GPU in one launch per clip (ops.resample_crop_normalize_u8, Pillow's bytes); a geometry "
          "over the kernel's tap limit is resized on the CPU")
        g("--gpu_decode", action="store_true", help="with --train_loader prefetch --gpu_resize: the frames' JPEG files are "
          "decoded on the GPU as well (ops.jpeg_decode_u8, Pillow's bytes): the loader threads read and parse, the compressed "
          "bytes are uploaded; a file the decoder does not take is decoded by Pillow")
        g("--vgg_weights", type=str, default="", help="torchvision vgg19 state dict (.pth) for the perceptual loss; the "
          "reference lets torchvision download it, which this tree cannot")
        g("--vgg_random_init", action="store_true", help="run the VGG loss path on seeded random weights (timing / tests)")
        g("--no_lsgan", action="store_true")
        g("--n_frames_D", type=int, default=3)
        g("--n_scales_temporal", type=int, default=2)
        g("--max_frames_per_gpu", type=int, default=1)
        g("--max_frames_backpropagate", type=int, default=1)
        g("--max_t_step", type=int, default=1)
        g("--n_frames_total", type=int, default=30)
        g("--niter_step", type=int, default=5)
        g("--niter_fix_global", type=int, default=0)
        g("--add_face_disc", action="store_true")
        g("--synthetic_data", action="store_true", help="train on seeded synthetic sequences (no dataset needed)")
