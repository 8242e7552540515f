"""Float64 reference, ReLU masks, the per-algorithm fp32 yardstick and the case table for the generator's backward pass
(text2video_amd/train.py: TrainableGenerator, TrainableLocalGenerator, TwoScaleGenerator through _ConvBlock, _CatParams and
_WarpComposite; text2video_amd/gradients.py: the Winograd-domain weight gradient collected over a clip's frames, the kept
input transform, the paired direct weight gradient, the flush).

A plain helper module (no fixtures, no hooks), shared by tests/test_cpu_generator_gradient_reference.py, which checks the
masked oracle against plain autograd, the Winograd restatement against F.conv2d, the conditions on every case's seeds and
the bound against injected faults, and by tests/test_gpu_generator_gradients.py, which runs the HIP modules.  U, FACTOR,
FLOOR, rel_err, bound, to_nhwc, to_nchw, format_rows and _MaskedLeaky are tests/module_gradient_reference.py's.

The comparison:
  * the reference is the project's own oracle (oracle.generator_ref.CompositeGenerator / CompositeLocalGenerator: stock
    torch.nn) in float64 with every nn.ReLU replaced by a site that records its pre-activation z in execution order and
    differentiates with a SUPPLIED mask (None: z > 0, plain autograd).  The oracle executes its ReLUs in the order of the
    conv_block calls of TrainableGenerator.forward / TrainableLocalGenerator.forward (model_down_seg, model_down_img,
    model_res_img, model_up_img, model_res_flow, model_up_flow), so the k-th relu=1 norm-apply call of the HIP forward is the
    k-th site; of a two-scale frame G0's sites come first, then G1's;
  * the loss is the linear functional sum <R, out> / (H W) over fake, raw, flow (2 channels) and weight of every frame, with
    fixed random R: on the HIP side the R are the grad_outputs;
  * error per tensor: ||t - t64||_2 / ||t64||_2;  bound per tensor: max(FACTOR x e32, FLOOR), e32 the error of the YARDSTICK:
    the same masked module in fp32 torch on the CPU under the same masks, in which every 3x3 stride-1 reflect-pad
    convolution (the ResnetBlock convs) is restated in the noisiest Winograd form the HIP path uses for that layer, forward
    or data gradient (winograd_level): F(4x4,3x3) anywhere -> the F(4x4) restatement, else F(2x2,3x3) anywhere -> F(2x2),
    else F.conv2d.  The restatement (winograd_conv) is torch ops only, so autograd through it is the Winograd-domain weight
    gradient and the transposed data gradient in fp32.  A bound taken from direct fp32 convolution cannot hold for a layer
    that runs F(4x4): its rounding noise is 2.5 .. 5 x the direct kernel's per layer;
  * the kink of a ReLU: a HIP mask may differ from the float64 sign only where |z64| <= delta, delta = 5 x bound(e32_z) x
    rms(z64), e32_z the yardstick's error of that pre-activation (a ReLU's output says nothing about z on the negative side,
    so delta comes from z itself);
  * the warp: the bilinear warp's derivative jumps at integer sample positions and at the border, and the cell the HIP kernel
    chose cannot be observed, so the seeds keep every float64 sample coordinate of a composited frame at least
    delta_w = max(1e-4 px, 20 x max |flow32 - flow64|) away from an integer (warp_condition).

No case takes the polyphase form of a stride-2 / transposed layer (ops.polyphase_pays is asserted false for every such layer:
it needs both channel counts >= 256): the yardstick has no polyphase restatement, training through polyphase layers is out
of scope here.

Sizes.  The algorithm a ResnetBlock conv takes is the library's choice (fewest GEMM rows), queried by layer_algorithms where
the library loads and written down in Case.wino so that the CPU checks need no library.  With ngf 32, n_downsample 2 (128
channels at H/4 x W/4) the library takes the direct kernel at 8x8, F(2x2) at 16x16 and F(4x4) from 24x24 on, and the
transposed data gradient needs H and W multiples of 4.  So the cases that are for the Winograd-domain weight gradient run
96x96 frames (bottleneck 24x24), the ragged one 88x104 (22x26: 6 x 7 tiles, the last row and column of tiles half outside;
its data gradient is the full-correlation form -- the transposed one is not offered for ragged shapes).  Those four cases
composite no frame (use_raw_only with the flow branch on: fake is raw, flow and weight are in the loss all the same): with
the F(4x4) yardstick's flow error of 1e-5 px delta_w is 2e-4 px there, within which about 7 of a 96x96 frame's 18432 sample
coordinates fall -- of the first five seeds tried per frame none had fewer than 4.  The warp's adjoint is compared in the
32x32 and 64x64 cases, G1's F(4x4) trunk behind it in `pair`.

Seeds (searched on the CPU, seeds x_seed = 1, 2, ... per frame until the conditions held; the figures are printed by
tests/test_cpu_generator_gradient_reference.py):
  * at most KINK_SHARE = 1e-4 of a case's ReLU elements lie within delta of the kink;
  * the warp condition above, flows < 8 px and > 0.05 px on average;
  * every tensor's bound(e32) <= BOUND_CAP = 2e-4, a tenth of what tests/test_gpu_train_step.py allows.
Outcome: the first seed of every frame that composites nothing.  Of the composited frames a seed was kept only where the
closest sample coordinate is also 2 x delta_w or more from an integer (3e-4 px at 32x32 and 32x48, 2.2e-4 px at 64x64), so
that another machine's fp32 rounding of the yardstick's flow cannot move delta_w across it: g0_direct took its 2nd seed,
g0_direct_pair_in its 1st and 7th, the G1 cases their 1st, pair's frames the 20th and 66th, pair_frozen the 20th.  The
figures with them are in profiles/generator_gradients_float64.txt: near-kink share about 1e-5 .. 2.4e-5, flows up to 3 .. 5
px and 0.7 .. 1 px on average, the yardstick's gradient error 1e-6 .. 2e-6 in the median, the largest bound of a case
below 3e-5."""
import collections
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

import kernel_variants as kv
from module_gradient_reference import (FACTOR, FLOOR, U, _MaskedLeaky, bound, format_rows, rel_err, to_nchw,  # noqa: F401
                                       to_nhwc)

KINK_SHARE = 1e-4
BOUND_CAP = 2e-4
WARP_MIN = 1e-4           # px

# id; net: g0 | g1 | pair; norm; no_flow; frame size; frames: (use_raw_only, need_flow) per frame; form: plain | step | step2;
# direct: T2V_CONV_ALGO=1; ngf_global / blocks: the local enhancer's (g1, pair); frozen: G0 of the pair; w_seed; x_seeds: one
# per frame; wino: the yardstick's restatement of the ResnetBlock convs, per net (0 plain, 2 F(2x2), 4 F(4x4))
Case = collections.namedtuple("Case", "id net norm no_flow H W frames form direct ngf_global blocks frozen w_seed x_seeds wino")
COMP, RAW, RAW_NOFLOW = (False, True), (True, True), (True, False)      # RAW: fake is raw, flow and weight still in the loss


def _c(id, net="g0", norm="batch", no_flow=False, H=32, W=32, frames=(COMP,), form="plain", direct=False, ngf_global=32,
       blocks=2, frozen=False, w_seed=3, x_seeds=(1,), wino=(0,)):
    assert len(frames) == len(x_seeds) and len(wino) == (2 if net == "pair" else 1)
    return Case(id, net, norm, no_flow, H, W, tuple(frames), form, direct, ngf_global, blocks, frozen, w_seed, tuple(x_seeds),
                tuple(wino))


CASES = [
    _c("g0_direct", direct=True, x_seeds=(2,)),
    _c("g0_direct_pair_in", norm="instance", frames=(COMP, COMP), form="step", direct=True, x_seeds=(1, 7)),
    _c("g0_wino", H=96, W=96, frames=(RAW,), x_seeds=(1,), wino=(4,)),
    _c("g0_ragged_step", H=88, W=104, frames=(RAW, RAW), form="step", x_seeds=(1, 2), wino=(4,)),
    _c("g0_kept_lazy", H=96, W=96, frames=(RAW, RAW), form="step2", x_seeds=(1, 2), wino=(4,)),
    _c("g0_fewer_uses", H=96, W=96, frames=(RAW_NOFLOW, RAW), form="step2", x_seeds=(1, 2), wino=(4,)),
    _c("g0_noflow", norm="instance", no_flow=True, H=32, W=48, x_seeds=(1,), wino=(2,)),
    # the first and the third of tests/test_gpu_train_two_scale.py's G1_CASES
    _c("g1_wino", net="g1", ngf_global=64, blocks=2, w_seed=11, x_seeds=(1,), wino=(2,)),
    _c("g1_small", net="g1", H=32, W=48, ngf_global=32, blocks=1, w_seed=11, x_seeds=(1,), wino=(2,)),
    # tests/test_gpu_train_two_scale.py's _pair_specs()
    _c("pair", net="pair", H=64, W=64, frames=(COMP, COMP), form="step", x_seeds=(20, 66), wino=(0, 4)),
    _c("pair_frozen", net="pair", H=64, W=64, form="step", frozen=True, x_seeds=(20,), wino=(0, 4)),
]
BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------------------------------------------
# case tensors
# ------------------------------------------------------------------------------------------------------------------
def specs(case):
    """the GeneratorSpec of each net of the case: (G0,), (G1,) or (G0, G1)"""
    from text2video_amd.generator import GeneratorSpec
    g0 = GeneratorSpec(ngf=32, n_downsample=2, n_blocks=2, no_flow=case.no_flow, norm=case.norm)
    g1 = GeneratorSpec(ngf=case.ngf_global // 2, n_blocks=case.blocks, no_flow=case.no_flow, norm=case.norm, is_local=True, scale=1)
    return {"g0": (g0,), "g1": (g1,), "pair": (g0, g1)}[case.net]


def prefixes(case):
    return ("G0.", "G1.") if case.net == "pair" else ("",)


def resblock_shape(spec, H, W):
    """(C, h, w) of the net's 3x3 stride-1 reflect-pad convolutions on an H x W frame"""
    n = spec.n_down
    return spec.ngf << n, H >> n, W >> n


def net_sizes(case):
    """the frame size each net of the case sees"""
    return {"g0": ((case.H, case.W),), "g1": ((case.H, case.W),),
            "pair": ((case.H // 2, case.W // 2), (case.H, case.W))}[case.net]


def site_shapes(spec, H, W, flow=True):
    """(C, h, w) of the net's ReLU sites in execution order; flow=False: without the flow branch's"""
    G, n = spec.ngf, spec.n_down
    C, h, w = resblock_shape(spec, H, W)
    enc = [(G << i, H >> i, W >> i) for i in range(n + 1)]
    dec = [(G << (n - 1 - i), H >> (n - 1 - i), W >> (n - 1 - i)) for i in range(n)]
    if spec.is_local:
        branch = [(C, h, w)] * spec.n_blocks + dec
        return enc + enc + branch + (branch if (flow and not spec.no_flow) else [])
    nb_enc, nb_res = spec.n_blocks - spec.n_blocks // 2, spec.n_blocks // 2
    enc = enc + [(C, h, w)] * nb_enc
    branch = [(C, h, w)] * nb_res + dec
    return enc + enc + branch + (branch if (flow and not spec.no_flow) else [])


def zero_bias_names(case):
    """conv biases in front of a norm layer: the norm removes the channel mean, their gradient is exactly zero"""
    from text2video_amd.generator import layer_keys
    return [p + ck + ".bias" for p, s in zip(prefixes(case), specs(case)) for ck, nk, _ in layer_keys(s) if nk is not None]


def _oracle(spec, ngf_global):
    from oracle.generator_ref import CompositeGenerator, CompositeLocalGenerator
    if spec.is_local:
        return CompositeLocalGenerator(9, 3, 6, ngf_global, spec.n_blocks, 1, spec.no_flow, spec.norm)
    return CompositeGenerator(9, 3, 6, spec.ngf, spec.n_downsample, spec.n_blocks, spec.no_flow, spec.norm)


_BUILT = {}


def build_case(case):
    """-> dict(sds, nets, frames): per net the state dict (upstream names, fp32) and the oracle module holding it (fp32, CPU,
    train mode); per frame a dict of pose, prev (prev0: the coarse scale's), img_c / flow_c (g1: the coarse features) and the
    seeds R_fake, R_raw, R_flow, R_weight of the loss, all fp32 on the CPU.  Built once per case and shared: nothing may
    write into it."""
    if case.id in _BUILT:
        return _BUILT[case.id]
    from text2video_amd.generator import synthetic_state_dict
    sds, nets = [], []
    for i, s in enumerate(specs(case)):
        sd = synthetic_state_dict(s, case.w_seed + 30 * i, "vid2vid", flow_gain=0.05 if s.is_local else 0.1)
        net = _oracle(s, case.ngf_global)
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected and all(("running" in k or "num_batches" in k) for k in missing), (missing, unexpected)
        sds.append(sd)
        nets.append(net.train())
    H, W = case.H, case.W
    frames = []
    for xs in case.x_seeds:
        g = torch.Generator().manual_seed(7000 + xs)
        fr = {"pose": torch.randn(1, 9, H, W, generator=g).clamp(-1, 1),
              # non-zero previous frames: an all-zero prev image makes the image encoder's norm layers 0/0
              "prev": torch.tanh(torch.randn(1, 6, H, W, generator=g))}
        for name, c in (("fake", 3), ("raw", 3), ("flow", 2), ("weight", 1)):
            fr["R_" + name] = torch.randn(1, c, H, W, generator=g)
        if case.net == "pair":
            fr["prev0"] = torch.tanh(torch.randn(1, 6, H // 2, W // 2, generator=g))
        if case.net == "g1":
            # the coarse scale's decoder outputs are relu(norm(.)): non-negative, unit scale
            fr["img_c"] = torch.relu(torch.randn(1, case.ngf_global, H // 2, W // 2, generator=g))
            fr["flow_c"] = torch.relu(torch.randn(1, case.ngf_global, H // 2, W // 2, generator=g))
        frames.append(fr)
    _BUILT[case.id] = dict(sds=sds, nets=nets, frames=frames)
    return _BUILT[case.id]


# ------------------------------------------------------------------------------------------------------------------
# which algorithm a ResnetBlock conv takes (needs the library)
# ------------------------------------------------------------------------------------------------------------------
def layer_algorithms(case):
    """per net of the case: dict(desc, xcs, fwd, dgrad, transposed, takes_forward_weights, level) of its 3x3 stride-1
    reflect-pad layers as _ConvBlock.forward / _data_gradient ask the library (honours T2V_CONV_ALGO as they do); level: the
    yardstick's restatement.  Also asserts that no stride-2 / transposed layer of the case takes the polyphase form."""
    import os
    from text2video_amd import ops
    from text2video_amd.backward import ConvDataGrad
    cap = int(os.environ.get("T2V_CONV_ALGO", "0"))
    out = []
    for s, (H, W) in zip(specs(case), net_sizes(case)):
        C, h, w = resblock_shape(s, H, W)
        desc = ops.conv_desc(h, w, C, C, 3, 1, 1, ops.PAD_REFLECT)
        fwd = ops.ALGO_DIRECT if cap == 1 else ops.best_conv_algo(desc, C, cap)
        dgrad = ConvDataGrad(desc).desc.algo
        # (the transposed algorithm reads the Winograd-domain weight gradient's workspace: only where the forward took F(4x4))
        transposed = fwd == ops.ALGO_WINOGRAD_F4 and ops.backward_weight_winograd_supported(desc, C, C) and \
            ops.backward_data_winograd_supported(desc, C, C)
        algos = {fwd, dgrad}
        level = 4 if (ops.ALGO_WINOGRAD_F4 in algos or transposed) else 2 if ops.ALGO_WINOGRAD in algos else 0
        out.append(dict(desc=desc, xcs=C, fwd=fwd, dgrad=dgrad, transposed=transposed, level=level,
                        takes_forward_weights=ops.backward_data_winograd_takes_forward_weights(desc, C, C)))
        G, n = s.ngf, s.n_down
        for i in range(n):
            for d in (ops.conv_desc(H >> i, W >> i, G << i, G << (i + 1), 3, 2, 1, ops.PAD_ZERO),
                      ops.conv_desc(H >> (i + 1), W >> (i + 1), G << (i + 1), G << i, 3, 2, 1, ops.PAD_ZERO, True)):
                assert not ops.polyphase_pays(d, ops.round_up(d.Cin, 4)), (case.id, d.H, d.W, d.Cin, d.Cout)
                assert ConvDataGrad(d).desc.algo != ops.ALGO_POLYPHASE, (case.id, d.H, d.W, d.Cin, d.Cout)
    return out


# ------------------------------------------------------------------------------------------------------------------
# the Winograd restatement of a 3x3 stride-1 convolution
# ------------------------------------------------------------------------------------------------------------------
def winograd_conv(xp, w, b, m):
    """conv2d(xp, w, b) of the (reflect-)padded map xp [B, C, H + 2, W + 2] as Winograd F(m x m, 3x3), m = 4 or 2, in xp's
    dtype with torch ops only: U = G g G^T (F(4x4): in float64, rounded once, as winograd4_weight_store does; F(2x2): in the
    working precision, as winograd_weight_kernel does), V = B^T d B on the (m + 2)^2 tiles of the map zero-extended to whole
    tiles, M = sum_c U V, Y = A^T M A cropped to H x W.  The matrices are kernel_variants.F4 / F2 (csrc's)."""
    K = kv.F4 if m == 4 else kv.F2
    dt = xp.dtype
    AT, G, BT = K["kAT"].double(), K["kG"].double(), K["kBT"].double()
    B_, C, Hp, Wp = xp.shape
    H, W, t = Hp - 2, Wp - 2, m + 2
    nh, nw = -(-H // m), -(-W // m)
    xp = F.pad(xp, (0, nw * m + 2 - Wp, 0, nh * m + 2 - Hp))
    d = xp.unfold(2, t, m).unfold(3, t, m)                                   # [B, C, nh, nw, t, t]
    if m == 4:
        Uw = torch.einsum("ik,ockl,jl->ocij", G, w.double(), G).to(dt)
    else:
        Uw = torch.einsum("ik,ockl,jl->ocij", G.to(dt), w, G.to(dt))
    V = torch.einsum("ik,bcxykl,jl->bcxyij", BT.to(dt), d, BT.to(dt))
    M = torch.einsum("ocij,bcxyij->boxyij", Uw, V)
    Y = torch.einsum("ki,boxyij,lj->boxykl", AT.to(dt), M, AT.to(dt))       # [B, O, nh, nw, m, m]
    y = Y.permute(0, 1, 2, 4, 3, 5).reshape(B_, w.shape[0], nh * m, nw * m)[:, :, :H, :W]
    return y + b.view(1, -1, 1, 1)


class _WinogradConv(nn.Module):
    """stands in a Sequential for a Conv2d(C, C, 3, padding=0) behind a ReflectionPad2d(1), holding the SAME parameters under
    the same names"""

    def __init__(self, conv, m):
        super().__init__()
        assert conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (0, 0)
        self.weight, self.bias, self.m = conv.weight, conv.bias, m

    def forward(self, xp):
        return winograd_conv(xp, self.weight, self.bias, self.m)


# ------------------------------------------------------------------------------------------------------------------
# the masked oracle
# ------------------------------------------------------------------------------------------------------------------
class _Tape:
    """the pre-activations of one forward call in execution order, and the masks its ReLU sites differentiate with"""

    def __init__(self):
        self.zs, self.masks = [], None


class _Site(nn.Module):
    """a ReLU that records its pre-activation on the net's tape and differentiates with the tape's mask for this site"""

    def __init__(self, tape):
        super().__init__()
        self.tape = [tape]          # (in a list: no attribute of the module tree)

    def forward(self, z):
        tape = self.tape[0]
        i = len(tape.zs)
        tape.zs.append(z)
        mk = None if tape.masks is None else tape.masks[i]
        if mk is None:
            mk = z.detach() > 0
        assert mk.shape == z.shape and mk.dtype == torch.bool, (i, tuple(mk.shape), tuple(z.shape))
        return _MaskedLeaky.apply(z, mk.to(z.device), 0.0)


def masked_oracle(net, wino=0):
    """-> (a deep copy of `net` in which every nn.ReLU of every Sequential -- ResnetBlock.conv_block's too; the oracle shares
    ONE in-place instance among them all -- is a _Site, the copy's _Tape).  wino = 4 / 2: the yardstick, every ResnetBlock
    conv restated as F(4x4) / F(2x2)."""
    from oracle.generator_ref import ResnetBlock
    net = copy.deepcopy(net)
    tape = _Tape()
    site = _Site(tape)
    for seq in [m for m in net.modules() if isinstance(m, nn.Sequential)]:
        for i, child in enumerate(seq):
            if isinstance(child, nn.ReLU):
                seq[i] = site
    if wino:
        for blk in [m for m in net.modules() if isinstance(m, ResnetBlock)]:
            for i in (1, 5):
                assert isinstance(blk.conv_block[i - 1], nn.ReflectionPad2d)
                blk.conv_block[i] = _WinogradConv(blk.conv_block[i], wino)
    assert not any(isinstance(m, nn.ReLU) for m in net.modules())
    return net, tape


OUT_NAMES = ("fake", "raw", "flow", "weight")
# outs[frame]: {fake, raw[, flow, weight]}; zs[frame]: the pre-activations of the frame's sites (G0's, then G1's);
# grads: {upstream parameter name (G0. / G1. in front for the pair) | img_feat_coarse | flow_feat_coarse: gradient or None}
# terms: {bias of a head conv (no norm behind it): its gradient's summands, dL/dc of every frame [frames, C, H, W]}
Result = collections.namedtuple("Result", "outs zs grads terms")

FAULTS = ("residual_identity_dropped", "reflect_fold_dropped", "drop_mean_dy", "ragged_tile_zeroed", "relu_mask_neighbour",
          "weight_adjoint_sign", "flow_weight_halves_swapped", "second_frame_wgrad_dropped", "flow_feat_coarse_dropped")


class _PadNoFold(nn.Module):
    """ReflectionPad2d(1) whose adjoint drops the folded border: dx is the interior of the padded gradient alone"""

    def forward(self, x):
        z = F.pad(x, (1, 1, 1, 1))
        return F.pad(x, (1, 1, 1, 1), mode="reflect").detach() + (z - z.detach())


class _NormNoMeanDy(nn.Module):
    """a norm layer (statistics per image: batches of one) whose adjoint drops the mean-of-dy term: the mean is a constant of
    the numerator (the variance's dependence on it vanishes anyway)"""

    def __init__(self, norm):
        super().__init__()
        self.weight, self.bias, self.eps = getattr(norm, "weight", None), getattr(norm, "bias", None), norm.eps

    def forward(self, c):
        mean = c.mean((2, 3), keepdim=True)
        var = ((c - mean) ** 2).mean((2, 3), keepdim=True)
        y = (c - mean.detach()) * (var + self.eps).rsqrt()
        return y if self.weight is None else y * self.weight.view(1, -1, 1, 1) + self.bias.view(1, -1, 1, 1)


def _first_resblock(net):
    from oracle.generator_ref import ResnetBlock
    return next(m for m in net.model_res_img.modules() if isinstance(m, ResnetBlock)) if hasattr(net, "model_res_img") \
        else next(m for m in net.model_up_img.modules() if isinstance(m, ResnetBlock))


def _inject_module_fault(net, fault):
    blk = _first_resblock(net)
    if fault == "residual_identity_dropped":
        blk.forward = lambda x: x.detach() + blk.conv_block(x)
    elif fault == "reflect_fold_dropped":
        blk.conv_block[4] = _PadNoFold()
    elif fault == "drop_mean_dy":
        blk.conv_block[2] = _NormNoMeanDy(blk.conv_block[2])
    elif fault == "ragged_tile_zeroed":
        def zero_last_tile(mod, args):
            def hook(g):
                g = g.clone()
                g[:, :, 4 * ((g.shape[2] - 1) // 4):, 4 * ((g.shape[3] - 1) // 4):] = 0
                return g
            args[0].register_hook(hook)
        blk.conv_block[4].register_forward_pre_hook(zero_last_tile)


def evaluate(case, data, dtype, device="cpu", masks=None, yardstick=False, fault=None, backward=True):
    """The case through the masked oracle in `dtype` on `device`: one forward call per frame (statistics of its own), the
    linear loss summed over the frames, so the parameter gradients are summed over them.  masks[frame][site]: a bool tensor
    or None (that site: its own sign); yardstick: the ResnetBlock convs restated as Case.wino says; fault: one of FAULTS,
    injected into the net that trains last (G0 alone, or G1); backward=False: the forward pass alone (no gradients).
    -> Result, detached."""
    from oracle.generator_ref import resample
    assert fault is None or fault in FAULTS
    built = [masked_oracle(n, w if yardstick else 0) for n, w in zip(data["nets"], case.wino)]
    nets = [n.to(device=device, dtype=dtype).train() for n, _ in built]
    tapes = [t for _, t in built]
    if fault is not None:
        _inject_module_fault(nets[-1], fault)
    if case.frozen:
        for p in nets[0].parameters():
            p.requires_grad_(False)
    HW = float(case.H * case.W)
    terms = collections.defaultdict(list)
    for pre, net in zip(prefixes(case), nets):
        for head in ("model_final_img", "model_final_flow", "model_final_w"):
            if hasattr(net, head) and getattr(net, head)[1].bias.requires_grad:
                key = pre + head + ".1.bias"
                getattr(net, head)[1].register_forward_hook(
                    lambda mod, args, c, key=key: c.requires_grad and c.register_hook(lambda g: terms[key].append(g.detach())) and None)
    pool = nn.AvgPool2d(3, stride=2, padding=[1, 1], count_include_pad=False)
    loss, outs, zs, coarse, frame_losses = 0.0, [], [], [], []
    for f, (fr, (raw_only, need_flow)) in enumerate(zip(data["frames"], case.frames)):
        t = {k: v.to(device=device, dtype=dtype) for k, v in fr.items()}
        mk = None if masks is None else list(masks[f])
        if fault == "relu_mask_neighbour":
            mk = [z > 0 for z in evaluate(case, data, dtype, device).zs[f]] if mk is None else mk
            # (the two ReLUs in front of the last ResnetBlock conv and its neighbour: same shape)
            sh = [tuple(m.shape) for m in mk]
            i = max(k for k in range(1, len(mk)) if sh[k] == sh[k - 1])
            mk[i] = mk[i - 1]
        for tape in tapes:
            tape.zs = []
        n0 = len(site_shapes(specs(case)[0], *net_sizes(case)[0]))
        if case.net == "g0":
            tapes[0].masks = mk
            o = nets[0](t["pose"], t["prev"], raw_only)
        elif case.net == "g1":
            tapes[0].masks = mk
            ic, fc = t["img_c"].requires_grad_(True), t["flow_c"].requires_grad_(True)
            coarse.append((ic, fc))
            o = nets[0](t["pose"], t["prev"], ic, fc, raw_only)
        else:
            tapes[0].masks, tapes[1].masks = (None, None) if mk is None else (mk[:n0], mk[n0:])
            o0 = nets[0](pool(t["pose"]), t["prev0"], raw_only)
            ff = o0[5].detach() if fault == "flow_feat_coarse_dropped" else o0[5]
            o = nets[1](t["pose"], t["prev"], o0[4], ff, raw_only)
        fake, flow, weight, raw = o[:4]
        out = {"fake": fake, "raw": raw}
        if not case.no_flow and need_flow:
            out.update(flow=flow, weight=weight)
            if fault == "weight_adjoint_sign" and not raw_only:
                warp = resample(t["prev"][:, -3:], flow).detach()
                dfake = t["R_fake"] / HW
                weight.register_hook(lambda g, a=(dfake * (raw.detach() - warp)).sum(1, keepdim=True): g - 2 * a)
        lf = sum((t["R_" + k] * v).sum() for k, v in out.items()) / HW
        frame_losses.append(lf)
        loss = loss + lf
        outs.append({k: v.detach() for k, v in out.items()})
        zs.append([z.detach() for tape in tapes for z in tape.zs])
    if not backward:
        return Result(outs, zs, {}, {})
    named = [(p + k, prm) for p, n in zip(prefixes(case), nets) for k, prm in n.named_parameters() if prm.requires_grad]
    extra = []
    if case.net == "g1":
        extra = [("img_feat_coarse", coarse[0][0])] + ([] if case.no_flow else [("flow_feat_coarse", coarse[0][1])])
    g = torch.autograd.grad(loss, [p for _, p in named + extra], allow_unused=True, retain_graph=fault is not None)
    grads = {k: (None if gi is None else gi.detach()) for (k, _), gi in zip(named + extra, g)}
    if fault == "flow_weight_halves_swapped":
        pre = prefixes(case)[-1]
        for kind in (".weight", ".bias"):
            kf, kw = pre + "model_final_flow.1" + kind, pre + "model_final_w.1" + kind
            cat = torch.cat([grads[kf], grads[kw]], 0)
            grads[kw], grads[kf] = cat[:1].clone(), cat[1:].clone()
    if fault == "second_frame_wgrad_dropped":
        k, p = next((k, p) for k, p in named if k.endswith("conv_block.5.weight"))
        grads[k] = torch.autograd.grad(frame_losses[0], p)[0].detach()
    return Result(outs, zs, grads, {k: torch.cat(v) for k, v in terms.items()})


def own_masks(res):
    return [[z > 0 for z in row] for row in res.zs]


def kink_deltas(y32, r64):
    """[frame][site] -> delta of near_kink from the yardstick and the float64 evaluation (module docstring)"""
    out = []
    for z32s, z64s in zip(y32.zs, r64.zs):
        row = []
        for z32, z64 in zip(z32s, z64s):
            z = z64.double().cpu()
            row.append(5.0 * bound(rel_err(z32, z)) * (z.norm() / z.numel() ** 0.5).item())
        out.append(row)
    return out


def near_kink(z64, delta):
    return z64.abs() <= delta


def near_kink_share(r64, deltas):
    """(elements within delta of the kink, all ReLU elements) of the case"""
    n = sum(int(near_kink(z, d).sum().item()) for zrow, drow in zip(r64.zs, deltas) for z, d in zip(zrow, drow))
    return n, sum(z.numel() for zrow in r64.zs for z in zrow)


def warp_condition(case, y32, r64):
    """per composited frame: (delta_w, sample coordinates within delta_w of an integer, max |flow|, mean |flow|) in float64"""
    out = []
    for f, (raw_only, need_flow) in enumerate(case.frames):
        if case.no_flow or raw_only:
            continue
        f64, f32 = r64.outs[f]["flow"].double().cpu(), y32.outs[f]["flow"].double().cpu()
        dw = max(WARP_MIN, 20.0 * (f32 - f64).abs().max().item())
        H, W = f64.shape[2:]
        xs = torch.arange(W, dtype=torch.float64).view(1, 1, W) + f64[:, 0]
        ys = torch.arange(H, dtype=torch.float64).view(1, H, 1) + f64[:, 1]
        near = sum(int(((c - c.round()).abs() <= dw).sum().item()) for c in (xs, ys))
        out.append((dw, near, f64.abs().max().item(), f64.abs().mean().item()))
    return out


def gradient_tensors(case, res):
    """{name: tensor} of what a case compares with float64: every gradient whose true value is neither zero nor absent"""
    zero = set(zero_bias_names(case))
    return {k: v for k, v in res.grads.items() if v is not None and k not in zero}


def bounds(case, y32, r64):
    """{gradient tensor: (e32, bound)} from the yardstick and the float64 evaluation under the same masks.

    The biases of the three head convolutions (no norm behind them) have 3, 2 and 1 elements, each a plain sum over the
    pixels of dL/dc (Result.terms), whose terms carry both signs: the sum is a few sqrt(n) of them.  The yardstick's error of
    such a tensor is ONE draw of a scalar error, the HIP error another, and of two independent draws of |N(0, s)| one exceeds
    4 x the other with probability (2 / pi) atan(1 / 4) = 16 %: FACTOR x one draw is no bound for a scalar (the many-element
    tensors' norms concentrate; theirs is).  It showed at once: under the HIP masks of g1_wino torch's pairwise sum hit
    model_final_w.1.bias to 0.6 u, where the same tensor's yardstick error is 3 u .. 110 u in the other ten cases.  So for
    these tensors e32 is not allowed to fall below the size the yardstick's own summand errors give the sum were they
    independent from pixel to pixel: ||t32 - t64||_2 / ||g64||_2 with t the summands (errors that are correlated from pixel
    to pixel -- they come through shared weights -- add up to more, so this is the cautious side).  On the CPU, float64
    masks, that figure is within 0.2 .. 5 x the drawn error wherever the summands' own error dominates (the composited
    cases) and below it where the summation's does; it never replaces a larger drawn error."""
    g64, g32 = gradient_tensors(case, r64), gradient_tensors(case, y32)
    assert set(g64) == set(g32)
    out = {}
    for k in g64:
        e32 = rel_err(g32[k], g64[k])
        if k in r64.terms:
            t64 = r64.terms[k].double().cpu()
            assert t64.shape[1] == g64[k].numel() <= 3
            e32 = max(e32, ((y32.terms[k].double().cpu() - t64).norm() / g64[k].double().cpu().norm()).item())
        out[k] = (e32, bound(e32))
    return out
