"""Train step of the vid2vid pose model on the HIP path.

torch.autograd is used as the TAPE only: every differentiable op below is a `torch.autograd.Function`
whose forward and backward are calls into libt2v_hip.so (implicit-GEMM conv, fused norm statistics,
weight-gradient kernel, norm backward, ...).  Tensors are NHWC fp32 on the device; parameters are
torch-layout fp32 `nn.Parameter`s (upstream state-dict names) that are re-packed for the kernels each
step.  Channel concat / crop / detach / scalar loss arithmetic stay torch-native plumbing.

Scope (what the reference's training command README.md:171-176 exercises): generator WITH its flow branch
(flow / weight heads, flow-warp compositor: every loss on the blended frame back-propagates through
raw*w + warp*(1-w) into flow, weight and raw -- `_WarpComposite`), or without it (--no_flow), multiscale image
discriminator (--num_D 2), face discriminator (--add_face_disc), temporal discriminators, LSGAN +
feature-matching losses, the VGG19 perceptual loss (frozen torchvision weights supplied with --vgg_weights), the
flow / warp / weight losses against a SUPPLIED reference flow (zero flow + its confidence mask by default:
FlowNet2, which produces it upstream, is not in the reference tree -- SURVEY 8d config 5), Adam(lr 2e-4,
beta1 0.5), data-parallel gradient all-reduce.  Beyond that recipe: upstream's high-resolution continuation, the two-scale
generator (--n_scales_spatial 2: TrainableLocalGenerator, TwoScaleGenerator) with --niter_fix_global.
"""
import collections
import contextlib
import os
import time

import torch

from . import ops
from .backward import ConvDataGrad
from .generator import GeneratorSpec, layer_keys, synthetic_state_dict  # noqa: F401
from .gradients import (STEP, GradBuckets, GradientExchange, GradSlot, ParamState, _acc, _batched_winograd_wgrad,  # noqa: F401
                        _desc_key, _keep_v_slot, _kept_winograd_wgrad, _paired_direct_wgrad, allreduce_gradients,
                        allreduce_gradients_begin, batched_weight_gradients, cached_pack, check_presence_across_ranks, clip_slots,
                        clips_per_rank,
                        deliver, deliver_direct, deliver_into, direct_weight_gradient, expect_gradient,
                        flush_pending_weight_gradients, grad_slot, invalidate_packs, owner, param_state, prefetch_packs,
                        side_gemm_hint, switch, wgrad_fork, wgrad_join, wgrad_stream_on, winograd_weight_gradient)


# ------------------------------------------------------------------------------------------------
# differentiable building blocks
# ------------------------------------------------------------------------------------------------
BN_MOMENTUM = 0.1     # nn.BatchNorm2d default ($SP/torch/nn/modules/batchnorm.py:16)
_BN_UPDATES = [1]     # running-statistics updates per forward (a forward that stands for two upstream forwards: 2)
_NO_PARAM_GRAD = set()   # ids of parameters whose gradients the backward pass under way must not produce
_NO_INPUT_DX = [False]   # the backward pass under way wants parameter gradients only: input layers skip their data gradient


@contextlib.contextmanager
def input_gradients_off():
    """Scope of a backward pass that asks for PARAMETER gradients of a loss network only (D's loss): the network's input
    layers (conv_block(..., need_dx=2)) skip the data-gradient conv into their input -- with one shared forward on the
    attached fake frames that input requires grad, but only G's backward pass (param_gradients_off) ever reads it."""
    old = _NO_INPUT_DX[0]
    _NO_INPUT_DX[0] = True
    try:
        yield
    finally:
        _NO_INPUT_DX[0] = old


@contextlib.contextmanager
def param_gradients_off(params):
    """Scope of a backward pass that runs THROUGH layers whose parameters belong to another loss: their nodes only
    propagate the data gradient (no weight-gradient kernels, nothing delivered to their gradient slots)."""
    ids = {id(owner(p)) for p in params}
    _NO_PARAM_GRAD.update(ids)
    try:
        yield
    finally:
        _NO_PARAM_GRAD.difference_update(ids)


@contextlib.contextmanager
def bn_updates(n):
    old = _BN_UPDATES[0]
    _BN_UPDATES[0] = n
    try:
        yield
    finally:
        _BN_UPDATES[0] = old


_BN_FROZEN = [False]


@contextlib.contextmanager
def bn_frozen():
    """no forward inside the scope moves running statistics, whatever bn_updates or a caller's `times` says (the clips of an
    optimiser step behind its first: Vid2VidTrainer.train_step)"""
    old = _BN_FROZEN[0]
    _BN_FROZEN[0] = True
    try:
        yield
    finally:
        _BN_FROZEN[0] = old


def running_stats(gamma, create=True):
    """[running_mean, running_var, num_batches_tracked] of the BatchNorm2d whose weight is `gamma` (kept on the parameter
    object; created at torch's initial values 0 / 1 / 0)."""
    st = param_state(gamma, create)
    if st is None:
        return None
    if st.running is None and create:
        st.running = [torch.zeros(gamma.numel(), dtype=torch.float32, device=gamma.device),
                      torch.ones(gamma.numel(), dtype=torch.float32, device=gamma.device), 0]
    return st.running


def running_update_args(gamma, n, times=None):
    """Every training-mode forward of a BatchNorm2d also moves its running statistics
    ($SP/torch/nn/modules/batchnorm.py:57-64, momentum 0.1, unbiased variance) -- never read on this path (upstream keeps
    the generator in train mode at test time) but part of a faithful checkpoint.  Returns (running_mean,
    running_var, momentum, times) for the finalize call, which moves them in its own launch, or None (no affine norm,
    fewer than two values per channel); counts the updates on the statistics' step counter."""
    if gamma is None or n < 2 or _BN_FROZEN[0]:
        return None
    times = _BN_UPDATES[0] if times is None else int(times)
    rs = running_stats(gamma)
    rs[2] += times
    return (rs[0], rs[1], BN_MOMENTUM, times)


_ZEROS = {}


def _zeros(n, device):
    """shared read-only zero vector (the exactly-zero bias gradients in front of norm layers)"""
    z = _ZEROS.get((n, device))
    if z is None:
        z = _ZEROS[(n, device)] = torch.zeros(n, dtype=torch.float32, device=device)
        if z.is_cuda:
            torch.cuda.current_stream().synchronize()      # (once per size: the vector is read from more than one stream)
    return z


# how a node makes its weight gradient (ConvMeta.wgrad)
WGRAD_DIRECT = 0                # the direct kernel (several uses of one layer in one launch: _paired_direct_wgrad)
WGRAD_WINOGRAD = 1              # in the Winograd domain, this node alone
WGRAD_WINOGRAD_COLLECTED = 2    # in the Winograd domain, counted on the weight: one reduction over every use of the step


# What _ConvBlock.forward leaves for its backward node.  ddesc: the layer's geometry with the direct algorithm (the weight- and
# data-gradient kernels' descriptor);  need_dx: 0 / 1 / 2 (an input layer: input_gradients_off);  mrs: the norm's (mean, rstd)
# per image or per pass;  wgrad: WGRAD_*;  kept: (workspace, slots, slot) where forward kept its input transform, or None
ConvMeta = collections.namedtuple("ConvMeta", "desc ddesc norm relu act need_dx mrs affine wgrad slope groups pt_skip kept")
# The gradient in front of a norm that is not written out: the norm backward has delivered its two sums, the one reader -- the
# weight gradient's transform of dy -- forms it per loaded element (ops.conv2d_backward_weight_winograd_dy_norm's leading arguments)
LazyDc = collections.namedtuple("LazyDc", "c dy mean_rstd gamma beta relu sums")


def _norm_adjoint(m, c, dy, y_act, gamma, beta, want_affine, sl_g, sl_bt, lazy, g0, gB, img0):
    """dy behind act(norm(.)) -> (dc in front of it, or None with a LazyDc in its place; d gamma; d beta).  The affine
    gradients are delivered by the norm backward's final pass where both have bucket slots (-> None)."""
    both = sl_g is not None and sl_bt is not None
    dgamma = dbeta = None

    def norm_backward(ci, dyi, mr, **kw):
        nonlocal dgamma, dbeta
        into = None
        if both:
            into = (sl_bt.view, sl_g.view, not sl_g.filled)
            sl_g.filled = sl_bt.filled = True
        dci, sums = ops.instance_norm_backward(ci, dyi, mr, gamma, beta, m.relu, affine_into=into, **kw)
        if want_affine and not both:       # [C,2] = (sum g, sum g*xhat) -> d beta, d gamma
            db_, dg_ = sums.t().contiguous().unbind(0)
            dbeta = db_ if dbeta is None else dbeta + db_
            dgamma = dg_ if dgamma is None else dgamma + dg_
        return dci, sums

    lazy_dc = None
    if lazy:
        _, sums = norm_backward(c[0], dy[0], m.mrs[0], sums_only=True)
        dc, lazy_dc = None, LazyDc(c[0], dy[0], m.mrs[0], gamma, beta, m.relu, sums)
    elif m.norm is None:
        # (act_backward's mode 2 is a plain sigmoid; the fused flow / weight head is its mode 4)
        dc = ops.act_backward(dy, y_act, 4 if m.act == ops.ACT_FLOW_W else m.act, m.slope) if m.act != ops.ACT_NONE else dy
    elif m.norm == "batch" and m.groups > 1:
        dc = torch.empty_like(c)
        for gi in range(g0, m.groups):       # statistics per pass: the norm's adjoint per pass
            sl = slice((gi - g0) * gB, (gi - g0 + 1) * gB)
            norm_backward(c[sl], dy[sl], m.mrs[gi], out=dc[sl])
    elif m.norm == "batch":
        dc, _ = norm_backward(c, dy, m.mrs[0])
    else:
        dc = torch.empty_like(c)
        for i in range(c.shape[0]):
            norm_backward(c[i], dy[i], m.mrs[img0 + i], out=dc[i])
    if both:
        deliver(sl_g)
        deliver(sl_bt)
    return dc, lazy_dc, dgamma, dbeta


def _bias_gradient(m, dc, slot, device):
    """a bias in front of a norm layer has an exactly zero gradient (the norm removes the channel mean)"""
    C = m.desc.Cout
    if m.norm is not None:
        if slot is None:
            return _zeros(C, device)
        deliver(slot, zero=True)
        return None

    def launch(out, accumulate):
        if out is None:
            return ops.channel_sum(dc, C)
        if accumulate:
            _acc(out, ops.channel_sum(dc, C), False)
        else:
            ops.channel_sum(dc, C, out=out)
    return deliver_into(slot, (dc,), launch)       # (off the dy -> dx chain too)


def _weight_gradient(m, w, x, dc, lazy_dc, slot):
    """-> (dW, or None: delivered into `slot` / left to the layer's last node; where the Winograd-domain collection holds this
    node's A dy A^T, or None)"""
    if m.wgrad == WGRAD_WINOGRAD_COLLECTED:
        if m.kept is not None:
            return _kept_winograd_wgrad(w, dc, m.ddesc, m.kept, slot, lazy_dc)
        return _batched_winograd_wgrad(w, x, dc, m.ddesc, slot)
    if m.wgrad == WGRAD_WINOGRAD:
        return winograd_weight_gradient(x, dc, m.ddesc, slot), None
    paired, dw = _paired_direct_wgrad(w, x, dc, m.ddesc, slot)
    if not paired:
        dw = deliver_direct(slot, (x, dc), lambda: direct_weight_gradient(x, dc, m.ddesc), m.ddesc, x.shape[-1])
    return dw, None


def _data_gradient(m, w, x, x_full, img0, dc, ycs, where):
    """dx of the images `x` = x_full[img0:] (the leading ones carry no gradient: exact zeros).  where: the weight gradient
    has just put A dy A^T of these images into its workspace and the transposed Winograd algorithm has the shape."""
    fdesc, xcs, B = m.ddesc, x.shape[-1], x.shape[0]
    if where is not None:
        # The data gradient by the TRANSPOSED Winograd algorithm reads A dy A^T from there -- U^T dM on the layer's own 256
        # tiles instead of the full-correlation form's 289 -> 320, no second transform of dy, no flipped filter transform
        ws, total, first = where
        # ... and where the fixed-grid GEMM has its [K][N] form for the shape, U^T is the forward pass's own packing read in
        # place (T2V_DGRAD_FORWARD_WEIGHTS=0: the transposed copy, same bits)
        fw = switch("T2V_DGRAD_FORWARD_WEIGHTS") and ops.backward_data_winograd_takes_forward_weights(fdesc, xcs, ycs)
        if fw:
            # (the forward pass ran this layer as F(4x4) and holds that packing under this key)
            f4 = ops.with_algo(fdesc, ops.ALGO_WINOGRAD_F4)
            ut = cached_pack(w, ("fwd",) + _desc_key(f4, xcs), lambda: ops.pack_conv_weight(w.detach().contiguous(), f4, xcs))
        else:
            ut = cached_pack(w, ("dgradT",) + _desc_key(fdesc, xcs), lambda: ops.pack_conv_weight_transposed(w.detach(), fdesc, xcs))
        dx = torch.empty_like(x)
        for i in range(B):
            ops.conv2d_backward_data_winograd(fdesc, total, first + i, ws, xcs, ut, out=dx[i], forward_weights=fw)
        return dx
    dg = ConvDataGrad(fdesc)
    dg.packed = cached_pack(w, ("dgrad",) + _desc_key(fdesc, xcs), lambda: dg.refresh(w.detach()).packed)
    if ops.round_up(fdesc.Cin, 4) == xcs:
        dx = torch.empty_like(x_full)
        if img0:
            ops.zero_(dx[:img0])
        dg.batch(dc, dx[img0:])
    else:   # x carries more channel storage than the layer reads: zero gradient there
        dx = torch.zeros_like(x_full)
        dx[img0:, ..., :ops.round_up(fdesc.Cin, 4)] = torch.stack([dg(dc[i]) for i in range(B)])
    return dx


class _ConvBlock(torch.autograd.Function):
    """y = act(norm(conv(x) + b)) + res  on a batch [B,H,W,cs].

    norm: None | 'instance' (statistics per image) | 'batch' (statistics over the batch, BatchNorm2d in
    train mode); relu: 0 none / 1 ReLU / 2 LeakyReLU(0.2) applied after the norm; without a norm the
    activation `act` (ACT_NONE / ACT_TANH / ACT_LRELU) is fused into the conv epilogue."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, res, desc, norm, relu, act, need_dx, slope=0.2, groups=1, bn_times=None, pt_skip=0):
        # groups > 1 (norm 'batch'): the batch is `groups` independent passes of B / groups images each -- the discriminators'
        # real / fake / raw passes in ONE node: one conv launch, one data-gradient launch, one weight-gradient launch over
        # all of them; the BatchNorm statistics (and their running averages, moved bn_times[g] times) stay per pass.
        # pt_skip: leading images nobody differentiates in a pass-through backward (param_gradients_off: the generator's
        # loss reaches the fake / raw passes only) -- that backward runs on the images [pt_skip:] alone.
        B = x.shape[0]
        assert B % groups == 0, "conv_block: batch %d is not %d equal passes" % (B, groups)
        if pt_skip and norm == "batch" and groups == 1:
            # (the statistics of ONE pass cover the skipped images too: the norm's adjoint on x[pt_skip:] alone would be wrong)
            raise ValueError("conv_block: pt_skip=%d with norm='batch' needs the skipped images in passes of their own "
                             "(groups > 1): one pass's batch statistics couple every image's gradient" % pt_skip)
        dev = x.device
        xcs = x.shape[-1]
        ho, wo = ops.conv_out_dims(desc)
        ycs = ops.round_up(desc.Cout, 4)
        fdesc = ops.conv_desc(desc.H, desc.W, desc.Cin, desc.Cout, desc.kH, desc.stride, desc.pad, desc.pad_mode,
                              bool(desc.transposed), act if norm is None else ops.ACT_NONE, slope, desc.output_padding)
        # 3x3 stride-1 layers (the ResnetBlock convs) run as Winograd where that is the smaller GEMM; the weight
        # gradient keeps the direct layout (ddesc)
        ddesc = fdesc
        # (convs with a fused activation -- the VGG19 loss network -- stay on the direct kernel: F(4x4)'s 5x larger rounding
        # noise flips visibly more ReLU / max-pool decisions in that 13-layer net -- input-gradient relative L2 error 3.7e-3
        # instead of 2.3e-3 -- for 2 ms of a 99 ms step)
        if fdesc.act == ops.ACT_NONE and ycs == desc.Cout and int(os.environ.get("T2V_CONV_ALGO", "0")) != 1:
            algo = ops.best_conv_algo(fdesc, xcs, int(os.environ.get("T2V_CONV_ALGO", "0")))
            if algo != ops.ALGO_DIRECT:
                fdesc = ops.with_algo(fdesc, algo)
            elif int(os.environ.get("T2V_CONV_ALGO", "0")) == 0 and desc.stride == 2 and ops.polyphase_pays(fdesc, xcs):
                # the deep stride-2 / transposed layers as polyphase Winograd F(4,2), as in the inference frames
                # (csrc/polyphase.hip); the weight gradient keeps the direct layout (ddesc), the data gradient is the
                # polyphase form of the adjoint geometry (backward.ConvDataGrad)
                fdesc = ops.with_algo(fdesc, ops.ALGO_POLYPHASE)
        pw = cached_pack(w, ("fwd",) + _desc_key(fdesc, xcs), lambda: ops.pack_conv_weight(w.detach().contiguous(), fdesc, xcs))
        c = torch.empty(B, ho, wo, ycs, dtype=torch.float32, device=dev)
        mrs = None
        # weight gradient in the Winograd domain where the forward took F(4x4,3x3) (a quarter of the FLOPs)
        wino_wgrad = fdesc.algo == ops.ALGO_WINOGRAD_F4 and ops.backward_weight_winograd_supported(ddesc, xcs, ycs) \
            and switch("T2V_WGRAD_WINOGRAD")
        # ... whose workspace, from the layer's second step on, takes this conv's input transform right now (_keep_v_slot)
        kept = _keep_v_slot(w, x, ddesc, xcs, ycs) if (wino_wgrad and ctx.needs_input_grad[1] and STEP.wg_batch) else None
        # (a batch of a direct-algorithm layer -- the discriminators' -- is ONE launch: ops.conv2d_auto_batch)
        if norm is None:
            if kept is not None:
                ops.conv2d_winograd(x[0], pw, b.detach(), fdesc, out=c[0], keep_v=kept)
            else:
                ops.conv2d_auto_batch(x, pw, b.detach(), fdesc, y_cs=ycs, out=c)
            y = c
        else:
            n = ops.conv_stats_buffer(fdesc, dev).numel()
            stats = torch.empty(B * n, dtype=torch.float32, device=dev)
            if kept is not None:
                ops.conv2d_winograd(x[0], pw, b.detach(), fdesc, stats=stats, out=c[0], keep_v=kept)
            else:
                ops.conv2d_auto_batch(x, pw, b.detach(), fdesc, y_cs=ycs, stats=stats, out=c)
            y = torch.empty_like(c)
            g = gamma.detach() if gamma is not None else None
            bt = beta.detach() if beta is not None else None
            # the residual add rides in the norm-apply pass (its gradient is the identity)
            rs = res.detach().contiguous() if (res is not None and res.shape == y.shape) else None
            # (the finalize launch also moves BatchNorm2d's running statistics: running_update_args)
            if norm == "batch" and groups > 1:
                gB, mrs = B // groups, []
                for gi in range(groups):
                    sl = slice(gi * gB, (gi + 1) * gB)
                    mrs.append(ops.batch_norm_finalize(stats[gi * gB * n:(gi + 1) * gB * n], fdesc, gB,
                                                       running=running_update_args(gamma, gB * ho * wo,
                                                                                   bn_times[gi] if bn_times else None)))
                    ops.instance_norm_apply(c[sl], mrs[gi], g, bt, res1=rs[sl] if rs is not None else None, relu=relu, out=y[sl])
            elif norm == "batch":
                mrs = [ops.batch_norm_finalize(stats, fdesc, B, running=running_update_args(gamma, B * ho * wo))]
                ops.instance_norm_apply(c, mrs[0], g, bt, res1=rs, relu=relu, out=y)
            else:
                mrs = []
                for i in range(B):       # BatchNorm2d(train) on a batch of one
                    mrs.append(ops.instance_norm_finalize(stats[i * n:(i + 1) * n], fdesc,
                                                          running=running_update_args(gamma, ho * wo)))
                    ops.instance_norm_apply(c[i], mrs[i], g, bt, res1=rs[i] if rs is not None else None, relu=relu, out=y[i])
            if rs is not None:
                res = None
        if res is not None:
            y = y + res   # residual add (plumbing-level elementwise; its gradient is the identity)
        # every use of the layer in this graph (one per frame of the clip) is counted on the weight: their Winograd-
        # domain gradients are reduced together by the last backward node to run (T2V_WGRAD_BATCH=0: one by one)
        wgrad = WGRAD_WINOGRAD if wino_wgrad else WGRAD_DIRECT
        if wino_wgrad and w.requires_grad and STEP.wg_batch:
            st = param_state(w)
            st.images += B
            st.seen += B
            wgrad = WGRAD_WINOGRAD_COLLECTED
        elif not wino_wgrad and w.requires_grad and STEP.dw_pair and \
                (B > 1 or ops.backward_weight_strided_supported(ddesc, xcs, ycs)):
            param_state(w).dw_uses += 1      # (two or more uses: _paired_direct_wgrad)
        for prm in (w, b, gamma, beta):
            expect_gradient(prm)
        # (an input nobody differentiates -- the discriminators' real pass -- needs no data-gradient conv)
        need_dx = int(need_dx) if (need_dx and ctx.needs_input_grad[0]) else 0      # 2: an input layer (input_gradients_off)
        ctx.meta = ConvMeta(desc, ddesc, norm, relu, act, need_dx, mrs, gamma is not None, wgrad, slope, groups, int(pt_skip), kept)
        ctx.save_for_backward(x, w, c, gamma, beta, y if (norm is None and act != ops.ACT_NONE) else None, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        m = ctx.meta
        x, w, c, gamma, beta, y_act, b = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.is_cuda:
            side_gemm_hint()
        want = [bool(v) for v in ctx.needs_input_grad]
        need_dx = 0 if (m.need_dx == 2 and _NO_INPUT_DX[0]) else m.need_dx
        g0, img0, x_full = 0, 0, x
        gB = x.shape[0] // m.groups
        # a backward pass that only passes THROUGH this layer (param_gradients_off): data gradient only
        if _NO_PARAM_GRAD and id(owner(w)) in _NO_PARAM_GRAD:
            want[1] = want[2] = want[3] = want[4] = False
            if m.pt_skip:
                # ... and only through the passes the loss reaches: the leading `pt_skip` images (the real pass) carry no
                # gradient in this backward -- their rows of dy are never read, their rows of dx are exact zeros
                img0 = m.pt_skip
                assert m.wgrad == WGRAD_DIRECT and 0 < img0 < x.shape[0] and (m.groups == 1 or img0 % gB == 0)
                g0 = img0 // gB if m.groups > 1 else 0
                x, c, dy = x[img0:], c[img0:], dy[img0:]
                y_act = y_act[img0:] if y_act is not None else None
        # parameters with a bucket slot get their gradients delivered in place (and None goes back to autograd)
        sl_w = grad_slot(w) if want[1] else None
        sl_b = grad_slot(b) if want[2] else None
        sl_g = grad_slot(gamma) if (m.affine and want[3]) else None
        sl_bt = grad_slot(beta) if (m.affine and want[4]) else None
        # Where this node's gradient in front of the norm would be read by nothing but the transform A dy A^T (the weight
        # gradient's workspace holds V already, the data gradient takes A dy A^T from there), it is not written at all: the
        # norm backward delivers its two sums, the transform forms the gradient per loaded element (T2V_DY_NORM_FUSED=0: off)
        dgrad_t = m.wgrad == WGRAD_WINOGRAD_COLLECTED and ops.backward_data_winograd_supported(m.ddesc, x.shape[-1], c.shape[-1])
        lazy = m.norm is not None and x.shape[0] == 1 and m.wgrad == WGRAD_WINOGRAD_COLLECTED and want[1] and m.kept is not None \
            and (dgrad_t or not need_dx) and switch("T2V_DY_NORM_FUSED")
        dc, lazy_dc, dgamma, dbeta = _norm_adjoint(m, c, dy, y_act, gamma, beta, m.affine and (want[3] or want[4]), sl_g, sl_bt,
                                                   lazy, g0, gB, img0)
        db = _bias_gradient(m, dc, sl_b, x.device) if want[2] else None
        # (frozen weights -- the VGG19 feature extractor -- / a pass-through backward: data gradient only)
        dw, where = _weight_gradient(m, w, x, dc, lazy_dc, sl_w) if want[1] else (None, None)
        dx = None
        if need_dx:
            dx = _data_gradient(m, w, x, x_full, img0, dc, c.shape[-1], where if dgrad_t else None)
        elif img0:
            raise RuntimeError("conv_block: pt_skip is for layers with a data gradient")
        return (dx, dw, db, dgamma, dbeta, (dy if ctx.needs_input_grad[5] else None)) + (None,) * 9


class _CatParams(torch.autograd.Function):
    """torch.cat([a, b], 0) of two parameters (the flow head and the weight head read the same features: one
    3-output conv).  Backward splits the gradient and delivers the halves into the parameters' bucket slots, like
    every other node that owns a parameter gradient."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.n = a.shape[0]
        ctx.save_for_backward(a, b)
        expect_gradient(a)
        expect_gradient(b)
        return torch.cat([a, b], 0)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga, gb = g[:ctx.n].contiguous(), g[ctx.n:].contiguous()
        out = []
        for p, gp, need in ((a, ga, ctx.needs_input_grad[0]), (b, gb, ctx.needs_input_grad[1])):
            sl = grad_slot(p) if need else None
            if sl is not None:
                deliver(sl, gp)
                out.append(None)
            else:
                out.append(gp if need else None)
        return tuple(out)


def conv_block(x, w, b, desc, gamma=None, beta=None, res=None, norm="instance", relu=1, act=ops.ACT_NONE,
               need_dx=True, slope=0.2, groups=1, bn_times=None, pt_skip=0):
    """slope: negative-side factor of act == ACT_LRELU (0.2 in the discriminators; 0 makes it a ReLU).
    groups / bn_times / pt_skip: several independent passes in one batch (_ConvBlock.forward)."""
    return _ConvBlock.apply(x, w, b, gamma, beta, res, desc, norm, relu, act, need_dx, slope, groups, bn_times, pt_skip)


class _AvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.hw = (x.shape[1], x.shape[2])
        return torch.stack([ops.avgpool3x3s2(x[i]) for i in range(x.shape[0])])

    @staticmethod
    def backward(ctx, dy):
        H, W = ctx.hw
        dy = dy.contiguous()
        return torch.stack([ops.avgpool3x3s2_backward(dy[i], H, W) for i in range(dy.shape[0])])


class _MseConst(torch.autograd.Function):
    """mean((x - c)^2) over the LOGICAL channel 0 of a [.., 4]-padded logit tensor."""

    @staticmethod
    def forward(ctx, x, c):
        logits = x[..., 0].contiguous()
        ctx.c, ctx.shape = c, x.shape
        ctx.save_for_backward(logits)
        return ops.sum_sq_diff_const(logits, c)[0] / logits.numel()

    @staticmethod
    def backward(ctx, g):
        (logits,) = ctx.saved_tensors
        d = ops.sum_sq_diff_const_backward(logits, ctx.c, 1.0 / logits.numel()) * g
        dx = torch.zeros(ctx.shape, dtype=torch.float32, device=logits.device)
        dx[..., 0] = d
        return dx, None


class _L1(torch.autograd.Function):
    """mean(|a - b|); gradient flows to `a` only (b is the detached real-branch feature)."""

    @staticmethod
    def forward(ctx, a, b, nlogical):
        ctx.save_for_backward(a, b)
        ctx.n = nlogical
        return ops.sum_abs_diff(a.contiguous(), b.contiguous())[0] / nlogical

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return ops.sum_abs_diff_backward(a.contiguous(), b.contiguous(), 1.0 / ctx.n) * g, None, None


class _WarpComposite(torch.autograd.Function):
    """out = raw*w + resample(prev[..., c0:c0+3], flow)*(1-w) on [B,H,W,4] tensors; fw = (flow_x, flow_y, w, 0).
    Backward: t2v_flow_warp_composite_backward (SpatialGridSamplerBilinear_updateGradInput, THCUNN.h:1055, fused
    with the blend's adjoint); the gradient with respect to `prev` only when autograd asks for it (the generated
    previous frames are detached: max_frames_backpropagate 1)."""

    @staticmethod
    def forward(ctx, raw, fw, prev, c0):
        ctx.c0 = c0
        ctx.save_for_backward(raw, fw, prev)
        out = torch.empty_like(raw)
        for i in range(raw.shape[0]):
            ops.flow_warp_composite(raw[i], fw[i], prev[i], c0, out=out[i])
        return out

    @staticmethod
    def backward(ctx, dy):
        raw, fw, prev = ctx.saved_tensors
        dy = dy.contiguous()
        res = [ops.flow_warp_composite_backward(dy[i], None, raw[i], fw[i], prev[i], ctx.c0, ctx.needs_input_grad[2])
               for i in range(raw.shape[0])]
        d_raw = torch.stack([r[0] for r in res]) if len(res) > 1 else res[0][0].unsqueeze(0)
        d_fw = torch.stack([r[1] for r in res]) if len(res) > 1 else res[0][1].unsqueeze(0)
        d_prev = None
        if ctx.needs_input_grad[2]:
            d_prev = torch.stack([r[2] for r in res])
        return d_raw, d_fw, d_prev, None


class _Resample(torch.autograd.Function):
    """resample(img[..., c0:c0+3], flow) -> [B,H,W,4]: the warp losses' plain grid_sample (same kernels, no blend)."""

    @staticmethod
    def forward(ctx, fw, img, c0):
        ctx.c0 = c0
        ctx.save_for_backward(fw, img)
        out = torch.empty(fw.shape[:3] + (4,), dtype=torch.float32, device=fw.device)
        for i in range(fw.shape[0]):
            ops.flow_warp(fw[i], img[i], c0, out=out[i])
        return out

    @staticmethod
    def backward(ctx, dy):
        fw, img = ctx.saved_tensors
        dy = dy.contiguous()
        res = [ops.flow_warp_composite_backward(None, dy[i], None, fw[i], img[i], ctx.c0, ctx.needs_input_grad[1])
               for i in range(fw.shape[0])]
        d_fw = torch.stack([r[1] for r in res])
        d_img = torch.stack([r[2] for r in res]) if ctx.needs_input_grad[1] else None
        return d_fw, d_img, None


class _MaskedL1(torch.autograd.Function):
    """vid2vid's MaskedL1Loss [RECALL upstream models/networks.py]: L1Loss(a*mask, b*mask), mean over ALL B*C*H*W
    elements; a, b: [B,H,W,cs] (b None: zero target), mask: [B,H,W] of {0,1} or None, over the channels
    [c0, c0+C) (the flow / weight planes of the fused head are read in place).  Gradient to `a` only."""

    @staticmethod
    def forward(ctx, a, b, mask, c0, C):
        a = a.contiguous()
        ctx.cw = (c0, C)
        ctx.n = (a.numel() // a.shape[-1]) * C
        ctx.save_for_backward(a, b, mask)
        return ops.sum_abs_diff_masked(a, b, mask, c0, C)[0] / ctx.n

    @staticmethod
    def backward(ctx, g):
        a, b, mask = ctx.saved_tensors
        return ops.sum_abs_diff_masked_backward(a, b, mask, ctx.cw[0], ctx.cw[1], 1.0 / ctx.n) * g, None, None, None, None


def masked_l1(a, b, mask, C, c0=0):
    return _MaskedL1.apply(a, b.detach().contiguous() if b is not None else None,
                           mask.contiguous() if mask is not None else None, c0, C)


# ------------------------------------------------------------------------------------------------
# networks
# ------------------------------------------------------------------------------------------------
def shift(prev, frame):
    """fake_B_prev = cat(fake_B_prev[1:], fake_B) on one scale's FIFO (n_frames_G 3), the new frame detached"""
    new = torch.zeros_like(prev)
    new[..., :3] = prev[..., 3:6]
    new[..., 3:6] = frame.detach()[..., :3]
    return new


class TrainableGenerator(torch.nn.Module):
    """CompositeGenerator with or without its flow branch, upstream parameter names."""

    LOCAL = False

    def __init__(self, spec, state_dict, device="cuda"):
        super().__init__()
        if bool(spec.is_local) != self.LOCAL:
            raise ValueError("%s: a spec with is_local=%s is built by %s" % (
                type(self).__name__, bool(spec.is_local), "TrainableLocalGenerator" if spec.is_local else "TrainableGenerator"))
        self.spec = spec
        self.keys = layer_keys(spec)
        self.params = torch.nn.ParameterDict()
        for k, v in state_dict.items():
            self.params[k.replace(".", "/")] = torch.nn.Parameter(v.to(device, torch.float32).contiguous())

    def p(self, key):
        return self.params[key.replace(".", "/")]

    def named_upstream_parameters(self):
        return {k.replace("/", "."): v for k, v in self.params.items()}

    def _heads(self, img_feat, flow_feat, prev, use_raw_only, off_tape=False):
        """The 7x7 heads on the decoders' outputs -> (fake, raw, flow_w) as forward(full=True) returns them; flow_feat None:
        no flow branch, or a raw-only frame whose flow nobody reads.  (forward() below keeps its own copy of these lines: the
        single-scale step does not pass through here.)
        off_tape: the coarse scale of a two-scale generator.  Its frame feeds only its own FIFO, no loss reads it (upstream
        scores the finest scale alone), so the heads run outside the autograd graph on detached features and detached views of
        their parameters: no backward node is announced for them (expect_gradient), nothing is counted on the weights."""
        s = self.spec
        G, H, W = s.ngf, img_feat.shape[1], img_feat.shape[2]
        d7 = ops.conv_desc(H, W, G, 3, 7, 1, 3, ops.PAD_REFLECT)

        def hp(key):
            t = self.p(key)
            if not off_tape:
                return t
            d = t.detach()
            d._t2v_owner = t
            return d

        with (torch.no_grad() if off_tape else contextlib.nullcontext()):
            if off_tape:
                img_feat = img_feat.detach()
                flow_feat = flow_feat.detach() if flow_feat is not None else None
            ck = next(k for k, _, kind in self.keys if kind == "head")
            raw = conv_block(img_feat, hp(ck + ".weight"), hp(ck + ".bias"), d7, norm=None, relu=0, act=ops.ACT_TANH)
            if flow_feat is None:
                return raw, (None if s.no_flow else raw), None
            kf, kw = next(k for k, _, kind in self.keys if kind == "flow_w")
            w3 = _CatParams.apply(hp(kf + ".weight"), hp(kw + ".weight"))
            b3 = _CatParams.apply(hp(kf + ".bias"), hp(kw + ".bias"))
            fw = conv_block(flow_feat, w3, b3, d7, norm=None, relu=0, act=ops.ACT_FLOW_W, slope=20.0 * (2 ** s.scale))
            fake = raw if use_raw_only else _WarpComposite.apply(raw, fw, prev, s.prev_nc - 3)
        return fake, raw, fw

    def forward(self, pose, prev, use_raw_only=False, full=False, need_flow=True, feats=False):
        """pose [1,H,W,12], prev [1,H,W,8] NHWC -> fake [1,H,W,4] (RGB in channels 0..2).  full=True returns
        (fake, raw, flow_w): raw = the tanh image before the blend, flow_w [1,H,W,4] = (flow_x, flow_y in pixels,
        weight, 0); both None without a flow branch.  use_raw_only: the first frame of a sequence under
        --no_first_img (fake is raw; flow and weight are still computed, the flow losses see them).
        feats=True (the coarse scale of TwoScaleGenerator): returns (fake, raw, flow_w, img_feat, flow_feat) -- the two
        decoder outputs [1,H,W,ngf] the heads read, attached; the heads themselves run off the tape (_heads)."""
        s = self.spec
        n, G = s.n_downsample, s.ngf
        H, W = pose.shape[1], pose.shape[2]
        norm = "instance"   # BatchNorm2d(train) with N=1 == instance norm + affine
        it = iter(self.keys)

        def cna(x, desc, relu=1, res=None, need_dx=True):
            ck, nk, kind = next(it)
            g = self.p(nk + ".weight") if s.norm == "batch" else None
            b = self.p(nk + ".bias") if s.norm == "batch" else None
            return conv_block(x, self.p(ck + ".weight"), self.p(ck + ".bias"), desc, g, b, res, norm, relu,
                              need_dx=need_dx)

        def encoder(x, in_nc, nb):
            h = cna(x, ops.conv_desc(H, W, in_nc, G, 7, 1, 3, ops.PAD_REFLECT), need_dx=False)
            for i in range(n):
                h = cna(h, ops.conv_desc(H >> i, W >> i, G << i, G << (i + 1), 3, 2, 1, ops.PAD_ZERO))
            return resblocks(h, nb)

        def resblocks(h, nb):
            C, hb, wb = G << n, H >> n, W >> n
            d = ops.conv_desc(hb, wb, C, C, 3, 1, 1, ops.PAD_REFLECT)
            for _ in range(nb):
                t = cna(h, d, relu=1)
                h = cna(t, d, relu=0, res=h)
            return h

        def decoder(h):
            for i in range(n):
                l = n - i
                h = cna(h, ops.conv_desc(H >> l, W >> l, G << l, G << (l - 1), 3, 2, 1, ops.PAD_ZERO, True))
            return h

        nb_enc, nb_res = s.n_blocks - s.n_blocks // 2, s.n_blocks // 2
        # (the independent halves -- the two encoders, the image and flow branches -- on a second stream, as the inference
        # path runs them, were tried in round 3: +0.7 % with the fixed-grid kernels on; removed)
        d = encoder(pose, s.input_nc, nb_enc) + encoder(prev, s.prev_nc, nb_enc)
        img_feat = decoder(resblocks(d, nb_res))
        if feats:
            next(it)        # (the image head's entry: _heads looks the heads up by kind)
            flow_feat = None if (s.no_flow or (use_raw_only and not need_flow)) else decoder(resblocks(d, nb_res))
            return self._heads(img_feat, flow_feat, prev, use_raw_only, off_tape=True) + (img_feat, flow_feat)
        ck, _, _ = next(it)
        raw = conv_block(img_feat, self.p(ck + ".weight"), self.p(ck + ".bias"),
                         ops.conv_desc(H, W, G, 3, 7, 1, 3, ops.PAD_REFLECT), norm=None, relu=0, act=ops.ACT_TANH)
        if s.no_flow:
            return (raw, None, None) if full else raw
        if use_raw_only and not need_flow:
            # raw-only first frame and no loss reads its flow / weight maps: the flow branch would be a dead part of
            # the graph (its batched weight-gradient slots would never be reduced) -- do not run it
            return (raw, raw, None) if full else raw
        flow_feat = decoder(resblocks(d, nb_res))
        (kf, kw), _, _ = next(it)
        # model_final_flow (2 outputs, x20) and model_final_w (1 output, sigmoid) read the same features: one
        # 3-output conv, as in the inference path; autograd's cat splits the gradient back onto the two parameters
        w3 = _CatParams.apply(self.p(kf + ".weight"), self.p(kw + ".weight"))
        b3 = _CatParams.apply(self.p(kf + ".bias"), self.p(kw + ".bias"))
        fw = conv_block(flow_feat, w3, b3, ops.conv_desc(H, W, G, 3, 7, 1, 3, ops.PAD_REFLECT), norm=None, relu=0,
                        act=ops.ACT_FLOW_W, slope=20.0 * (2 ** s.scale))
        fake = raw if use_raw_only else _WarpComposite.apply(raw, fw, prev, s.prev_nc - 3)
        return (fake, raw, fw) if full else fake

    # what the trainer's frame loop asks of a generator (TwoScaleGenerator answers the same three calls)
    def check_geometry(self, H, W):
        pass

    def zero_prev(self, H, W, device):
        """the FIFO in front of a sequence's first frame: [1,H,W,8]"""
        return torch.zeros(1, H, W, ops.round_up(self.spec.prev_nc, 4), dtype=torch.float32, device=device)

    def frame(self, pose, prev, use_raw_only=False, need_flow=True):
        """-> forward(full=True)'s (fake, raw, flow_w), the FIFO this frame read, the FIFO behind it"""
        fake, raw, fw = self(pose, prev, use_raw_only=use_raw_only, full=True, need_flow=need_flow)
        return fake, raw, fw, prev, shift(prev, fake)


class TrainableLocalGenerator(TrainableGenerator):
    """CompositeLocalGenerator: the fine-scale enhancer netG{s >= 1}, fed by the coarse scale's two decoder
    outputs; upstream parameter names (layer_keys of a local spec).  spec.ngf is this scale's own width (ngf_global / 2^scale)."""
    LOCAL = True

    def forward(self, pose, prev, img_feat_coarse, flow_feat_coarse, use_raw_only=False, full=False, need_flow=True):
        """pose [1,H,W,12], prev [1,H,W,8], img_feat_coarse / flow_feat_coarse [1,H/2,W/2,2*ngf] (flow_feat_coarse None where
        the flow branch does not run) -> what TrainableGenerator.forward returns."""
        s = self.spec
        G = s.ngf
        H, W = pose.shape[1], pose.shape[2]
        if H % 2 or W % 2 or tuple(img_feat_coarse.shape[1:]) != (H // 2, W // 2, 2 * G):
            raise ValueError("TrainableLocalGenerator: a %d x %d frame with ngf %d takes coarse features [1, %d, %d, %d], not %s"
                             % (H, W, G, H // 2, W // 2, 2 * G, list(img_feat_coarse.shape)))
        norm = "instance"   # BatchNorm2d(train) with N=1 == instance norm + affine
        it = iter(self.keys)

        def cna(x, desc, relu=1, res=None, need_dx=True):
            ck, nk, kind = next(it)
            g = self.p(nk + ".weight") if s.norm == "batch" else None
            b = self.p(nk + ".bias") if s.norm == "batch" else None
            return conv_block(x, self.p(ck + ".weight"), self.p(ck + ".bias"), desc, g, b, res, norm, relu,
                              need_dx=need_dx)

        def encoder(x, in_nc, res=None):
            h = cna(x, ops.conv_desc(H, W, in_nc, G, 7, 1, 3, ops.PAD_REFLECT), need_dx=False)
            return cna(h, ops.conv_desc(H, W, G, 2 * G, 3, 2, 1, ops.PAD_ZERO), res=res)

        def up(h):
            d3 = ops.conv_desc(H // 2, W // 2, 2 * G, 2 * G, 3, 1, 1, ops.PAD_REFLECT)
            for _ in range(s.n_blocks):
                t = cna(h, d3, relu=1)
                h = cna(t, d3, relu=0, res=h)
            return cna(h, ops.conv_desc(H // 2, W // 2, 2 * G, G, 3, 2, 1, ops.PAD_ZERO, True))

        # model_down_seg(x) + model_down_img(prev): the second encoder's last block takes the first one's output as its
        # residual, so the add rides in that block's norm-apply pass (y = relu(norm(c)) + res)
        d = encoder(prev, s.prev_nc, res=encoder(pose, s.input_nc))
        img_feat = up(d + img_feat_coarse)
        next(it)        # (the image head's entry: _heads looks the heads up by kind)
        flow_feat = None
        if not (s.no_flow or (use_raw_only and not need_flow)):
            flow_feat = up(d + flow_feat_coarse)
        out = self._heads(img_feat, flow_feat, prev, use_raw_only)
        return out if full else out[0]


class TwoScaleGenerator(torch.nn.Module):
    """--n_scales_spatial 2: the global generator G0 on the H/2 x W/2 level of the pyramid and the local enhancer G1 on the
    frame itself, per frame what Vid2VidModelG.inference_nhwc_batch does.  The coarse pose window is ops.avgpool3x3s2 of the
    fine one; each scale keeps the FIFO of its OWN generated frames (detached); G0's two decoder outputs reach G1 attached, so
    the losses -- all on G1's outputs -- train G0's trunk through them.  G0's three head convolutions feed only its FIFO and
    receive no gradient (as upstream): head_params() names them, the trainer keeps them out of the optimiser and the buckets."""

    def __init__(self, G0, G1):
        super().__init__()
        self.G0, self.G1 = G0, G1
        self.spec = G1.spec

    def head_params(self):
        return [p for k, p in self.G0.named_upstream_parameters().items() if k.startswith("model_final_")]

    def check_geometry(self, H, W):
        m = 2 ** (self.G0.spec.n_downsample + 1)
        if H % m or W % m:
            raise ValueError("two-scale generator: a %d x %d frame is no multiple of %d = 2^(n_downsample_G %d + 1) in both "
                             "dimensions (the coarse scale halves it, G0 halves that %d times)"
                             % (H, W, m, self.G0.spec.n_downsample, self.G0.spec.n_downsample))

    def zero_prev(self, H, W, device):
        """the FIFOs in front of a sequence's first frame: (finest scale's [1,H,W,8], coarse scale's [1,H/2,W/2,8])"""
        cs = ops.round_up(self.spec.prev_nc, 4)
        return (torch.zeros(1, H, W, cs, dtype=torch.float32, device=device),
                torch.zeros(1, H // 2, W // 2, cs, dtype=torch.float32, device=device))

    def forward(self, pose, prev, use_raw_only=False, need_flow=True):
        """pose [1,H,W,12]; prev = (fine FIFO, coarse FIFO) -> (fake, raw, flow_w) of the finest scale as
        TrainableGenerator.forward(full=True) returns them, the coarse scale's frame [1,H/2,W/2,4] (detached), and the pair of
        FIFOs behind this frame."""
        H, W = pose.shape[1], pose.shape[2]
        self.check_geometry(H, W)
        prev1, prev0 = prev
        with torch.no_grad():
            pose0 = ops.avgpool3x3s2(pose[0]).unsqueeze(0)
        fake0, _, _, img_feat, flow_feat = self.G0(pose0, prev0, use_raw_only=use_raw_only, full=True, need_flow=need_flow,
                                                   feats=True)
        fake, raw, fw = self.G1(pose, prev1, img_feat, flow_feat, use_raw_only=use_raw_only, full=True, need_flow=need_flow)
        return fake, raw, fw, fake0, (shift(prev1, fake), shift(prev0, fake0))

    def frame(self, pose, prev, use_raw_only=False, need_flow=True):
        """TrainableGenerator.frame on the pair of FIFOs; the FIFO the frame read is the finest scale's: the losses read that scale"""
        fake, raw, fw, _, behind = self(pose, prev, use_raw_only=use_raw_only, need_flow=need_flow)
        return fake, raw, fw, prev[0], behind


def global_generator_frozen(epoch, niter_fix_global):
    """--niter_fix_global N (upstream's update_fixed_params): with two spatial scales only the local enhancer trains during
    the epochs 1 .. N; from epoch N + 1 on both generators do.  N = 0: both from the start."""
    return 1 <= epoch <= niter_fix_global


class TrainableDiscriminator(torch.nn.Module):
    """MultiscaleDiscriminator (num_D PatchGANs, getIntermFeat), upstream parameter names
    `scale{i}_layer{j}.{0,1}.*`; BatchNorm statistics over the batch."""

    def __init__(self, input_nc, state_dict, ndf=64, n_layers=3, num_D=2, norm="batch", device="cuda"):
        super().__init__()
        self.input_nc, self.n_layers, self.num_D, self.norm = input_nc, n_layers, num_D, norm
        self.params = torch.nn.ParameterDict()
        for k, v in state_dict.items():
            if "running" in k or "num_batches" in k:
                continue
            self.params[k.replace(".", "/")] = torch.nn.Parameter(v.to(device, torch.float32).contiguous())
        self.ndfs = [min(ndf * 2 ** (num_D - 1 - i), 64) for i in range(num_D)]
        self._frozen = False

    def p(self, key):
        t = self.params[key.replace(".", "/")]
        if not self._frozen:
            return t
        d = t.detach()
        d._t2v_owner = t
        return d

    def named_upstream_parameters(self):
        return {k.replace("/", "."): v for k, v in self.params.items()}

    def _single(self, x, i, groups=1, bn_times=None, pt_skip=0):
        ndf = self.ndfs[i]
        chans = [(self.input_nc, ndf, 2, False)]
        nf = ndf
        for _ in range(1, self.n_layers):
            nf_prev, nf = nf, min(nf * 2, 512)
            chans.append((nf_prev, nf, 2, True))
        nf_prev, nf = nf, min(nf * 2, 512)
        chans += [(nf_prev, nf, 1, True), (nf, 1, 1, False)]
        feats, cur = [], x
        for j, (cin, cout, stride, has_norm) in enumerate(chans):
            pre = "scale%d_layer%d" % (i, j)
            desc = ops.conv_desc(cur.shape[1], cur.shape[2], cin, cout, 4, stride, 2, ops.PAD_ZERO)
            last = j == len(chans) - 1
            if has_norm:
                g = self.p(pre + ".1.weight") if self.norm == "batch" else None
                b = self.p(pre + ".1.bias") if self.norm == "batch" else None
                cur = conv_block(cur, self.p(pre + ".0.weight"), self.p(pre + ".0.bias"), desc, g, b, None, self.norm, 2,
                                 groups=groups, bn_times=bn_times, pt_skip=pt_skip)
            else:
                cur = conv_block(cur, self.p(pre + ".0.weight"), self.p(pre + ".0.bias"), desc, norm=None, relu=0,
                                 act=ops.ACT_NONE if last else ops.ACT_LRELU, need_dx=2 if j == 0 else True,
                                 groups=groups, pt_skip=pt_skip)
            feats.append(cur)
        return feats

    def forward(self, x, frozen=False, groups=1, bn_times=None, pt_skip=0):
        """x [B,H,W,cs] -> result[i] = stage outputs of the i-th finest scale.  frozen=True: the parameters enter
        detached (the generator-side passes: only the data gradient is wanted, so the backward nodes skip the
        weight-gradient kernels; the packed-weight cache is keyed on the parameter either way).
        groups > 1: x holds that many independent passes of B / groups images (real | fake | raw): every layer is ONE
        launch over all of them, the BatchNorm statistics stay per pass and move their running averages bn_times[g]
        times; pt_skip: leading images a pass-through backward (the generator's loss) skips (_ConvBlock)."""
        self._frozen = frozen
        try:
            result = []
            for i in range(self.num_D):
                result.append(self._single(x, self.num_D - 1 - i, groups, bn_times, pt_skip))
                if i != self.num_D - 1:
                    x = _AvgPool.apply(x)
            return result
        finally:
            self._frozen = False


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.maxpool2x2(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.maxpool2x2_backward(x, dy.contiguous())


# torchvision vgg19 `features` ($SP/torchvision/models/vgg.py:82, cfg 'E'): conv indices and their widths up to
# relu5_1; 'M' = MaxPool2d(2,2).  The five taps are relu1_1, relu2_1, relu3_1, relu4_1, relu5_1 (features[1], [6],
# [11], [20], [29]) [RECALL upstream models/networks.py Vgg19 slices].
VGG19_CFG = [(0, 3, 64, True), (2, 64, 64, False), "M", (5, 64, 128, True), (7, 128, 128, False), "M",
             (10, 128, 256, True), (12, 256, 256, False), (14, 256, 256, False), (16, 256, 256, False), "M",
             (19, 256, 512, True), (21, 512, 512, False), (23, 512, 512, False), (25, 512, 512, False), "M",
             (28, 512, 512, True)]
VGG_WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)


def vgg19_random_state_dict(seed=0):
    """He-initialised stand-in for torchvision's vgg19 weights (which are not in the reference tree): the same keys
    and shapes, for tests and timing."""
    import numpy as np
    rng = np.random.default_rng(seed)
    sd = {}
    for item in VGG19_CFG:
        if item == "M":
            continue
        idx, cin, cout, _ = item
        sd["features.%d.weight" % idx] = torch.from_numpy(
            (rng.standard_normal((cout, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32))
        sd["features.%d.bias" % idx] = torch.from_numpy((rng.standard_normal(cout) * 0.05).astype(np.float32))
    return sd


class HipVGG19Features(torch.nn.Module):
    """Frozen VGG19 feature extractor of the perceptual loss: 3x3 zero-padded convs with the
    ReLU fused in the conv epilogue, 2x2 max-pools; forward returns the five relu*_1 maps.  Weights: a torchvision
    `vgg19` state dict (keys features.N.weight / .bias)."""

    def __init__(self, state_dict, device="cuda"):
        super().__init__()
        self.w = {}
        for item in VGG19_CFG:
            if item == "M":
                continue
            idx = item[0]
            self.w[idx] = (state_dict["features.%d.weight" % idx].to(device, torch.float32).contiguous(),
                           state_dict["features.%d.bias" % idx].to(device, torch.float32).contiguous())

    def forward(self, x):
        """x [B,H,W,cs>=3] in [-1,1] (no ImageNet normalisation, as upstream) -> [relu1_1, ..., relu5_1]."""
        taps, cur = [], x
        for item in VGG19_CFG:
            if item == "M":
                cur = _MaxPool.apply(cur)
                continue
            idx, cin, cout, tap = item
            desc = ops.conv_desc(cur.shape[1], cur.shape[2], cin, cout, 3, 1, 1, ops.PAD_ZERO)
            w, b = self.w[idx]
            cur = conv_block(cur, w, b, desc, norm=None, relu=0, act=ops.ACT_LRELU, slope=0.0)
            if tap:
                taps.append(cur)
        return taps


def vgg_loss(vgg, fake, real, real_feats=None):
    """VGGLoss [RECALL upstream models/networks.py]: sum_i w_i * L1(vgg(fake)_i, vgg(real)_i.detach()),
    w = 1/32, 1/16, 1/8, 1/4, 1.  Upstream first halves inputs wider than 1024 px with AvgPool2d(2, 2); that only
    happens in two-scale training at 2048 px, which stays refused here."""
    if fake.shape[2] > 1024:
        raise NotImplementedError("vgg_loss: inputs wider than 1024 px (upstream's AvgPool2d(2,2) pre-scaling)")
    fr = real_feats          # the real frames' taps, when the caller already has them (two fake inputs, one real)
    if fr is None:
        with torch.no_grad():
            fr = vgg(real)
    ff = vgg(fake)
    return sum(wi * _L1.apply(a, b, a.numel()) for wi, a, b in zip(VGG_WEIGHTS, ff, fr))


def _plus(total, term):
    """total + term, where None is the empty sum (no `0.0 + term` node in the graph)"""
    return term if total is None else total + term


def gan_loss(pred_scales, target_is_real):
    return sum(_MseConst.apply(st[-1], 1.0 if target_is_real else 0.0) for st in pred_scales)


def feature_matching_loss(pred_fake, pred_real, n_layers=3, lambda_feat=10.0):
    num_D = len(pred_fake)
    total = 0.0
    for i in range(num_D):
        for j in range(len(pred_fake[i]) - 1):
            f, r = pred_fake[i][j], pred_real[i][j].detach()
            total = total + _L1.apply(f, r, f.numel()) * ((1.0 / num_D) * (4.0 / (n_layers + 1)) * lambda_feat)
    return total


class LossBook:
    """The scalar loss terms of one train step, evaluated together (ops.loss_terms: one launch for the values AND the
    gradient seeds of all terms, one per-term final pass).

    Every term's weight is a host number -- lambda_feat, the 1/2 of the discriminator loss, face_weight, 1 / n of the
    mean -- so the gradient of the total with respect to a term's operand is known without any device scalar: the term
    kernel writes it (the `seed`) in the same pass that reduces the value, and the backward passes start from those seeds
    (torch.autograd.grad(outputs=<operands>, grad_outputs=<seeds>)) instead of from a scalar graph of one-element
    multiplies and adds.  Values come back in one vector: `read()` sums them by name on the host."""

    CHUNK = 1 << 14

    def __init__(self, device):
        self.dev = torch.device(device)
        self.terms = []
        self.out = None
        self.zero_names = []      # named terms that are switched off in this step: reported as 0.0
        self._host = self._devb = self._part = None
        self._pending = None

    def reset(self):
        self.terms, self.out, self.zero_names = [], None, []

    def mse(self, name, x, target, weight, seed=None):
        """weight * mean((x[..., 0] - target)^2): x a contiguous [.., cs] block of logit rows (LSGAN; THCUNN.h:356); seed (same
        block of a gradient tensor) receives weight * 2 (x - target) / n in channel 0 and zeros in the pad channels"""
        cs = x.shape[-1]
        n = x.numel() // cs
        assert x.is_contiguous() and (seed is None or (seed.is_contiguous() and seed.shape == x.shape))
        self.terms.append((name, 0, x, None, seed, n, cs, float(target), weight / n, weight / n))

    def l1(self, name, a, b, weight, seed=None):
        """weight * mean(|a - b|) (feature matching; THCUNN.h:18), gradient with respect to `a` only"""
        n = a.numel()
        assert a.is_contiguous() and b.is_contiguous() and a.shape == b.shape
        assert seed is None or (seed.is_contiguous() and seed.shape == a.shape)
        self.terms.append((name, 1, a, b, seed, n, 1, 0.0, weight / n, weight / n))

    def zero(self, seed):
        """rows of a gradient tensor no loss term reaches in that backward pass: exact zeros"""
        assert seed.is_contiguous()
        self.terms.append((None, 2, seed, None, seed, seed.numel(), 1, 0.0, 0.0, 0.0))

    def run(self):
        """enqueue the launch for the terms collected so far"""
        import numpy as np
        T = len(self.terms)
        if T == 0:
            return
        ch = self.CHUNK
        counts = [max(1, -(-t[5] // ch)) for t in self.terms]
        NC = sum(counts)
        # one staging buffer, 8-byte aligned segments: term_ptrs | chunk_off | term_ints | chunk_term | term_chunk0 | term_floats
        segs, o = {}, 0
        for key, nbytes in (("tp", 32 * T), ("co", 8 * NC), ("ti", 8 * T), ("ct", 4 * NC), ("t0", 4 * (T + 1)), ("tf", 12 * T)):
            segs[key] = (o, nbytes)
            o += -(-nbytes // 8) * 8
        if self._host is None or self._host.numel() < o:
            cap = max(o, 1 << 16)
            self._host = torch.empty(cap, dtype=torch.uint8).pin_memory()
            self._devb = torch.empty(cap, dtype=torch.uint8, device=self.dev)
        if self._part is None or self._part.numel() < NC + T:
            self._part = torch.empty(max(NC + T, 1 << 14), dtype=torch.float32, device=self.dev)
        if self._pending is not None:
            self._pending.synchronize()      # the previous launch's table copy has left the pinned staging buffer
        hv = self._host.numpy()

        def view(key, dt):
            a, nb = segs[key]
            return hv[a:a + nb].view(dt)
        tp, co, ti, ct, t0, tf = view("tp", np.int64), view("co", np.int64), view("ti", np.int32), view("ct", np.int32), \
            view("t0", np.int32), view("tf", np.float32)
        c0 = 0
        for t, (name, op, a, b, seed, n, cs, c, ss, vs) in enumerate(self.terms):
            tp[4 * t:4 * t + 4] = (a.data_ptr(), b.data_ptr() if b is not None else 0, seed.data_ptr() if seed is not None else 0, n)
            ti[2 * t:2 * t + 2] = (op, cs)
            tf[3 * t:3 * t + 3] = (c, ss, vs)
            t0[t] = c0
            k = counts[t]
            ct[c0:c0 + k] = t
            co[c0:c0 + k] = np.arange(k, dtype=np.int64) * ch
            c0 += k
        t0[T] = c0
        self._devb[:o].copy_(self._host[:o], non_blocking=True)

        def dev(key):
            a, nb = segs[key]
            return self._devb[a:a + nb]
        self.out = self._part[NC:NC + T]
        ops.loss_terms(dev("tp"), dev("ti"), dev("tf"), dev("ct"), dev("co"), dev("t0"), T, NC, ch, self._part, self.out)
        self._pending = torch.cuda.current_stream().record_event()
        # the launch is enqueued: let go of the operands (views into the step's autograd graph -- held here they would keep
        # the whole graph alive into the next step's forward pass); the names stay for read()
        self.terms = [(t[0],) for t in self.terms]

    def value_tensors(self):
        """{name: [indices into self.out]} of the named terms"""
        idx = {}
        for t, term in enumerate(self.terms):
            if term[0] is not None:
                idx.setdefault(term[0], []).append(t)
        return idx

    def read(self, extra=None):
        """one host read for the step: {name: value} of the named terms (+ the one-element device tensors in `extra`)"""
        names = self.value_tensors()
        keys = list((extra or {}).keys())
        parts = ([self.out] if self.out is not None else []) + [extra[k].detach().reshape(1).float() for k in keys]
        if not parts:
            return {}
        host = torch.cat(parts).tolist()
        T = len(self.terms) if self.out is not None else 0
        res = {k: sum(host[i] for i in ix) for k, ix in names.items()}
        for j, k in enumerate(keys):
            res[k] = host[T + j]
        return res


def read_losses(named, book):
    """A step's reported losses, in `named`'s order -- the order the step built its terms in, whichever form built them.
    named: {name: one-element device tensor | host number | None = `book` holds the terms of that name (or lists it in
    zero_names)}.  One host read for the step (LossBook.read: the book's values and the device tensors together)."""
    host = book.read({k: v for k, v in named.items() if torch.is_tensor(v)})
    if host:
        ops.check_async_errors()      # (the read-back above synchronised: errors the step's kernels could only flag)
    for k in book.zero_names:
        host.setdefault(k, 0.0)
    return {k: host[k] if k in host else float(v) for k, v in named.items()}


# ------------------------------------------------------------------------------------------------
# optimiser + data-parallel gradient exchange
# ------------------------------------------------------------------------------------------------
class FusedAdam:
    """torch-0.4.1 Adam semantics ($SP/torch/optim/adam.py:48-98), one fused HIP kernel per tensor.  As there,
    `state['step']` is per parameter and only advances when that parameter has a gradient (adam.py:58-60, 82): a
    discriminator that sits out the first iterations (temporal windows not yet full, no face box) starts its bias
    correction at 1 when it first trains."""

    def __init__(self, params, lr=2e-4, betas=(0.5, 0.999), eps=1e-8):
        self.params = [p for p in params]
        self.lr, self.betas, self.eps = lr, betas, eps
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.steps = [0] * len(self.params)

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    CHUNK = 1 << 16

    def _tables(self):
        """static device tables of the multi-tensor launch (parameter / moment addresses, lengths, chunk map)"""
        if getattr(self, "_tab", None) is None:
            dev = self.params[0].device
            import math
            ct, co = [], []
            for t, p in enumerate(self.params):
                for c in range(math.ceil(p.numel() / self.CHUNK)):
                    ct.append(t)
                    co.append(c * self.CHUNK)
            self._tab = {
                "nelem": torch.tensor([p.numel() for p in self.params], dtype=torch.int64, device=dev),
                "chunk_tensor": torch.tensor(ct, dtype=torch.int32, device=dev),
                "chunk_off": torch.tensor(co, dtype=torch.int64, device=dev),
                "ptrs_host": torch.zeros(len(self.params), 4, dtype=torch.int64).pin_memory(),
                "ss_host": torch.zeros(len(self.params), dtype=torch.float32).pin_memory(),
                "ptrs": torch.zeros(len(self.params), 4, dtype=torch.int64, device=dev),
                "ss": torch.zeros(len(self.params), dtype=torch.float32, device=dev),
            }
        return self._tab

    def step(self):
        """One launch for all tensors (T2V_ADAM_MULTI=0: one launch per tensor).  Every parameter keeps its own step
        count; a parameter without gradient is skipped, moments included."""
        import math
        if not switch("T2V_ADAM_MULTI") or not self.params:
            for i, (p, m, v) in enumerate(zip(self.params, self.m, self.v)):
                if p.grad is not None:
                    self.steps[i] += 1
                    ops.adam_step(p.data, p.grad.contiguous(), m, v, self.lr, self.betas[0], self.betas[1], self.eps,
                                  self.steps[i])
                    invalidate_packs(p)   # written through the raw pointer: no tensor version bump
            prefetch_packs(self.params)
            return
        tab = self._tables()
        if getattr(self, "_pending", None) is not None:
            self._pending[1].synchronize()    # the previous step's table copies have left the pinned staging buffers
        grads = []        # kept alive until the launch is enqueued
        ph, sh = tab["ptrs_host"], tab["ss_host"]
        b1, b2 = self.betas
        for i, (p, m, v) in enumerate(zip(self.params, self.m, self.v)):
            g = p.grad
            if g is None:
                ph[i, 1] = 0
                continue
            g = g.contiguous()
            grads.append(g)
            self.steps[i] += 1
            k = self.steps[i]
            ph[i, 0], ph[i, 1], ph[i, 2], ph[i, 3] = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            sh[i] = self.lr * math.sqrt(1.0 - b2 ** k) / (1.0 - b1 ** k)
            invalidate_packs(p)
        tab["ptrs"].copy_(ph, non_blocking=True)
        tab["ss"].copy_(sh, non_blocking=True)
        ops.adam_step_multi(tab["ptrs"], tab["nelem"], tab["ss"], tab["chunk_tensor"], tab["chunk_off"], self.CHUNK, b1, b2,
                            self.eps)
        # the pinned staging tables are reused by the next step: make sure this step's copies have been issued from them
        self._pending = (grads, torch.cuda.current_stream().record_event())
        prefetch_packs(self.params)


# ------------------------------------------------------------------------------------------------
# face discriminator crop (--add_face_disc) and the training loop
# ------------------------------------------------------------------------------------------------
from .keypoints import get_face_region      # noqa: E402,F401 -- the face crop of --add_face_disc (also test.py --metrics)


def discriminator_state_dict(input_nc, ndf, n_layers, num_D, norm, seed):
    """seeded random init in upstream key names (weights_init: N(0,0.02) convs, N(1,0.02) BN weight)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    sd = {}
    for i in range(num_D):
        nd = min(ndf * 2 ** (num_D - 1 - i), 64)
        chans = [(input_nc, nd, False)]
        nf = nd
        for _ in range(1, n_layers):
            nf_prev, nf = nf, min(nf * 2, 512)
            chans.append((nf_prev, nf, True))
        nf_prev, nf = nf, min(nf * 2, 512)
        chans += [(nf_prev, nf, True), (nf, 1, False)]
        for j, (cin, cout, has_norm) in enumerate(chans):
            pre = "scale%d_layer%d" % (i, j)
            sd[pre + ".0.weight"] = torch.from_numpy(rng.normal(0, 0.02, (cout, cin, 4, 4)).astype("float32"))
            b = 1.0 / (cin * 16) ** 0.5
            sd[pre + ".0.bias"] = torch.from_numpy(rng.uniform(-b, b, (cout,)).astype("float32"))
            if has_norm and norm == "batch":
                sd[pre + ".1.weight"] = torch.from_numpy(rng.normal(1, 0.02, (cout,)).astype("float32"))
                sd[pre + ".1.bias"] = torch.zeros(cout)
    return sd


class Vid2VidTrainer:
    """One rank of the data-parallel train step: 1 sequence per GPU, `max_frames_per_gpu`
    frames per chunk, previous frames detached (max_frames_backpropagate 1)."""

    def __init__(self, opt, device="cuda:0", seed=1):
        self.opt, self.device = opt, device
        # flags of upstream's train.py that would train a DIFFERENT configuration here: refuse instead of ignoring
        for flag, bad, why in (("no_lsgan", bool(getattr(opt, "no_lsgan", False)), "only the LSGAN (MSE) objective is built"),
                               ("n_scales_spatial", getattr(opt, "n_scales_spatial", 1) > 2,
                                "two spatial scales are built (the global generator and one local enhancer), not %d"
                                % getattr(opt, "n_scales_spatial", 1)),
                               ("max_frames_backpropagate", getattr(opt, "max_frames_backpropagate", 1) > 1,
                                "generated previous frames are always detached (the recipe's default, 1)"),
                               ("use_single_G", bool(getattr(opt, "use_single_G", False)), "no first-frame generator"),
                               ("fg", bool(getattr(opt, "fg", False)), "no foreground / background generators"),
                               ("arith", getattr(opt, "arith", "fp32") != "fp32",
                                "the split-bf16 trunk is a forward-only form; training computes in fp32")):
            if bad:
                raise NotImplementedError("--%s: %s" % (flag, why))
        if getattr(opt, "pool_size", 1) > 1:
            print("warning: --pool_size has no effect here (no image pool)", flush=True)
        input_nc = opt.label_nc if opt.label_nc != 0 else opt.input_nc
        self.spec = GeneratorSpec(input_nc=input_nc * opt.n_frames_G, prev_nc=(opt.n_frames_G - 1) * opt.output_nc,
                                  ngf=opt.ngf, n_downsample=opt.n_downsample_G, n_blocks=opt.n_blocks,
                                  no_flow=bool(opt.no_flow), norm=opt.norm)
        self.two_scale = getattr(opt, "n_scales_spatial", 1) == 2
        # fix_global: G0 is frozen (--niter_fix_global, the first epochs of a two-scale run: set_epoch)
        self.fix_global = False
        if self.two_scale:
            from .model import generator_specs
            self.spec, spec1 = generator_specs(opt)
            self.G = TwoScaleGenerator(TrainableGenerator(self.spec, synthetic_state_dict(self.spec, seed, "vid2vid"), device),
                                       TrainableLocalGenerator(spec1, synthetic_state_dict(spec1, seed + 30, "vid2vid"), device))
            self.nets_G = [("G0", self.G.G0), ("G1", self.G.G1)]
        else:
            self.G = TrainableGenerator(self.spec, synthetic_state_dict(self.spec, seed, "vid2vid"), device)
            self.nets_G = [("G0", self.G)]
        d_in = input_nc + opt.output_nc
        self.D = TrainableDiscriminator(d_in, discriminator_state_dict(d_in, opt.ndf, opt.n_layers_D, opt.num_D, opt.norm,
                                                                       seed + 1), opt.ndf, opt.n_layers_D, opt.num_D,
                                        opt.norm, device)
        self.Df = None
        if opt.add_face_disc:
            nf = max(1, opt.num_D - 2)
            self.Df = TrainableDiscriminator(d_in, discriminator_state_dict(d_in, opt.ndf, opt.n_layers_D, nf, opt.norm,
                                                                            seed + 2), opt.ndf, opt.n_layers_D, nf,
                                             opt.norm, device)
        # temporal discriminators netD_T{s}: a multiscale PatchGAN over n_frames_D frames spaced
        # n_frames_D**s apart + the n_frames_D-1 optical flows between them (13 channels).  FlowNet2 is not in the
        # reference tree, so the flow channels are zero; the frame channels train as upstream.
        self.tD = opt.n_frames_D
        self.DT = []
        for s in range(max(0, opt.n_scales_temporal)):
            dt_in = opt.output_nc * self.tD + 2 * (self.tD - 1)
            self.DT.append(TrainableDiscriminator(dt_in, discriminator_state_dict(dt_in, opt.ndf, opt.n_layers_D, opt.num_D,
                                                                                  opt.norm, seed + 10 + s),
                                                  opt.ndf, opt.n_layers_D, opt.num_D, opt.norm, device))
        self._hist_real, self._hist_fake = [], []    # frames of the running sequence (fakes detached)
        self._hist_slots = {}                        # clip j of a step of several clips (train_step(micro=)) -> its pair
        # where the reference flow comes from when the caller passes none: "zero", "lk" = ops.optical_flow on the real frames,
        # or "lkhs" = the same with the Horn-Schunck refinement (--flow_refine_iters steps per level, --flow_alpha)
        self.flow_ref_mode = getattr(opt, "flow_ref", "zero")
        self._flow_kw = {}
        if self.flow_ref_mode == "lkhs":
            self._flow_kw = dict(refine_iters=int(getattr(opt, "flow_refine_iters", None) or 64),
                                 alpha=float(getattr(opt, "flow_alpha", None) or 0.2))
        d_params = list(self.D.parameters()) + (list(self.Df.parameters()) if self.Df else [])
        for dt in self.DT:
            d_params += list(dt.parameters())
        # perceptual loss (the reference trains with it: README.md:171-176 passes no --no_vgg); its weights come from
        # torchvision's download in the reference and from --vgg_weights here
        self.vgg = None
        if not opt.no_vgg:
            if getattr(opt, "vgg_weights", ""):
                self.vgg = HipVGG19Features(torch.load(opt.vgg_weights, map_location="cpu"), device)
            elif getattr(opt, "vgg_random_init", False):
                self.vgg = HipVGG19Features(vgg19_random_state_dict(seed + 20), device)
            else:
                print("VGG loss off: no --vgg_weights <torchvision vgg19 .pth> given (the file is not in the reference "
                      "tree; --no_vgg silences this)", flush=True)
        lr_g = lr_d = opt.lr
        betas = (opt.beta1, 0.999)
        if getattr(opt, "TTUR", False):    # [RECALL upstream: two time-scale update rule]
            betas, lr_g, lr_d = (0.0, 0.9), opt.lr / 2.0, opt.lr * 2.0
        self.lr_scale = (lr_g / opt.lr, lr_d / opt.lr)
        if self.two_scale:      # (the first epoch's phase; run_train calls set_epoch at every epoch's start)
            self.fix_global = global_generator_frozen(1, getattr(opt, "niter_fix_global", 0))
        self.optG = FusedAdam(self._trainable_generator_params(), lr_g, betas)
        self.optD = FusedAdam(d_params, lr_d, betas)
        # persistent flat gradient buckets (the backward nodes write into them; exchanged in place)
        self.bucketsG = GradBuckets(self.optG.params, name="G")
        self.bucketsD = GradBuckets(self.optD.params, name="D")
        if getattr(opt, "load_pretrain", ""):
            self.load(opt.which_epoch, opt.load_pretrain)
        self.comm_bytes, self.comm_ms = 0, 0.0
        self.time_comm = os.environ.get("T2V_TRAIN_COMM_TIMING", "0") == "1"
        # keep_visuals: a step leaves `visuals` = {name: tensor of the chunk's LAST frame} for TrainDisplay (train.py
        # --display_web): pose [H,W,12], fake, raw, real [H,W,4] and, with the flow branch, fw [H,W,4] = (flow_x, flow_y,
        # weight, 0), flow_ref [H,W,4], conf_ref [H,W].  References into the step's own tensors: no copy, no kernel.
        self.keep_visuals, self.visuals = False, None

    def _trainable_generator_params(self):
        """What optG and bucketsG hold.  One scale: every generator parameter.  Two scales: G1's, and -- unless G0 is frozen
        (fix_global) -- G0's trunk; G0's three head convolutions never receive a gradient (TwoScaleGenerator), so they are in
        neither: not updated, no Adam moments, not exchanged, and no bucket waits for them.  Sets requires_grad on G0 to match."""
        if not self.two_scale:
            return list(self.G.parameters())
        for p in self.G.G0.parameters():
            p.requires_grad_(not self.fix_global)
        heads = {id(p) for p in self.G.head_params()}
        g0 = [] if self.fix_global else [p for p in self.G.G0.parameters() if id(p) not in heads]
        return g0 + list(self.G.G1.parameters())

    def set_epoch(self, epoch):
        """--niter_fix_global N with two spatial scales: G0 is frozen during the epochs 1 .. N (global_generator_frozen).  Where
        `epoch` changes the phase, the optimiser's parameter tables and the gradient buckets are rebuilt over the new trainable
        set: a parameter that stays keeps its Adam moments and step count, one that joins starts from zero moments."""
        if not self.two_scale:
            return
        frozen = global_generator_frozen(epoch, getattr(self.opt, "niter_fix_global", 0))
        if frozen == self.fix_global:
            return
        self.fix_global = frozen
        old = self.optG
        if getattr(old, "_pending", None) is not None:
            old._pending[1].synchronize()     # (its last step's table copies have left its pinned staging buffers)
        for p in old.params:
            param_state(p).gslot = None
        kept = {id(p): i for i, p in enumerate(old.params)}
        self.optG = FusedAdam(self._trainable_generator_params(), old.lr, old.betas, old.eps)
        for j, p in enumerate(self.optG.params):
            i = kept.get(id(p))
            if i is not None:
                self.optG.m[j], self.optG.v[j], self.optG.steps[j] = old.m[i], old.v[i], old.steps[i]
        self.bucketsG = GradBuckets(self.optG.params, name="G")
        print("epoch %d: the global generator G0 %s (--niter_fix_global %d): %d generator tensors train"
              % (epoch, "is frozen" if frozen else "trains with G1", getattr(self.opt, "niter_fix_global", 0),
                 len(self.optG.params)), flush=True)

    def _d_input(self, A3, img4):
        z = torch.zeros(A3.shape[:-1] + (2,), dtype=torch.float32, device=A3.device)
        return torch.cat([A3, img4[..., :3], z], -1).contiguous()

    def _vgg_term(self, fake, raw, real):
        """lambda_feat * VGGLoss(fake, real) (+ the same on the raw frame with a flow branch) [RECALL upstream: criterionVGG],
        or None without a VGG19"""
        if self.vgg is None:
            return None
        with torch.no_grad():
            real_taps = self.vgg(real)
        loss = vgg_loss(self.vgg, fake, real, real_taps) * self.opt.lambda_feat
        if raw is not None:
            loss = loss + vgg_loss(self.vgg, raw, real, real_taps) * self.opt.lambda_feat
        return loss

    def _flow_terms(self, fake, fw_all, real, real_prev, prevs, flow_ref, conf_ref, first):
        """-> (sum of the flow / warp / weight losses, {name: term})"""
        opt, dev = self.opt, fake.device
        F_, H, W = fake.shape[0], fake.shape[1], fake.shape[2]
        # flow / warp / weight losses [RECALL upstream Vid2VidModelD.forward, compute_flow_losses]:
        #   F_Flow = MaskedL1(flow, flow_ref, conf) * lambda_F      F_Warp = MaskedL1(resample(real_B_prev, flow), real_B, conf) * lambda_T
        #   W      = MaskedL1(weight, 0, conf)  (--no_first_img)    G_Warp = MaskedL1(fake_B, resample(fake_B_prev, flow_ref), conf) * lambda_T
        # flow_ref / conf_ref come from FlowNet2 upstream; here they are inputs (zero flow by default)
        with torch.no_grad():
            if flow_ref is None and self.flow_ref_mode in ("lk", "lkhs"):
                # --flow_ref lk / lkhs: the dense Lucas-Kanade estimate between the real frames (lkhs: refined) stands in for
                # FlowNet2's
                flow_ref = torch.stack([ops.optical_flow(real[i], real_prev[i], **self._flow_kw) for i in range(F_)])
            if flow_ref is None:
                if not getattr(self, "_warned_zero_flow", False):
                    self._warned_zero_flow = True
                    print("warning: flow / warp / weight losses run against a synthetic ZERO reference flow (FlowNet2 is not "
                          "in the reference tree; pass flow_ref / conf_ref or --flow_ref lk / lkhs, or --no_flow to train without the "
                          "flow branch)", flush=True)
                flow_ref = torch.zeros(F_, H, W, 4, dtype=torch.float32, device=dev)
                real_prev_warp = real_prev
            else:
                real_prev_warp = torch.stack([ops.flow_warp(flow_ref[i], real_prev[i], 0) for i in range(F_)])
            if conf_ref is None:
                conf_ref = ((real[..., :3] - real_prev_warp[..., :3]).norm(dim=-1) < 0.02).float()
            if self.keep_visuals:
                self.visuals["flow_ref"], self.visuals["conf_ref"] = flow_ref[-1], conf_ref[-1]
            fake_prev = torch.cat(prevs, 0)
            fake_prev_warp = torch.stack([ops.flow_warp(flow_ref[i], fake_prev[i], self.spec.prev_nc - 3)
                                          for i in range(F_)])
            if first:
                # no generated previous frame exists for a sequence's first frame: upstream warps the REAL previous
                # frame there (fake_B_prev = real_B_prev[:, 0:1] when there is no previous chunk [RECALL
                # compute_fake_B_prev]); the all-zero FIFO stays the generator's INPUT only
                fake_prev_warp[0] = real_prev_warp[0]
        loss_F_flow = masked_l1(fw_all, flow_ref, conf_ref, 2, 0) * opt.lambda_F
        loss_F_warp = masked_l1(_Resample.apply(fw_all, real_prev.contiguous(), 0), real, conf_ref, 3) * opt.lambda_T
        # the weight-map loss exists only under --no_first_img upstream (zero otherwise) [RECALL]
        loss_W = masked_l1(fw_all, None, conf_ref, 1, 2) if getattr(opt, "no_first_img", False) else 0.0
        loss_G_warp = masked_l1(fake, fake_prev_warp, conf_ref, 3) * opt.lambda_T
        return (loss_F_flow + loss_F_warp + loss_W + loss_G_warp,
                {"F_Flow": loss_F_flow, "F_Warp": loss_F_warp, "W": loss_W, "G_Warp": loss_G_warp})

    def _temporal_flows(self, reals, ends, d):
        """--flow_ref lk: the flows between consecutive REAL frames of every temporal window (frames t - (tD-1) d, ..., t - d,
        t for t in ends) -> [len(ends),H,W,2*(tD-1)], channels 2k, 2k+1 = (u, v) of optical_flow(w[k+1], w[k]); the real
        and the generated stack of a temporal discriminator both carry them (upstream: flow_ref_skipped).  None under
        --flow_ref zero: those channels stay zero."""
        if self.flow_ref_mode not in ("lk", "lkhs"):
            return None
        with torch.no_grad():
            rows = []
            for t in ends:
                w = [reals[t - (self.tD - 1 - k) * d] for k in range(self.tD)]
                rows.append(torch.cat([ops.optical_flow(w[k + 1], w[k], **self._flow_kw)[..., :2] for k in range(self.tD - 1)], -1))
            return torch.stack(rows)

    def _temporal_stack(self, frames, ends, d, dt, flows=None):
        """Input of temporal discriminator dt: per window its tD frames' colour channels, then `flows` (_temporal_flows) or
        zeros in the 2*(tD-1) flow channels, zero-padded to the storage width"""
        H, W, dev = frames[0].shape[0], frames[0].shape[1], frames[0].device
        rows = []
        for j, t in enumerate(ends):
            w = [frames[t - (self.tD - 1 - k) * d][..., :3] for k in range(self.tD)]
            nz = ops.round_up(dt.input_nc, 4) - 3 * self.tD
            if flows is not None:
                w.append(flows[j])
                nz -= flows.shape[-1]
            rows.append(torch.cat(w + [torch.zeros(H, W, nz, dtype=torch.float32, device=dev)], -1))
        return torch.stack(rows).contiguous()

    def _d_jobs(self, A3, real, fake, raw, face_boxes):
        """The step's discriminator work, one job at a time: (net, [real input, fake input(, raw input)], (D, G_GAN,
        G_GAN_Feat) names of the reported sums, face_weight) -- the image discriminator, the face discriminator where there are
        boxes, every temporal scale that has a full window.  A generator: a job's inputs (autograd nodes on the generated
        frames) are built when the caller asks for it, so whatever the caller builds between two jobs stays between them in the
        graph; the sequence history is trimmed once the last job has been taken."""
        F_ = real.shape[0]
        # with a flow branch upstream scores fake_B_raw with the same discriminator (and VGG) as well
        yield self.D, [self._d_input(A3, t) for t in (real, fake) + (() if raw is None else (raw,))], \
            ("D", "G_GAN", "G_GAN_Feat"), 1.0
        if self.Df is not None and face_boxes is not None:
            def crop(t):
                return torch.stack([t[i, b[0]:b[1], b[2]:b[3]] for i, b in enumerate(face_boxes)]).contiguous()
            cA = crop(A3)
            # face_weight = 2 on the generator's face terms [RECALL upstream Vid2VidModelD.forward]
            yield self.Df, [self._d_input(cA, crop(real)), self._d_input(cA, crop(fake))], ("D_f", "G_f_GAN", "G_f_GAN_Feat"), 2.0
        # temporal discriminators: every window (t-2d, t-d, t), d = n_frames_D**s, that ends on a frame of this chunk;
        # older frames come from the sequence history (generated ones detached)
        if self.DT:
            n_old = len(self._hist_real)
            reals = self._hist_real + [real[i] for i in range(F_)]
            fks = self._hist_fake + [fake[i] for i in range(F_)]
            for sc, dt in enumerate(self.DT):
                d = self.tD ** sc
                ends = [t for t in range(n_old, n_old + F_) if t - (self.tD - 1) * d >= 0]
                if not ends:
                    continue
                flows = self._temporal_flows(reals, ends, d)
                yield dt, [self._temporal_stack(frames, ends, d, dt, flows) for frames in (reals, fks)], \
                    ("D_T%d" % sc, "G_T_GAN%d" % sc, "G_T_GAN_Feat%d" % sc), 1.0
            keep = (self.tD - 1) * self.tD ** (len(self.DT) - 1)
            self._hist_real = [r.detach() for r in reals][-keep:]
            self._hist_fake = [f.detach() for f in fks][-keep:]

    def _d_pass(self, net, inputs, book, names, face_weight=1.0):
        """One discriminator on its real input and its one or two generated inputs (fake, raw) as ONE batch of passes
        (TrainableDiscriminator.forward(groups=...)): every layer is one conv launch, one data-gradient launch and one
        weight-gradient launch for all passes.  Registers the LSGAN and feature-matching terms of compute_loss_D /
        compute_loss_G [RECALL upstream Vid2VidModelD] with `book` and returns (tensors, seeds for G's backward, tensors,
        seeds for D's backward).
        The one forward on a generated input serves both losses (as T2V_D_SHARED_FWD did for the one-pass-per-launch path): D's
        loss reaches D's parameters through it, G's loss reaches the frames through it with D's parameter gradients switched
        off (param_gradients_off); the running statistics still move twice for those passes (upstream's two forwards).
        names = (D, G_GAN, G_GAN_Feat) of the reported sums: D = 0.5 (real + fake [+ raw, with the real term counted again
        as upstream does])."""
        opt = self.opt
        n_d, n_gan, n_feat = names
        P = len(inputs)
        F_ = inputs[0].shape[0]
        feats = net(torch.cat(inputs, 0), groups=P, bn_times=[1] + [2] * (P - 1), pt_skip=F_)
        num_D = len(feats)
        fm_w = 0.0 if opt.no_ganFeat else (1.0 / num_D) * (4.0 / (opt.n_layers_D + 1)) * opt.lambda_feat * face_weight
        tG, sG, tD, sD = [], [], [], []
        if not fm_w:
            book.zero_names.append(n_feat)        # (--no_ganFeat: the term is reported as 0, as the pass-by-pass form does)
        for st in feats:
            logits = st[-1]
            gG, gD = torch.empty_like(logits), torch.empty_like(logits)
            book.zero(gG[:F_])
            book.mse(n_d, logits[:F_], 1.0, 0.5 * (P - 1), seed=gD[:F_])
            for g in range(1, P):
                sl = slice(g * F_, (g + 1) * F_)
                book.mse(n_d, logits[sl], 0.0, 0.5, seed=gD[sl])
                book.mse(n_gan, logits[sl], 1.0, face_weight, seed=gG[sl])
            tG.append(logits); sG.append(gG); tD.append(logits); sD.append(gD)
            if fm_w:
                for f in st[:-1]:
                    gf = torch.empty_like(f)
                    book.zero(gf[:F_])
                    for g in range(1, P):
                        sl = slice(g * F_, (g + 1) * F_)
                        book.l1(n_feat, f[sl], f[:F_], fm_w, seed=gf[sl])
                    tG.append(f); sG.append(gf)
        return tG, sG, tD, sD

    def _d_terms(self, net, inputs, face_weight, shared):
        """_d_pass's test twin (T2V_D_BATCHED=0, which also serves T2V_D_SHARED_FWD=0): the same job one launch per pass and
        per loss term, the scalar graph on autograd -> (G's GAN term, G's feature-matching term, D's term).
        compute_loss_D(netD, real_A, real_B, fake) [RECALL upstream Vid2VidModelD]: real pass, fake pass on the detached
        frame (D's loss), fake pass for G's GAN + feature-matching loss with D's parameters detached (only their data gradient
        is wanted).  shared: one forward on a generated input serves both losses, as in _d_pass; the running statistics
        still move twice.  A second generated input (raw) adds its terms to the first's, and the real term once more: upstream's
        second real pass returns the values of the first (same weights, same batch)."""
        opt = self.opt
        pr = net(inputs[0])
        d_real = d_fake = g_gan = g_fm = None
        for x in inputs[1:]:
            if shared:
                with bn_updates(2):
                    pfd = pfg = net(x)
            else:
                pfd, pfg = net(x.detach()), net(x, frozen=True)
            d_real, d_fake = _plus(d_real, gan_loss(pr, True)), _plus(d_fake, gan_loss(pfd, False))
            g_gan = _plus(g_gan, gan_loss(pfg, True))
            if not opt.no_ganFeat:
                g_fm = _plus(g_fm, feature_matching_loss(pfg, pr, opt.n_layers_D, opt.lambda_feat))
        if g_fm is None:
            g_fm = 0.0
        if face_weight != 1.0:
            g_gan, g_fm = g_gan * face_weight, g_fm * face_weight
        return g_gan, g_fm, 0.5 * (d_fake + d_real)

    def _d_backward_on_its_own_stream(self, outputs, seeds, d_params):
        """The discriminators' own backward pass (their LSGAN terms: seeds on the logits only) without the autograd engine:
        every output is the end of a chain of _ConvBlock nodes, a node object is its own `ctx`, so each chain is
        `dy = _ConvBlock.backward(node, dy)[0]` from the logits down to the layer that owes no data gradient
        (input_gradients_off).  The nodes deliver their parameter gradients into the bucket slots as under the engine -- the
        same kernels on the same operands in the same order: the same bits -- but on THIS call's stream, the trainer's
        `_d_stream`, which waits for everything the current stream holds (forward passes, loss seeds) and which the caller
        joins before it touches D's gradients.  The engine would run these nodes on the stream of their forward, i.e. behind
        the generator's whole backward pass.  The graph stays alive until the step returns (the generator's pass retains it),
        so the saved tensors both passes read are not handed back to the allocator while this stream still reads them.
        Returns the stream, or None: not switched on (T2V_D_BWD_STREAM=1; OFF by default: the step is 1 ms faster with it where
        no process group exists -- scripts/train_bench.py, 86.9 -> 85.9 ms -- and 3 ms SLOWER in bench.py's block, which runs
        the step as a rank of a job: 84.4 -> 87.3 ms) or not applicable (a parameter without a bucket slot --
        T2V_GRAD_DIRECT=0 -- or an output that is no _ConvBlock result): the caller takes the engine."""
        if os.environ.get("T2V_D_BWD_STREAM", "0") != "1" or not outputs or not outputs[0].is_cuda:
            return None
        node_cls = _ConvBlock._backward_cls
        if any(grad_slot(p) is None for p in d_params) or any(not isinstance(y.grad_fn, node_cls) for y in outputs):
            return None
        if getattr(self, "_d_stream", None) is None:
            self._d_stream = torch.cuda.Stream()
        side = self._d_stream
        side.wait_stream(torch.cuda.current_stream())
        # the weight gradients of these nodes stay ON this stream (it is a side stream already): on the shared weight-gradient
        # stream they would stand in front of every bucket the generator's pass sends off (GradBuckets._launch orders a
        # collective behind that stream) -- the filler would hold the exchange up (measured with the join of that time:
        # 90.5 ms with the exchange against 82.1 without).  Two streams carry GEMMs from here on: one block per CU
        if switch("T2V_TRAIN_SK_HINT") and wgrad_stream_on(outputs[0]):
            STEP.gemm = True
        STEP.inline = True
        try:
            with torch.cuda.stream(side), input_gradients_off():
                for y, g in zip(outputs, seeds):
                    node = y.grad_fn
                    while g is not None and isinstance(node, node_cls):
                        res = _ConvBlock.backward(node, g)
                        if any(r is not None for r in res[1:]):
                            raise RuntimeError("discriminator backward by hand: a node returned a gradient it should have delivered")
                        g, node = res[0], node.next_functions[0][0]
        finally:
            STEP.inline = False
        side_gemm_hint()
        return side

    def _backward_and_update(self, tG, sG, tD, sD, off_in_g_pass, update=True):
        """Both backward passes, the gradient exchange and both optimiser steps.  tG / sG: the tensors G's pass starts from and
        their gradient seeds (None: a scalar), tD / sD: the same for D's pass; off_in_g_pass: the parameters whose gradients
        are switched off during G's pass -- D's, wherever one D forward serves both losses.
        The pass-by-pass form comes with ([loss_G], [None], [loss_D], [None], ...): a scalar loss is the result of a
        multiplication or an addition, never of a _ConvBlock, so _d_backward_on_its_own_stream declines it before it touches
        anything (its isinstance test on grad_fn) and D's pass takes the engine, whatever T2V_D_BWD_STREAM says.
        update=False (a clip of the optimiser step that is not its last): the buckets keep the clip's gradients in their
        accumulators, nothing is exchanged and no optimiser steps."""
        g_params, d_params = self.optG.params, self.optD.params
        # G's backward: the nodes deliver into bucketsG and launch its buckets' collectives as they complete; what is
        # left goes out in absorb() -- all of it in flight under the discriminators' backward pass
        self.bucketsG.seal()
        self.bucketsD.seal()
        # D's loss reaches D's parameters through plain chains of _ConvBlock nodes (logits -> ... -> first layer, no data
        # gradient into the frames) and shares nothing with the generator's backward pass but the saved tensors both read:
        # with T2V_D_BWD_STREAM=1 the chains are walked by hand on a stream of their own BEFORE the generator's pass is
        # enqueued, so that the GPU runs them beside its first ~20 ms, which otherwise have no second queue (measured both
        # ways, off by default: DESIGN 6b "the discriminators' own backward pass beside the generator's")
        d_side = self._d_backward_on_its_own_stream(tD, sD, d_params)
        with param_gradients_off(off_in_g_pass):
            gG = torch.autograd.grad(tG, g_params, grad_outputs=sG, retain_graph=True, allow_unused=True)
        gG = flush_pending_weight_gradients(g_params, gG)
        self.bucketsG.absorb(gG)
        if d_side is not None:
            torch.cuda.current_stream().wait_stream(d_side)
            gD = [None] * len(d_params)
        else:
            with input_gradients_off():      # D's loss: no data gradient into the (attached) generated frames
                gD = torch.autograd.grad(tD, d_params, grad_outputs=sD, allow_unused=True)
        gD = flush_pending_weight_gradients(d_params, gD)      # (a discriminator layer one of whose passes fed no loss term)
        self.bucketsD.absorb(gD)
        if self.time_comm:       # T2V_TRAIN_COMM_TIMING=1: what of the exchange is still running once the backward kernels
            torch.cuda.synchronize()      # have drained = its exposed (not hidden) part
        t0 = time.perf_counter()
        self.comm_bytes = self.bucketsG.finish() + self.bucketsD.finish()
        if self.time_comm and self.comm_bytes:
            torch.cuda.synchronize()
            self.comm_ms = 1e3 * (time.perf_counter() - t0)
        if not update:
            return
        check_presence_across_ranks([self.bucketsG, self.bucketsD], tD[0].device)
        self.optG.step()
        self.optD.step()

    def train_step(self, pose, real, face_boxes=None, prev=None, real_prev=None, flow_ref=None, conf_ref=None, micro=(0, 1)):
        """pose [F,H,W,12] (sliding windows), real [F,H,W,4] NHWC on the device; face_boxes: list of
        (ys,ye,xs,xe) per frame; prev: the carried FIFO of generated frames (None: a new sequence starts).
        With the flow branch: real_prev [F,H,W,4] = the real frame before each frame enables the flow / warp
        losses against flow_ref [F,H,W,4] (flow_x, flow_y in pixels; default zero flow) and its confidence mask
        conf_ref [F,H,W] (default: ||real - resample(real_prev, flow_ref)|| < 0.02, the rule upstream's FlowNet2
        wrapper applies [RECALL]).  Returns (dict of scalar losses, FIFO for the next chunk).
        micro = (j, K): this chunk belongs to clip j of the K clips the rank walks in lock-step (--batchSize above the
        number of ranks).  Every call is one clip's complete forward and backward passes; the gradient buckets sum the K
        clips' gradients in the order j = 0 .. K-1 and the call with j = K-1 exchanges their mean and steps both optimisers
        (GradBuckets.begin_step).  The caller carries each clip's FIFO; the frame history of the temporal discriminators is
        kept here per clip.  BatchNorm running statistics move with clip 0 only, as on DataParallel's replica 0."""
        j, K = micro
        if K > 1:
            self._hist_real, self._hist_fake = self._hist_slots.get(j, ([], []))
        try:
            with batched_weight_gradients(self.optG.params + self.optD.params), \
                    (bn_frozen() if j > 0 else contextlib.nullcontext()):
                return self._train_step(pose, real, face_boxes, prev, real_prev, flow_ref, conf_ref, micro)
        finally:
            if K > 1:
                self._hist_slots[j] = (self._hist_real, self._hist_fake)

    def _train_step(self, pose, real, face_boxes, prev, real_prev=None, flow_ref=None, conf_ref=None, micro=(0, 1)):
        dev = pose.device
        F_, H, W = pose.shape[0], pose.shape[1], pose.shape[2]
        self.bucketsG.begin_step(micro)
        self.bucketsD.begin_step(micro)
        flow_on = not self.spec.no_flow
        first = prev is None
        if first:   # a new sequence starts: zero previous frames, raw-only first frame (--no_first_img)
            self.G.check_geometry(H, W)
            prev = self.G.zero_prev(H, W, dev)
            self._hist_real, self._hist_fake = [], []
        # `prev` is what the generator carries from frame to frame (two scales: the pair of FIFOs); `prevs` are the FIFOs the
        # frames read at the finest scale, the scale every loss below reads
        fakes, raws, fws, prevs = [], [], [], []
        for f in range(F_):
            fk, rw, fw, read, prev = self.G.frame(pose[f:f + 1], prev, use_raw_only=first and f == 0,
                                                  need_flow=real_prev is not None)
            fakes.append(fk)
            raws.append(rw)
            fws.append(fw)
            prevs.append(read)
        fake = torch.cat(fakes, 0)
        raw = torch.cat(raws, 0) if flow_on else None
        fw_all = torch.cat(fws, 0) if (flow_on and real_prev is not None) else None
        A3 = pose[..., 6:9]
        if self.keep_visuals:
            self.visuals = {"pose": pose[-1], "fake": fakes[-1][0].detach(), "real": real[-1],
                            "raw": (raws[-1] if raws[-1] is not None else fakes[-1])[0].detach()}
            if fws[-1] is not None:
                self.visuals["fw"] = fws[-1][0].detach()
        # One D forward on a generated input serves both losses (T2V_D_SHARED_FWD=0: two forwards, as upstream runs them): D's
        # loss reaches D's parameters through it, G's loss reaches the frames through it with D's parameter gradients
        # switched off for that backward pass (param_gradients_off) -- the same values either way, a D forward less per
        # generated input.
        shared = switch("T2V_D_SHARED_FWD")
        # batched (the default): every discriminator runs its real / fake / raw passes as one batch (_d_pass), the LSGAN and
        # feature-matching terms are one launch (LossBook), and both backward passes start from the terms' gradient seeds.
        # T2V_D_BATCHED=0: one launch per pass and per loss term, the scalar graph on autograd (_d_terms; the form the batched
        # one replaced, kept as its test twin).  The flow / warp / weight and VGG terms are scalar nodes of the graph in both.
        batched = shared and switch("T2V_D_BATCHED")
        book = self.book = getattr(self, "book", None) or LossBook(dev)
        book.reset()
        tG, sG, tD, sD = [], [], [], []     # batched: the tensors the two backward passes start from, their gradient seeds
        loss_G = loss_D = None              # the sums on the scalar graph
        named = {}                          # what the step reports, in this order (read_losses)
        for net, inputs, names, face_weight in self._d_jobs(A3, real, fake, raw, face_boxes):
            if batched:
                for have, new in zip((tG, sG, tD, sD), self._d_pass(net, inputs, book, names, face_weight)):
                    have += new
                g_gan = g_fm = l_d = None       # (the book has them)
            else:
                g_gan, g_fm, l_d = self._d_terms(net, inputs, face_weight, shared)
                loss_G, loss_D = _plus(_plus(loss_G, g_gan), g_fm), _plus(loss_D, l_d)
            n_d, n_gan, n_feat = names
            named.update({n_gan: g_gan, n_feat: g_fm, n_d: l_d})
            if net is not self.D:
                continue
            # behind the image discriminator and in front of the others: the generator's terms no discriminator is part of
            vgg_term = self._vgg_term(fake, raw, real)
            if vgg_term is not None:
                loss_G, named["G_VGG"] = _plus(loss_G, vgg_term), vgg_term
            if fw_all is not None:
                flow_sum, flow_named = self._flow_terms(fake, fw_all, real, real_prev, prevs, flow_ref, conf_ref, first)
                loss_G = _plus(loss_G, flow_sum)
                named.update(flow_named)
        if batched:
            book.run()          # values and gradient seeds of all LSGAN / feature-matching terms: one launch
            if torch.is_tensor(loss_G) and loss_G.requires_grad:
                tG, sG = tG + [loss_G], sG + [None]
        else:
            tG, sG, tD, sD = [loss_G], [None], [loss_D], [None]
        self._backward_and_update(tG, sG, tD, sD, self.optD.params if shared else [], update=micro[0] == micro[1] - 1)
        return read_losses(named, book), prev

    def update_learning_rate(self, epoch):
        """linear decay to zero over the niter_decay epochs after `niter` [RECALL upstream update_learning_rate]"""
        lr = self.opt.lr * max(0.0, 1.0 - (epoch - self.opt.niter) / float(max(1, self.opt.niter_decay)))
        print("update learning rate: %f -> %f" % (self.optG.lr / self.lr_scale[0], lr), flush=True)
        self.optG.lr, self.optD.lr = lr * self.lr_scale[0], lr * self.lr_scale[1]

    def load(self, epoch_label, directory=None):
        """--continue_train / --load_pretrain DIR: the nets saved by save() (upstream file names); missing files keep
        their initialisation"""
        import os
        d = directory or os.path.join(self.opt.checkpoints_dir, self.opt.name)
        nets = self.nets_G + [("D", self.D)] + ([("D_f", self.Df)] if self.Df is not None else []) + \
               [("D_T%d" % sc, dt) for sc, dt in enumerate(self.DT)]
        for tag, net in nets:
            path = os.path.join(d, "%s_net_%s.pth" % (epoch_label, tag))
            if not os.path.exists(path):
                print("continue_train: %s not found, keeping the initial weights" % path, flush=True)
                continue
            sd = torch.load(path, map_location="cpu")
            sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}    # saved from nn.DataParallel
            with torch.no_grad():
                for k, p in net.named_upstream_parameters().items():
                    if k not in sd:
                        print("continue_train: %s has no %s, keeping its initial value" % (path, k), flush=True)
                        continue
                    p.copy_(sd[k].to(p.device, torch.float32))
                    st = param_state(p)
                    st.packs = st.repack = None
                    if k.endswith(".weight") and p.dim() == 1 and k[:-len("weight")] + "running_mean" in sd:
                        base = k[:-len("weight")]
                        nbt = sd.get(base + "num_batches_tracked")
                        st.running = [sd[base + "running_mean"].to(p.device, torch.float32).clone(),
                                      sd[base + "running_var"].to(p.device, torch.float32).clone(),
                                      int(nbt) if nbt is not None else 0]

    def save(self, epoch_label, progress=None):
        """progress = (epoch, samples done in it): written to iter.txt beside the nets every time `latest` is saved, so
        that --continue_train never pairs newer weights with an older position."""
        import os
        d = os.path.join(self.opt.checkpoints_dir, self.opt.name)
        os.makedirs(d, exist_ok=True)
        if progress is not None and epoch_label == "latest":
            with open(os.path.join(d, "iter.txt"), "w") as fh:
                fh.write("%d\n%d\n" % (int(progress[0]), int(progress[1])))
        def state_dict(net):
            """upstream's file layout: the parameters plus, for every BatchNorm2d (a 1-D `.weight`), the buffers torch
            0.4.1's module carries ($SP/torch/nn/modules/batchnorm.py: running_mean, running_var, num_batches_tracked)
            so that the file also loads strictly into the reference's own modules.  The norm layers run on batch
            statistics in training AND at test time, so the running statistics are never read: they are
            tracked all the same (running_update_args: momentum 0.1, unbiased variance, one update per forward) and
            written as they stand."""
            sd = {}
            for k, v in net.named_upstream_parameters().items():
                sd[k] = v.detach().cpu()
                if k.endswith(".weight") and v.dim() == 1 and self.opt.norm == "batch":
                    base = k[:-len("weight")]
                    rs = running_stats(v)
                    sd[base + "running_mean"] = rs[0].detach().cpu()
                    sd[base + "running_var"] = rs[1].detach().cpu()
                    sd[base + "num_batches_tracked"] = torch.tensor(rs[2], dtype=torch.long)
            return sd

        for tag, net in self.nets_G:      # (G0, and with two spatial scales G1: create_model loads the pair)
            torch.save(state_dict(net), os.path.join(d, "%s_net_%s.pth" % (epoch_label, tag)))
        torch.save(state_dict(self.D), os.path.join(d, "%s_net_D.pth" % epoch_label))
        if self.Df is not None:
            torch.save(state_dict(self.Df), os.path.join(d, "%s_net_D_f.pth" % epoch_label))
        for sc, dt in enumerate(self.DT):
            torch.save(state_dict(dt), os.path.join(d, "%s_net_D_T%d.pth" % (epoch_label, sc)))


class _ClipFeeder:
    """--train_loader prefetch: clips from TrainPoseDataset.iter_clips, assembled in pinned host memory, uploaded on a
    copy stream one clip ahead of the compute stream (an event orders the two), and finished on the device once per clip:
    real_all [T,H,W,4] = the normalised frames, of which every chunk's `real` and `real_prev` are slices.  Under
    --gpu_resize the loader hands over the decoded frames and ONE launch (ops.resample_crop_normalize_u8) resizes, crops
    and normalises them; a geometry over the kernel's tap limit is resized with Pillow here instead.
    k: clips per iteration (run_train walks them in lock-step): k clips are held while the next k are staged.  real_all is
    kept per held clip and geometry, its pad channel zeroed when it is created; the upload buffers rotate through 2 k slots."""

    def __init__(self, ds, opt, dev, schedule, k=1):
        import collections
        import threading
        self.opt, self.dev = opt, dev
        self.gpu_resize = bool(getattr(opt, "gpu_resize", False))
        self.gpu_decode = self.gpu_resize and bool(getattr(opt, "gpu_decode", False))
        self._jpeg_ws = None                              # the decode calls' workspace (used on the copy stream only)
        self.k = k
        self._jpeg_status = [None] * (2 * k)              # slot -> (device int32, pinned int32) of its clip's statuses
        self.jpeg_clips = self.jpeg_fallback_frames = self.h2d_bytes = 0
        self.copy_stream = torch.cuda.Stream(device=dev)
        self._free = collections.defaultdict(list)      # shape -> pinned tensors not in use
        self._pinned = {}                                 # address of a handed-out array -> its pinned tensor
        self._slots = {}                                  # (slot, what, shape) -> device uint8 buffer
        self._slot_done = [None] * (2 * k)                # compute-stream event: the slot's last clip has been consumed
        self._real_all = {}                               # (held clip j, T, H, W) -> [T,H,W,4] fp32
        self._n = 0
        self._staged = collections.deque()
        self._held = []                                   # (slot, pinned tensors) of the clips being consumed, at most k
        self._lock = threading.Lock()
        self._it = ds.iter_clips(schedule, ahead=2 * k, gpu_resize=self.gpu_resize, alloc=self._alloc, gpu_decode=self.gpu_decode)

    def _alloc(self, shape):      # called from the loader's threads
        shape = tuple(int(v) for v in shape)
        with self._lock:
            t = self._free[shape].pop() if self._free[shape] else None
        if t is None:
            t = torch.empty(shape, dtype=torch.uint8, pin_memory=True)
        a = t.numpy()
        with self._lock:
            self._pinned[a.ctypes.data] = t
        return a

    def _upload(self, arr, slot, what):
        with self._lock:
            t = self._pinned.pop(arr.ctypes.data)
        key = (slot, what, tuple(t.shape))      # (a clip's pose maps and resized frames have one shape)
        d = self._slots.get(key)
        if d is None:
            d = self._slots[key] = torch.empty(t.shape, dtype=torch.uint8, device=self.dev)
        d.copy_(t, non_blocking=True)
        self.h2d_bytes += t.numel()
        return t, d

    def _decode(self, clip, slot):
        """--gpu_decode, on the copy stream: upload the clip's compressed bytes and enqueue the decode call into the slot's
        raw-frame buffer; the statuses travel back to pinned memory behind it.  -> (pinned buffer, raw frames on the device)"""
        from . import jpeg_decode, ops as _ops
        g, _ = clip["jpeg"]
        pj, dj = self._upload(g.buf, slot, "J")
        key = (slot, "B", (g.n, g.H, g.W, 3))
        Bu = self._slots.get(key)
        if Bu is None:
            Bu = self._slots[key] = torch.empty(g.n, g.H, g.W, 3, dtype=torch.uint8, device=self.dev)
        st = self._jpeg_status[slot]
        if st is None or st[0].numel() != g.n:
            st = self._jpeg_status[slot] = (torch.empty(g.n, dtype=torch.int32, device=self.dev),
                                            torch.empty(g.n, dtype=torch.int32, pin_memory=True))
        need = _ops.jpeg_decode_workspace_bytes(g.H, g.W, g.sampling, g.n, g.capacity)
        if self._jpeg_ws is None or self._jpeg_ws.numel() < need:
            self._jpeg_ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        jpeg_decode.decode_uploaded(g, dj, 3, dst=Bu, status=st[0], workspace=self._jpeg_ws)
        st[1].copy_(st[0], non_blocking=True)
        self.jpeg_clips += 1
        return pj, Bu

    def stage(self):
        """take the next clips from the loader (waits for them if the loader is behind) and start their uploads, until k
        are staged"""
        while len(self._staged) < self.k and self._stage_one():
            pass

    def _stage_one(self):
        clip = next(self._it, None)
        if clip is None:
            return False
        slot = self._n % (2 * self.k)
        self._n += 1
        if self._slot_done[slot] is not None:
            self.copy_stream.wait_event(self._slot_done[slot])
        with torch.cuda.stream(self.copy_stream):
            pa, A = self._upload(clip["A"], slot, "A")
            if "jpeg" in clip:
                pb, Bu = self._decode(clip, slot)
            else:
                pb, Bu = self._upload(clip["raw"] if self.gpu_resize else clip["B"], slot, "B")
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self._staged.append((clip, slot, A, Bu, ev, [pa, pb]))
        return True

    def take(self):
        """-> (clip, A uint8 [T,H,W,3] on the device, real_all fp32 [T,H,W,4]); None when the schedule is exhausted.  The
        k clips of an iteration are taken one after the other and stay valid until the next iteration's first take."""
        from . import ops as _ops
        if not self._staged:
            self.stage()
        if not self._staged:
            return None
        clip, slot, A, Bu, ev, pinned = self._staged.popleft()
        if len(self._held) >= self.k:
            with self._lock:      # the previous clips are done with their host arrays (their uploads completed long ago)
                for _, ts in self._held:
                    for t in ts:
                        self._free[tuple(t.shape)].append(t)
            self._held = []
        j = len(self._held)
        self._held.append((slot, pinned))
        torch.cuda.current_stream().wait_event(ev)
        T_, H, W = A.shape[0], A.shape[1], A.shape[2]
        real_all = self._real_all.get((j, T_, H, W))
        if real_all is None:
            real_all = self._real_all[(j, T_, H, W)] = torch.zeros(T_, H, W, 4, device=self.dev)
        prm = clip["params"]
        if "jpeg" in clip:
            # the statuses came with the event the step waits on anyway (the clip was staged a step ago); a frame the
            # decoder gave up on is decoded by Pillow from the bytes the loader read, before the resample launch
            from . import jpeg_decode
            ev.synchronize()
            for i in self._jpeg_status[slot][1].numpy().nonzero()[0].tolist():
                Bu[i].copy_(torch.from_numpy(jpeg_decode.pillow_rgb(clip["jpeg"][1][i])))
                self.jpeg_fallback_frames += 1
        if self.gpu_resize:
            (w, h), (nw, nh) = clip["size"], prm["new_size"]
            if max(_ops.pillow_bicubic_taps(w, nw), _ops.pillow_bicubic_taps(h, nh)) <= _ops.RESAMPLE_MAX_TAPS:
                _ops.resample_crop_normalize_u8(Bu, prm["new_size"], prm["crop_pos"], prm["crop_size"], out=real_all)
            else:      # over the kernel's limit (a very strong downscale): the CPU path, on the frames as decoded
                import numpy as np
                from PIL import Image
                ev.synchronize()
                (cx, cy), (cw, ch) = prm["crop_pos"], prm["crop_size"]
                B = np.stack([np.asarray(Image.fromarray(f).resize((nw, nh), Image.BICUBIC).crop((cx, cy, cx + cw, cy + ch)))
                              for f in (clip["raw"] if "raw" in clip else
                                        [jpeg_decode.pillow_rgb(b) for b in clip["jpeg"][1]])])
                real_all[..., :3] = (torch.from_numpy(B).to(self.dev).float() / 255.0 - 0.5) / 0.5
        else:
            real_all[..., :3] = (Bu.float() / 255.0 - 0.5) / 0.5
        return clip, A, real_all

    def consumed(self):
        """the held clips' last chunk has been launched: the upload slot of each may be overwritten once the compute stream
        gets here"""
        ev = torch.cuda.Event()
        ev.record()
        for slot, _ in self._held:
            self._slot_done[slot] = ev

    def close(self):
        self._it.close()


def run_train(opt, steps=None, watch=None):
    """train.py main: one process per GPU under torchrun (the reference used nn.DataParallel threads).

    Epoch structure of upstream train.py [RECALL]: `niter` epochs at the initial learning rate + `niter_decay` epochs
    of linear decay to zero; an epoch is one clip per training sequence, `batch` = ranks x K clips per iteration
    (K = batchSize // ranks clips per rank where --batchSize is above the number of ranks, else 1: clips_per_rank);
    `latest` checkpoints every `save_latest_freq` samples and at every `save_epoch_freq`-th epoch end (also
    under the epoch number), with `iter.txt` = (epoch, samples done in it) beside them; `--continue_train` reloads
    the `which_epoch` nets, reads iter.txt and resumes there (fresh Adam moments: upstream saves none).
    `steps` caps the total number of iterations (tests, benches); `watch`: a dict that receives the run's "trainer" and,
    under --display_web on rank 0, its "display" (tests).

    --display_web: rank 0 shows the last frame of the step that completes every `display_freq` samples (the rule of
    `save_latest_freq`) through TrainDisplay -- rendered on the GPU behind the step, written by a thread -- and appends
    every printed iteration line to loss_log.txt.

    K > 1: the batch is `batch` global clip slots, slot s = rank * K + j the rank's j-th clip (clip_slots): which clip and
    which synthetic-data generator a slot reads depends on s and the iteration alone, so --gpu_ids 0,1 --batchSize 2 and
    --gpu_ids 0 --batchSize 2 train on the same batch (promised for --synthetic_data; a real dataset keeps one
    TrainPoseDataset per rank, whose random draws depend on the rank).  The rank's K clips walk their chunks in lock-step:
    per chunk K micro-steps train_step(micro=(j, K)), the last of which exchanges the mean gradient and steps the
    optimisers.  Each clip carries its own FIFO; a printed loss is the mean over the rank's K clips."""
    import os
    import time
    import numpy as np
    from . import distributed as Dm
    if "WORLD_SIZE" in os.environ:
        rank, local_rank, world = Dm.init_from_env()
    else:       # a plain single-device run computes on --gpu_ids[0], as the reference's single-GPU recipes do
        rank, local_rank, world = 0, (opt.gpu_ids[0] if getattr(opt, "gpu_ids", None) else 0), 1
    dev = "cuda:%d" % local_rank
    torch.cuda.set_device(local_rank)
    K, batch_warning = clips_per_rank(getattr(opt, "batchSize", world), world)
    batch = world * K
    trainer = Vid2VidTrainer(opt, dev)
    display = None
    if rank == 0 and getattr(opt, "display_web", False):
        from .train_display import TrainDisplay
        display = TrainDisplay(opt)
        trainer.keep_visuals = True
    if watch is not None:
        watch["trainer"], watch["display"] = trainer, display
    Dm.rendezvous("trainer built")      # (before the first gradient exchange: a rank that died building its replica is named)
    if rank == 0 and batch_warning:
        print(batch_warning, flush=True)
    F_ = opt.max_frames_per_gpu
    synthetic = getattr(opt, "synthetic_data", False)
    ds = None
    if not synthetic:
        from .pose_dataset import TrainPoseDataset
        ds = TrainPoseDataset(opt, seed=1000 + rank)
    per_epoch = 1 if synthetic else max(1, len(ds) // batch)          # iterations per epoch (`batch` clips each)
    iter_path = os.path.join(opt.checkpoints_dir, opt.name, "iter.txt")
    start_epoch, epoch_iter = 1, 0
    if opt.continue_train:
        trainer.load(opt.which_epoch)
        try:
            start_epoch, epoch_iter = [int(v) for v in np.loadtxt(iter_path, delimiter=",", dtype=int)]
        except (OSError, ValueError):
            start_epoch, epoch_iter = 1, 0
        if rank == 0:
            print("Resuming from epoch %d at iteration %d" % (start_epoch, epoch_iter), flush=True)
        if start_epoch > opt.niter:
            trainer.update_learning_rate(start_epoch - 1)
        if ds is not None and start_epoch > opt.niter_step:
            ds.update_training_batch((start_epoch - 1) // max(1, opt.niter_step))

    def checkpoint(label, epoch, done):
        if rank == 0:
            trainer.save(label, (epoch, done))

    # synthetic data: every clip slot has its own sequence
    rngs = [np.random.default_rng(100 + s) for s, _ in clip_slots(0, rank, world, K)]
    tG = opt.n_frames_G
    feeder = None
    if ds is not None and getattr(opt, "train_loader", "sync") == "prefetch":
        def schedule():
            """(clip index, n_frames_total) of every iteration from the resume point on: clips are drawn ahead of the
            epoch ends at which update_training_batch doubles the clip length, so each carries the length of its epoch"""
            cap = getattr(opt, "max_frames_total", 10 ** 9)
            first_k = epoch_iter // batch
            for e in range(start_epoch, opt.niter + opt.niter_decay + 1):
                ratio = (e - 1) // max(1, opt.niter_step)
                nft = min(cap, opt.n_frames_total * 2 ** ratio) if ratio > 0 else opt.n_frames_total
                for kk in range(first_k, per_epoch):
                    for _, index in clip_slots((e - 1) * per_epoch + kk, rank, world, K):      # (in slot order)
                        yield (index, nft)
                first_k = 0
        feeder = _ClipFeeder(ds, opt, dev, schedule(), K)
    elif ds is not None and getattr(opt, "gpu_resize", False) and rank == 0:
        print("warning: --gpu_resize has no effect without --train_loader prefetch", flush=True)
    last_pos = (start_epoch, epoch_iter)
    stats, it, total_samples = [], 0, (start_epoch - 1) * per_epoch * batch + epoch_iter
    last_epoch = opt.niter + opt.niter_decay
    for epoch in range(start_epoch, last_epoch + 1):
        trainer.set_epoch(epoch)      # (--niter_fix_global with two spatial scales; a resumed run enters its epoch's phase here)
        for k in range(epoch_iter // batch, per_epoch):
            if steps is not None and it >= steps:
                break
            ts = time.perf_counter()
            visuals = trainer.visuals
            per_clip = []       # the reported losses of the iteration's last chunk, per clip of this rank
            if synthetic:
                H = W = opt.fineSize
                for j, rng in enumerate(rngs):
                    pose_np = np.where(rng.random((F_, H, W, 1)) < 0.02, rng.uniform(-1, 1, (F_, H, W, 9)), -1.0).astype(np.float32)
                    pose = torch.zeros(F_, H, W, 12, device=dev)
                    pose[..., :9] = torch.from_numpy(pose_np).to(dev)
                    real = torch.zeros(F_, H, W, 4, device=dev)
                    real[..., :3] = torch.tanh(torch.from_numpy(rng.standard_normal((F_, H, W, 3)).astype(np.float32))).to(dev)
                    side = max(8, opt.fineSize // 32 * 8)
                    boxes = [(H // 8, H // 8 + side, (W - side) // 2, (W - side) // 2 + side)] * F_ if opt.add_face_disc else None
                    real_prev = None
                    if not trainer.spec.no_flow:    # the real frame before each frame (flow / warp losses)
                        real_prev = torch.cat([torch.tanh(torch.from_numpy(rng.standard_normal((1, H, W, 4)).astype(np.float32))).to(dev),
                                               real[:-1]], 0)
                        real_prev[..., 3] = 0
                    losses, _ = trainer.train_step(pose, real, boxes, real_prev=real_prev, micro=(j, K))
                    per_clip.append(losses)
                    if j == 0:
                        visuals = trainer.visuals
                what = ""
            else:
                # K clips per rank per iteration (one where --batchSize does not exceed the ranks), walked together in chunks
                # of max_frames_per_gpu frames with each clip's generated frames carried over (detached) from chunk to
                # chunk, one optimiser step per chunk -- upstream's truncated recurrence
                clips = []      # (clip, A [T,H,W,3] uint8, B uint8 or None, real_all or None)
                for _, index in clip_slots((epoch - 1) * per_epoch + k, rank, world, K):
                    if feeder is not None:
                        # the same clip, prepared ahead; real_all [T,H,W,4]: its frames normalised once, pad channel zero
                        clip, A, real_all = feeder.take()
                        clips.append((clip, A, None, real_all))
                    else:
                        clip = ds.sample(index)
                        clips.append((clip, torch.from_numpy(clip["A"]).to(dev),                      # [T,H,W,3] uint8
                                      torch.from_numpy(clip["B"]).to(dev), None))
                # every clip of the batch runs the same number of chunks (one gradient all-reduce per chunk)
                T_ = min(A.shape[0] for _, A, _, _ in clips)
                if world > 1:
                    import torch.distributed as dist
                    tmin = torch.tensor([T_], device=dev)
                    dist.all_reduce(tmin, op=dist.ReduceOp.MIN)
                    T_ = int(tmin.item())
                prevs = [None] * K
                for c0 in range(tG - 1, T_, F_):
                    fr = list(range(c0, min(c0 + F_, T_)))
                    per_clip = []
                    for j, (clip, A, B, real_all) in enumerate(clips):
                        H, W = A.shape[1], A.shape[2]
                        pose = torch.zeros(len(fr), H, W, 12, device=dev)
                        for jj, t in enumerate(fr):
                            for f in range(tG):                                    # window: oldest frame first
                                ops.pose_u8_to_f32(A[t - tG + 1 + f], pose[jj], 3 * f)
                        real_prev = None
                        if real_all is not None:      # slices of the clip's frames: no arithmetic per chunk
                            real = real_all[fr[0]:fr[-1] + 1]
                            if not trainer.spec.no_flow:
                                real_prev = real_all[fr[0] - 1:fr[-1]]
                        else:
                            real = torch.zeros(len(fr), H, W, 4, device=dev)
                            real[..., :3] = (B[fr].float() / 255.0 - 0.5) / 0.5
                            if not trainer.spec.no_flow:
                                real_prev = torch.zeros(len(fr), H, W, 4, device=dev)
                                real_prev[..., :3] = (B[[t - 1 for t in fr]].float() / 255.0 - 0.5) / 0.5
                        boxes = None
                        if opt.add_face_disc:      # one region for the chunk (upstream boxes the whole batch of frames)
                            box = get_face_region(clip["A"][fr], opt.fineSize)
                            if world > 1:
                                # the face terms decide which parameters (D_f) have gradients: every rank must take the same
                                # branch, or the ranks' gradient buckets would differ in size and order -- the face
                                # discriminator trains on a chunk only when the chunk of EVERY rank's clip j shows a face
                                import torch.distributed as dist
                                has = torch.tensor([1 if box is not None else 0], device=dev if dist.get_backend() == "nccl" else "cpu")
                                dist.all_reduce(has, op=dist.ReduceOp.MIN)
                                if int(has.item()) == 0:
                                    box = None
                            boxes = [box] * len(fr) if box is not None else None
                        losses, prevs[j] = trainer.train_step(pose, real, boxes, prevs[j], real_prev=real_prev, micro=(j, K))
                        per_clip.append(losses)
                        if j == 0:
                            visuals = trainer.visuals
                if feeder is not None:
                    feeder.consumed()
                    if steps is None or it + 1 < steps:
                        feeder.stage()      # the next clips' uploads run beside these clips' chunks
                clip, A = clips[0][0], clips[0][1]
                what = ", seq %s, %d frames %dx%d step %d" % (clip["seq"], T_ - tG + 1, A.shape[1], A.shape[2], clip["t_step"])
            if K > 1 and per_clip:       # the mean over the rank's clips, summed in float64; a term a clip does not have (no
                names = list(dict.fromkeys(name for lc in per_clip for name in lc))      # face region) counts as 0 there
                losses = {name: float(np.sum(np.array([lc.get(name, 0.0) for lc in per_clip], dtype=np.float64)) / K) for name in names}
            if display is not None and (total_samples + batch) % max(1, opt.display_freq) < batch:
                display.show(visuals, epoch, total_samples + batch)      # (clip 0's; enqueued behind the step; no host wait)
            torch.cuda.synchronize()
            stats.append(time.perf_counter() - ts)
            it += 1
            total_samples += batch
            if rank == 0 and ((it - 1) % max(1, opt.print_freq // 100) == 0 or it == steps):
                line = "(iter %d, epoch %d%s, %.0f ms, all-reduce %.1f MB%s) %s" \
                    % (it - 1, epoch, what, 1e3 * stats[-1], trainer.comm_bytes / 2**20,
                       ", %.1f ms exposed" % trainer.comm_ms if trainer.time_comm else "",
                       " ".join("%s: %.3f" % kv for kv in losses.items()))
                print(line, flush=True)
                if display is not None:
                    display.log(line)
            last_pos = (epoch, (k + 1) * batch)
            if total_samples % max(1, opt.save_latest_freq) < batch:
                checkpoint("latest", epoch, (k + 1) * batch)
        else:
            epoch_iter = 0
            last_pos = (epoch + 1, 0)
            if epoch % max(1, opt.save_epoch_freq) == 0:
                checkpoint("latest", epoch + 1, 0)
                checkpoint(str(epoch), epoch + 1, 0)
            if epoch > opt.niter:
                trainer.update_learning_rate(epoch)
            if ds is not None and epoch % max(1, opt.niter_step) == 0:
                ds.update_training_batch(epoch // max(1, opt.niter_step))
            continue
        break   # the step cap was reached
    if feeder is not None:
        feeder.close()
    if world > 1:
        # the replicas started from the same seed and applied the same averaged gradients: their weights must still be
        # equal -- a cheap end-of-run check that the exchange reached every parameter on every rank
        import torch.distributed as dist
        chk = torch.stack([p.detach().double().sum() for p in trainer.optG.params + trainer.optD.params]).sum().reshape(1)
        allc = [torch.zeros_like(chk) for _ in range(world)]
        dist.all_gather(allc, chk)
        if any(float(c) != float(allc[0]) for c in allc):
            raise RuntimeError("data-parallel replicas diverged: parameter checksums %s" % [float(c) for c in allc])
        if rank == 0:
            print("replicas in sync after %d steps (parameter checksum %.9g on all %d ranks)" % (it, float(allc[0]), world),
                  flush=True)
    if display is not None:
        display.close()      # (every picture, the page and the log are on disk before the final checkpoint)
    if rank == 0:      # the final (or step-capped) save carries its position too
        trainer.save("latest", last_pos)
    if world > 1:
        Dm.leave_group()
    return {"ms_per_step": 1e3 * float(np.median(stats)) if stats else 0.0, "steps": it, "world": world}
