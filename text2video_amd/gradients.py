"""Gradient delivery of the train step (train.py): the state the step keeps per parameter (`ParamState`) and per step
(`STEP`), the one way a gradient kernel reaches a bucket slot (`deliver_into`), the weight gradients a layer collects over
its uses in one graph, and the flat buckets the slots live in with their data-parallel exchange (`GradBuckets`)."""
import collections
import contextlib
import os
import struct
import types

import torch

from . import ops


def switch(name):
    """a default-on T2V_* switch ("0": off), read where it is used: the tests change them between two steps"""
    return os.environ.get(name, "1") != "0"


def _desc_key(d, xcs):
    return (d.H, d.W, d.Cin, d.Cout, d.kH, d.stride, d.pad, d.pad_mode, d.transposed, d.output_padding, d.algo, xcs)


class PackCache:
    """packed copies of a parameter while its version is `version`: key -> copy, key -> how it was made, the keys used since
    the last write; event: made ahead on the side stream (prefetch_packs), complete after it; made: key -> (stream, event)
    of a copy made on the spot"""
    __slots__ = ("version", "copies", "makers", "used", "event", "made")

    def __init__(self, version, copies=None, makers=None):
        self.version, self.copies, self.makers = version, copies or {}, makers or {}
        self.used, self.event, self.made = set(), None, {}


class WinogradCollection:
    """Workspace of one layer's Winograd-domain weight gradient over every image of the step: slot k holds V and A dy A^T of
    one image, one reduction runs over all `total` slots.  kept: the forward convs wrote V (_keep_v_slot) and the slots are
    handed out from the top; else the backward nodes fill the slots 0, 1, ... as they arrive."""
    __slots__ = ("ws", "desc", "xcs", "ycs", "key", "total", "filled", "kept")

    def __init__(self, desc, xcs, ycs, total, device, kept):
        self.ws = ops.backward_weight_winograd_workspace(desc, xcs, total, device)
        self.desc, self.xcs, self.ycs, self.key = desc, xcs, ycs, _desc_key(desc, xcs)
        self.total, self.filled, self.kept = total, [False] * total, kept


# (x, dY) of the backward nodes of a direct-kernel layer that have arrived so far (_paired_direct_wgrad)
DirectStash = collections.namedtuple("DirectStash", "desc parts")


class ParamState:
    """What the train step keeps on one parameter (param_state):
    packs / repack: PackCache / {key: maker} of the copies the last step used (invalidate_packs -> prefetch_packs);
    gslot: GradSlot;  running: [running_mean, running_var, num_batches_tracked] of a BatchNorm2d weight;
    wino: WinogradCollection of the step under way;  images: Winograd-domain images forward has counted and no reduction
    has taken yet;  seen: all of them, this step;  expect: what the previous step saw (the size of a kept workspace);
    dw_stash: DirectStash;  dw_uses: uses of the direct weight-gradient kernel forward has counted."""
    __slots__ = ("packs", "repack", "gslot", "running", "wino", "images", "seen", "expect", "dw_stash", "dw_uses")

    def __init__(self):
        self.packs = self.repack = self.gslot = self.running = None
        self.expect = 0
        self.clear_step()

    def clear_step(self):
        """Nothing counted, nothing parked: the entry of a step scope, and its exit by an exception -- operand lists and
        workspaces are GPU memory a retry needs.  `expect` is left alone: a step that failed says nothing about the next."""
        self.wino = self.dw_stash = None
        self.images = self.seen = self.dw_uses = 0
        return self

    def end_step(self):
        """the normal exit of a step scope: what the layer saw in this step is what the next one prepares for"""
        self.expect = self.seen
        self.clear_step()


def owner(p):
    """`p`, or the parameter a detached view of it names as its `_t2v_owner` (frozen passes hand views to the layers)"""
    return getattr(p, "_t2v_owner", p)


def param_state(p, create=True):
    p = owner(p)
    st = getattr(p, "_t2v_state", None)
    if st is None and create:
        st = p._t2v_state = ParamState()
    return st


# The step under way (batched_weight_gradients sets and restores the first three).  wg_batch: layers that run once per frame
# collect their Winograd-domain weight gradients;  dw_pair: a direct-kernel layer used several times reduces all uses in one
# launch;  gemm: the side stream carries GEMMs in this step (side_gemm_hint);  inline: weight gradients stay on the current
# stream (the discriminators' pass on a stream of its own);  stream / pending: the side stream / kernels on it nobody joined
STEP = types.SimpleNamespace(wg_batch=False, dw_pair=False, gemm=False, inline=False, stream=None, pending=False)


# ------------------------------------------------------------------------------------------------
# packed weight copies
# ------------------------------------------------------------------------------------------------
def cached_pack(w, key, make):
    """Packed (or Winograd-transformed) layout of parameter `w`, kept until the optimiser next writes it: a step
    runs every generator layer once per frame and every discriminator layer on real and fake inputs, all with the
    same weights.  The cache lives on the parameter object itself (freed with it; autograd hands the same object to
    backward; a detached view of a parameter -- frozen passes -- shares its parameter's).  T2V_TRAIN_PACK_CACHE=0 re-packs
    per call (saves the memory of the transformed copies)."""
    if not switch("T2V_TRAIN_PACK_CACHE"):
        return make()
    w = owner(w)
    st = param_state(w)
    c = st.packs
    if c is None or c.version != w._version:
        c = st.packs = PackCache(w._version)
    elif c.event is not None:
        # packed ahead on the side stream (prefetch_packs): a use waits for that batch (on whichever stream it runs; a wait
        # for an event that has completed costs nothing)
        torch.cuda.current_stream().wait_event(c.event)
    if key not in c.copies:
        c.copies[key] = make()
        c.makers[key] = make
        if w.is_cuda:      # made on the spot (a first step, T2V_PACK_PREFETCH=0): by whom, and when it is complete
            cur = torch.cuda.current_stream()
            c.made[key] = (cur, cur.record_event())
    elif w.is_cuda:
        # the discriminators' layers are used from two streams in one step (their own backward pass on the trainer's
        # `_d_stream`, the generator's pass through them on the current one): a copy made on the other stream is waited for
        m = c.made.get(key)
        if m is not None and m[0] != torch.cuda.current_stream():
            torch.cuda.current_stream().wait_event(m[1])
    c.used.add(key)
    return c.copies[key]


def invalidate_packs(p):
    """the optimiser has written `p` (through its raw pointer: no version bump): drop the packed copies, remember how
    they were made"""
    st = param_state(p)
    c = st.packs
    # (only the copies the last step actually used: a geometry or mode that is gone is not made again for ever)
    st.repack = {k: c.makers[k] for k in c.used} if (c is not None and c.used) else None
    st.packs = None


def prefetch_packs(params):
    """After the optimiser step: every packed / Winograd-transformed / transposed copy the last step used is made again
    from the new weights NOW, on the side stream -- ~150 small memory-bound kernels per step (36 filter transforms of
    151 MB each among them) that depend on nothing but the weights and would otherwise sit in front of each layer's
    first use on the critical path; here they run under the next step's first convs.  T2V_PACK_PREFETCH=0: lazily."""
    todo = [(p, st) for p, st in ((p, param_state(p, create=False)) for p in params) if st is not None and st.repack]
    if not todo or not switch("T2V_PACK_PREFETCH") or not todo[0][0].is_cuda:
        for _, st in todo:
            st.repack = None
        return
    with wgrad_fork(gemm=False):
        for p, st in todo:
            st.packs = PackCache(p._version, {k: mk() for k, mk in st.repack.items()}, dict(st.repack))
            st.repack = None
        ev = torch.cuda.current_stream().record_event()
    for _, st in todo:
        st.packs.event = ev


# ------------------------------------------------------------------------------------------------
# gradient slots: every trainable parameter owns a slice ("slot") of a persistent flat exchange bucket
# (GradBuckets below).  Inside a train step the backward nodes DELIVER their weight / bias / affine gradients
# straight into the slot -- the first node of a step writes, later nodes of the same parameter add (kernels with
# an accumulate flag) -- and return None to autograd: no AccumulateGrad adds, no torch.cat / copy-back around the
# collective, and a bucket's all-reduce starts the moment its last gradient has landed.
# ------------------------------------------------------------------------------------------------
class GradSlot:
    __slots__ = ("owner", "bucket", "idx", "view", "expect", "got", "_filled", "zero_valid")

    def __init__(self, owner, bucket, idx, view):
        self.owner, self.bucket, self.idx, self.view = owner, bucket, idx, view
        self.expect = self.got = 0
        self._filled = False      # the slot holds this step's (partial) gradient
        # the slot's memory holds exact zeros put there by deliver(zero=True) and nothing has written it since: the ~100
        # biases in front of norm layers get that delivery every step -- one 4 KB memset each, once, instead of per step
        # (an exchange averages zeros with the other ranks' zeros: the same layers are zero-delivered on every rank)
        self.zero_valid = False

    @property
    def filled(self):
        return self._filled

    @filled.setter
    def filled(self, v):
        self._filled = bool(v)
        if v:                     # every writer of the slot's memory marks it filled: the zeros are gone
            self.zero_valid = False


def grad_slot(p):
    """the slot of parameter `p` if its buckets are collecting (inside a train step), else None"""
    st = param_state(p, create=False)
    sl = st.gslot if st is not None else None
    return sl if (sl is not None and sl.owner.collecting) else None


def expect_gradient(p):
    """forward side: one more backward node will deliver a gradient for `p` in this step"""
    sl = grad_slot(p) if p is not None and p.requires_grad else None
    if sl is not None:
        sl.expect += 1


def deliver(sl, tensor=None, zero=False):
    """backward side: add `tensor` (or nothing / an exact zero) to slot `sl` and count the node as done"""
    if tensor is not None:
        _acc(sl.view, tensor, not sl.filled)
        sl.filled = True
    elif zero and not sl.filled:
        if not sl.zero_valid:
            _zero(sl.view)
        sl._filled, sl.zero_valid = True, True
    sl.owner.node_done(sl)


def deliver_into(slot, keep, launch, count=True):
    """One gradient kernel `launch(out, accumulate)`.  Without a slot its result is returned.  With one it writes (adds to)
    the slot -- on the side stream where that is on and `keep` names the operands to keep alive for it --, the slot is filled,
    the node counted (count=False: the flush, no node) and None goes back to autograd.  The node is counted OUTSIDE the
    side-stream scope: that may launch a bucket's collective, which must see the MAIN stream as current."""
    if slot is None:
        return launch(None, False)
    with (wgrad_fork(*keep) if (keep and wgrad_stream_on(keep[0])) else contextlib.nullcontext()):
        launch(slot.view, slot.filled)
    slot.filled = True
    if count:
        slot.owner.node_done(slot)
    return None


def deliver_direct(slot, keep, packed, fdesc, xcs, count=True):
    """deliver_into for the direct kernels: `packed()` -> dW in their layout, unpacked into the slot or a tensor of its own"""
    def launch(out, accumulate):
        dwp = packed()
        if out is None:
            return ops.unpack_conv_weight(dwp, fdesc, xcs)
        ops.unpack_conv_weight_into(dwp, fdesc, xcs, out, accumulate)
    return deliver_into(slot, keep, launch, count)


# ---- weight gradients on a second stream ---------------------------------------------------------------------------
# Nothing in the backward pass waits for a weight gradient: the chain that has to run in order is dy -> norm backward ->
# data gradient -> the next layer's dy.  With gradients delivered straight into bucket slots (GradBuckets) the weight-
# gradient kernels of a node can therefore run on a side stream, next to the data-gradient kernels of the following
# layers: the tails of one launch (4.5-round grids, split-K partial combines, transforms of 36 small matrices) are
# filled by the other stream's blocks, as in the two-stream inference frames.  The side stream waits for the node's dc;
# the main stream waits for the side stream before anything reads a slot (bucket collectives, absorb, finish).
# T2V_WGRAD_STREAM=0: everything on one stream.
# From the step's first weight gradient on the side stream to the end of the step BOTH streams carry fixed-grid GEMMs (data
# gradient | Winograd-domain weight gradient).  A two-per-CU grid keeps every CU full until its last block leaves: the other
# stream's launch -- and the bandwidth-bound kernels between two of the main stream's GEMMs -- queue behind it, the step was
# the sum of its kernels (585 us per ResnetBlock layer of the second frame's backward pass against 591 us of kernels).  With
# the overlap hint 2 (ops.set_overlap_hint) those kernels launch ONE block per CU and are resident side by side: 513 us per
# layer, the same bits (profiles/r06_train_two_queues_{two,one}_per_cu.txt).  The hint is per thread and the backward nodes run on the
# autograd engine's thread: every node (and the flush on the calling thread) sets it from the shared flag.
# T2V_TRAIN_SK_HINT=0: two blocks per CU throughout.
def wgrad_stream_on(t):
    return t.is_cuda and not STEP.inline and switch("T2V_WGRAD_STREAM")


def side_gemm_hint():
    """this thread's launches from here on: one block per CU for the fixed-grid GEMMs while the side stream has GEMMs of its
    own in this step, the library's default otherwise"""
    ops.set_overlap_hint(2 if STEP.gemm else 0)


@contextlib.contextmanager
def wgrad_fork(*tensors, gemm=True):
    """kernels launched in this scope run on the side stream, after everything the current stream holds so far; the
    tensors named (inputs allocated on the current stream) stay allocated until the side stream is done with them.
    gemm: the scope launches weight-gradient GEMMs (not the repacking of weights after the optimiser step)"""
    if STEP.stream is None:
        STEP.stream = torch.cuda.Stream()
    side = STEP.stream
    side.wait_stream(torch.cuda.current_stream())
    for t in tensors:
        if t is not None:
            t.record_stream(side)
    STEP.pending = True
    if gemm and not STEP.gemm and switch("T2V_TRAIN_SK_HINT"):
        STEP.gemm = True
        side_gemm_hint()
    with torch.cuda.stream(side):
        yield


def wgrad_join():
    """the current stream waits for the weight gradients in flight on the side stream"""
    if STEP.pending:
        torch.cuda.current_stream().wait_stream(STEP.stream)
        STEP.pending = False


# ---- a layer that runs several times in one step reduces its weight gradient once -----------------------------------
@contextlib.contextmanager
def batched_weight_gradients(params):
    """Scope of one train step (forward and backward inside): layers that run once per frame reduce their weight
    gradients over all frames at once.  The per-weight counters are cleared on entry, so a graph that was built but never
    back-propagated cannot leave a stale count behind.  T2V_WGRAD_BATCH=0 / T2V_WGRAD_PAIR=0: off."""
    states = [param_state(p).clear_step() for p in params]
    cuda = bool(params) and params[0].is_cuda
    STEP.wg_batch, STEP.dw_pair, STEP.gemm = switch("T2V_WGRAD_BATCH"), switch("T2V_WGRAD_PAIR"), False
    if cuda:
        side_gemm_hint()
    try:
        yield
    except BaseException:       # (OOM, an asynchronous error)
        for st in states:
            st.clear_step()
        raise
    finally:
        STEP.wg_batch = STEP.dw_pair = STEP.gemm = False
    if cuda:
        side_gemm_hint()
    # a backward pass inside this scope that did not end with flush_pending_weight_gradients() would silently lose the
    # gradients still parked on the weights (the first half of a pair, transformed slots waiting for their reduction)
    left = [i for i, st in enumerate(states) if st.dw_stash is not None or (st.wino is not None and any(st.wino.filled))]
    for st in states:
        st.end_step()
    if left:
        raise RuntimeError("batched_weight_gradients: %d parameter(s) (first: #%d) left the scope with an unreduced weight "
                           "gradient -- call flush_pending_weight_gradients(params, grads) after the backward pass" % (len(left), left[0]))


_WGRAD_MAX_BYTES = 0x7fff0000        # the weight-gradient kernel addresses its operands with 32-bit byte offsets (capi.hip)


def direct_weight_gradient(x, dc, fdesc):
    """packed dW of a batch [B,...] in as few launches as the kernel's 2 GiB operand limit allows: ONE for every shape of the
    512 / 1024 configs; a batch whose x or dY (or padded x) would pass the limit -- many frames per GPU at 2048x1024 -- is
    reduced in chunks of images, accumulating (three passes in one batch are 3x the single pass)."""
    B = x.shape[0]
    padded = (x.shape[1] + 8) * (x.shape[2] + 8) * x.shape[3] if x.dim() == 4 else x[0].numel()     # (the kernel pads x by <= 3 px)
    per = 4 * max(padded, dc[0].numel(), 1)
    step = max(1, min(B, (_WGRAD_MAX_BYTES - 1) // per))
    dwp = None
    for i in range(0, B, step):
        dwp = ops.conv2d_backward_weight(x[i:i + step], dc[i:i + step], fdesc, accumulate_into=dwp)
    return dwp


def _paired_direct_wgrad(w, x, dc, fdesc, slot):
    """Direct (non-Winograd) weight gradient of a layer that ran several times in this step's graph (counted in forward:
    `ParamState.dw_uses`): the backward nodes leave their (x, dY) on the weight, the LAST one to arrive launches ONE reduction
    over all of them -- the kernel pays a fixed ~8 stage times per block, so one long reduction beats several short ones:
      * two uses of one image each (the generator's stride-2 / transposed layers on the clip's two frames):
        ops.conv2d_backward_weight_pair -- two base pointers, no copy; blocks 36 -> 73 stages, 0.64 -> 0.73 of peak;
      * anything else (the discriminators' layers: real, fake and raw pass of two frames each -- round 5): the operands are
        concatenated (a few MB per layer) and reduced as one batch: 3 launches of ~180 us at 0.39 of peak -> one.
    Returns (taken, dW or None): not taken -> the caller reduces this node alone."""
    st = param_state(w)
    if not STEP.dw_pair or st.dw_uses < 2:
        return False, None
    if st.dw_stash is None:
        st.dw_stash = DirectStash(fdesc, [])
    parts = st.dw_stash.parts
    parts.append((x, dc))
    if len(parts) < st.dw_uses:
        if slot is not None:
            deliver(slot)
        return True, None
    st.dw_stash, st.dw_uses = None, 0
    return True, _reduce_stashed(parts, fdesc, slot)


def _reduce_stashed(parts, fdesc, slot, from_node=True):
    """one weight-gradient launch over the stashed (x, dY) of a layer; into the bucket slot (-> None) or returned.
    from_node: called by the backward node that brought the last operands (side stream, the node counts as delivered);
    False: the flush after the backward pass (current stream; every node has been counted already)"""
    xcs = parts[0][0].shape[-1]

    def packed():
        if len(parts) == 2 and all(pr[0].shape[0] == 1 for pr in parts) and \
                ops.backward_weight_strided_supported(fdesc, xcs, parts[0][1].shape[-1]):
            (x0, dc0), (x1, dc1) = parts
            return ops.conv2d_backward_weight_pair(x0[0], dc0[0], x1[0], dc1[0], fdesc)
        if len(parts) == 1:
            return direct_weight_gradient(parts[0][0], parts[0][1], fdesc)
        return direct_weight_gradient(torch.cat([pr[0] for pr in parts]), torch.cat([pr[1] for pr in parts]), fdesc)
    return deliver_direct(slot, [t for pr in parts for t in pr] if from_node else (), packed, fdesc, xcs, count=from_node)


def _keep_v_slot(w, x, ddesc, xcs, ycs):
    """Forward side of a batched Winograd-domain weight gradient (use number `ParamState.images` of this step, not counted
    yet): from a layer's second step on, the workspace of its weight gradient exists BEFORE the forward pass -- sized for
    the images the previous step counted (`ParamState.expect`) -- and the forward conv writes its input transform V straight
    into a slot of it: backward transforms dy only (72 input transforms of 13.5 us fewer per step of the 512x512 config).
    The slots are handed out from the top, so that the backward nodes -- which arrive in reverse -- fill them in the order
    the un-kept path would: the same reduction order, the same bits.  Returns (workspace, slots, slot) or None: not kept
    (first step, a batch, more uses than expected, T2V_WGRAD_KEEP_V=0)."""
    st = param_state(w)
    expect, idx = st.expect, st.images
    if x.shape[0] != 1 or expect < 1 or idx >= expect or xcs != ddesc.Cin or not switch("T2V_WGRAD_KEEP_V"):
        return None
    col = st.wino
    if col is None:
        if idx != 0:
            return None       # an earlier use of this step went without: stay on that path
        col = st.wino = WinogradCollection(ddesc, xcs, ycs, expect, x.device, kept=True)
    if not col.kept or col.key != _desc_key(ddesc, xcs):
        return None
    return col.ws, expect, expect - 1 - idx


def _zero_unfilled_slots(col):
    """slots of a workspace whose A dy A^T never came (and whose V may never have been written): zero both -- a zero image
    contributes nothing, whatever bit pattern the allocation held would (0 x NaN is not 0)"""
    total = col.total
    if all(col.filled):
        return
    tp = ops.winograd_tile_rows(col.desc)      # slot pitch of the batch-wide tile lists
    nv = 36 * total * tp * col.xcs
    v = col.ws[:nv].view(36, total, tp * col.xcs)
    md = col.ws[nv:nv + 36 * total * tp * col.desc.Cout].view(36, total, tp * col.desc.Cout)
    for k, f in enumerate(col.filled):
        if not f:
            v[:, k].zero_()
            md[:, k].zero_()


def _reduce_collection(col, slot, from_node):
    """the one reduction over every slot of `col`, the slots nobody filled zeroed first; from_node: as in _reduce_stashed"""
    _zero_unfilled_slots(col)
    return deliver_into(slot, (col.ws,) if from_node else (),
                        lambda out, accumulate: ops.conv2d_backward_weight_winograd_reduce(
                            col.desc, col.ws, col.total, col.xcs, col.ycs, out=out, accumulate=accumulate), count=from_node)


def winograd_weight_gradient(x, dc, fdesc, slot):
    """Winograd-domain weight gradient of the images of one node, reduced on the spot"""
    return deliver_into(slot, (x, dc), lambda out, accumulate: ops.conv2d_backward_weight_winograd(
        x, dc, fdesc, accumulate_into=out if accumulate else None, out=out))


def _kept_winograd_wgrad(w, dc, fdesc, kept, slot=None, lazy_dc=None):
    """backward side of _keep_v_slot: A dy A^T of this node's image into ITS slot; the node that completes the set -- every
    use the forward pass counted has come back -- zeroes the slots nobody filled (a step with fewer uses than expected)
    and runs the one reduction.  lazy_dc (a LazyDc of train.py: conv output, gradient behind the norm, mean_rstd, gamma,
    beta, relu, sums) instead of dc: the gradient in front of the norm is formed inside the transform.
    Returns (dW or None, where this node's A dy A^T sits: (workspace, slots, slot))."""
    ws, total, k = kept
    st = param_state(w)
    col = st.wino
    assert col is not None and col.ws is ws and not col.filled[k]
    if lazy_dc is not None:
        ops.conv2d_backward_weight_winograd_dy_norm(*lazy_dc, fdesc, ws, total, k, col.xcs)
    else:
        ops.conv2d_backward_weight_winograd_dy(dc, fdesc, ws, total, k, col.xcs)
    col.filled[k] = True
    dw = None
    if sum(col.filled) == min(st.images, total):
        st.wino, st.images = None, 0
        dw = _reduce_collection(col, slot, True)
    elif slot is not None:
        deliver(slot)
    return dw, kept


def _batched_winograd_wgrad(w, x, dc, fdesc, slot=None):
    """Weight gradient of one use of a layer whose forward counted `ParamState.images` images in this graph: the
    images are transformed into their slots of a workspace kept on the weight; the node that brings the last ones
    runs the single reduction over all of them and returns dW, the earlier ones return None (a zero gradient --
    autograd sums the nodes' results).  One K = images x tiles reduction instead of one short one per frame.
    Returns (dW or None, where this node's A dy A^T sits: (workspace, slots, first slot) -- the data gradient reads it too
    (transposed algorithm) -- or None: reduced on the spot)."""
    st = param_state(w)
    col, nb = st.wino, x.shape[0]
    # (a kept workspace belongs to the uses that kept their V (_keep_v_slot); this one did not)
    total = 0 if (col is not None and col.kept) else st.images
    if total < nb:     # no count on this object: reduce on the spot
        return winograd_weight_gradient(x, dc, fdesc, slot), None
    if col is None:
        col = st.wino = WinogradCollection(fdesc, x.shape[-1], dc.shape[-1], total, x.device, kept=False)
    assert col.key == _desc_key(fdesc, x.shape[-1]), "one layer, two geometries in one step: set T2V_WGRAD_BATCH=0"
    ws, done = col.ws, sum(col.filled)       # (the slots fill in order)
    col.filled[done:done + nb] = [True] * nb
    last = done + nb == total
    side = slot is not None and wgrad_stream_on(x)
    if side or not last:
        # the transforms always here (the data gradient of this node reads A dy A^T); with a slot and the side stream on, the
        # reduction over all slots goes there
        ops.conv2d_backward_weight_winograd_stages(x, dc, fdesc, ws, total, done, False)
    dw = None
    if last:
        st.wino, st.images = None, 0
        if side:
            _reduce_collection(col, slot, True)
        else:       # transforms and reduction in one call
            dw = deliver_into(slot, (), lambda out, accumulate: ops.conv2d_backward_weight_winograd_stages(
                x, dc, fdesc, ws, total, done, True, out=out, accumulate=accumulate))
    elif slot is not None:
        deliver(slot)      # (every node counts as delivered)
    return dw, (ws, total, done)


def flush_pending_weight_gradients(params, grads):
    """After the backward pass: a layer whose forward counted more uses than its backward nodes delivered (part of
    the graph fed no loss -- e.g. the flow head of a raw-only first frame when no flow loss is on) has operands or
    transformed slots waiting for a reduction that no node will run.  Reduce what is there: of a Winograd-domain collection
    the slots that were never filled are zeroed (a zero image contributes nothing) and the reduction runs over the whole
    workspace.  Returns `grads` with those gradients filled in."""
    out = list(grads)
    wgrad_join()
    if params and params[0].is_cuda:
        side_gemm_hint()       # (this thread: the backward nodes set theirs on the autograd engine's)
    for i, p in enumerate(params):
        st = param_state(p)
        stash, col = st.dw_stash, st.wino
        st.dw_stash = st.wino = None
        st.dw_uses = st.images = 0
        left = []
        if stash is not None:       # a layer whose remaining uses never came back: reduce the ones that did
            left.append(_reduce_stashed(stash.parts, stash.desc, grad_slot(p), from_node=False))
        if col is not None and any(col.filled):
            left.append(_reduce_collection(col, grad_slot(p), False))
        for dw in left:
            if dw is not None:
                out[i] = dw if out[i] is None else out[i] + dw
    return out


# ------------------------------------------------------------------------------------------------
# the buckets and their exchange
# ------------------------------------------------------------------------------------------------
def _acc(dst, src, overwrite):
    """dst (+)= src on flat views: HIP kernel on device tensors; host tensors only occur in the gloo CPU tests of the
    bucket bookkeeping (the trainer itself cannot exist without the GPU)"""
    if dst.is_cuda:
        ops.accumulate_(dst, src.contiguous().view(-1), overwrite=overwrite)
    elif overwrite:
        dst.view(-1).copy_(src.reshape(-1))
    else:
        dst.view(-1).add_(src.reshape(-1))


def _zero(x):
    ops.zero_(x) if x.is_cuda else x.zero_()


def _scale(x, f):
    ops.scale_(x, f) if x.is_cuda else x.mul_(f)


def _fold(grad, acc, mode, scale):
    """ops.grad_fold on flat views (HIP kernel on device tensors); on host tensors the same two fp32 operations in torch"""
    if grad.is_cuda:
        ops.grad_fold(grad, acc, mode, scale)
    elif mode == ops.GRAD_FOLD_OPEN:
        acc.copy_(grad)
    elif mode == ops.GRAD_FOLD_ADD:
        acc.add_(grad)
    else:
        torch.add(acc, grad, out=grad)
        grad.mul_(scale)


def clips_per_rank(batch_size, world):
    """--batchSize on `world` ranks -> (K, warning or None).  K = batchSize // world clips per rank and optimiser step; up
    to one clip per rank (batchSize <= world) the batch stays one clip per rank, with a warning where that is not what the
    flag says; above, batchSize must be a multiple of world (ValueError)."""
    batch_size, world = int(batch_size), int(world)
    if batch_size <= world:
        warn = None
        if batch_size not in (1, world):
            warn = ("warning: --batchSize %d, but the batch is one clip per rank = %d (list %d devices in --gpu_ids)"
                    % (batch_size, world, batch_size))
        return 1, warn
    if batch_size % world:
        raise ValueError("--batchSize %d is not a multiple of the %d ranks (devices in --gpu_ids): every rank walks "
                         "batchSize / ranks clips per optimiser step" % (batch_size, world))
    return batch_size // world, None


def clip_slots(iteration, rank, world, K):
    """[(slot, clip index)] of rank `rank` in iteration `iteration` (counted from the start of training): the batch is
    world * K global clip slots, slot s = rank * K + j for the rank's j-th clip, and slot s of iteration i reads clip
    i * (world * K) + s -- whichever way the slots are split over ranks.  K = 1: clip i * world + rank."""
    batch = world * K
    return [(rank * K + j, iteration * batch + rank * K + j) for j in range(K)]


class GradBuckets:
    """Persistent flat gradient buckets of one optimiser's parameters + their data-parallel exchange.

    Layout (static, identical on every rank): the parameters in REVERSE order -- backward reaches the last layers
    first -- packed into buckets of <= bucket_mb; every parameter's gradient lives at a fixed slice of its bucket
    (`GradSlot.view`, handed to Adam as p.grad).  During a train step the backward nodes deliver into the slots
    (`deliver` / the accumulate flags of the weight-gradient kernels); when the last expected node of the last
    parameter of a bucket has delivered, the bucket's collective is launched from inside the backward pass --
    asynchronously on the process group's stream (RCCL over xGMI; gloo in the single-GPU tests), buckets strictly in
    index order so that every rank issues the same sequence.  Replaces DataParallel's gradient reduce onto GPU 0 through
    10 MiB coalesced copies + re-broadcast of the weights ($SP/torch/cuda/comm.py:24,76-86; nn/parallel/_functions.py)
    and round 2's cat -> all_reduce -> divide -> copy-back (three extra passes over 1.1-1.5 GB per step): the bytes
    on the wire are the gradients themselves, in place.

    T2V_GRAD_RS_AG=1: reduce-scatter + all-gather per bucket instead of one all-reduce (what a ring all-reduce does
    internally; lets a sharded optimiser step sit between the two halves later).  T2V_GRAD_BUCKET_MB overrides 64."""

    def __init__(self, params, bucket_mb=None, name="", register=True):
        """register=False: the parameters keep the gradient slots they have (a temporary set of buckets over parameters a
        trainer owns must not take the trainer's slots away: ADVICE r3)"""
        import torch.distributed as dist
        self.params = list(params)
        self.name = name
        self.collecting = False
        self.world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        # (T2V_TRAIN_FORCE_DIST=1 runs the collectives on a 1-rank group too: the RCCL path on a single GPU)
        self.exchange = self.world > 1 or (os.environ.get("T2V_TRAIN_FORCE_DIST") == "1" and dist.is_available()
                                            and dist.is_initialized())
        self.rs_ag = os.environ.get("T2V_GRAD_RS_AG", "0") == "1"
        if bucket_mb is None:
            bucket_mb = float(os.environ.get("T2V_GRAD_BUCKET_MB", "64"))
        limit = max(1, int(bucket_mb * (1 << 20) // 4))
        pad = 256 * max(1, self.world)     # bucket sizes divisible by the world size (reduce-scatter shards) and 1 KiB
        order = list(range(len(self.params)))[::-1]
        bounds, members, off, cur, cur_n = [], [], 0, [], 0
        for i in order:
            n = self.params[i].numel()
            if cur and cur_n + n > limit:
                size = (cur_n + pad - 1) // pad * pad
                bounds.append((off, off + size))
                members.append(cur)
                off += size
                cur, cur_n = [], 0
            cur.append((i, cur_n))
            cur_n += n
        if cur:
            size = (cur_n + pad - 1) // pad * pad
            bounds.append((off, off + size))
            members.append(cur)
            off += size
        dev = self.params[0].device if self.params else "cpu"
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        self.bounds = bounds
        self.slots = [None] * len(self.params)
        self.bucket_of = [None] * len(self.params)
        for bi, mem in enumerate(members):
            for i, rel in mem:
                p = self.params[i]
                view = self.flat[bounds[bi][0] + rel: bounds[bi][0] + rel + p.numel()].view(p.shape)
                self.slots[i] = GradSlot(self, bi, i, view)
                if register:
                    param_state(p).gslot = self.slots[i]
                self.bucket_of[i] = bi
        self.members = [[i for i, _ in mem] for mem in members]
        self.nbytes = 0
        self._works, self._open, self._launched = [], [], 0
        # several clips per optimiser step (begin_step(micro=(j, K)), K > 1): `acc`, of the size of `flat`, takes the sum of
        # the clips' gradients bucket by bucket (_launch); _any: parameters a clip of the step so far has delivered to
        self.acc, self._micro, self._any = None, (0, 1), [False] * len(self.params)
        self._written = [False] * len(self.params)      # a kernel wrote the slot in a micro-step of this optimiser step
        self._mean = 1.0                                # fp32(1 / K) of the K last seen

    # -- one train step -----------------------------------------------------------------------------
    def begin_step(self, micro=(0, 1)):
        """micro = (j, K): clip j of the K this rank walks before the optimiser step (micro-steps).  Every micro-step is a
        step of its own for the backward nodes -- the first node of a parameter writes its slot, later ones add --; a bucket
        that is complete (_launch) is folded into `acc`, and in the last micro-step the mean over the K clips goes back
        into `flat` in front of the bucket's collective:  ((g_0 + g_1) + ... + g_{K-1}) * fp32(1 / K)."""
        j, K = micro
        if not 0 <= j < K:
            raise ValueError("begin_step: micro-step %d of %d" % (j, K))
        if j == 0:
            self._any = [False] * len(self.params)
            self._written = [False] * len(self.params)
        elif self._micro != (j - 1, K):
            raise RuntimeError("begin_step: micro-step %d of %d follows micro-step %d of %d" % ((j, K) + self._micro))
        if K != self._micro[1]:
            self._mean = struct.unpack("f", struct.pack("f", 1.0 / K))[0]      # fp32(1 / K), as the kernel receives it
        self._micro = (j, K)
        if K > 1 and self.acc is None:
            self.acc = torch.zeros_like(self.flat)
        for sl in self.slots:
            sl.expect = sl.got = 0
            sl.filled = False
        self._main = torch.cuda.current_stream() if (self.params and self.params[0].is_cuda) else None
        self._open = [len(m) for m in self.members]      # parameters of each bucket still waiting for nodes
        self._done = [False] * len(self.params)
        self._works, self._launched, self.nbytes = [], 0, 0
        # T2V_GRAD_DIRECT=0: the backward nodes hand their gradients to autograd as before and absorb() copies the sums
        # into the slots afterwards (one extra pass, no launch from inside the backward pass): the A/B baseline
        self.collecting = switch("T2V_GRAD_DIRECT")

    def seal(self):
        """The forward pass is over: parameters no node will deliver to (unused in this step) no longer hold their
        bucket back."""
        if not self.collecting:
            return
        for sl in self.slots:
            if sl.expect == 0 and not self._done[sl.idx]:
                self._done[sl.idx] = True
                self._open[sl.bucket] -= 1
        # (nothing is launched here: a launch from the first delivering node keeps the bucket order intact)

    def node_done(self, sl):
        sl.got += 1
        if sl.got == sl.expect and not self._done[sl.idx]:
            self._done[sl.idx] = True
            self._open[sl.bucket] -= 1
            self._launch_ready()

    def _launch_ready(self):
        """launch, in bucket order, every bucket whose parameters have all received their last expected gradient"""
        while self._launched < len(self.bounds) and self._open[self._launched] == 0:
            self._launch(self._launched)
            self._launched += 1

    def _launch(self, b):
        # parameters no backward node reached contribute exact zeros (and get no optimiser step: see finish)
        for i in self.members[b]:
            if not self.slots[i].filled and not self.slots[i].zero_valid:
                _zero(self.slots[i].view)
        j, K = self._micro
        fold = None if K == 1 else (ops.GRAD_FOLD_OPEN if j == 0 else ops.GRAD_FOLD_CLOSE if j == K - 1 else ops.GRAD_FOLD_ADD)
        # (the bucket goes out with the step's last clip only)
        issue = self.exchange and j == K - 1
        if fold is None and not issue:
            return
        if fold is not None:
            # CLOSE rewrites the whole bucket with the mean.  A slot whose zeros are on record (zero_valid) keeps them only if
            # no kernel wrote it in any micro-step of this optimiser step: (0 + 0) * s = 0; otherwise the record goes
            for i in self.members[b]:
                sl = self.slots[i]
                if sl.filled and not sl.zero_valid:
                    self._written[i] = True
                if fold == ops.GRAD_FOLD_CLOSE and self._written[i]:
                    sl.zero_valid = False
        # The collective is ordered behind the stream it is issued on, and it needs the weight-gradient stream's kernels AND the
        # current stream's (and the step's main stream's, when this node runs on another).  With weight gradients in flight it
        # is issued FROM the weight-gradient stream, which first takes in what the other streams hold so far: the backward
        # pass itself does not stop.  (Until round 6 the current stream joined the weight-gradient stream here, 36 times per
        # step: the data-gradient chain waited for every layer's weight gradient, and the two queues of DESIGN 6b ran one
        # after the other again whenever the exchange was on.)  T2V_EXCHANGE_FROM_SIDE=0: the join.
        cur = torch.cuda.current_stream() if self.flat.is_cuda else None
        side = STEP.stream if (cur is not None and STEP.pending and switch("T2V_EXCHANGE_FROM_SIDE")) else None
        if side is not None and side != cur:
            side.wait_stream(cur)
            if self._main is not None and cur != self._main:
                side.wait_stream(self._main)
            with torch.cuda.stream(side):
                self._fold_and_issue(b, fold, issue)
            return
        wgrad_join()
        if self._main is not None and torch.cuda.current_stream() != self._main:
            torch.cuda.current_stream().wait_stream(self._main)
        self._fold_and_issue(b, fold, issue)

    def _fold_and_issue(self, b, fold, issue):
        """on the stream the bucket's collective is issued from, behind everything that wrote the bucket: its fold into (the
        last clip: out of) the accumulator, then the collective"""
        if fold is not None:
            lo, hi = self.bounds[b]
            _fold(self.flat[lo:hi], self.acc[lo:hi], fold, self._mean)
        if issue:
            self._issue(b)

    def _issue(self, b):
        import torch.distributed as dist
        lo, hi = self.bounds[b]
        buf = self.flat[lo:hi]
        avg = dist.get_backend() == "nccl"       # RCCL averages in the collective; gloo sums (scaled in finish)
        op = dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM
        if self.rs_ag:      # (also on a forced 1-rank group: the RCCL entry points run on device tensors)
            shard = (hi - lo) // self.world
            r = dist.get_rank()
            mine = buf[r * shard:(r + 1) * shard]
            if avg:     # RCCL: in-place reduce-scatter (output = this rank's shard of the input), then the all-gather,
                w1 = dist.reduce_scatter_tensor(mine, buf, op=op, async_op=True)      # both stream-ordered
                self._works.append((w1, None, None, None))
                w2 = dist.all_gather_into_tensor(buf, mine, async_op=True)
                self._works.append((w2, buf, avg, None))
            else:       # gloo (tests): works are not ordered among themselves -- the all-gather is issued in finish()
                out = torch.empty_like(mine)
                w1 = dist.reduce_scatter_tensor(out, buf, op=op, async_op=True)
                self._works.append((w1, buf, avg, (mine, out)))
        else:
            self._works.append((dist.all_reduce(buf, op=op, async_op=True), buf, avg, None))
        self.nbytes += 4 * sum(self.params[i].numel() for i in self.members[b])     # payload (the padding travels too)

    def absorb(self, grads):
        """After autograd.grad: gradients that came back as tensors (parameters reached through torch-native plumbing,
        e.g. the cat of the two flow-head convs; a flushed Winograd reduction) are added into their slots; then every
        bucket not yet launched goes out, in order."""
        wgrad_join()
        for i, g in enumerate(grads):
            if g is not None:
                sl = self.slots[i]
                _acc(sl.view, g, not sl.filled)
                sl.filled = True
        for b in range(self._launched, len(self.bounds)):
            self._launch(b)
        self._launched = len(self.bounds)
        self.collecting = False

    def finish(self):
        """Wait for the collectives; p.grad = the slot (None where no rank-local node delivered, in any clip of the optimiser
        step so far: Adam then skips the parameter, as torch 0.4.1's does).  Returns the bytes exchanged."""
        import torch.distributed as dist
        wgrad_join()
        for work, buf, avg, shard in self._works:
            work.wait()
            if shard is not None:
                shard[0].copy_(shard[1])
                dist.all_gather_into_tensor(buf, shard[0].clone())
            if buf is not None and not avg and self.world > 1:
                _scale(buf, 1.0 / self.world)
        self._works = []
        for k, (p, sl) in enumerate(zip(self.params, self.slots)):
            if sl.filled:
                self._any[k] = True
            p.grad = sl.view if self._any[k] else None
        return self.nbytes

    def presence(self):
        """a checksum of WHICH parameters received gradients on this rank: must agree across ranks, or the replicas'
        optimiser steps differ (Adam skips parameters without gradient)"""
        return float(sum((k + 1) * (k + 7) for k, sl in enumerate(self.slots) if sl.filled or self._any[k]) % 1000003)


def check_presence_across_ranks(buckets, device):
    """Every rank must have delivered gradients to the same parameters.  One tiny MAX / MIN all-reduce per step."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return
    v = [b.presence() for b in buckets]
    dev = device if dist.get_backend() == "nccl" else "cpu"
    t = torch.tensor(v + [-x for x in v], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    t = t.cpu().tolist()
    n = len(v)
    if any(t[k] != -t[n + k] for k in range(n)):
        raise RuntimeError("data-parallel ranks disagree on which parameters received gradients this step (checksums "
                           "max %s / min %s): their optimiser steps would diverge" % (t[:n], [-x for x in t[n:]]))


class GradientExchange:
    """Stand-alone form for gradients that already sit in p.grad (tests, callers outside the trainer): the gradients
    are moved into a temporary GradBuckets (one pass), exchanged bucket by bucket, and p.grad ends as the averaged slot."""

    def __init__(self, params, bucket_mb=64):
        ps = [p for p in params if p.grad is not None]
        self.b = GradBuckets(ps, bucket_mb, register=False) if ps else None
        if self.b is not None:
            self.b.begin_step()
            self.b.absorb([p.grad for p in ps])

    def finish(self):
        return self.b.finish() if self.b is not None else 0


def allreduce_gradients_begin(params, bucket_mb=64):
    return GradientExchange(params, bucket_mb)


def allreduce_gradients(params, bucket_mb=64):
    """Data-parallel gradient exchange of gradients already in p.grad: bucketed, averaged over ranks; returns the bytes
    exchanged.  Replaces DataParallel's reduce-to-GPU-0 + re-broadcast: replicas are persistent, so
    one collective per bucket is all the communication a step needs."""
    return GradientExchange(params, bucket_mb).finish()
