"""JPEG files -> uint8 RGB device tensors, decoded on the GPU (ops.jpeg_decode_u8).

    tensors, fallback = decode_files(blobs, device)

The result is always what Pillow's Image.open(...).convert("RGB") gives.  A file the GPU decoder does not take (jpeg.parse
refuses it: progressive, grey, CMYK, restart markers, not a JPEG at all, a geometry outside 8..2048) and a file whose status
comes back non-zero (its code stream did not synchronise, or it is corrupt) is decoded by Pillow into its slot; `fallback`
names them.

`pack` / `upload_and_decode` are the two halves the train loader uses on its own threads and streams: the first is host work
(parse, one page-locked buffer), the second only enqueues.
"""
import io

import numpy as np

from ._xp import torch
from . import jpeg as J
from . import ops

CAPACITY_STEP = 256      # a group's scan capacity is its longest scan rounded up to this
BUFFER_STEP = 1 << 16    # a buffer taken from a caller's allocator is rounded up to this, so that the allocator can reuse it


class Group(object):
    """files of one (H, W, sampling), packed for one decode call: .buf is the page-locked buffer as a uint8 array
    [scans n x capacity | tables n x TABLE_BYTES | lengths n x uint32 | slack], .host the tensor that owns it (None where
    the caller's allocator does), .index the files' positions in the caller's list"""
    __slots__ = ("H", "W", "sampling", "index", "capacity", "buf", "host")

    @property
    def n(self):
        return len(self.index)

    def lengths(self):
        """the uint32 scan lengths as they stand in the page-locked buffer (a view)"""
        at = self.n * (self.capacity + J.TABLE_BYTES)
        return self.buf[at:at + 4 * self.n].view(np.uint32)


def pillow_rgb(blob):
    """what the decoder must equal: uint8 [H,W,3]"""
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as im:
        return np.array(im.convert("RGB"))


def pack(blobs, alloc=None):
    """Host work: parse every file and pack the accepted ones by (H, W, sampling) into page-locked buffers.
    -> (groups, refused): refused is [(index, reason)] of the files jpeg.parse or the decoder's geometry check turns away.
    alloc((nbytes,)) -> uint8 array: where a group's buffer comes from instead (page-locked memory the caller recycles)."""
    parsed, refused, by_key = {}, [], {}
    for i, blob in enumerate(blobs):
        try:
            p = J.parse(blob)
            if not ops.jpeg_decode_supported(p.H, p.W, p.sampling):
                raise J.JpegUnsupported("a frame of %dx%d (8..2048 per dimension)" % (p.H, p.W))
        except J.JpegUnsupported as e:
            refused.append((i, e.reason))
            continue
        parsed[i] = p
        by_key.setdefault((p.H, p.W, p.sampling), []).append(i)
    groups = []
    for (H, W, sampling), index in by_key.items():
        g = Group()
        g.H, g.W, g.sampling, g.index = H, W, sampling, index
        n = len(index)
        g.capacity = ops.round_up(max(parsed[i].scan_length for i in index), CAPACITY_STEP)
        need = n * (g.capacity + J.TABLE_BYTES + 4)
        if alloc is None:
            g.host = torch.empty(need, dtype=torch.uint8, pin_memory=True)
            buf = g.buf = g.host.numpy()
        else:
            g.host = None
            buf = g.buf = alloc((ops.round_up(need, BUFFER_STEP),))
        lengths = np.empty(n, np.uint32)
        for j, i in enumerate(index):
            p = parsed[i]
            buf[j * g.capacity:j * g.capacity + p.scan_length] = np.frombuffer(blobs[i], np.uint8, p.scan_length, p.scan_offset)
            at = n * g.capacity + j * J.TABLE_BYTES
            buf[at:at + J.TABLE_BYTES] = np.frombuffer(p.tables, np.uint8)
            lengths[j] = p.scan_length
        g.lengths()[:] = lengths
        groups.append(g)
    return groups, refused


def decode_uploaded(group, dev, out_cs=3, dst=None, status=None, workspace=None):
    """Enqueue on the current stream the decode call for a group whose buffer stands in the uint8 device tensor `dev`.
    -> (dst [n,H,W,out_cs], status int32 [n]), both on the device"""
    n = group.n
    scans = dev.narrow(0, 0, n * group.capacity)
    tables = dev.narrow(0, n * group.capacity, n * J.TABLE_BYTES)
    lengths = dev.narrow(0, n * (group.capacity + J.TABLE_BYTES), n * 4)
    return ops.jpeg_decode_u8(scans, group.capacity, lengths, tables, group.H, group.W, group.sampling, n, dst=dst, dst_cs=out_cs,
                              status=status, workspace=workspace)


def upload_and_decode(group, device, out_cs=3, dst=None):
    """Enqueue on the current stream: one upload of the group's buffer, one decode call.  -> (dst [n,H,W,out_cs], status
    int32 [n]), both on the device; nothing waits."""
    return decode_uploaded(group, group.host.to(device, non_blocking=True), out_cs, dst)


def _slot(arr, out_cs):
    """a Pillow array as one [1,H,W,out_cs] host tensor"""
    if out_cs == 4:
        arr = np.concatenate([arr, np.zeros(arr.shape[:2] + (1,), np.uint8)], -1)
    return torch.from_numpy(np.ascontiguousarray(arr[None]))


def decode_files(blobs, device, out_cs=3):
    """blobs: the files' bytes.  -> (tensors, fallback): tensors[i] the uint8 device tensor [H,W,out_cs] of file i (channel 3,
    if asked for, is 0); fallback [(index, reason)] of the files Pillow decoded.  Every group is uploaded as one page-locked
    buffer and decoded by one call; the statuses come back behind one event."""
    if out_cs not in (3, 4):
        raise ValueError("decode_files: out_cs %d (3 or 4)" % out_cs)
    groups, fallback = pack(blobs)
    out = [None] * len(blobs)
    launched = []
    for g in groups:
        dst, status = upload_and_decode(g, device, out_cs)
        host = torch.empty(g.n, dtype=torch.int32, pin_memory=True)
        host.copy_(status, non_blocking=True)
        launched.append((g, dst, host))
    if launched:
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
    for g, dst, host in launched:
        status = host.numpy()
        for j, i in enumerate(g.index):
            slot = dst.narrow(0, j, 1)
            if status[j]:
                fallback.append((i, "status %d: %s" % (status[j], " and ".join(
                    w for bit, w in ((1, "the code stream did not synchronise"), (2, "corrupt stream")) if status[j] & bit))))
                slot.copy_(_slot(pillow_rgb(blobs[i]), out_cs))
            out[i] = slot.view(g.H, g.W, out_cs)
    for i, _ in fallback:
        if out[i] is None:
            arr = pillow_rgb(blobs[i])
            out[i] = _slot(arr, out_cs).to(device).view(arr.shape[0], arr.shape[1], out_cs)
    return out, sorted(fallback)
