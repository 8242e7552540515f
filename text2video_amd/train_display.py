"""What a training run shows of itself (vid2vid/train.py --display_web), with upstream's layout [RECALL util/visualizer.py]:
    <checkpoints_dir>/<name>/web/index.html                         one table row per displayed step, newest first
    <checkpoints_dir>/<name>/web/images/epoch%03d_iter%07d_<label>.jpg
    <checkpoints_dir>/<name>/loss_log.txt                           a dated header, then every printed iteration line

The pictures are rendered on the GPU (ops.train_visuals: tensor2im bytes, unit maps as grey, flow fields as hue =
direction / brightness = magnitude) on the compute stream right behind the step whose tensors they read, copied to one
of two pinned slots on a side stream, and encoded by one writer thread (Pillow): the training loop waits for no file."""
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor

LABELS = ("input_image", "fake_image", "fake_raw_image", "real_image", "flow", "weight", "flow_ref", "conf_ref")
REFRESH_S = 30


def panels_of(visuals):
    """Vid2VidTrainer.visuals -> [(label, kind, tensor, c0)] in the order of LABELS; flow, weight, flow_ref and conf_ref only
    where the step formed them."""
    from . import ops
    out = [("input_image", ops.VISUALS_IMAGE, visuals["pose"], 6),      # the window's newest pose map
           ("fake_image", ops.VISUALS_IMAGE, visuals["fake"], 0),
           ("fake_raw_image", ops.VISUALS_IMAGE, visuals["raw"], 0),
           ("real_image", ops.VISUALS_IMAGE, visuals["real"], 0)]
    if visuals.get("fw") is not None:
        out += [("flow", ops.VISUALS_FLOW, visuals["fw"], 0), ("weight", ops.VISUALS_UNIT, visuals["fw"], 2)]
    if visuals.get("flow_ref") is not None:
        out.append(("flow_ref", ops.VISUALS_FLOW, visuals["flow_ref"], 0))
    if visuals.get("conf_ref") is not None:
        out.append(("conf_ref", ops.VISUALS_UNIT, visuals["conf_ref"], 0))
    return out


class TrainDisplay:
    """Rank 0's display.  show() needs the GPU; write_panels() and log() -- what the writer thread and the loop call -- do not."""

    def __init__(self, opt):
        self.dir = os.path.join(opt.checkpoints_dir, opt.name)
        self.web_dir = os.path.join(self.dir, "web")
        self.img_dir = os.path.join(self.web_dir, "images")
        os.makedirs(self.img_dir, exist_ok=True)
        self.name = opt.name
        self.scale = int(getattr(opt, "display_scale", 1))
        self.rows = []                # (epoch, iter, [labels]) in display order
        self.last_panels = {}         # label -> uint8 [h,w,3] of the last display, before JPEG
        self.log_path = os.path.join(self.dir, "loss_log.txt")
        self._log = open(self.log_path, "a")
        self._log.write("================ Training Loss (%s) ================\n" % time.strftime("%c"))
        self._log.flush()
        self._writer = ThreadPoolExecutor(max_workers=1)      # one thread: pictures and page are written in display order
        self._pending = []
        self._slots, self._shown = None, 0

    # ---- host side -------------------------------------------------------------------------------------------------
    def log(self, line):
        self._log.write(line + "\n")
        self._log.flush()

    @staticmethod
    def image_name(epoch, total_samples, label):
        return "epoch%03d_iter%07d_%s.jpg" % (epoch, total_samples, label)

    def write_panels(self, panels, epoch, total_samples):
        """panels: {label: uint8 HWC array} -> the JPEGs under web/images and a rewritten index.html; returns the paths."""
        from PIL import Image
        import numpy as np
        paths = []
        for label, arr in panels.items():
            path = os.path.join(self.img_dir, self.image_name(epoch, total_samples, label))
            Image.fromarray(np.ascontiguousarray(arr)).save(path)
            paths.append(path)
        self.last_panels = dict(panels)
        self.rows.append((epoch, total_samples, list(panels)))
        self.write_index()
        return paths

    def write_index(self):
        doc = ["<!DOCTYPE html>", "<html>", "<head>", "  <title>Experiment name = %s</title>" % self.name,
               '  <meta http-equiv="refresh" content="%d">' % REFRESH_S, "</head>", "<body>"]
        for epoch, total, labels in reversed(self.rows):
            doc.append("  <h3>epoch [%d], iter [%d]</h3>" % (epoch, total))
            doc.append('  <table border="1" style="table-layout: fixed;">')
            doc.append("    <tr>")
            for label in labels:
                rel = "images/" + self.image_name(epoch, total, label)
                doc.append('      <td style="word-wrap: break-word;" halign="center" valign="top"><p><a href="%s">'
                           '<img src="%s"></a><br><p>%s</p></p></td>' % (rel, rel, label))
            doc.append("    </tr>")
            doc.append("  </table>")
        doc += ["</body>", "</html>"]
        tmp = os.path.join(self.web_dir, "index.html.tmp")
        with open(tmp, "w") as fh:
            fh.write("\n".join(doc) + "\n")
        os.replace(tmp, os.path.join(self.web_dir, "index.html"))      # (a browser that reloads never reads half a page)

    # ---- device side -----------------------------------------------------------------------------------------------
    def _slot(self, n, h, w, device):
        import torch
        if self._slots is None or tuple(self._slots[0]["dev"].shape) != (n, h, w, 3):
            self.flush()
            self._slots = []
            for _ in range(2):
                taken = threading.Event()
                taken.set()
                self._slots.append({"dev": torch.empty(n, h, w, 3, dtype=torch.uint8, device=device),
                                    "host": torch.empty(n, h, w, 3, dtype=torch.uint8).pin_memory(),
                                    "copied": None, "taken": taken})
            self._side = torch.cuda.Stream(device=device)
        return self._slots[self._shown % 2]

    def show(self, visuals, epoch, total_samples):
        """Enqueue the render of `visuals` (Vid2VidTrainer.visuals) on the current stream -- behind the step that produced
        them, ahead of the next one that may reuse their memory --, the copy to a pinned slot on the side stream, and
        hand the rest to the writer thread."""
        import torch
        from . import ops
        done = [f for f in self._pending if f.done()]
        self._pending = [f for f in self._pending if not f.done()]
        for f in done:
            f.result()                # (a writer's exception surfaces at the next display, not at the end of the run)
        named = panels_of(visuals)
        first = named[0][2]
        H, W = first.shape[0], first.shape[1]
        slot = self._slot(len(named), H // self.scale, W // self.scale, first.device)
        slot["taken"].wait()          # the writer took its copy of this slot's display two shows ago (a memcpy, no file)
        slot["taken"].clear()
        compute = torch.cuda.current_stream()
        if slot["copied"] is not None:
            compute.wait_event(slot["copied"])      # (on the GPU) the slot's device buffer has been read out
        try:
            ops.train_visuals([(kind, t, c0) for _, kind, t, c0 in named], self.scale, out=slot["dev"])
        except Exception:
            slot["taken"].set()
            raise
        rendered = torch.cuda.Event()
        rendered.record(compute)
        self._side.wait_event(rendered)
        with torch.cuda.stream(self._side):
            slot["host"].copy_(slot["dev"], non_blocking=True)
            slot["copied"] = torch.cuda.Event()
            slot["copied"].record(self._side)
        self._shown += 1
        self._pending.append(self._writer.submit(self._write, slot, slot["copied"], [l for l, _, _, _ in named], epoch,
                                                 total_samples))

    def _write(self, slot, copied, labels, epoch, total_samples):
        try:
            copied.synchronize()
            arr = slot["host"].numpy().copy()
        finally:
            slot["taken"].set()
        self.write_panels({label: arr[i] for i, label in enumerate(labels)}, epoch, total_samples)

    def flush(self):
        """wait for every picture and the page to be on disk (a writer's exception is raised here)"""
        pending, self._pending = self._pending, []
        for f in pending:
            f.result()

    def close(self):
        self.flush()
        self._writer.shutdown(wait=True)
        self._log.close()
