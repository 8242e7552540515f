"""Result writer with the reference's output layout (SURVEY.md App. F `Visualizer.save_images`):
    <results_dir>/<name>/<phase>_<which_epoch>/<seq>/<label>_<basename of the test_img file>.jpg
which is what text2video_audio.sh:39-40 cleans and image2video*.py globs (`fake_B_*.jpg`).
JPEG encoding runs on a small thread pool so it overlaps the GPU work of the next frames; files that arrive encoded
(test.py --gpu_jpeg: ops.jpeg_encode_u8; --frame_format png: ops.png_encode_u8) are only written by it."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from PIL import Image


def tensor2im_np(x_chw):
    """util.tensor2im: float CHW in [-1,1] -> uint8 HWC (truncating cast, like numpy astype)."""
    a = (np.transpose(np.asarray(x_chw, np.float32), (1, 2, 0)) + 1) / 2.0 * 255.0
    return np.clip(a, 0, 255).astype(np.uint8)


class Visualizer:
    def __init__(self, opt, workers=4, quality=None, ext=".jpg"):
        """quality: the JPEG quality of save_images (None: Pillow's default, 75); ext: the extension, and with it the format,
        of the files save_images writes (".png" under --frame_format png)"""
        self.quality = quality
        self.ext = ext
        self.save_dir = os.path.join(opt.results_dir, opt.name, "%s_%s" % (opt.phase, opt.which_epoch))
        self.pool = ThreadPoolExecutor(max_workers=workers)
        self.pending = []
        self._made = set()

    def _write(self, path, arr):
        if self.quality is None:
            Image.fromarray(arr).save(path)
        else:
            Image.fromarray(arr).save(path, quality=self.quality)

    @staticmethod
    def _write_bytes(path, blob):
        with open(path, "wb") as fh:
            fh.write(blob)

    def save_bytes(self, files, a_path, ext=".jpg"):
        """files: {label: the finished file as bytes}; ext: what they are (".jpg", ".png").  Same names as save_images;
        returns the written paths."""
        return self._save(files, a_path, self._write_bytes, lambda blob: blob, ext)

    def save_images(self, visuals, a_path):
        """visuals: {label: uint8 HWC array}.  Returns the written paths."""
        return self._save(visuals, a_path, self._write, np.ascontiguousarray, self.ext)

    def _save(self, items, a_path, write, prepare, ext):
        sub = os.path.basename(os.path.dirname(a_path))
        name = os.path.splitext(os.path.basename(a_path))[0]
        d = os.path.join(self.save_dir, sub)
        if d not in self._made:
            os.makedirs(d, exist_ok=True)
            self._made.add(d)
        out = []
        for label, item in items.items():
            path = os.path.join(d, "%s_%s%s" % (label, name, ext))
            self.pending.append(self.pool.submit(write, path, prepare(item)))
            out.append(path)
        return out

    def flush(self):
        for f in self.pending:
            f.result()
        self.pending = []

    def close(self):
        """flush and release the encoder threads (a resident server builds one Visualizer per request)"""
        self.flush()
        self.pool.shutdown(wait=True)
