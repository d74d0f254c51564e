"""What a batch of frames is written to: the five destinations of the Predictor's annotated video and mesh overlay
(dropin/core/outputs.py: write_gpu_video, write_mesh_overlay), each a small class with the same three methods; `open_sink` is the one
place that chooses among them, `write_all` the one loop that fills them.

    put(numbers, images)   frame numbers int[b], images u8[b,H,W,3] on the device
    close() -> path        finishes the output; raises what a failed encoder child raises
    abort()                releases everything for a caller that is handling an error of its own, and raises nothing over it"""
import os
import shlex

import numpy as np

from . import _media, jpeg, mjpeg, png, y4m

CODECS = ("", "mjpeg", "png", "y4m")


def save_png(path, rgb):
    """u8[H,W,3] RGB -> PNG with Pillow, else matplotlib."""
    try:
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(rgb)).save(path)
    except ImportError:
        import matplotlib.image
        matplotlib.image.imsave(path, np.ascontiguousarray(rgb))


class AviSink:
    """`stem`.avi: the images encoded to baseline JPEG on the GPU at `quality` (4:2:0, a restart marker per MCU row; a frame that
    overflows its default slot again with the slot no file exceeds) and stored as Motion-JPEG: only the files' bytes leave the device.
    close() returns the first file; past 1 GiB the frames continue in <name>.001.avi, ... beside it (mjpeg.AviWriter).  abort() is
    close(): the index is written and the headers patched, so what was put can be played."""

    def __init__(self, stem, width, height, fps, bgr, quality):
        self.path, self.bgr, self.quality = stem + ".avi", bgr, quality
        self._avi = mjpeg.AviWriter(self.path, width, height, fps)

    def put(self, numbers, images):
        encode = lambda images, capacity: jpeg.encode_frames(images, quality=self.quality, bgr=self.bgr, capacity=capacity)
        bound = jpeg.encode_bound(int(images.shape[1]), int(images.shape[2]))
        for data in _media.encode_files(encode, images.contiguous(), None, bound, "jpeg.encode_frames"):
            self._avi.write(data)

    def close(self):
        self._avi.close()
        return self.path

    abort = close


class _Folder:
    """`stem`/%09d.png by frame number.  Nothing is held between two puts: close() and abort() have nothing to release."""

    def __init__(self, stem, bgr):
        self.path, self.bgr = stem, bgr
        os.makedirs(stem, exist_ok=True)

    def file(self, number):
        return os.path.join(self.path, "{0:09d}.png".format(int(number)))

    def close(self):
        return self.path

    def abort(self):
        pass


class PngSink(_Folder):
    """The images encoded to PNG on the GPU (adaptive filters, run-length deflate; png.encode_frames): only the files' bytes leave
    the device.  A slot holds half the raw size, which rendered canvases stay far below; a frame that overflows it (noise does)
    is encoded again alone with the slot no file exceeds."""

    def put(self, numbers, images):
        H, W = int(images.shape[1]), int(images.shape[2])
        encode = lambda images, capacity: png.encode_frames(images, bgr=self.bgr, capacity=capacity)
        bound = png.encode_bound(H, W)
        files = _media.encode_files(encode, images.contiguous(), min(bound, 4096 + H * W * 3 // 2), bound, "png.encode_frames")
        for f, data in zip(numbers, files):
            with open(self.file(f), "wb") as fh:
                fh.write(data)


class PillowSink(_Folder):
    """The frames downloaded and written one by one (save_png)."""

    def put(self, numbers, images):
        for f, im in zip(numbers, images.cpu().numpy()):
            save_png(self.file(f), im[..., ::-1] if self.bgr else im)


class Y4mSink:
    """`stem`.y4m: the images converted to Y'CbCr on the GPU (y4m.encode_frames: `matrix`, 'auto' being 709 above 576 rows; limited
    range; `chroma`, odd sides of a subsampled layout padded to even) as a YUV4MPEG2 stream -- or, with `encoder` (a command line
    containing {output}), fed to that command, {output} replaced by `stem` + `encoder_ext`.  Never a shell; close() raises
    RuntimeError naming a failed encoder's status, abort() reaps it and raises nothing."""

    def __init__(self, stem, width, height, fps, bgr, chroma, encoder, encoder_ext, matrix):
        if matrix == "auto":
            matrix = "709" if height > 576 else "601"
        self.path = stem + (encoder_ext if encoder else ".y4m")
        to = dict(command=[a.replace("{output}", self.path) for a in shlex.split(encoder)]) if encoder else dict(dst=self.path)
        self._writer = y4m.Writer(width=width, height=height, fps=fps, chroma=chroma, matrix=matrix, full_range=False, bgr=bgr,
                                  pad_even=chroma in ("420jpeg", "420mpeg2", "422"), **to)

    def put(self, numbers, images):
        self._writer.put(images)

    def close(self):
        self._writer.close()
        return self.path

    def abort(self):
        self._writer.abort()


class Cv2Sink:
    """`stem`.mp4 through cv2.VideoWriter ('mp4v'): the frames are downloaded, cv2 only writes the container."""

    def __init__(self, cv2, stem, width, height, fps, bgr):
        self.path, self.bgr = stem + ".mp4", bgr
        self._vw = cv2.VideoWriter(self.path, 0x7634706d, float(fps), (width, height))

    def put(self, numbers, images):
        for im in images.cpu().numpy():
            self._vw.write(im if self.bgr else np.ascontiguousarray(im[..., ::-1]))

    def close(self):
        self._vw.release()
        return self.path

    abort = close


def open_sink(codec, stem, width, height, fps, bgr, quality=90, chroma="420mpeg2", encoder="", encoder_ext=".mp4", matrix="601"):
    """The sink of `codec` for `width` x `height` frames (RGB, or BGR with `bgr`) at `fps`, named after `stem`:
    'mjpeg' `stem`.avi at `quality`; 'png' `stem`/%09d.png encoded on the GPU; 'y4m' `stem`.y4m in `chroma` and `matrix`, or `stem`
    + `encoder_ext` through the `encoder` command; '' `stem`.mp4 through cv2 where it is importable, else `stem`/%09d.png through
    Pillow.  This only makes names, folders, files and (for an encoder) a child process: nothing touches the GPU before the first
    put().  Any other codec raises ValueError."""
    if codec == "mjpeg":
        return AviSink(stem, width, height, fps, bgr, quality)
    if codec == "png":
        return PngSink(stem, bgr)
    if codec == "y4m":
        return Y4mSink(stem, width, height, fps, bgr, chroma, encoder, encoder_ext, matrix)
    if codec != "":
        raise ValueError(f"codec {codec!r} is not known: one of {CODECS}")
    try:
        import cv2
    except ImportError:
        return PillowSink(stem, bgr)
    return Cv2Sink(cv2, stem, width, height, fps, bgr)


def write_all(sink, batches):
    """Every (numbers, images) of `batches` into `sink` -> the path close() returns.  Whatever raises on the way -- the iterator,
    an encoder, the disk -- aborts the sink and is raised as it is."""
    try:
        for numbers, images in batches:
            sink.put(numbers, images)
    except BaseException:
        sink.abort()
        raise
    return sink.close()
