"""The reference's front end (lib/utils/funcs_utils.py:18-53: decode the video, downscale it, write `<output>/tmp/%09d.jpg`) for
a Motion-JPEG AVI, without OpenCV: the container is read in Python (mjpeg.AviReader), every frame is decoded on the GPU
(jpeg.decode_files), downscaled on the GPU by the integer bilinear contract of include/poserisk_hip.h (section j3;
csrc/resize_host.cc, csrc/resize.hip) and, where a tracker needs files, encoded on the GPU (jpeg.encode_frames).
A YUV4MPEG2 stream (a `.y4m` file, a y4m.Reader, or "-" for standard input: what a decoder of any codec pipes out) takes the
same way through y4m.decode: chroma upsampling, colour matrix and the same downscale in one kernel (section j6; csrc/yuv.hip).

    target_size    the reference's rule: wider than 800 -> 800 wide, elif higher than 450 -> 450 high
    resize_frames  u8[F,H,W,3] -> u8[F,h,w,3] on the device
    read_video     a Motion-JPEG AVI or a YUV4MPEG2 stream -> (frames on the device at the target size, fps)
    prepare        the same inputs -> a folder of %09d.jpg + fps.txt; with a tracking.pkl added it is an input of
                   Predictor.load_front_end.   python -m poserisk_release_amd.frontend prepare <video> <dir>"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib, _media, jpeg, mjpeg

MODE_COPY, MODE_HALF, MODE_LINEAR = 0, 1, 2
MAX_CHUNK = 1024


def target_size(W, H, max_w=800, max_h=450):
    """(w, h) of the reference's front end for a W x H video; max_w = 0 or max_h = 0 switches that arm off.  `elif` as in the
    reference: a frame that was narrowed is not checked for its height (1080 x 1920 becomes 800 x 1422)."""
    W, H = int(W), int(H)
    if max_w and W > max_w:
        return int(max_w), int(H * max_w / W)
    if max_h and H > max_h:
        return int(W * max_h / H), int(max_h)
    return W, H


def resize_plan(H, W, h, w):
    """pr_resize_plan -> (xofs int32[w], xcoef int16[2w], yofs int32[h], ycoef int16[2h], mode)."""
    xofs, xcoef = np.zeros(max(int(w), 0), np.int32), np.zeros(2 * max(int(w), 0), np.int16)
    yofs, ycoef = np.zeros(max(int(h), 0), np.int32), np.zeros(2 * max(int(h), 0), np.int16)
    mode = np.full(1, -1, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().pr_resize_plan(int(H), int(W), int(h), int(w), ptr(xofs), ptr(xcoef), ptr(yofs), ptr(ycoef), ptr(mode)),
               "pr_resize_plan")
    return xofs, xcoef, yofs, ycoef, int(mode[0])


def _resize_tables(key, device):
    """The uploaded tables of key = (H, W, h, w) on `device` -> (u8 tensor [xofs | yofs | xcoef | ycoef], mode)."""
    def make():
        xofs, xcoef, yofs, ycoef, mode = resize_plan(*key)
        return xofs.tobytes() + yofs.tobytes() + xcoef.tobytes() + ycoef.tobytes(), mode
    return _media.device_plan(("resize",) + key, device, make)


def resize_frames(frames, h, w, out=None):
    """u8[F,H,W,3] on the device -> u8[F,h,w,3] (`out`, or a new tensor) by the bilinear contract; exactly half in both axes is
    the 2 x 2 mean, the same size a copy.  Asynchronous on the current stream; with `out` given and the size pair seen before
    it allocates and synchronises nothing."""
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda):
        raise _lib.PoseRiskHipError("resize_frames: the resize runs on the GPU only (no CPU fallback)")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError(f"resize_frames: frames must be a contiguous uint8 [F, H, W, 3] tensor, got {frames.dtype} {tuple(frames.shape)}")
    device, (F, H, W, _) = frames.device, frames.shape
    h, w = int(h), int(w)
    with torch.cuda.device(device):
        tables, mode = _resize_tables((H, W, h, w), device)
        if out is None:
            out = torch.empty((F, h, w, 3), dtype=torch.uint8, device=device)
        if tuple(out.shape) != (F, h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device:
            raise ValueError(f"resize_frames: out must be a contiguous uint8 {[F, h, w, 3]} tensor on {device}")
        base = tables.data_ptr()
        stream = torch.cuda.current_stream(device)
        _lib.check(_lib.load().pr_resize_frames(frames.data_ptr(), F, H, W, out.data_ptr(), h, w, base, base + 4 * w + 4 * h,
                                                base + 4 * w, base + 8 * w + 4 * h, mode, stream.cuda_stream), "pr_resize_frames")
    return out


def chunk_frames(H, W, max_bytes, frame_bytes=0):
    """Frames decoded per call: the largest count <= 1024 whose source-size pixels plus decoder workspace fit max_bytes; at
    least 1.  frame_bytes > 0 (the largest file of the video) sizes the workspace as pr_jpeg_decode_sync needs it, which keeps
    60 bytes per 128 compressed bytes and per restart segment (at most one per row of blocks assumed) on top."""
    if frame_bytes:
        space = lambda n: jpeg.sync_workspace_bytes(n, H, W, n * frame_bytes, n * ((H + 7) // 8 + 1))
    else:
        space = lambda n: jpeg.workspace_bytes(n, H, W)
    need = lambda n: n * H * W * 3 + space(n)
    n = max(1, min(MAX_CHUNK, int(max_bytes) // max(need(1), 1)))      # the workspace grows with the frame count, in steps at most
    while n > 1 and need(n) > max_bytes:
        n -= 1
    return n


def _raise_refused(path, part, lo, H, W, fallback, progressive=False):
    _, _, _, pst, *_ = jpeg.parse_scans(part, H, W) if progressive else jpeg.parse(part, H, W)
    bad = np.nonzero(pst)[0]
    if bad.size:
        raise RuntimeError(f"{path!r}: frame {lo + int(bad[0])} cannot be decoded: {jpeg.scan_refusal_name(pst[bad[0]])}")
    raise RuntimeError(f"{path!r}: frames {lo}..{lo + len(part) - 1} cannot be decoded: {fallback}")


def _y4m_source(path):
    """The y4m.Reader of `path` where it is a YUV4MPEG2 source (a Reader, "-", or a file that starts with the signature), else None."""
    from . import y4m
    if isinstance(path, y4m.Reader):
        return path
    if isinstance(path, (str, os.PathLike)) and (os.fspath(path) == "-" or y4m.is_y4m(path)):
        return y4m.Reader(path)
    return None


def read_y4m(reader, device, max_w=800, max_h=450, bgr=False, max_bytes=16 << 30, matrix="601", full_range=None, fused=None):
    """read_video's YUV4MPEG2 arm: `reader` is a y4m.Reader -> (frames u8[F,h,w,3] on `device`, fps), (w, h) = target_size of the
    stream's own size, downscaled by the same contract as an AVI's frames (in the conversion kernel itself unless fused=False).
    A stream that ends inside a frame raises ValueError naming the frame's index."""
    from . import y4m
    w, h = target_size(reader.width, reader.height, max_w, max_h)
    if h < 1 or w < 1:
        raise ValueError(f"{reader.path!r}: {reader.width} x {reader.height} frames would become {w} x {h}")
    frames = y4m.decode(reader, device, matrix=matrix, full_range=full_range, bgr=bgr, size=(h, w), fused=fused, max_bytes=max_bytes)
    if frames.shape[0] == 0:
        raise ValueError(f"{reader.path!r}: the video stream holds no frames")
    return frames, float(reader.fps)


def read_video(path, device, max_w=800, max_h=450, bgr=False, max_bytes=16 << 30, entropy="auto", progressive=False, matrix="601"):
    """A YUV4MPEG2 stream (a path, a y4m.Reader, or "-" for standard input) goes to read_y4m with `matrix` ("601" | "709" | "auto").
    A Motion-JPEG AVI -> (frames u8[F,h,w,3] on `device`, fps): demuxed on the host, decoded on the GPU at the source size,
    chunk by chunk into one reused buffer, each chunk downscaled into its slice of the result ((w, h) = target_size of the first
    frame's own size).  RGB, or BGR with bgr=True.  A refused or damaged frame raises RuntimeError naming its index in the file
    and the reason; a file that is no Motion-JPEG AVI raises ValueError (mjpeg.AviReader).  `path` may be an AviReader already made.
    `entropy` is jpeg.decode_files' ("auto" | "serial" | "sync"), and so is `progressive`: False refuses a progressive frame by
    name, True decodes it (pr_jpeg_decode_scans)."""
    device = _media.cuda_device(device, "read_video", "decoding and resizing run")
    y4m_reader = None if isinstance(path, mjpeg.AviReader) else _y4m_source(path)
    if y4m_reader is not None:
        return read_y4m(y4m_reader, device, max_w=max_w, max_h=max_h, bgr=bgr, max_bytes=max_bytes, matrix=matrix)
    reader = path if isinstance(path, mjpeg.AviReader) else mjpeg.AviReader(path)
    path = reader.path
    blobs = reader.frames()
    F = len(blobs)
    if F == 0:
        raise ValueError(f"{path!r}: the video stream holds no frames")
    _, _, _, pst, H, W, *_ = jpeg.parse_scans(blobs[:1]) if progressive else jpeg.parse(blobs[:1])
    if pst[0]:
        raise RuntimeError(f"{path!r}: frame 0 cannot be decoded: {jpeg.scan_refusal_name(pst[0])}")
    w, h = target_size(W, H, max_w, max_h)
    if h < 1 or w < 1:
        raise ValueError(f"{path!r}: {W} x {H} frames would become {w} x {h}")
    same = (h, w) == (H, W)
    n = min(chunk_frames(H, W, int(max_bytes), 0 if entropy == "serial" else max(map(len, blobs))), F)
    with torch.cuda.device(device):
        result = torch.empty((F, h, w, 3), dtype=torch.uint8, device=device)
        buffer = None if same else torch.empty((n, H, W, 3), dtype=torch.uint8, device=device)
        for lo in range(0, F, n):
            part = blobs[lo:lo + n]
            m = len(part)
            into = result[lo:lo + m] if same else buffer[:m]
            try:
                _, status = jpeg.decode_files(part, device, bgr=bgr, chunk=m, out=into, entropy=entropy, progressive=progressive)
            except (ValueError, _lib.PoseRiskHipError) as e:     # the chunk's first accepted frame has another size, or none was accepted
                _raise_refused(path, part, lo, H, W, str(e), progressive)
            bad = jpeg.bad_frames(part, status, progressive=progressive)
            if bad:
                raise RuntimeError(f"{path!r}: frame {lo + bad[0][0]} cannot be decoded: {bad[0][1]}"
                                   + (f" (and {len(bad) - 1} more frames of its chunk)" if len(bad) > 1 else ""))
            if not same:
                resize_frames(into, h, w, out=result[lo:lo + m])
    return result, float(reader.fps)


def write_frame_folder(frames, out_dir, quality=95, fps=None, bgr=False, chunk=64):
    """u8[F,H,W,3] on the device -> out_dir/%09d.jpg (4:2:0, a restart marker per MCU row, encoded on the GPU) and, with `fps`,
    fps.txt.  Returns the files' bytes in frame order."""
    os.makedirs(out_dir, exist_ok=True)
    F, H, W, _ = frames.shape
    files = []
    encode = lambda images, capacity: jpeg.encode_frames(images, quality=quality, subsampling="4:2:0", restart_rows=1, bgr=bgr,
                                                         capacity=capacity)
    for lo in range(0, F, chunk):
        part = _media.encode_files(encode, frames[lo:lo + chunk], None, jpeg.encode_bound(H, W, "4:2:0", -1), "jpeg.encode_frames")
        for i, data in enumerate(part, lo):
            with open(os.path.join(out_dir, "{0:09d}.jpg".format(i)), "wb") as f:
                f.write(data)
            files.append(data)
    if fps is not None:
        with open(os.path.join(out_dir, "fps.txt"), "w") as f:
            f.write(repr(float(fps)))
    return files


def prepare(path, out_dir, quality=95, device=None, max_w=800, max_h=450, max_bytes=16 << 30, progressive=False, matrix="601"):
    """A Motion-JPEG AVI or a YUV4MPEG2 stream (read_video's inputs) -> out_dir/%09d.jpg + fps.txt: the folder the reference's front end leaves for its tracker (quality 95 is
    cv2.imwrite's default), written without OpenCV.  Returns (number of frames, (w, h), fps)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    frames, fps = read_video(path, device, max_w=max_w, max_h=max_h, max_bytes=max_bytes, progressive=progressive, matrix=matrix)
    write_frame_folder(frames, out_dir, quality=quality, fps=fps)
    return int(frames.shape[0]), (int(frames.shape[2]), int(frames.shape[1])), fps


def track(path, weights, out=None, device=None, img_size=(416, 416), conf_thres=0.1, nms_thres=0.4, max_age=1, min_hits=3, iou_thres=0.3,
          batch=8, max_w=800, max_h=450, matrix="601", precision="fp32"):
    """A Motion-JPEG AVI or a YUV4MPEG2 stream (read_video's inputs) -> `out` (default `<stem>.tracking.pkl` beside the video):
    multi_person_tracker's dict, boxes in the downscaled frames' coordinates, made by this package's own detector (YOLOv3 on the
    GPU, `weights` = a darknet yolov3.weights file; precision 'fp32' | 'bf16') and SORT.  Returns (out, the dict, number of frames)."""
    import pickle
    from . import detector, sort
    detector.check_precision(precision)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    frames, _ = read_video(path, device, max_w=max_w, max_h=max_h, progressive=True, matrix=matrix)
    det = detector.Detector(weights, img_size=img_size, device=device, max_batch=batch, precision=precision)
    dets = det.detect(frames, conf_thres=conf_thres, nms_thres=nms_thres)
    det.close()
    tracking = sort.track_frames(dets, max_age=max_age, min_hits=min_hits, iou_thres=iou_thres)
    if not tracking:
        raise RuntimeError(f"{path!r}: no person track in {len(dets)} frames ({sum(len(d) for d in dets)} detections at conf_thres "
                           f"{conf_thres:g}, nms_thres {nms_thres:g}; a track needs {min_hits} consecutive hits)")
    out = out or os.path.splitext(os.fspath(path))[0] + ".tracking.pkl"
    with open(out, "wb") as f:
        pickle.dump(tracking, f)
    return out, tracking, len(dets)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m poserisk_release_amd.frontend")
    sub = ap.add_subparsers(dest="command", required=True)
    p = sub.add_parser("prepare", help="Motion-JPEG AVI, .y4m file or - (a YUV4MPEG2 stream on standard input) -> a folder of %%09d.jpg + fps.txt for a tracker and for Predictor")
    p.add_argument("video")
    p.add_argument("out_dir")
    p.add_argument("--quality", type=int, default=95)
    p.add_argument("--max-w", type=int, default=800)
    p.add_argument("--max-h", type=int, default=450)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--matrix", choices=("601", "709", "auto"), default="601",
                   help="the colour matrix of a YUV4MPEG2 input (auto: 709 above 576 rows); a Motion-JPEG AVI ignores it")
    t = sub.add_parser("track", help="Motion-JPEG AVI or .y4m file -> <stem>.tracking.pkl by the built-in detector (YOLOv3) and SORT")
    t.add_argument("video")
    t.add_argument("out", nargs="?", default=None)
    t.add_argument("--weights", required=True, help="a darknet yolov3.weights file")
    t.add_argument("--img-size", type=int, nargs=2, default=(416, 416), metavar=("ROWS", "COLUMNS"))
    t.add_argument("--conf-thres", type=float, default=0.1)
    t.add_argument("--nms-thres", type=float, default=0.4)
    t.add_argument("--batch", type=int, default=8)
    t.add_argument("--gpu", type=int, default=0)
    t.add_argument("--precision", choices=("fp32", "bf16"), default="fp32", help="the detector's arithmetic (bf16: faster; its agreement "
                   "with fp32 on trained weights is unmeasured: python -m poserisk_release_amd.detector compare)")
    a = ap.parse_args(argv)
    if a.command == "track":
        out, tracking, n = track(a.video, a.weights, a.out, device=torch.device("cuda", a.gpu), img_size=tuple(a.img_size),
                                 conf_thres=a.conf_thres, nms_thres=a.nms_thres, batch=a.batch, precision=a.precision)
        print(f"{out}: {len(tracking)} tracks over {n} frames")
        return
    n, (w, h), fps = prepare(a.video, a.out_dir, quality=a.quality, device=torch.device("cuda", a.gpu), max_w=a.max_w, max_h=a.max_h,
                             progressive=True, matrix=a.matrix)
    print(f"{a.out_dir}: {n} frames of {w} x {h} at {fps:g} frames/s; add tracking.pkl (multi_person_tracker's dict) to score it")


if __name__ == "__main__":
    main()
