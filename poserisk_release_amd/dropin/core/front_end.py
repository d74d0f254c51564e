"""Where Predictor.__call__'s frames and tracking come from (the reference's DataProcessing, lib/core/base.py:34-74): `load_front_end`
routes an input path to a folder of decoded or encoded frames, a Motion-JPEG AVI, a YUV4MPEG2 file, a decoder child or the reference's
own cv2 + multi_person_tracker path, and `track_frames` is this package's own detector and tracker.  Plain functions of the predictor
(`pred`: its device and its video_decoder knob, read when called); they call back into it by its public names only."""
import os
import os.path as osp

import numpy as np
import torch

from core.config import cfg


def _jpeg_options():                                   # what every jpeg.decode_files call of the front end takes from cfg.DATASET
    return dict(entropy=cfg.DATASET.get('jpeg_entropy', 'auto'), progressive=bool(cfg.DATASET.get('jpeg_progressive', True)))


def _front_limits():                                   # the front end's downscale rule (frontend.target_size) from cfg.DATASET
    return dict(max_w=cfg.DATASET.get('front_max_w', 800), max_h=cfg.DATASET.get('front_max_h', 450))


def _yuv_matrix():                                     # the Y'CbCr matrix of the YUV4MPEG2 reader from cfg.DATASET (the sink's too)
    return str(cfg.DATASET.get('yuv_matrix', '601'))


def _tracker_weights():
    return str(cfg.get('TRACKER', {}).get('weights', '') or '')


def _reference_tracker():
    """-> multi_person_tracker's MPT with the reference's arguments (base.py:38-46), still to be given `device=`.  ImportError where
    the package is not importable."""
    import functools
    from multi_person_tracker import MPT
    return functools.partial(MPT, batch_size=8, display=False, detection_threshold=0.1, detector_type='yolo', output_format='dict',
                             yolo_img_size=416)


def _folder_sidecars(pred, folder, frames=None):
    """What every frame folder carries beside its frames -> (fps, tracking): `fps.txt` (optional, 30.0 without it) and
    `tracking.pkl`; without that file and with cfg.TRACKER.weights set, the built-in tracker's dict for `frames`."""
    import pickle
    if frames is not None and _tracker_weights() and not osp.isfile(osp.join(folder, 'tracking.pkl')):
        tracking = pred.track_frames(frames, bgr=False)
    else:
        with open(osp.join(folder, 'tracking.pkl'), 'rb') as f:
            tracking = pickle.load(f)
    fps_file = osp.join(folder, 'fps.txt')
    fps = float(open(fps_file).read()) if osp.isfile(fps_file) else 30.0
    return fps, tracking


def load_front_end(pred, input_path, output_path, tracking_results=None):
    """Decoded frames + tracker output for `input_path` -> (frames u8[F,H,W,3], bgr, fps, tracking dict).

    Video decoding and multi-person tracking are outside the accelerated path; this only finds them:
      1. a directory with `frames.npy` (uint8 [F,H,W,3] RGB) and `tracking.pkl` (multi_person_tracker's
         dict {id: {'bbox': [n,4] (cx,cy,w,h), 'frames': [n]}}), optional `fps.txt`;
      2. a directory without `frames.npy` but with JPEG frames (`*.jpg` / `*.jpeg`, sorted by name: what the reference's
         front end leaves under <output>/tmp, what `ffmpeg -i video %09d.jpg` or a camera writes) and `tracking.pkl`,
         optional `fps.txt`: the files are decoded on the GPU, bit-exact with cv2.imread's pixels
         (poserisk_release_amd/jpeg.py), and the frames come back as a device tensor, RGB.  A frame that is not
         baseline JPEG, has another size than the first or is damaged raises, naming the file and the reason;
      2b. a directory without `frames.npy`, with `tracking.pkl`, at least one `*.png` name and no `*.jpg` / `*.jpeg` name
         (what `ffmpeg -i video %09d.png`, screen recorders and this package's own report path write): the files are
         decoded on the GPU, exact with zlib and libpng (poserisk_release_amd/png.py), RGB on the device, gray replicated
         and alpha dropped; optional `fps.txt`.  A file that is not an 8-bit non-interlaced PNG, has another size than
         the first or is damaged raises, naming the file and the reason.  A folder that mixes the two kinds of names
         goes to 2 and is refused there;
      3. a Motion-JPEG AVI file (a camera's, `ffmpeg -c:v mjpeg`'s, this package's own <TITLE>_video.avi): demuxed in
         Python, decoded and downscaled on the GPU by the reference's rule (poserisk_release_amd/frontend.py;
         cfg.DATASET.front_max_w / front_max_h), no OpenCV anywhere.  Its tracking is, in this order, the
         `tracking_results` given to __call__, `<stem>.tracking.pkl` beside the video (boxes in the downscaled frames'
         coordinates), or multi_person_tracker where importable, run on a folder of JPEGs encoded on the GPU; the frames
         are then the pixels decoded back from those files, as the reference's CropDataset would read them.  An AVI of
         another codec, or a damaged one, goes on to 3c and 4;
      3b. a YUV4MPEG2 file (one that starts with `YUV4MPEG2 `: what `ffmpeg -f yuv4mpegpipe`, mpv, x264 and the AV1 tools
         write): read in chunks into pinned memory, converted to RGB (cfg.DATASET.yuv_matrix, '601') and downscaled by the
         same rule in one kernel on the GPU (poserisk_release_amd/y4m.py).  Its tracking comes from the same sources as 3's,
         in the same order;
      3c. with cfg.DATASET.video_decoder / args.video_decoder set (off, '', by default), any other regular file: the knob
         is a command line containing `{input}`, e.g. `ffmpeg -v error -i {input} -f yuv4mpegpipe -pix_fmt yuv420p -`; it
         is started as a fresh child process (shlex.split, no shell), its standard output is read as YUV4MPEG2 exactly as
         3b reads a file, and it is always reaped.  A child that exits non-zero or writes no stream header raises
         RuntimeError naming the command, the exit status and the tail of its standard error;
      With cfg.TRACKER.weights set (off, '', by default) the tracking of cases 3, 3b and 3c comes from this package's own
      detector and tracker (`track_frames`: YOLOv3 on the GPU + SORT) after the dict given and the sidecar and before
      multi_person_tracker, and the folders of cases 1, 2 and 2b are accepted without `tracking.pkl`;
      4. otherwise the reference's own front end when `cv2` and `multi_person_tracker` are importable:
         frames are decoded and resized as funcs_utils.get_images does (width <= 800, else height <= 450),
         written as JPEGs under <output>/tmp for the tracker (base.py:47-56) and read back, so the crops see
         the same JPEG-decoded pixels as the reference's CropDataset."""
    if osp.isdir(input_path) and osp.isfile(osp.join(input_path, 'frames.npy')):
        frames = np.load(osp.join(input_path, 'frames.npy'))
        return (frames, False) + _folder_sidecars(pred, input_path, frames)
    if osp.isdir(input_path) and (osp.isfile(osp.join(input_path, 'tracking.pkl')) or _tracker_weights()):
        from poserisk_release_amd import jpeg, png
        module, opts = jpeg, _jpeg_options()
        if png.list_frames(input_path) and not any(n.lower().endswith(('.jpg', '.jpeg')) for n in os.listdir(input_path)):
            module, opts = png, {}
        names = module.list_frames(input_path)
        if names:
            frames = _decode_frames(pred, module, [osp.join(input_path, n) for n in names], **opts)
            return (frames, False) + _folder_sidecars(pred, input_path, frames)
    not_mjpeg = None
    if osp.isfile(input_path):
        from poserisk_release_amd import mjpeg, y4m
        if mjpeg.is_avi(input_path):
            try:
                reader = mjpeg.AviReader(input_path)
            except ValueError as e:
                not_mjpeg = e                              # an AVI, but not one to read here: cv2 may still open it
            else:
                return _video_front_end(pred, reader, input_path, output_path, tracking_results, **_jpeg_options())
        if y4m.is_y4m(input_path):
            with y4m.Reader(input_path) as reader:
                return _video_front_end(pred, reader, input_path, output_path, tracking_results, matrix=_yuv_matrix())
        if pred.video_decoder:
            return _decoder_front_end(pred, input_path, output_path, tracking_results)
    try:
        import cv2
        new_tracker = _reference_tracker()
    except ImportError as e:
        raise RuntimeError(
            f"{input_path!r} is neither a directory with frames.npy + tracking.pkl nor one with JPEG frames "
            f"(*.jpg, decoded on the GPU) or PNG frames (*.png, decoded on the GPU) + tracking.pkl, and the reference's front end "
            f"(cv2 video decoding, multi_person_tracker) is not importable here ({e}); decode and track outside, "
            "then call Predictor.score_frames(frames, tracking_results, info)"
            + (f" [as a Motion-JPEG AVI it was refused: {not_mjpeg}]" if not_mjpeg is not None else "")) from e
    import shutil
    image_path = osp.join(output_path, 'tmp')
    shutil.rmtree(image_path, ignore_errors=True)
    os.makedirs(image_path, exist_ok=True)
    cap = cv2.VideoCapture(input_path)
    fps = cap.get(cv2.CAP_PROP_FPS)
    width, height = cap.get(cv2.CAP_PROP_FRAME_WIDTH), cap.get(cv2.CAP_PROP_FRAME_HEIGHT)
    if width > 800:
        width, height = 800, int(height * 800 / width)
    elif height > 450:
        width, height = int(width * 450 / height), 450
    n = 0
    while cap.isOpened():
        ok, frame = cap.read()
        if not ok:
            break
        cv2.imwrite(osp.join(image_path, '{0:09d}.jpg'.format(n)), cv2.resize(frame, (int(width), int(height))))
        n += 1
    cap.release()
    tracking = new_tracker(device=pred.device)(image_path)
    frames = np.stack([cv2.imread(osp.join(image_path, '{0:09d}.jpg'.format(i))) for i in range(n)])
    shutil.rmtree(image_path, ignore_errors=True)
    return frames, True, fps, tracking


def _decode_frames(pred, module, paths, written_to=None, **opts):
    """`paths` (files, or their bytes) decoded by `module` (jpeg | png: decode_files with `opts`) -> the frames on the device.  The
    first bad frame raises RuntimeError naming its file -- for bytes written to a tracker's folder `written_to`, its number there."""
    frames, status = module.decode_files(paths, pred.device, **opts)
    bad = module.bad_frames(paths, status, **{k: opts[k] for k in ('progressive',) if k in opts})
    if bad and written_to is not None:
        raise RuntimeError(f"{written_to!r}: frame {bad[0][0]} written for the tracker cannot be decoded: {bad[0][1]}")
    if bad:
        raise RuntimeError(f"{paths[bad[0][0]]!r} cannot be decoded: {bad[0][1]}"
                           + (f" (and {len(bad) - 1} more frames)" if len(bad) > 1 else ""))
    return frames


def _video_front_end(pred, reader, input_path, output_path, tracking_results=None, **opts):
    """load_front_end's cases 3, 3b and 3c: `reader` is the mjpeg.AviReader of `input_path` (`opts`: the JPEG options), or the
    y4m.Reader of `input_path` or of a decoder's standard output (`opts`: the colour matrix)."""
    from poserisk_release_amd import frontend
    frames, fps = frontend.read_video(reader, pred.device, **_front_limits(), **opts)
    return _tracking_for(pred, frames, fps, input_path, output_path, tracking_results)


def _decoder_front_end(pred, input_path, output_path, tracking_results=None):
    """load_front_end's case 3c: pred.video_decoder, with {input} replaced, runs as a child process whose standard output
    is read as YUV4MPEG2.  Never a shell and never this process's own program; the child is reaped whatever happens."""
    import shlex
    from poserisk_release_amd import _child, y4m
    if '{input}' not in pred.video_decoder:
        raise ValueError(f"video_decoder {pred.video_decoder!r} must be a command line containing {{input}}")
    child = _child.Child([a.replace('{input}', input_path) for a in shlex.split(pred.video_decoder)],
                         f"{input_path!r}: the video decoder", feed=False)
    failure, read_to_the_end = None, False
    try:
        try:
            reader = y4m.Reader(child.pipe)
        except ValueError as e:
            failure = f"it wrote no YUV4MPEG2 stream header ({e})"
        else:
            try:
                return_value = _video_front_end(pred, reader, input_path, output_path, tracking_results, matrix=_yuv_matrix())
                read_to_the_end = True
            except ValueError as e:                         # the stream broke off: the child's status says why
                failure = str(e)
    finally:
        child.pipe.close()                  # a child still writing gets EPIPE and ends by itself; its status raises nothing
        child.finish(60 if read_to_the_end else 5, failure, raising=read_to_the_end or failure is not None)    # over another error
    return return_value


# ---- the built-in tracker (cfg.TRACKER; off while its weights are '') --------------------------------------------------
def track_frames(pred, frames, bgr=False):
    """frames u8[F,H,W,3] (device tensor or numpy) -> multi_person_tracker's dict, by this package's own detector
    (poserisk_release_amd.detector, YOLOv3 on the GPU; kept on `pred` until a cfg.TRACKER knob it was built from changes) and
    tracker (poserisk_release_amd.sort).  No person found anywhere raises RuntimeError naming the threshold used."""
    from poserisk_release_amd import detector, sort
    t = cfg.TRACKER
    key = (_tracker_weights(), tuple(t.img_size), int(t.batch), str(t.get('precision', 'fp32')))
    detector.check_precision(key[3])        # 'fp32' | 'bf16', anything else raises naming the two
    if pred._detector is None or pred._detector_key != key:
        pred._detector = detector.Detector(key[0], img_size=key[1], device=pred.device, max_batch=key[2], precision=key[3])
        pred._detector_key = key
    dets = pred._detector.detect(frames, bgr=bgr, conf_thres=float(t.conf_thres), nms_thres=float(t.nms_thres))
    tracking = sort.track_frames(dets, max_age=int(t.max_age), min_hits=int(t.min_hits), iou_thres=float(t.iou_thres))
    if not tracking:
        raise RuntimeError(f"the built-in tracker found no person track in {len(dets)} frames ({sum(len(d) for d in dets)} "
                           f"detections at conf_thres {float(t.conf_thres):g}, nms_thres {float(t.nms_thres):g}; a track needs "
                           f"{int(t.min_hits)} consecutive hits)")
    return tracking


def _tracking_for(pred, frames, fps, input_path, output_path, tracking_results=None):
    """The second half of cases 3, 3b and 3c: the tracking of a video file's decoded, downscaled `frames`, in this order: the
    `tracking_results` given, `<stem>.tracking.pkl`, the built-in tracker where cfg.TRACKER.weights names a weight file,
    multi_person_tracker where importable, else the named error."""
    import pickle
    import shutil
    from poserisk_release_amd import frontend, jpeg
    if tracking_results is not None:
        return frames, False, fps, tracking_results
    sidecar = osp.splitext(input_path)[0] + '.tracking.pkl'
    if osp.isfile(sidecar):
        with open(sidecar, 'rb') as f:
            return frames, False, fps, pickle.load(f)
    if _tracker_weights():
        return frames, False, fps, pred.track_frames(frames, bgr=False)
    try:
        new_tracker = _reference_tracker()
    except ImportError as e:
        raise RuntimeError(
            f"{input_path!r}: {frames.shape[0]} frames of {frames.shape[2]} x {frames.shape[1]} were decoded, but there is no "
            f"tracking for them: {sidecar!r} (multi_person_tracker's dict, boxes in the downscaled frames' coordinates) does not "
            f"exist, no tracking_results were given and multi_person_tracker is not importable here ({e}).  Write the frames for "
            f"a tracker with `python -m poserisk_release_amd.frontend prepare {input_path} <dir>`, add its tracking.pkl to <dir> "
            "and pass <dir>") from e
    image_path = osp.join(output_path, 'tmp')
    shutil.rmtree(image_path, ignore_errors=True)
    try:
        files = frontend.write_frame_folder(frames, image_path, quality=95)      # cv2.imwrite's default quality
        tracking = new_tracker(device=pred.device)(image_path)
        frames = _decode_frames(pred, jpeg, files, written_to=image_path, **_jpeg_options())
    finally:
        shutil.rmtree(image_path, ignore_errors=True)
    return frames, False, fps, tracking


def load_on_rank0(pred, input_path, output_path, rank, **given):
    """Several ranks (one per GPU): the front end writes, runs the tracker in and deletes <output>/tmp, so it runs on
    rank 0 ONLY and its output is broadcast -- every rank then shards the SAME track (a tracker run per rank may select
    different tracks; one rank's rmtree would delete JPEGs another rank is still reading).  The metadata goes as one
    pickled object, the frames as one uint8 tensor (on this rank's GPU with RCCL, on the host with gloo)."""
    import torch.distributed as dist
    meta, err = [None], None
    frames = None
    if rank == 0:
        try:
            frames, bgr, fps, tracking = pred.load_front_end(input_path, output_path, **given)
            # a device tensor (the JPEG folder case) stays where it is; arrays become one contiguous host tensor
            frames = frames.contiguous() if isinstance(frames, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(frames))
            meta = [dict(shape=tuple(frames.shape), bgr=bool(bgr), fps=float(fps), tracking=tracking)]
        except Exception as e:               # the other ranks are waiting in the broadcast: tell them, then raise
            meta, err = [dict(error=f"{type(e).__name__}: {e}")], e
    dist.broadcast_object_list(meta, src=0)
    m = meta[0]
    if 'error' in m:
        raise err if err is not None else RuntimeError(f"rank 0's front end failed: {m['error']}")
    on_gpu = dist.get_backend() == 'nccl'
    if rank != 0:
        frames = torch.empty(m['shape'], dtype=torch.uint8, device=pred.device if on_gpu else 'cpu')
    elif on_gpu:
        frames = frames.to(pred.device)
    else:
        frames = frames.cpu()                    # gloo broadcasts host memory
    dist.broadcast(frames, src=0)
    return frames, m['bgr'], m['fps'], m['tracking']
