"""The person detector (include/poserisk_hip.h, section j8): YOLOv3 on the GPU, the half of multi_person_tracker that finds
people (lib/core/base.py:38-46,59); sort.py is the half that follows them.

    yolo_layers()    the topology of darknet's yolov3.cfg as a list of dicts, in pure Python (synth.yolo_weights and
                     tests/det_ref.py walk it; tests compare it with the library's own table, pr_det_topology)
    load_darknet     a darknet weight file -> its float body, checked against the topology
    save_darknet     the reverse (what the tests and synth use to make a file)
    fold_pack_bf16   the bf16 contract's packed blob (pr_det_fold_pack_bf16), as bytes
    Detector         the handle (precision "fp32" | "bf16"): letterbox, network, network_until, postprocess, detect_raw on device tensors, and
                     detect(frames) -> one array of boxes per frame

`img_size` is (S_h, S_w), rows first, each a multiple of 32: (416, 416) is the reference's yolo_img_size; (256, 416) suits
800 x 450 frames at 0.62 of the work."""
import ctypes as C
import warnings

import numpy as np

from . import _lib

CONV, SHORTCUT, ROUTE, UPSAMPLE, YOLO = range(5)
NUM_LAYERS = 107
WEIGHT_FLOATS = 62001757
HEAD_LAYERS = (82, 94, 106)
STRIDES = (32, 16, 8)
ANCHORS = ((10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326))
ANCHOR_MASKS = ((6, 7, 8), (3, 4, 5), (0, 1, 2))
MAX_CAND = 1024
PRECISIONS = {"fp32": 0, "bf16": 1}
STATUS_CAND_OVERFLOW, STATUS_DET_OVERFLOW, STATUS_NONFINITE = 1, 2, 4


def status_text(status, conf_thres, max_det):
    """A frame's status word -> what happened to it, every set bit named ('' for 0; a bit this module does not know by its number)."""
    status = int(status)
    parts = []
    if status & STATUS_CAND_OVERFLOW:
        parts.append("more than %d candidates above conf_thres %g" % (MAX_CAND, conf_thres))
    if status & STATUS_DET_OVERFLOW:
        parts.append("more than %d boxes after NMS" % max_det)
    if status & STATUS_NONFINITE:
        parts.append("a head value that is not finite (NaN or infinite) took at least one cell out")
    rest = status & ~(STATUS_CAND_OVERFLOW | STATUS_DET_OVERFLOW | STATUS_NONFINITE)
    if rest:
        parts.append("unknown status bits 0x%x" % rest)
    return "; ".join(parts)


def yolo_layers():
    """[{type, cin, cout, ksize, stride, bn, from (absolute indices), down}] for layers 0..106."""
    L = []

    def add(type, **kw):
        prev = L[-1] if L else {"cout": 3, "down": 1}
        d = {"type": type, "cin": prev["cout"], "cout": prev["cout"], "ksize": 0, "stride": 0, "bn": 0, "from": (), "down": prev["down"]}
        d.update(kw)
        L.append(d)

    def conv(filters, k, stride=1, bn=1):
        add(CONV, cout=filters, ksize=k, stride=stride, bn=bn, down=(L[-1]["down"] if L else 1) * stride)

    def block(planes, n):
        for _ in range(n):
            conv(planes // 2, 1), conv(planes, 3), add(SHORTCUT, **{"from": (len(L) - 3,)})

    def route(*src):
        add(ROUTE, cin=sum(L[s]["cout"] for s in src), cout=sum(L[s]["cout"] for s in src), down=L[src[0]]["down"], **{"from": src})

    def neck(planes):
        for _ in range(3):
            conv(planes, 1), conv(2 * planes, 3)
        conv(255, 1, bn=0), add(YOLO)

    conv(32, 3)
    for planes, n in ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4)):
        conv(planes, 3, 2), block(planes, n)
    neck(512)
    route(len(L) - 4), conv(256, 1), add(UPSAMPLE, stride=2, down=L[-1]["down"] // 2), route(len(L) - 1, 61)
    neck(256)
    route(len(L) - 4), conv(128, 1), add(UPSAMPLE, stride=2, down=L[-1]["down"] // 2), route(len(L) - 1, 36)
    neck(128)
    assert len(L) == NUM_LAYERS
    return L


def weight_floats(layers=None):
    """Floats of the darknet body the layers read: per BatchNorm convolution 4 O + O I k k, per head convolution O + O I k k."""
    layers = yolo_layers() if layers is None else layers
    return sum(l["cout"] * (4 if l["bn"] else 1) + l["cout"] * l["cin"] * l["ksize"] ** 2 for l in layers if l["type"] == CONV)


def load_darknet(path):
    """A darknet weight file -> its float body f32[62001757], unchanged.  Header: major, minor, revision as int32, then `seen`
    as int64 when major * 10 + minor >= 2, else int32.  A header that is not one, or a body of another length than the
    topology's, is refused by name."""
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) < 16:
        raise ValueError(f"{path!r}: {len(blob)} bytes are no darknet weight file (the header alone has 16 or 20)")
    major, minor, revision = (int(v) for v in np.frombuffer(blob, "<i4", 3))
    if not (0 <= major <= 100 and 0 <= minor <= 1000 and 0 <= revision <= 100000):
        raise ValueError(f"{path!r}: bad darknet header (version {major}.{minor}.{revision})")
    head = 12 + (8 if major * 10 + minor >= 2 else 4)
    body = blob[head:]
    if len(body) != 4 * WEIGHT_FLOATS:
        raise ValueError(f"{path!r}: the body holds {len(body) / 4:g} floats, YOLOv3 with 80 classes holds {WEIGHT_FLOATS} "
                         f"(header version {major}.{minor}.{revision}, {head} bytes)")
    return np.frombuffer(body, "<f4").astype(np.float32, copy=False)


def save_darknet(path, weights, version=(0, 2, 0), seen=0):
    weights = np.ascontiguousarray(weights, "<f4")
    with open(path, "wb") as f:
        f.write(np.asarray(version, "<i4").tobytes())
        f.write(np.asarray([seen], "<i8" if version[0] * 10 + version[1] >= 2 else "<i4").tobytes())
        f.write(weights.tobytes())


def topology(n_layers=NUM_LAYERS):
    """pr_det_topology -> a list of dicts (the library's own table, packed offsets included)."""
    arr = (_lib.DetLayer * n_layers)()
    _lib.check(_lib.load().pr_det_topology(int(n_layers), arr), "pr_det_topology")
    return [{n: getattr(a, n) for n, _ in _lib.DetLayer._fields_} for a in arr]


def fold_pack(weights, n_layers=NUM_LAYERS, bn_eps=1e-5):
    """pr_det_fold_pack on the host -> the packed blob f32[pr_det_packed_floats(n_layers)]."""
    lib = _lib.load()
    weights = np.ascontiguousarray(weights, np.float32)
    out = np.empty(lib.pr_det_packed_floats(int(n_layers)), np.float32)
    _lib.check(lib.pr_det_fold_pack(int(n_layers), weights.ctypes.data_as(C.c_void_p), weights.size, float(bn_eps),
                                    out.ctypes.data_as(C.c_void_p), out.size), "pr_det_fold_pack")
    return out


def fold_pack_bf16(weights, n_layers=NUM_LAYERS, bn_eps=1e-5):
    """pr_det_fold_pack_bf16 on the host -> the packed blob u8[pr_det_packed_bytes_bf16(n_layers)]: per convolution bias f32[cout_pad],
    then w bf16[cout_pad][kpad] (layer 0: w f32), BatchNorm folded in float64 and rounded to nearest even."""
    lib = _lib.load()
    weights = np.ascontiguousarray(weights, np.float32)
    out = np.empty(lib.pr_det_packed_bytes_bf16(int(n_layers)), np.uint8)
    _lib.check(lib.pr_det_fold_pack_bf16(int(n_layers), weights.ctypes.data_as(C.c_void_p), weights.size, float(bn_eps),
                                         out.ctypes.data_as(C.c_void_p), out.size), "pr_det_fold_pack_bf16")
    return out


def check_precision(precision):
    """'fp32' | 'bf16' -> the library's flag; anything else raises naming the two."""
    if precision not in PRECISIONS:
        raise ValueError(f"detector precision {precision!r} unknown: one of 'fp32', 'bf16'")
    return PRECISIONS[precision]


def letterbox_geometry(H, W, S_h, S_w):
    """(h', w', ox, oy) of the header's integer rule."""
    if W * S_h >= H * S_w:
        w2, h2 = S_w, min(S_h, max(1, (2 * H * S_w + W) // (2 * W)))
    else:
        h2, w2 = S_h, min(S_w, max(1, (2 * W * S_h + H) // (2 * H)))
    return h2, w2, (S_w - w2) // 2, (S_h - h2) // 2


def unmap(boxes, count, frame_size, img_size):
    """pr_det_unmap, in place: boxes f32[B,max_det,4] (CUDA, letterbox pixels of an img_size = (S_h, S_w) input) -> frame pixels of
    frame_size = (H, W) frames, clipped, for the rows below count i32[B]; the other rows are left as they are.  The map
    detect_raw ends with, without a handle.  -> boxes."""
    import torch
    for t, dtype, what in ((boxes, torch.float32, "boxes"), (count, torch.int32, "count")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous {dtype} CUDA tensor")
    if boxes.dim() != 3 or boxes.shape[2] != 4 or tuple(count.shape) != (boxes.shape[0],) or count.device != boxes.device:
        raise ValueError(f"boxes must be [B, max_det, 4] and count [B] on one device, got {tuple(boxes.shape)} and {tuple(count.shape)}")
    (H, W), (S_h, S_w) = frame_size, img_size
    with torch.cuda.device(boxes.device):
        _lib.check(_lib.load().pr_det_unmap(boxes.data_ptr(), count.data_ptr(), boxes.shape[0], boxes.shape[1], int(H), int(W), int(S_h), int(S_w),
                                    torch.cuda.current_stream(boxes.device).cuda_stream), "pr_det_unmap")
    return boxes


class Detector:
    """weights: a darknet file's path or its float body.  Every method works on CUDA tensors of `device`, asynchronously on
    the current stream; detect() alone copies to the host.  precision: 'fp32' (default) or 'bf16' (include/poserisk_hip.h, j8,
    paragraph "bf16": bf16 activations and weights, fp32 accumulation, fp32 head tensors; inputs and outputs keep their types)."""

    def __init__(self, weights, img_size=(416, 416), device=None, max_batch=8, bn_eps=1e-5, max_det=100, precision="fp32"):
        import torch
        self.precision = precision
        flag = check_precision(precision)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PoseRiskHipError("Detector: the detector runs on the GPU only (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        body = load_darknet(weights) if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__") else weights
        body = np.ascontiguousarray(body, np.float32)
        self.S_h, self.S_w = (int(img_size), int(img_size)) if np.isscalar(img_size) else (int(img_size[0]), int(img_size[1]))
        self.max_batch, self.max_det = int(max_batch), int(max_det)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            lib = _lib.declare_stream(self.device)
            _lib.check(lib.pr_det_create_p(self.device.index, body.ctypes.data_as(C.c_void_p), body.size, self.S_h, self.S_w,
                                           self.max_batch, float(bn_eps), flag, C.byref(self._h)), "pr_det_create_p")
        self.grids = [(self.S_h // s, self.S_w // s) for s in STRIDES]

    def close(self):
        if getattr(self, "_h", None):
            import torch
            with torch.cuda.device(self.device):
                torch.cuda.synchronize(self.device)
                _lib.check(_lib.declare_stream(self.device).pr_det_destroy(self._h), "pr_det_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, t, dtype, what):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == self.device and t.dtype == dtype and t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous {dtype} tensor on {self.device}")
        return t

    def _out(self, out, shape, dtype, what):
        import torch
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if tuple(out.shape) != tuple(shape):
            raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(out.shape)}")
        return self._check(out, dtype, what)

    def layer_shape(self, layer):
        gh, gw, ch = C.c_int(), C.c_int(), C.c_int()
        _lib.check(_lib.load().pr_det_grid(self._h, int(layer), C.byref(gh), C.byref(gw), C.byref(ch)), "pr_det_grid")
        return gh.value, gw.value, ch.value

    def layer_dtype(self, layer):
        """The dtype network_until returns for `layer`: torch.float32, or on a bf16 handle torch.bfloat16 for every layer but the
        head convolutions and their yolo layers."""
        import torch
        return torch.bfloat16 if _lib.load().pr_det_elem_bytes(self._h, int(layer)) == 2 else torch.float32

    def letterbox(self, frames, bgr=False, out=None):
        """u8[B,H,W,3] -> f32[B,S_h,S_w,4] (R, G, B, 0)."""
        import torch
        self._check(frames, torch.uint8, "frames")
        B, H, W, _ = frames.shape
        out = self._out(out, (B, self.S_h, self.S_w, 4), torch.float32, "out")
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pr_det_letterbox(self._h, frames.data_ptr(), B, H, W, int(bool(bgr)), out.data_ptr(), self._stream()),
                       "pr_det_letterbox")
        return out

    def network(self, x, out=None):
        """f32[B,S_h,S_w,4] -> the three head tensors f32[B,gh,gw,255] (strides 32, 16, 8)."""
        import torch
        self._check(x, torch.float32, "x")
        B = x.shape[0]
        outs = [self._out(None if out is None else out[i], (B, gh, gw, 255), torch.float32, f"out[{i}]") for i, (gh, gw) in enumerate(self.grids)]
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pr_det_network(self._h, x.data_ptr(), B, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                                  self._stream()), "pr_det_network")
        return outs

    def network_until(self, x, layer, out=None):
        import torch
        self._check(x, torch.float32, "x")
        B = x.shape[0]
        out = self._out(out, (B,) + self.layer_shape(layer), self.layer_dtype(layer), "out")
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pr_det_network_until(self._h, x.data_ptr(), B, int(layer), out.data_ptr(), self._stream()),
                       "pr_det_network_until")
        return out

    def _post_outs(self, B, max_det, out):
        import torch
        out = out or {}
        return (self._out(out.get("boxes"), (B, max_det, 4), torch.float32, "boxes"), self._out(out.get("scores"), (B, max_det), torch.float32, "scores"),
                self._out(out.get("count"), (B,), torch.int32, "count"), self._out(out.get("status"), (B,), torch.int32, "status"))

    def postprocess(self, heads, conf_thres=0.1, nms_thres=0.4, max_det=None, out=None):
        """The three head tensors -> (boxes f32[B,max_det,4] in letterbox pixels, scores f32[B,max_det], count i32[B], status i32[B])."""
        import torch
        for i, t in enumerate(heads):
            self._check(t, torch.float32, f"heads[{i}]")
        B = heads[0].shape[0]
        max_det = self.max_det if max_det is None else int(max_det)
        boxes, scores, count, status = self._post_outs(B, max_det, out)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pr_det_postprocess(self._h, heads[0].data_ptr(), heads[1].data_ptr(), heads[2].data_ptr(), B,
                                                      float(conf_thres), float(nms_thres), max_det, boxes.data_ptr(), scores.data_ptr(),
                                                      count.data_ptr(), status.data_ptr(), self._stream()), "pr_det_postprocess")
        return boxes, scores, count, status

    def detect_raw(self, frames, bgr=False, conf_thres=0.1, nms_thres=0.4, max_det=None, out=None):
        """u8[B,H,W,3], B <= max_batch -> postprocess' outputs with the boxes in FRAME pixels."""
        import torch
        self._check(frames, torch.uint8, "frames")
        B, H, W, _ = frames.shape
        max_det = self.max_det if max_det is None else int(max_det)
        boxes, scores, count, status = self._post_outs(B, max_det, out)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pr_det_detect(self._h, frames.data_ptr(), B, H, W, int(bool(bgr)), float(conf_thres), float(nms_thres),
                                                 max_det, boxes.data_ptr(), scores.data_ptr(), count.data_ptr(), status.data_ptr(),
                                                 self._stream()), "pr_det_detect")
        return boxes, scores, count, status

    def detect(self, frames, bgr=False, conf_thres=0.1, nms_thres=0.4):
        """u8[F,H,W,3] (a CUDA tensor, or numpy: uploaded) -> a list of F arrays f32[n,5] (x1, y1, x2, y2, score) in frame pixels,
        best score first; runs in chunks of max_batch.  A frame with more than MAX_CAND candidates (the best MAX_CAND took
        part), more than max_det boxes or a cell taken out by a head value that is not finite is reported with a warning naming
        it (status_text), never cut silently."""
        import torch
        if not isinstance(frames, torch.Tensor):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        frames = frames.to(self.device).contiguous()
        results = []
        for lo in range(0, frames.shape[0], self.max_batch):
            part = frames[lo:lo + self.max_batch]
            boxes, scores, count, status = (t.cpu().numpy() for t in self.detect_raw(part, bgr, conf_thres, nms_thres))
            for i in range(part.shape[0]):
                if status[i]:
                    warnings.warn(f"detector: frame {lo + i}: " + status_text(status[i], conf_thres, self.max_det), RuntimeWarning)
                n = int(count[i])
                results.append(np.concatenate([boxes[i, :n], scores[i, :n, None]], axis=1).astype(np.float32))
        return results


def compare(weights, clip, img_size=(416, 416), device=None, batch=8, conf_thres=0.1, nms_thres=0.4, match_iou=0.5, report=print):
    """Both precisions on one clip (a video file frontend.read_video reads, or frames u8[F,H,W,3]): per frame and in total the boxes kept by both
    (greedy matching by IoU >= match_iou, best first), the boxes kept by one only, and the largest corner distance of matched
    boxes in frame pixels.  The way to find out how far the bf16 detector agrees with fp32 on TRAINED weights: nobody has
    measured that (no trained yolov3.weights exists where this package is built and tested)."""
    import torch
    from . import frontend
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    frames = frontend.read_video(clip, device, progressive=True)[0] if isinstance(clip, (str, bytes)) or hasattr(clip, "__fspath__") else clip
    dets = {}
    for precision in ("fp32", "bf16"):
        d = Detector(weights, img_size=img_size, device=device, max_batch=batch, precision=precision)
        dets[precision] = d.detect(frames, conf_thres=conf_thres, nms_thres=nms_thres)
        d.close()
    total = {"both": 0, "fp32_only": 0, "bf16_only": 0, "max_corner_px": 0.0}
    rows = []
    for f, (a, b) in enumerate(zip(dets["fp32"], dets["bf16"])):
        free, both, worst = list(range(len(b))), 0, 0.0
        for box in a:
            best, best_iou = -1, match_iou
            for j in free:
                iw = min(box[2], b[j][2]) - max(box[0], b[j][0])
                ih = min(box[3], b[j][3]) - max(box[1], b[j][1])
                inter = max(iw, 0.0) * max(ih, 0.0)
                union = (box[2] - box[0]) * (box[3] - box[1]) + (b[j][2] - b[j][0]) * (b[j][3] - b[j][1]) - inter
                iou = inter / union if union > 0 else 0.0
                if iou >= best_iou:
                    best, best_iou = j, iou
            if best >= 0:
                free.remove(best)
                both += 1
                worst = max(worst, float(np.abs(box[:4] - b[best][:4]).max()))
        row = {"frame": f, "both": both, "fp32_only": len(a) - both, "bf16_only": len(free), "max_corner_px": worst}
        rows.append(row)
        report("frame %(frame)d: both %(both)d, fp32 only %(fp32_only)d, bf16 only %(bf16_only)d, max corner distance %(max_corner_px).3f px" % row)
        for k in ("both", "fp32_only", "bf16_only"):
            total[k] += row[k]
        total["max_corner_px"] = max(total["max_corner_px"], worst)
    report("total over %d frames: both %d, fp32 only %d, bf16 only %d, max corner distance %.3f px"
           % (len(rows), total["both"], total["fp32_only"], total["bf16_only"], total["max_corner_px"]))
    return rows, total


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(prog="python -m poserisk_release_amd.detector")
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("compare", help="run the fp32 and the bf16 detector on a clip and report how far their boxes agree")
    c.add_argument("clip")
    c.add_argument("--weights", required=True, help="a darknet yolov3.weights file")
    c.add_argument("--img-size", type=int, nargs=2, default=(416, 416), metavar=("ROWS", "COLUMNS"))
    c.add_argument("--conf-thres", type=float, default=0.1)
    c.add_argument("--nms-thres", type=float, default=0.4)
    c.add_argument("--batch", type=int, default=8)
    c.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args()
    import torch
    compare(a.weights, a.clip, tuple(a.img_size), torch.device("cuda", a.gpu), a.batch, a.conf_thres, a.nms_thres)
