"""References of the person detector (include/poserisk_hip.h, section j8), independent of the library: the network as a torch
CPU forward in a chosen dtype with BatchNorm UNFOLDED (float64 is the reference, float32 the yardstick that sizes the
tolerance), and letterbox, decode, NMS and the map back to the frame in numpy.  A helper module, not a test."""
import numpy as np
import torch
import torch.nn.functional as F

import resize_ref
from poserisk_release_amd.detector import (ANCHOR_MASKS, ANCHORS, CONV, MAX_CAND, ROUTE, SHORTCUT, STRIDES, UPSAMPLE, YOLO,
                                           letterbox_geometry, yolo_layers)

HEAD_CONVS = (81, 93, 105)


def split_weights(body, layers=None):
    """The darknet float body -> per convolution layer index a dict of numpy arrays (beta, gamma, mean, var | bias; w OIHW)."""
    layers = yolo_layers() if layers is None else layers
    out, p = {}, 0
    for i, l in enumerate(layers):
        if l["type"] != CONV:
            continue
        o, d = l["cout"], {}
        for name in (("beta", "gamma", "mean", "var") if l["bn"] else ("bias",)):
            d[name] = body[p:p + o]
            p += o
        n = o * l["cin"] * l["ksize"] ** 2
        d["w"] = body[p:p + n].reshape(o, l["cin"], l["ksize"], l["ksize"])
        p += n
        out[i] = d
    return out, p


def numpy_fold_pack(body, layers, eps):
    """The header's packed layout from the darknet body, BatchNorm folded in float64."""
    out, p = [], 0
    for l in layers:
        if l["type"] != CONV:
            continue
        o, cin, k = l["cout"], l["cin"], l["ksize"]
        cin_pad, cout_pad = -(-cin // 4) * 4, -(-o // 64) * 64
        kpad = -(-(k * k * cin_pad) // 32) * 32
        if l["bn"]:
            beta, gamma, mean, var = (body[p + i * o:p + (i + 1) * o].astype(np.float64) for i in range(4))
            p += 4 * o
            scale = gamma / np.sqrt(var + eps)
            shift = beta - mean * scale
        else:
            shift, scale = body[p:p + o].astype(np.float64), np.ones(o)
            p += o
        w = body[p:p + o * cin * k * k].reshape(o, cin, k, k).astype(np.float64) * scale[:, None, None, None]
        p += o * cin * k * k
        packed = np.zeros((cout_pad, kpad), np.float32)
        taps = np.zeros((o, k * k, cin_pad), np.float32)
        taps[:, :, :cin] = w.transpose(0, 2, 3, 1).reshape(o, k * k, cin).astype(np.float32)
        packed[:o, :k * k * cin_pad] = taps.reshape(o, -1)
        bias = np.zeros(cout_pad, np.float32)
        bias[:o] = shift.astype(np.float32)
        out += [bias, packed.ravel()]
    return np.concatenate(out), p


def forward(body, x_nhwc4, dtype=torch.float64, bn_eps=1e-5, until=None, threads=None):
    """x f32[B,S_h,S_w,4] (the letterbox's output; channel 3 is ignored) -> {layer: NHWC numpy array in `dtype`} for every layer
    up to `until` (default: all 107).  A yolo layer's output is the head convolution's, unchanged."""
    layers = yolo_layers()
    params, _ = split_weights(np.asarray(body), layers)
    until = len(layers) - 1 if until is None else until
    if threads:
        torch.set_num_threads(threads)
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc4[..., :3])).to(dtype).permute(0, 3, 1, 2)
    outs = []
    with torch.no_grad():
        for i, l in enumerate(layers[:until + 1]):
            t = l["type"]
            if t == CONV:
                p = {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in params[i].items()}
                y = F.conv2d(x, p["w"], None if l["bn"] else p["bias"], stride=l["stride"], padding=l["ksize"] // 2)
                if l["bn"]:
                    y = F.batch_norm(y, p["mean"], p["var"], p["gamma"], p["beta"], False, 0.0, bn_eps)
                    y = F.leaky_relu(y, 0.1)
            elif t == SHORTCUT:
                y = outs[i - 1] + outs[l["from"][0]]
            elif t == ROUTE:
                y = torch.cat([outs[s] for s in l["from"]], dim=1)
            elif t == UPSAMPLE:
                y = F.interpolate(x, scale_factor=2, mode="nearest")
            else:
                assert t == YOLO
                y = x
            outs.append(y)
            x = y
    return {i: o.permute(0, 2, 3, 1).contiguous().numpy() for i, o in enumerate(outs)}


def letterbox(frames, S_h, S_w, bgr=False):
    """u8[B,H,W,3] -> f32[B,S_h,S_w,4], the header's contract in numpy."""
    frames = np.asarray(frames)
    B, H, W, _ = frames.shape
    h2, w2, ox, oy = letterbox_geometry(H, W, S_h, S_w)
    small = resize_ref.resize(frames, h2, w2)
    if bgr:
        small = small[..., ::-1]
    canvas = np.full((B, S_h, S_w, 3), 128, np.uint8)
    canvas[:, oy:oy + h2, ox:ox + w2] = small
    out = np.zeros((B, S_h, S_w, 4), np.float32)
    out[..., :3] = canvas.astype(np.float32) * np.float32(1.0 / 255.0)
    return out


def _sigmoid(t):
    return 1.0 / (1.0 + np.exp(-t))


def _decode_head(v, hd, dtype, out):
    """One head's cells (v f32[anchor,cy,cx,85]) -> obj, score, box [n,4], each expression in `dtype`, then obj, score and the box
    terms converted to `out` and the corners formed there (a product, then a sum)."""
    gh, gw = v.shape[1:3]
    vd = v.astype(dtype)
    cy, cx = np.meshgrid(np.arange(gh), np.arange(gw), indexing="ij")
    stride = dtype(STRIDES[hd])
    an = np.array([ANCHORS[k] for k in ANCHOR_MASKS[hd]], dtype)
    bx = ((_sigmoid(vd[..., 0]) + cx[None].astype(dtype)) * stride).astype(out)
    by = ((_sigmoid(vd[..., 1]) + cy[None].astype(dtype)) * stride).astype(out)
    bw = (an[:, 0, None, None] * np.exp(vd[..., 2])).astype(out)
    bh = (an[:, 1, None, None] * np.exp(vd[..., 3])).astype(out)
    so = _sigmoid(vd[..., 4])
    sc = (so * _sigmoid(vd[..., 5])).astype(out)
    hw, hh = bw * out(0.5), bh * out(0.5)
    return so.astype(out).ravel(), sc.ravel(), np.stack([bx - hw, by - hh, bx + hw, by + hh], -1).reshape(-1, 4)


def decode(heads, dtype=np.float64, out=None):
    """heads: three f32[B,gh,gw,255] -> per frame a dict of arrays over ALL cells in flat order (head, anchor, cy, cx):
    obj, score, box [n,4] (x1, y1, x2, y2), each expression in `dtype`; `out` (default: `dtype`) is the type they are converted to
    before the corners are formed: decode(heads, np.float64, np.float32) is the header's contract to the letter (float64
    expressions rounded to fp32 once, fp32 corners).
    person (bool): no other class value is greater than class 0's -- tc[c] > tc[0] for no c, which a NaN among the other 79 never
    satisfies and which every comparison with a NaN tc[0] fails (that cell passes; its score is NaN).
    nan_obj (bool): the objectness logit is NaN.  finite (bool): the CONTRACT's fp32 score and four fp32 corners are all finite,
    whatever `dtype` is: what select() leaves out and nonfinite() reports is the same for every dtype."""
    B = heads[0].shape[0]
    out = dtype if out is None else out
    frames = []
    for b in range(B):
        obj, score, person, boxes, nan_obj, finite = [], [], [], [], [], []
        for hd, t in enumerate(heads):
            gh, gw = t.shape[1:3]
            v = np.asarray(t[b], np.float32).reshape(gh, gw, 3, 85).transpose(2, 0, 1, 3)      # anchor, cy, cx, 85
            with np.errstate(all="ignore"):
                so, sc, box = _decode_head(v, hd, dtype, out)
                _, sc32, box32 = _decode_head(v, hd, np.float64, np.float32)
            obj.append(so), score.append(sc), boxes.append(box)
            person.append((~np.any(v[..., 6:] > v[..., 5:6], axis=-1)).ravel())
            nan_obj.append(np.isnan(v[..., 4]).ravel())
            finite.append(np.isfinite(sc32) & np.isfinite(box32).all(axis=1))
        frames.append({"obj": np.concatenate(obj), "score": np.concatenate(score), "person": np.concatenate(person),
                       "box": np.concatenate(boxes), "nan_obj": np.concatenate(nan_obj), "finite": np.concatenate(finite)})
    return frames


def candidates(cells, conf_thres):
    """-> (bool over all cells: passes the candidate test and is finite; the frame's PR_DET_STATUS_NONFINITE: an objectness logit
    is NaN, or a cell passes the test with a score or corner that is not finite in fp32)."""
    with np.errstate(invalid="ignore"):
        passes = (cells["obj"] >= cells["obj"].dtype.type(conf_thres)) & cells["person"] & ~cells["nan_obj"]
    return passes & cells["finite"], bool(cells["nan_obj"].any() or (passes & ~cells["finite"]).any())


def iou(a, b):
    """The contract's IoU of box a with boxes b [n,4], in the arrays' dtype."""
    z = a.dtype.type(0)
    with np.errstate(all="ignore"):      # 0 / 0 (two empty boxes) and an area past the format's largest: NaN or 0, no overlap
        iw = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), z)
        ih = np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), z)
        inter = iw * ih
        union = ((a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) - inter
        return inter / union


def select(cells, conf_thres, nms_thres, max_cand=MAX_CAND):
    """One frame's decode() dict -> (flat indices of the candidates in order, cut at max_cand; flat indices kept by the greedy
    NMS, in order; overflow flag; every pair's IoU among the participants, for the margin assertions).
    Candidates: candidates() -- a cell a non-finite head value took out is none and does not count towards max_cand.  Order: score
    descending, then the flat index ascending.  The first max_cand take part.  A participant is dropped iff an earlier KEPT one has
    IoU > nms_thres with it (thresholds in the boxes' dtype); a NaN IoU (0 / 0: two empty boxes) is greater than nothing."""
    cand = np.nonzero(candidates(cells, conf_thres)[0])[0]
    order = cand[np.lexsort((cand, -cells["score"][cand]))]
    overflow = order.size > max_cand
    order = order[:max_cand]
    boxes = cells["box"][order]
    kept, ious = [], np.zeros((order.size, order.size))
    alive = np.ones(order.size, bool)
    for i in range(order.size):
        v = iou(boxes[i], boxes)
        ious[i] = v
        if alive[i]:
            kept.append(i)
            drop = v > boxes.dtype.type(nms_thres)
            drop[:i + 1] = False
            alive &= ~drop
    return order, order[np.array(kept, int)], overflow, ious


def unmap(boxes, H, W, S_h, S_w, dtype=np.float64):
    """Letterbox pixels -> frame pixels, clipped: (x - ox) * (W / w'), (y - oy) * (H / h') in `dtype`."""
    h2, w2, ox, oy = letterbox_geometry(H, W, S_h, S_w)
    b = np.asarray(boxes).astype(dtype)
    sx, sy = dtype(W) / dtype(w2), dtype(H) / dtype(h2)
    out = np.empty_like(b)
    out[:, 0::2] = np.clip((b[:, 0::2] - dtype(ox)) * sx, 0, dtype(W))
    out[:, 1::2] = np.clip((b[:, 1::2] - dtype(oy)) * sy, 0, dtype(H))
    return out
