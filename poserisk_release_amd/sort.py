"""SORT (Bewley et al., "Simple Online and Realtime Tracking", 2016) in float64 numpy: the half of multi_person_tracker that
follows the detector's boxes from frame to frame.  A few boxes a frame, so it runs on the host.  This project's own
restatement of the published algorithm and of abewley/sort's constants, taken from memory of that code [unpinned: nothing
in the reference tree holds it]; deterministic (no global state: ids count from 1 in every Sort).

    KalmanBoxTracker  7-state constant-velocity filter over z = (cx, cy, area, aspect), x = (z, d cx, d cy, d area)
    Sort              predict, associate (scipy's linear_sum_assignment on -IoU; a match needs IoU >= iou_thres), update,
                      report a track while matched this frame and (hit_streak >= min_hits or frame <= min_hits); detections
                      without width or height (clipped away at the frame's edge) are ignored
    track_frames      per-frame detections -> multi_person_tracker's dict {id: {'bbox': f32[n,4] (cx, cy, w, h with
                      w = h = max(w, h)), 'frames': int[n]}}"""
import numpy as np


def iou_matrix(a, b):
    """IoU of every box of a [n,4] with every box of b [m,4] (x1, y1, x2, y2) -> [n,m]."""
    a, b = np.asarray(a, np.float64)[:, None, :], np.asarray(b, np.float64)[None, :, :]
    w = np.maximum(0.0, np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]))
    h = np.maximum(0.0, np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]))
    inter = w * h
    union = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(union > 0, inter / union, 0.0)


def box_to_z(box):
    w, h = box[2] - box[0], box[3] - box[1]
    return np.array([box[0] + w / 2.0, box[1] + h / 2.0, w * h, w / float(h)], np.float64)


def z_to_box(x):
    with np.errstate(invalid="ignore", divide="ignore"):      # a predicted area below zero gives NaN: Sort.update drops that track
        w = np.sqrt(x[2] * x[3])
        h = x[2] / w
    return np.array([x[0] - w / 2.0, x[1] - h / 2.0, x[0] + w / 2.0, x[1] + h / 2.0], np.float64)


class KalmanBoxTracker:
    F = np.eye(7)
    F[0, 4] = F[1, 5] = F[2, 6] = 1.0
    H = np.eye(4, 7)
    R = np.diag([1.0, 1.0, 10.0, 10.0])
    Q = np.diag([1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001])
    P0 = np.diag([10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4])

    def __init__(self, box, track_id):
        self.x = np.zeros(7)
        self.x[:4] = box_to_z(box)
        self.P = self.P0.copy()
        self.id = track_id
        self.time_since_update = 0
        self.hits = 0
        self.hit_streak = 0
        self.age = 0

    def predict(self):
        if self.x[6] + self.x[2] <= 0:
            self.x[6] = 0.0
        self.x = self.F @ self.x
        self.P = self.F @ self.P @ self.F.T + self.Q
        self.age += 1
        if self.time_since_update > 0:
            self.hit_streak = 0
        self.time_since_update += 1
        return z_to_box(self.x)

    def update(self, box):
        self.time_since_update = 0
        self.hits += 1
        self.hit_streak += 1
        y = box_to_z(box) - self.H @ self.x
        S = self.H @ self.P @ self.H.T + self.R
        K = self.P @ self.H.T @ np.linalg.inv(S)
        self.x = self.x + K @ y
        self.P = (np.eye(7) - K @ self.H) @ self.P

    def box(self):
        return z_to_box(self.x)


def associate(dets, trks, iou_thres):
    """-> (matches [k,2] (detection, tracker), unmatched detections, unmatched trackers)."""
    from scipy.optimize import linear_sum_assignment
    if len(trks) == 0 or len(dets) == 0:
        return np.empty((0, 2), int), list(range(len(dets))), list(range(len(trks)))
    iou = iou_matrix(dets, trks)
    rows, cols = linear_sum_assignment(-iou)
    matches = [(d, t) for d, t in zip(rows, cols) if iou[d, t] >= iou_thres]
    md, mt = {d for d, _ in matches}, {t for _, t in matches}
    return (np.array(matches, int).reshape(-1, 2), [d for d in range(len(dets)) if d not in md],
            [t for t in range(len(trks)) if t not in mt])


class Sort:
    def __init__(self, max_age=1, min_hits=3, iou_thres=0.3):
        self.max_age, self.min_hits, self.iou_thres = int(max_age), int(min_hits), float(iou_thres)
        self.trackers = []
        self.frame_count = 0
        self.next_id = 1

    def update(self, dets):
        """dets [n,4+] (x1, y1, x2, y2, ...) of one frame -> [k,5] (x1, y1, x2, y2, id) of the tracks reported for it."""
        dets = np.asarray(dets, np.float64).reshape(-1, np.shape(dets)[-1] if np.size(dets) else 5)[:, :4]
        # a box clipped to the frame's edge can have no width or no height: it has no aspect and cannot be followed
        dets = dets[(dets[:, 2] > dets[:, 0]) & (dets[:, 3] > dets[:, 1]) & np.isfinite(dets).all(axis=1)]
        self.frame_count += 1
        predicted, alive = [], []
        for t in self.trackers:
            b = t.predict()
            if np.all(np.isfinite(b)):
                predicted.append(b), alive.append(t)
        self.trackers = alive
        matches, new_dets, _ = associate(dets, np.array(predicted).reshape(-1, 4), self.iou_thres)
        for d, t in matches:
            self.trackers[t].update(dets[d])
        for d in new_dets:
            self.trackers.append(KalmanBoxTracker(dets[d], self.next_id))     # its creation is no hit: hits = hit_streak = 0
            self.next_id += 1
        out = []
        for t in self.trackers:
            if t.time_since_update < 1 and (t.hit_streak >= self.min_hits or self.frame_count <= self.min_hits):
                out.append(np.concatenate([t.box(), [t.id]]))
        self.trackers = [t for t in self.trackers if t.time_since_update <= self.max_age]
        return np.array(out, np.float64).reshape(-1, 5)


def track_frames(dets, max_age=1, min_hits=3, iou_thres=0.3):
    """dets: per frame an array [n,4+] (x1, y1, x2, y2, ...) -> {id: {'bbox': f32[n,4] (cx, cy, w, h with w = h = max(w, h): the
    squared box multi_person_tracker returns), 'frames': int[n]}} in order of first appearance."""
    sort = Sort(max_age, min_hits, iou_thres)
    tracks = {}
    for f, d in enumerate(dets):
        for x1, y1, x2, y2, tid in sort.update(d):
            w, h = x2 - x1, y2 - y1
            side = max(w, h)
            t = tracks.setdefault(int(tid), {"bbox": [], "frames": []})
            t["bbox"].append([x1 + w / 2.0, y1 + h / 2.0, side, side])
            t["frames"].append(f)
    return {k: {"bbox": np.asarray(v["bbox"], np.float32).reshape(-1, 4), "frames": np.asarray(v["frames"], np.int64)}
            for k, v in tracks.items()}
