"""Tracker hand-off: what `DataProcessing.__call__` does with multi_person_tracker's output
before the crops are cut (lib/core/base.py:47-74, lib/utils/funcs_utils.py:55-64).  Pure host logic on small
arrays.  MPT itself stays outside this package; detector.py (YOLOv3 on the GPU) and sort.py (SORT) are this package's own
stand-in for it, opt-in through cfg.TRACKER, and return the same dict.

tracking_results: {person_id: {'bbox': f32[n,4] (cx,cy,w,h), 'frames': int[n]}}  (MPT output_format='dict').
"""
import numpy as np

MIN_FRAME_RATIO = 0.33   # lib/core/config.py:33
MIN_FRAME_CAP = 1000     # base.py:55


def filter_tracks(tracking_results, n_frames, min_frame_ratio=MIN_FRAME_RATIO):
    """base.py:53-69: keep tracks seen in >= min(ratio*n_frames, 1000) frames; if none qualifies keep all.
    Returns a list in the dict's iteration order (what `select_target_id` indexes)."""
    need = n_frames * min_frame_ratio
    if need > MIN_FRAME_CAP:
        need = MIN_FRAME_CAP
    kept = [t for t in tracking_results.values() if np.asarray(t['frames']).shape[0] >= need]
    return kept if kept else list(tracking_results.values())


def select_target_id(results):
    """funcs_utils.py:55-64: index of the track with the largest mean bbox area (first one on ties)."""
    areas = [(np.asarray(r['bbox'])[:, 2] * np.asarray(r['bbox'])[:, 3]).mean() for r in results]
    return int(np.argmax(np.array(areas)))


def people_tracks(tracking_results, n_frames, min_frame_ratio=MIN_FRAME_RATIO):
    """-> [(person_id, bbox f32[n,4], frames int[n])]: every track `filter_tracks` keeps (its "keep all if none qualifies"
    rule included), by descending mean box area, ties in the dict's iteration order.  Element 0 is the track `target_track`
    returns: the areas are select_target_id's own numbers and the sort is stable, as np.argmax takes the first maximum.  (No
    counterpart in the reference, which scores one person.)"""
    need = min(n_frames * min_frame_ratio, MIN_FRAME_CAP)
    ids = [i for i, t in tracking_results.items() if np.asarray(t['frames']).shape[0] >= need] or list(tracking_results)
    area = {i: (np.asarray(tracking_results[i]['bbox'])[:, 2] * np.asarray(tracking_results[i]['bbox'])[:, 3]).mean() for i in ids}
    # np.argmax takes the first NaN (the mean of a track without frames) as the maximum: so does this order
    return [(i, np.asarray(tracking_results[i]['bbox'], np.float32), np.asarray(tracking_results[i]['frames']))
            for i in sorted(ids, key=lambda i: (0, 0.0) if np.isnan(area[i]) else (1, -area[i]))]


def target_track(tracking_results, n_frames, min_frame_ratio=MIN_FRAME_RATIO):
    """-> (bbox f32[n,4], frames int[n]) of the person the reference scores (base.py:71-73)."""
    kept = filter_tracks(tracking_results, n_frames, min_frame_ratio)
    t = kept[select_target_id(kept)]
    return np.asarray(t['bbox'], np.float32), np.asarray(t['frames'])
