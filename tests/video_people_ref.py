"""The people contract of include/poserisk_hip.h (section r3, pr_compose_people) restated in numpy, from the contract's text and
from tests/video_ref.py's pieces (the outline, the area resample, the coverage blend): K boxes painted on the source in index
order, the resample, tag lines blended over the image region, panel lines over the black panel.  It is the only oracle for
the people canvases' pixels (tests/test_people_gpu.py and tests/test_people_native.py compare every byte)."""
import numpy as np

from video_ref import area_resample, draw_box, draw_text


def compose_people(frames, src_idx, box, box_rgb, lines, text, L_img, cov, adv, ascent, dst_h, dst_w, panel_w, canvases=None):
    """-> (out u8[N,dst_h,dst_w+panel_w,3], status int32[N]); box int[N,K,4] or None, box_rgb u8[N,K,4], lines int[N,L,5] or
    None; only the canvases named in `canvases` are computed (the others stay zero)."""
    n_frames = frames.shape[0]
    N = len(src_idx) if src_idx is not None else n_frames
    out = np.zeros((N, dst_h, dst_w + panel_w, 3), np.uint8)
    status = np.zeros(N, np.int32)
    for n in range(N):
        f = int(src_idx[n]) if src_idx is not None else n
        status[n] = 0 if 0 <= f < n_frames else 1
        if canvases is not None and n not in canvases:
            continue
        if not status[n]:
            img = frames[f]
            for k in range(box.shape[1] if box is not None else 0):
                img = draw_box(img, box[n, k], box_rgb[n, k])                      # later slots over earlier ones
            out[n, :, :dst_w] = area_resample(img, dst_h, dst_w)
        if lines is not None:
            draw_text(out[n][:, :dst_w], 0, lines[n, :L_img], text[n, :L_img], cov, adv, ascent)      # tags: the image region only
            draw_text(out[n], dst_w, lines[n, L_img:], text[n, L_img:], cov, adv, ascent)             # panel lines: the panel only
    return out, status
