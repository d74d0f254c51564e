"""Mirror of lib/core/config.py: the global `cfg` and `update_config` that main/run.py:8 and
lib/core/base.py:19 import by the bare name `core.config`.

    from core.config import cfg, update_config           main/run.py:8
    cfg.DATASET.batch_size / workers / min_frame_ratio / bbox_scale / default_information     config.py:30-35
    cfg.SPIN.SMPL_MEAN_PARAMS / checkpoint / SMPL_MODEL_DIR / FOCAL_LENGTH / IMG_RES           config.py:44-50

Same knob names, same defaults, attribute and item access like the reference's `easydict` (which is not a
dependency here).  The reference computes its paths from the location of its own config.py
(`root_dir = lib/core/../../`); this file lives in another repository, so the root of the PoseRisk checkout is
found as: $POSERISK_ROOT, else the directory above the reference's `lib/` that main/__init_path.py:16-17 put on
sys.path, else the current directory (the reference is run from its root: lib/utils/smpl.py:9 is CWD-relative).
`cfg.DATASET.hip_batch_size` (not in the reference) is the frames per `pr_frames_forward` call of the MI355X path;
`cfg.DATASET.batch_size` (8) stays what the reference hands to the tracker.  The other knobs of the MI355X path, all
absent from the reference and all optional:
    cfg.SPIN.precision        'fp32' (default: the reference's arithmetic) | 'bf16' (encoder on the bf16 MFMAs, fp32
                              accumulate; regressor and SMPL stay fp32: BASELINE configs[2])
    cfg.SPIN.conv_form        'default' | 'direct' | 'winograd5' ... (fp32 encoder; poserisk_release_amd.hmr.CONV_FORMS)
    cfg.DATASET.hip_lanes     whole batches in flight on separate HIP streams (2)
    cfg.DATASET.hip_world_size  0 = whatever the launcher says ($WORLD_SIZE of torch.distributed.run, else 1); N > 1 insists
                              on N ranks, one per GPU, frames sharded and gathered once over RCCL
    cfg.DATASET.render_mesh   False | True: Predictor.__call__ also draws the fitted mesh over every track frame
                              (<TITLE>_mesh.mp4, or <TITLE>_mesh/%09d.png without cv2; args.render_mesh overrides it)
    cfg.DATASET.gpu_video     False | True: Predictor.__call__ composes <TITLE>_video on the GPU (pr_compose_video) instead of
                              drawing it with OpenCV (<TITLE>_video.mp4, or <TITLE>_video/%09d.png without cv2;
                              args.gpu_video overrides it)
    cfg.DATASET.gpu_video_codec  '' (default: the two outputs above as they are) | 'mjpeg': <TITLE>_video.avi and <TITLE>_mesh.avi,
                              baseline JPEG frames encoded on the GPU (pr_jpeg_encode) in a Motion-JPEG AVI written in Python,
                              with or without cv2 | 'png': <TITLE>_video/%09d.png and <TITLE>_mesh/%09d.png, lossless frames
                              encoded on the GPU (pr_png_encode), with or without cv2 | 'y4m': <TITLE>_video.y4m and
                              <TITLE>_mesh.y4m, YUV4MPEG2 converted on the GPU (pr_yuv_encode), with or without cv2
                              (args.video_codec overrides it); any other name raises
    cfg.DATASET.video_encoder  '' (off) | a command line containing {output}, e.g. `ffmpeg -v error -y -f yuv4mpegpipe -i -
                              -c:v libx264 -pix_fmt yuv420p {output}`: implies gpu_video_codec 'y4m'; the stream is piped to it as
                              a child process (no shell) and the files are <TITLE>_video and <TITLE>_mesh + video_encoder_ext
                              (args.video_encoder overrides it); a failing command raises RuntimeError naming its exit status
    cfg.DATASET.video_encoder_ext  '.mp4': the ending of the files that command writes
    cfg.DATASET.video_chroma  '420mpeg2' | '420jpeg' | '422' | '444' | 'mono': the layout of that stream; the matrix is yuv_matrix,
                              the range limited, odd sides of a subsampled layout are padded to even by replication
    cfg.DATASET.gpu_video_quality  the JPEG quality of those frames, 1..100 (90)
    cfg.DATASET.front_max_w, front_max_h  800, 450: the reference's front-end rule for a Motion-JPEG AVI input (wider than
                              front_max_w -> that width, else higher than front_max_h -> that height; 0 switches an arm off),
                              applied on the GPU by poserisk_release_amd.frontend.read_video
    cfg.DATASET.jpeg_entropy  'auto' | 'serial' | 'sync': how JPEG frames (a folder's, a Motion-JPEG AVI's) are entropy-decoded
                              (poserisk_release_amd.jpeg.decode_files): one lane per restart segment, self-synchronising
                              sub-sequences inside a segment, or (auto) the latter where a chunk holds restart-free frames
    cfg.DATASET.jpeg_progressive  True: progressive JPEG frames, and sequential ones whose components come in several scans, are
                              decoded too (jpeg.decode_files(progressive=True), pr_jpeg_decode_scans); False refuses them by
                              name, as the single-scan parser does
    cfg.DATASET.yuv_matrix    '601' | '709' | 'auto' (709 above 576 rows): the colour matrix of a YUV4MPEG2 input
                              (poserisk_release_amd.y4m.decode); '601' is what swscale's unconfigured conversion uses at every size
    cfg.DATASET.video_decoder  '' (off) | a command line containing {input}, e.g. `ffmpeg -v error -i {input} -f yuv4mpegpipe
                              -pix_fmt yuv420p -`: a regular file that is neither a Motion-JPEG AVI nor a YUV4MPEG2 file is decoded
                              by running it as a child process (no shell) and reading its standard output as YUV4MPEG2
                              (args.video_decoder overrides it)
    cfg.DATASET.persons       'target' (default: the reference's one person, nothing else) | 'all': Predictor.__call__ scores every
                              track tracks.people_tracks keeps in one pass (Predictor.score_people) and adds <output>/person_<id>/,
                              <output>/people.json and, with gpu_video, <TITLE>_people (pr_compose_people); every other output
                              stays what 'target' writes (args.persons overrides it)
    cfg.DATASET.people_mesh   False | True, with persons 'all' only (anything else raises): Predictor.score_people also returns every
                              person's SMPL parameters, and with gpu_video the image region of <TITLE>_people is the frame with
                              everybody's fitted mesh over it, the people depth-tested against each other (pr_render_people), also
                              written on its own as <TITLE>_people_mesh (args.people_mesh overrides it)
    cfg.DATASET.smooth_median_radius  0 (off) .. 15, in FRAMES: each track's joint rotations (and cam, betas) are replaced by the
                              medoid of their window of that many frames on each side before scoring: removes single-frame
                              outliers (args.smooth_median_radius overrides it)
    cfg.DATASET.smooth_sigma  0.0 (off) or the standard deviation, in FRAMES, of the Gaussian that then averages each track's
                              poses over min(ceil(3 sigma), 15) frames on each side: removes jitter.  With both at 0 nothing
                              changes anywhere (args.smooth_sigma overrides it; pr_smooth_tracks)
    cfg.TRACKER               the built-in person detector and tracker (poserisk_release_amd.detector: YOLOv3 on the GPU,
                              poserisk_release_amd.sort: SORT on the host).  All of it is inert while `weights` is '':
                              weights '' | the path of a darknet yolov3.weights file; img_size (416, 416) = (rows, columns) of the
                              network input, multiples of 32 ((256, 416) suits 800 x 450 frames); conf_thres 0.1 (the reference's
                              detection_threshold); nms_thres 0.4; max_age 1, min_hits 3, iou_thres 0.3 (SORT); batch 8 frames a call;
                              precision 'fp32' (default) | 'bf16' (the detector on the bf16 MFMAs: `TRACKER: {precision: bf16}`;
                              its agreement with fp32 on trained weights is unmeasured).
                              With weights set, a video file's tracking comes from it after the tracking given and the sidecar
                              and before multi_person_tracker, and a frame folder without tracking.pkl is accepted
    cfg.ACTIVITY              REBA's activity score and RULA's muscle use derived from each track's motion instead of taken as 0
                              (poserisk_release_amd.activity, pr_activity_tracks).  derive False (default:
                              nothing changes anywhere; args.derive_activity overrides it) | True: every scored person's rows get
                              +1 REBA activity for a scored joint held within static_deg (10) for longer than hold_seconds (60),
                              +1 for more than rep_events (8: more than four out-and-back actions) movements of move_deg (15)
                              within hold_seconds, +1 for a change of rapid_deg (45) within rapid_seconds (1), and +1 RULA muscle
                              use per group (left arm, right arm, neck-trunk-legs) held or repeated; a step of more than
                              gap_seconds (0.2) between two frames of a track breaks a window.  The values are ADDED to the
                              information file's constants (leave those at 0) and <output>/activity.json is written.  The
                              degrees are this project's choice: the worksheets give none, and nobody has measured the rule on
                              real footage
main/run.py has its `--cfg` option commented out (run.py:20-24), so a YAML of overrides named by $POSERISK_CFG is applied
when this module is imported -- `POSERISK_CFG=bf16.yaml python main/run.py ...` with the one line `SPIN: {precision: bf16}`.
"""
import os
import os.path as osp
import sys


class _Cfg(dict):
    """dict with attribute access (the part of easydict the reference uses); nested dicts convert on assignment."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __setattr__(self, name, value):
        self[name] = value

    def __setitem__(self, key, value):
        if isinstance(value, dict) and not isinstance(value, _Cfg):
            value = _Cfg(value)
        super().__setitem__(key, value)

    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in dict(d or {}, **kw).items():
            self[k] = v


edict = _Cfg


def _reference_root():
    env = os.environ.get('POSERISK_ROOT')
    if env:
        return osp.abspath(env)
    here = osp.dirname(osp.abspath(__file__))
    for p in sys.path:
        if not p:
            continue
        cand = osp.join(p, 'core', 'base.py')
        if osp.isfile(cand) and osp.abspath(osp.join(p, 'core')) != here:
            return osp.abspath(osp.join(p, '..'))       # p is the reference's lib/
    return osp.abspath(os.getcwd())


def _defaults(root):
    """The reference's knobs and default values (config.py:17-60), as one table."""
    core_dir = osp.join(root, 'lib', 'core')
    spin_dir = osp.join(root, 'lib', 'SPIN')
    spin_data = osp.join(spin_dir, 'data')
    return {
        'root_dir': root, 'cur_dir': core_dir, 'data_dir': osp.join(root, 'data'),
        'smpl_dir': osp.join(root, 'smplpytorch'),
        'DATASET': {'workers': 16, 'batch_size': 8, 'min_frame_ratio': 0.33, 'bbox_scale': 1.2,
                    'default_information': osp.join(core_dir, 'default_information.json'),
                    'hip_batch_size': 64, 'hip_lanes': 2, 'hip_world_size': 0,
                    'render_mesh': False, 'gpu_video': False, 'gpu_video_codec': '', 'gpu_video_quality': 90,
                    'front_max_w': 800, 'front_max_h': 450, 'jpeg_entropy': 'auto', 'jpeg_progressive': True,
                    'yuv_matrix': '601', 'video_decoder': '', 'video_encoder': '', 'video_encoder_ext': '.mp4',
                    'video_chroma': '420mpeg2', 'persons': 'target', 'people_mesh': False,
                    'smooth_median_radius': 0, 'smooth_sigma': 0.0},
        'MODEL': {'input_shape': (224, 224)},
        'SPIN': {'spin_dir': spin_dir, 'SMPL_MEAN_PARAMS': osp.join(spin_data, 'smpl_mean_params.npz'),
                 'checkpoint': osp.join(spin_data, 'model_checkpoint.pt'),
                 'SMPL_MODEL_DIR': osp.join(spin_data, 'smpl'), 'FOCAL_LENGTH': 5000, 'IMG_RES': 224,
                 'precision': 'fp32', 'conv_form': 'default'},
        'AUG': {'flip': False, 'rotate_factor': 0},
        'TEST': {},
        'TRACKER': {'weights': '', 'img_size': (416, 416), 'conf_thres': 0.1, 'nms_thres': 0.4, 'max_age': 1, 'min_hits': 3,
                    'iou_thres': 0.3, 'batch': 8, 'precision': 'fp32'},
        'ACTIVITY': {'derive': False, 'hold_seconds': 60.0, 'static_deg': 10.0, 'move_deg': 15.0, 'rep_events': 8,
                     'rapid_seconds': 1.0, 'rapid_deg': 45.0, 'gap_seconds': 0.2},
    }


cfg = edict(_defaults(_reference_root()))


def update_config(config_file):
    """YAML overrides with the reference's rules (config.py:63-85): a top-level or nested key that `cfg` does
    not already hold raises ValueError; nested sections are updated key by key, scalars replaced."""
    import yaml
    with open(config_file) as f:
        overrides = yaml.safe_load(f) or {}
    for section, value in overrides.items():
        if section not in cfg:
            raise ValueError("{} not exist in config.py".format(section))
        if not isinstance(value, dict):
            cfg[section] = value
            continue
        unknown = [k for k in value if k not in cfg[section]]
        if unknown:
            raise ValueError("{}.{} not exist in config.py".format(section, unknown[0]))
        for k, v in value.items():
            cfg[section][k] = v


if os.environ.get('POSERISK_CFG'):
    update_config(os.environ['POSERISK_CFG'])
