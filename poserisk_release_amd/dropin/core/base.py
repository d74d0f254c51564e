"""Mirror of the hot-path half of lib/core/base.py::Predictor.

    predictor = Predictor(args)                                       main/run.py:31
    result, joint_cam, images, debug_result = predictor.get_pose_estimation_results(loader)   base.py:126
    reba_results = predictor.reba(result, joint_cam, add_info)        base.py:151
    final, scores, logs = predictor.post_processing(reba_results, ...)  base.py:153

`get_pose_estimation_results` is the reference's loop (base.py:211-240) with the per-frame Python
removed: every batch is one `pr_frames_forward` call on the GPU, results stay on the device until the
end of the loop, and with `torch.distributed` initialised every rank takes a contiguous frame shard and
the per-frame records are all-gathered once.  Tracking and the decoding of videos other than Motion-JPEG AVI
(base.py:47-74) are outside the accelerated path: `__call__` takes decoded frames + the tracker's
dict, finds them in a directory, reads a Motion-JPEG AVI on the GPU (poserisk_release_amd/frontend.py), or runs the
reference's own front end when cv2 and multi_person_tracker are importable; it writes the
result text files, the score plots, the debug CSVs and the annotated video (drawn by OpenCV where cv2 is importable, or
composed on the GPU with the gpu_video knob).
"""
import json
import os
import os.path as osp

import numpy as np
import torch

from poserisk_release_amd import pipeline as pl
from poserisk_release_amd import sinks, synth
from poserisk_release_amd.hmr import hmr

from core.config import cfg
from reba import REBA
from rula import RULA
from smpl import SMPL


def aggregate(scores):
    """base.py:263-271: sort desc; mean, top-50 %, top-10 % (NaN when N < 10), max, mode; 3 dp."""
    from scipy.stats import mode
    import warnings
    s = np.sort(np.asarray(scores))[::-1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        top50 = round(s[:len(s) // 2].mean(), 3)
        top10 = round(s[:len(s) // 10].mean(), 3)
    return (round(s.mean(), 3), top50, top10, round(s.max(), 3), mode(s).mode.item())


PRECISIONS = {'fp32': 'fp32', 'f32': 'fp32', 'float32': 'fp32', 'float': 'fp32',
              'bf16': 'bf16', 'bfloat16': 'bf16'}


def encoder_precision(args=None):
    """'fp32' | 'bf16': `args.dtype` when the caller's namespace has one (SURVEY.md section 5 asks for a --dtype next to
    the reference's flags; main/run.py:11-19 has none, so unmodified it is the config's), else cfg.SPIN.precision."""
    want = getattr(args, 'dtype', None) if args is not None else None
    if want is None:
        want = cfg.SPIN.get('precision', 'fp32')
    if isinstance(want, torch.dtype):
        want = str(want).replace('torch.', '')
    key = str(want).lower()
    if key not in PRECISIONS:
        raise ValueError(f"encoder precision {want!r} unknown: one of {sorted(set(PRECISIONS))} "
                         "(cfg.SPIN.precision / args.dtype)")
    return PRECISIONS[key]


def load_spin_model(smpl_mean_params=None, checkpoint=None, precision=None, conv_form=None):
    """base.py:81-84 with the reference's file locations (lib/core/config.py:45-47):

        spin_model = hmr(cfg.SPIN.SMPL_MEAN_PARAMS)
        checkpoint = torch.load(cfg.SPIN.checkpoint);  spin_model.load_state_dict(checkpoint['model'], strict=False)

    Both files are licensed downloads (reference README.md:36-37); a missing one is reported by name here, at
    construction, instead of as a KeyError inside the first forward."""
    mean_path = smpl_mean_params if smpl_mean_params is not None else cfg.SPIN.SMPL_MEAN_PARAMS
    ckpt_path = checkpoint if checkpoint is not None else cfg.SPIN.checkpoint
    for what, path, knob in (("SMPL mean parameters", mean_path, "cfg.SPIN.SMPL_MEAN_PARAMS"),
                             ("SPIN checkpoint", ckpt_path, "cfg.SPIN.checkpoint")):
        if isinstance(path, str) and not osp.isfile(path):
            raise FileNotFoundError(
                f"{what} not found at '{path}' ({knob}, lib/core/config.py:46-47; PoseRisk root taken as "
                f"'{cfg.root_dir}', override with $POSERISK_ROOT): download it as the reference's README.md:36-37 "
                "describes, or pass spin_model= / spin_checkpoint= / smpl_mean_params= to Predictor")
    model = hmr(mean_path, precision=precision if precision is not None else encoder_precision(),
                conv_form=conv_form if conv_form is not None else cfg.SPIN.get('conv_form', 'default'))
    import pickle
    try:
        ckpt = torch.load(ckpt_path, map_location='cpu')            # base.py:83 lacks map_location (Q23)
    except pickle.UnpicklingError:
        # torch >= 2.6 loads with weights_only=True by default; SPIN's checkpoint also pickles optimizer / scheduler
        # objects, which that mode refuses.  Only THAT refusal falls back to full unpickling (the reference's own
        # behaviour, base.py:83: the file is the user's licensed download); any other failure is raised as it is.
        ckpt = torch.load(ckpt_path, map_location='cpu', weights_only=False)
    if 'model' not in ckpt:
        raise KeyError(f"'{ckpt_path}' has no 'model' entry (base.py:84 reads checkpoint['model']); keys: {list(ckpt)[:8]}")
    missing, _ = model.load_state_dict(ckpt['model'], strict=False)
    if missing:     # the reference's strict=False would run on with torchvision's ImageNet init; there is none here
        raise KeyError(f"'{ckpt_path}': checkpoint['model'] lacks {len(missing)} of the encoder/regressor tensors, "
                       f"e.g. {missing[:4]}")
    return model


def default_information():
    """The `add_info` used when --info is not a file (base.py:140-142).  The reference points
    cfg.DATASET.default_information at lib/core/default_information.json while the file ships as
    main/default_information.json; either is read when present, else the same values built in."""
    for path in (cfg.DATASET.default_information, osp.join(cfg.root_dir, 'main', 'default_information.json')):
        if osp.isfile(path):
            with open(path, 'r') as f:
                return json.load(f)
    return synth.DEFAULT_INFO


def _information(add_info):
    """`add_info` as the scorers take it: None is default_information(), a string the path of a json file, a dict itself."""
    if isinstance(add_info, str):
        with open(add_info, 'r') as f:
            return json.load(f)
    return default_information() if add_info is None else add_info


def _knob(args, name, key, default):
    """`args.<name>` when the caller's namespace has one that is not None, else cfg.DATASET.<key>, else (absent or empty) `default`."""
    knob = getattr(args, name, None)
    return knob if knob is not None else cfg.DATASET.get(key, default) or default


def _jpeg_options():                                   # what every jpeg.decode_files call of the front end takes from cfg.DATASET
    return dict(entropy=cfg.DATASET.get('jpeg_entropy', 'auto'), progressive=bool(cfg.DATASET.get('jpeg_progressive', True)))


def _front_limits():                                   # the front end's downscale rule (frontend.target_size) from cfg.DATASET
    return dict(max_w=cfg.DATASET.get('front_max_w', 800), max_h=cfg.DATASET.get('front_max_h', 450))


def _yuv_matrix():                                     # the Y'CbCr matrix the YUV4MPEG2 reader and sink take from cfg.DATASET
    return str(cfg.DATASET.get('yuv_matrix', '601'))


class Predictor:
    def __init__(self, args, spin_model=None, smpl_model=None, batch_size=None, spin_checkpoint=None,
                 smpl_mean_params=None):
        """`Predictor(args)` as main/run.py:31 calls it (args fields gpu,type,input,info,output,visualize,debug,
        debug_joints,debug_frame): SMPL() from the reference's CWD-relative model directory (lib/utils/smpl.py:9),
        SPIN weights and mean parameters from cfg.SPIN.checkpoint / cfg.SPIN.SMPL_MEAN_PARAMS (base.py:80-84);
        FileNotFoundError names whichever file is absent.  Models may also be injected (tests, other locations).
        `batch_size`: frames per GPU call, default cfg.DATASET.hip_batch_size (64)."""
        self.device = torch.device('cuda') if torch.cuda.is_available() else torch.device('cpu')
        self.world_size = self._join_world(args)        # one process per GPU; may move self.device to this rank's GPU
        self.smpl_model = smpl_model if smpl_model is not None else SMPL()
        self.precision = encoder_precision(args)        # args.dtype, else cfg.SPIN.precision ('fp32' | 'bf16')
        if spin_model is None:
            spin_model = load_spin_model(smpl_mean_params, spin_checkpoint, precision=self.precision)
        self.spin_model = spin_model.to(self.device)
        self.batch_size = int(batch_size if batch_size is not None else cfg.DATASET.get('hip_batch_size', 64))
        # whole batches in flight (pipeline.FramePipeline): args.lanes, else cfg.DATASET.hip_lanes
        self.lanes = int(getattr(args, 'lanes', None) or cfg.DATASET.get('hip_lanes', 2))
        self._pipe = None
        debug = bool(getattr(args, 'debug', False))
        self.reba, self.rula = REBA(debug), RULA(debug)
        scores = str(getattr(args, 'type', 'REBA,RULA')).replace(' ', '').upper().split(',')
        self.run_reba = 'REBA' in scores
        self.run_rula = 'RULA' in scores
        self.debugging = debug
        self.debug_frame = getattr(args, 'debug_frame', -1)
        # the mesh overlay (render_overlay): args.render_mesh, else cfg.DATASET.render_mesh (False; $POSERISK_CFG can set it)
        self.render_mesh = bool(_knob(args, 'render_mesh', 'render_mesh', False))
        # the annotated score video composed on the GPU (write_gpu_video): args.gpu_video, else cfg.DATASET.gpu_video (False)
        self.gpu_video = bool(_knob(args, 'gpu_video', 'gpu_video', False))
        # whom __call__ scores: args.persons, else cfg.DATASET.persons.  'target' (default): the reference's one person; 'all':
        # every kept track in one pass (score_people), with person_<id>/, people.json and <TITLE>_people beside the target's outputs
        self.persons = str(_knob(args, 'persons', 'persons', 'target'))
        if self.persons not in ('target', 'all'):
            raise ValueError(f"persons {self.persons!r} is not known: 'target' or 'all' (cfg.DATASET.persons / args.persons)")
        # the mesh of EVERY scored person over every frame, depth-tested against each other (render_people, pr_render_people):
        # args.people_mesh, else cfg.DATASET.people_mesh (False).  A knob of its own: render_mesh stays the target's overlay
        self.people_mesh = bool(_knob(args, 'people_mesh', 'people_mesh', False))
        if self.people_mesh and self.persons != 'all':
            raise ValueError(f"people_mesh draws the people that persons 'all' scores, but persons is {self.persons!r} "
                             "(cfg.DATASET.people_mesh / args.people_mesh, cfg.DATASET.persons / args.persons)")
        # temporal smoothing of each track's poses before scoring (poserisk_release_amd/smooth.py, pr_smooth_tracks), both in
        # FRAMES: args.smooth_median_radius, else cfg.DATASET.smooth_median_radius (0); args.smooth_sigma, else
        # cfg.DATASET.smooth_sigma (0.0).  Both 0 = off: _score_tracks takes the path it always took
        from poserisk_release_amd.smooth import check_parameters
        self.smooth_median_radius, self.smooth_sigma = check_parameters(_knob(args, 'smooth_median_radius', 'smooth_median_radius', 0),
                                                                        _knob(args, 'smooth_sigma', 'smooth_sigma', 0.0))
        # REBA's activity score and RULA's muscle use derived from each track's motion (poserisk_release_amd/activity.py,
        # pr_activity_tracks): args.derive_activity, else cfg.ACTIVITY.derive (False).  Off = None: _score_tracks takes the path it
        # always took.  On: cfg.ACTIVITY's other keys, refused by name here where they make no sense at any frame rate
        self.activity = self._activity_knob(args)
        # how write_gpu_video and the mesh overlay store their frames (poserisk_release_amd/sinks.py): args.video_codec, else
        # cfg.DATASET.gpu_video_codec.  '' (default) = mp4 through cv2 where importable, else one PNG per frame; 'mjpeg' = encoded
        # to JPEG on the GPU into <TITLE>_video.avi / <TITLE>_mesh.avi, with or without cv2; 'png' = lossless, encoded on the GPU
        # into <TITLE>_video/%09d.png / <TITLE>_mesh/%09d.png, with or without cv2; 'y4m' = converted to Y'CbCr on the GPU into
        # <TITLE>_video.y4m / <TITLE>_mesh.y4m, or, with the video_encoder knob, piped to that command, which writes
        # <TITLE>_video.mp4 / <TITLE>_mesh.mp4 in the codec it names
        self.gpu_video_codec = str(_knob(args, 'video_codec', 'gpu_video_codec', ''))
        if self.gpu_video_codec not in sinks.CODECS:
            raise ValueError(f"gpu_video_codec {self.gpu_video_codec!r} is not known: '' (mp4 through cv2, else PNG frames), 'mjpeg', "
                             "'png' or 'y4m' (any other codec: 'y4m' with the video_encoder knob)")
        # args.video_encoder, else cfg.DATASET.video_encoder ('' = off): a command line with {output} that reads YUV4MPEG2 on its
        # standard input; it implies the 'y4m' codec.  video_encoder_ext ('.mp4') ends the file's name, video_chroma the layout
        self.video_encoder = str(_knob(args, 'video_encoder', 'video_encoder', ''))
        self.video_encoder_ext = str(_knob(args, 'video_encoder_ext', 'video_encoder_ext', '.mp4'))
        self.video_chroma = str(cfg.DATASET.get('video_chroma', '420mpeg2') or '420mpeg2')
        if self.video_encoder:
            if '{output}' not in self.video_encoder:
                raise ValueError(f"video_encoder {self.video_encoder!r} must be a command line containing {{output}}")
            if self.gpu_video_codec not in ('', 'y4m'):
                raise ValueError(f"video_encoder is fed YUV4MPEG2: it goes with gpu_video_codec 'y4m' (or ''), not "
                                 f"{self.gpu_video_codec!r}")
            self.gpu_video_codec = 'y4m'
        self.gpu_video_quality = int(cfg.DATASET.get('gpu_video_quality', 90))
        # load_front_end's case 3c: args.video_decoder, else cfg.DATASET.video_decoder ('' = off): a command line with {input}
        # whose standard output is read as YUV4MPEG2
        self.video_decoder = str(_knob(args, 'video_decoder', 'video_decoder', ''))
        dj = str(getattr(args, 'debug_joints', '')).replace(' ', '').split(',')
        if dj == ['']:
            self.debug_joints = None
        else:
            for joint in dj:
                if joint.upper() not in self.smpl_model.joints_name_upper:
                    print("\n\nInvalid Joint name!\n\n")
                    assert 0
            self.debug_joints = dj

    @staticmethod
    def _activity_knob(args):
        """None (off), or cfg.ACTIVITY's parameters without `derive`, checked (at 1 fps, the lowest rate at which seconds still
        round to whole frames: what is refused there is refused at every rate)."""
        from poserisk_release_amd.activity import DEFAULTS, check_parameters
        section = cfg.get('ACTIVITY', None) or {}
        derive = getattr(args, 'derive_activity', None)
        if not bool(section.get('derive', False) if derive is None else derive):
            return None
        parameters = {k: section.get(k, v) for k, v in DEFAULTS.items() if k != 'derive'}
        unknown = sorted(set(section) - set(DEFAULTS))
        if unknown:
            raise ValueError(f"cfg.ACTIVITY holds unknown key(s) {unknown}: {sorted(DEFAULTS)}")
        check_parameters(1.0, **parameters)
        return parameters

    def _join_world(self, args):
        """One process per GPU.  The world size asked for: `args.world_size` when the namespace has one,
        else cfg.DATASET.hip_world_size, else (0) whatever the launcher exported as $WORLD_SIZE.  With more than one rank
        and no process group yet, this rank joins one over RCCL (`nccl`) on the GPU $LOCAL_RANK names -- main/run.py:26
        narrows CUDA_VISIBLE_DEVICES to --gpu first, so `--gpu 0,1,...` has to list a GPU per rank.  A mismatch between
        what was asked for and what the launcher started is an error, never a silent single-GPU run."""
        import torch.distributed as dist
        want = int(_knob(args, 'world_size', 'hip_world_size', 0))
        launched = int(os.environ.get('WORLD_SIZE', '1'))
        if dist.is_available() and dist.is_initialized():
            have = dist.get_world_size()
            if want > 1 and want != have:
                raise RuntimeError(f"world size {want} asked for (args.world_size / cfg.DATASET.hip_world_size) but the "
                                   f"initialised process group has {have} ranks")
            return have
        if want > 1 and launched != want:
            raise RuntimeError(
                f"world size {want} asked for (args.world_size / cfg.DATASET.hip_world_size) but this process was started "
                f"with WORLD_SIZE={launched}: launch one rank per GPU, e.g. `python -m torch.distributed.run --nnodes=1 "
                f"--nproc-per-node {want} --master-addr 127.0.0.1 main/run.py --gpu {','.join(str(i) for i in range(want))} ...`")
        if launched <= 1:
            return 1
        if self.device.type != 'cuda':
            raise RuntimeError("several ranks need a GPU each (there is no CPU path)")
        local = int(os.environ.get('LOCAL_RANK', os.environ.get('RANK', '0')))
        if os.environ.get('POSERISK_SHARE_GPU') == '1':
            local = 0        # rehearsal only (a one-GPU box, gloo): every rank on cuda:0, like bench.py --share-gpu
        if local >= torch.cuda.device_count():
            raise RuntimeError(f"rank with LOCAL_RANK={local} sees {torch.cuda.device_count()} GPU(s): list one per rank in "
                               "--gpu (main/run.py:26 sets CUDA_VISIBLE_DEVICES from it)")
        self.device = torch.device('cuda', local)
        torch.cuda.set_device(self.device)
        pl.init_distributed(os.environ.get('POSERISK_DIST_BACKEND', 'nccl'), self.device)
        return dist.get_world_size()

    # ---- base.py:211-240 -------------------------------------------------------------------------
    def get_pose_estimation_results(self, crop_dataloader, keep_images=True, n_total=None, smpl_params=None):
        """Iterable of f32[b,3,224,224] batches -> (result f64[N,24,3] Euler deg, joint_cam f32[N,24,3] mm,
        images f32[N,3,224,224], debug_result f32[N,24,3] axis-angle with root rows = 3.14,0,0).
        `smpl_params`: a dict that receives the network's rotmat f32[N,24,3,3], betas f32[N,10] and cam f32[N,3] (host
        arrays, gathered like the others; the mesh overlay draws from them), or None: the return value is the same.

        `n_total` (multi-GPU): the loader holds only this rank's contiguous shard
        `pipeline.shard_bounds(n_total, world, rank)`; the per-frame results of all ranks are all-gathered
        once after the loop (RCCL with the nccl backend), so every rank returns all `n_total` frames in
        frame order.  `images` stays local."""
        self.spin_model.eval()
        if self._pipe is None:
            # the scorers run afterwards on all frames with the caller's add_info (base.py:151,168)
            self._pipe = pl.FramePipeline(self.spin_model, self.smpl_model.layer['neutral'], None, lanes=self.lanes)
        pipe = self._pipe
        eul, jc, aa, st, images = [], [], [], [], []
        params = {'rotmat': [], 'betas': [], 'cam': []} if smpl_params is not None else None
        # host batches cross PCIe from PINNED staging buffers (one per batch in flight + 1): a `.to(device, non_blocking=True)`
        # from pageable memory -- what a DataLoader without pin_memory yields -- is a synchronous copy that stalls the loop
        stage, n_stage, uploads = [], self.lanes + 1, 0
        with torch.no_grad():
            for batch in crop_dataloader:
                batch = torch.as_tensor(batch)
                if batch.device.type == 'cpu' and not batch.is_pinned():
                    k = uploads % n_stage
                    if len(stage) <= k:
                        stage.append([None, None])
                    buf, ev = stage[k]
                    if buf is None or buf.shape[0] < batch.shape[0] or buf.shape[1:] != batch.shape[1:] or buf.dtype != batch.dtype:
                        buf = torch.empty((max(batch.shape[0], self.batch_size),) + tuple(batch.shape[1:]), dtype=batch.dtype).pin_memory()
                        ev = None
                    if ev is not None:
                        ev.synchronize()                    # the upload that last used this buffer has left the host
                    buf[:batch.shape[0]].copy_(batch)
                    dbatch = buf[:batch.shape[0]].to(self.device, non_blocking=True)
                    stage[k] = [buf, torch.cuda.current_stream(self.device).record_event()]
                    uploads += 1
                else:
                    dbatch = batch.to(self.device, non_blocking=True)
                out = pipe(dbatch)
                pl.FramePipeline.wait(out)      # the copies below queue behind this batch; the next one overlaps
                eul.append(out['euler'].clone()); jc.append(out['joint_cam'].clone())
                aa.append(out['axis_angle'].clone()); st.append(out['status'].clone())
                if params is not None:
                    for k in params:
                        params[k].append(out[k].clone())
                if keep_images:
                    images.append(batch.cpu().numpy())
        dev = self.device
        cat = lambda parts, shape, dt: torch.cat(parts) if parts else torch.empty((0,) + shape, dtype=dt, device=dev)
        eul, jc = cat(eul, (24, 3), torch.float64), cat(jc, (24, 3), torch.float32)
        aa, st = cat(aa, (24, 3), torch.float32), cat(st, (), torch.int32)
        if params is not None:
            for k, shape in (('rotmat', (24, 3, 3)), ('betas', (10,)), ('cam', (3,))):
                params[k] = cat(params[k], shape, torch.float32)
        if n_total is not None:
            eul, jc, aa, st = (pl.gather_padded(t, n_total) for t in (eul, jc, aa, st))
            if params is not None:
                params = {k: pl.gather_padded(t, n_total) for k, t in params.items()}
        if params is not None:
            smpl_params.update({k: t.cpu().numpy() for k, t in params.items()})
        status = st.cpu().numpy()
        if np.any(status != 0):     # coord_utils.py:70,91: the reference aborts on these
            raise AssertionError(f"invalid rotation in frames {np.nonzero(status)[0].tolist()}")
        result = eul.cpu().numpy()
        joint_cam = jc.cpu().numpy()
        debug_result = aa.cpu().numpy()
        images = np.concatenate(images) if images else np.zeros((0, 3, 224, 224), np.float32)
        return result, joint_cam, images, debug_result

    # ---- base.py:242-271 (aggregation; the score plot is reporting and lives outside the path) ------
    def post_processing(self, results, joint_names=None, timestamp=None, output_path=None, title=''):
        scores = np.array([r['score'] for r in results])
        logs = np.array([r['log_score'] for r in results])
        return aggregate(scores), np.copy(scores), logs

    # ---- the accelerated half of __call__ (base.py:126-182 without tracking / reporting) ------------
    def _on_device(self, frames):
        """frames u8[F,H,W,3] (torch tensor or numpy) -> a CUDA tensor; one that is on a GPU already stays where it is."""
        frames = torch.as_tensor(frames)
        return frames if frames.device.type == 'cuda' else frames.to(self.device)

    def _run_scorers(self, out, add_info, rows=None):
        """REBA / RULA and the aggregation over out['result'], out['joint_cam'] -> out['reba'], out['rula'] = (final, scores,
        logs, level).  Returns {key: the rows this call added to that scorer's angle log} (none without args.debug).
        `rows`: None, or the derived addends int[n,4] of these rows (activity.ADDS): column 0 goes to REBA's activity score,
        columns 1..3 to RULA's muscle use, row by row, on top of add_info's constants."""
        added = {}
        for key, run, scorer in (('reba', self.run_reba, self.reba), ('rula', self.run_rula, self.rula)):
            if run:
                seen = len(scorer.log)
                if rows is None:
                    results = scorer(out['result'], out['joint_cam'], add_info)
                else:
                    results = scorer(out['result'], out['joint_cam'], add_info,
                                     rows=np.ascontiguousarray(rows[:, 0] if key == 'reba' else rows[:, 1:4]))
                final, scores, logs = self.post_processing(results)
                out[key] = (final, scores, logs, scorer.action_level(final[4]))
                added[key] = scorer.log[seen:]
        return added

    def score_crops(self, crop_batches, add_info=None, n_total=None, with_smpl_params=False):
        """crops -> dict(result, joint_cam, reba=(final, scores, logs, level), rula=(...)).
        `n_total`: see get_pose_estimation_results (the batches are this rank's shard of n_total frames).
        `with_smpl_params`: the dict also holds rotmat, betas, cam and the add_info used (what render_overlay needs)."""
        add_info = _information(add_info)
        params = {} if with_smpl_params else None
        result, joint_cam, _, debug_result = self.get_pose_estimation_results(crop_batches, keep_images=False,
                                                                              n_total=n_total, smpl_params=params)
        out = dict(result=result, joint_cam=joint_cam, debug_result=debug_result)
        if with_smpl_params:
            out.update(params, add_info=add_info)
        self._run_scorers(out, add_info)
        return out

    def _smooth_rows(self, smpl, people, fidx, median_radius, sigma):
        """The smoothing knobs' half of _score_tracks: every person's rows of the network's rotmat, betas and cam (`smpl`, host
        arrays, person after person) are smoothed along their track in ONE call (smooth.smooth_tracks: windows on the frame
        numbers `fidx`, never across people), `smpl` is updated with the smoothed arrays, and the back half is run again from
        the smoothed rotations as get_pose_estimation_results runs it: ops.pose_to_euler, then the SMPL layer's joint_cam,
        which overwrites the axis-angle root rows with (3.14, 0, 0) -> (result, joint_cam, debug_result, {'status',
        'replaced'} i32[n])."""
        from poserisk_release_amd import ops, smooth
        layer = self.smpl_model.layer['neutral']
        dev = layer.device
        track_start = np.cumsum([0] + [len(f) for _, _, f in people]).astype(np.int64)
        sm = smooth.smooth_tracks(torch.as_tensor(smpl['rotmat'], device=dev), np.asarray(fidx, np.int64), track_start, median_radius,
                                  sigma, betas=torch.as_tensor(smpl['betas'], device=dev), cam=torch.as_tensor(smpl['cam'], device=dev))
        aa, eul, st = ops.pose_to_euler(sm['rotmat'])
        n = aa.shape[0]
        joint_cam = torch.empty((n, 24, 3), dtype=torch.float32, device=dev)
        for lo in range(0, n, self.batch_size):                     # the SMPL layer takes batch_size rows a call
            layer.joint_cam(aa[lo:lo + self.batch_size], out=joint_cam[lo:lo + self.batch_size])
        status = st.cpu().numpy()
        if np.any(status != 0):     # as get_pose_estimation_results: the reference aborts on these
            raise AssertionError(f"invalid rotation after smoothing in rows {np.nonzero(status)[0].tolist()}")
        smpl.update({k: sm[k].cpu().numpy() for k in ('rotmat', 'betas', 'cam')})
        flags = {k: sm[k].cpu().numpy() for k in ('status', 'replaced')}
        return eul.cpu().numpy(), joint_cam.cpu().numpy(), aa.cpu().numpy(), flags

    def _activity_rows(self, rotmat, people, fidx, fps, parameters):
        """The activity knob's half of _score_tracks: ONE activity.activity_tracks call over everybody's rows of `rotmat` (host
        f32[n,24,3,3], person after person; windows on the frame numbers `fidx`, never across people) -> (flags i32[n,4],
        adds i32[n,4], the parameters in seconds and frames), host arrays."""
        from poserisk_release_amd import activity
        dev = self.smpl_model.layer['neutral'].device
        track_start = np.cumsum([0] + [len(f) for _, _, f in people]).astype(np.int64)
        act = activity.activity_tracks(torch.as_tensor(rotmat, device=dev), np.asarray(fidx, np.int64), track_start, fps, **parameters)
        return act['flags'].cpu().numpy(), act['adds'].cpu().numpy(), act['parameters']

    def _score_tracks(self, frames, people, add_info, bgr, bbox_scale, shard=None, with_smpl_params=False, fps=None):
        """The one scoring pass under score_frames and score_people: people [(id, bboxes f32[n,4], frame indices int[n])] -> (a
        dict per person as score_frames returns it, each person's rows of the scorers' angle logs).  Everybody's (frame index,
        box) rows are concatenated, cut into batches of self.batch_size across person boundaries (sum(n_p) / batch_size launches,
        rounded up once), cropped and run through get_pose_estimation_results once, and split back by offsets; the scorers and
        the aggregation run per person on the host.  `shard(bboxes, fidx)`, a sharding caller's, runs after the range check ->
        (lo, hi, n_total): the crops cover rows [lo, hi), this rank's, of the n_total the results are gathered to.
        With a smoothing knob positive (smooth_median_radius, smooth_sigma) the rows go through _smooth_rows between the model
        and the split: each dict then holds the smoothed values and 'smooth'; with both 0 nothing here differs.
        With the activity knob on (self.activity) the rotations -- the smoothed ones where smoothing is on -- go through
        _activity_rows once, each person's derived addends reach the scorers as `rows`, and each dict holds 'activity'
        (parameters, flags, adds); `fps` is then needed (ValueError without).  Off, nothing here differs."""
        from poserisk_release_amd import ops
        deriving = getattr(self, 'activity', None)
        if deriving is not None and fps is None:
            raise ValueError("the activity knob (cfg.ACTIVITY.derive / args.derive_activity) needs fps to turn its seconds into "
                             "frames: pass fps= to score_frames / score_people (Predictor.__call__ does)")
        frames = self._on_device(frames)
        if bbox_scale is None:
            bbox_scale = cfg.DATASET.bbox_scale                                   # base.py:121
        add_info = _information(add_info)
        bboxes = np.concatenate([b.reshape(-1, 4) for _, b, _ in people]) if people else np.zeros((0, 4), np.float32)
        fidx = np.concatenate([np.asarray(f).reshape(-1) for _, _, f in people]) if people else np.zeros((0,), np.int64)
        if len(fidx) and (int(np.min(fidx)) < 0 or int(np.max(fidx)) >= frames.shape[0]):
            raise ValueError(f"tracking results name frames {int(np.min(fidx))}..{int(np.max(fidx))} but only "
                             f"{frames.shape[0]} frames were decoded (tracking.pkl does not belong to these frames)")
        lo, hi, n_total = shard(bboxes, fidx) if shard is not None else (0, len(fidx), None)

        def batches():
            for i in range(lo, hi, self.batch_size):
                j = min(i + self.batch_size, hi)
                yield ops.crop_frames(frames, bboxes[i:j], fidx[i:j].astype(np.int32), scale=bbox_scale, bgr=bgr)
        smooth_m, smooth_sigma = getattr(self, 'smooth_median_radius', 0), getattr(self, 'smooth_sigma', 0.0)
        smoothing = smooth_m > 0 or smooth_sigma > 0
        smpl = {} if with_smpl_params or smoothing or deriving is not None else None
        result, joint_cam, _, debug_result = self.get_pose_estimation_results(batches(), keep_images=False, n_total=n_total,
                                                                              smpl_params=smpl)
        if smoothing:
            # every rank holds all rows after the gather and smooths the same ones: no further collective
            result, joint_cam, debug_result, smooth_flags = self._smooth_rows(smpl, people, fidx, smooth_m, smooth_sigma)
        if deriving is not None:
            # as with smoothing, every rank computes on the gathered rows
            act_flags, act_adds, act_parameters = self._activity_rows(smpl['rotmat'], people, fidx, fps, deriving)
        outs, pose_logs, at = [], [], 0
        for _, box_p, frames_p in people:
            rows = slice(at, at + len(frames_p))
            out = dict(result=result[rows], joint_cam=joint_cam[rows], debug_result=debug_result[rows])
            if with_smpl_params:
                out.update({k: v[rows] for k, v in smpl.items()}, add_info=add_info)
            if smoothing:
                out['smooth'] = dict(median_radius=smooth_m, sigma=smooth_sigma, status=smooth_flags['status'][rows],
                                     replaced=smooth_flags['replaced'][rows])
            if deriving is not None:
                out['activity'] = dict(parameters=act_parameters, flags=act_flags[rows], adds=act_adds[rows])
                pose_logs.append(self._run_scorers(out, add_info, rows=act_adds[rows]))
            else:
                pose_logs.append(self._run_scorers(out, add_info))
            out['frames'], out['bboxes'] = frames_p, box_p
            if with_smpl_params:
                out['bbox_scale'] = float(bbox_scale)
            outs.append(out)
            at = rows.stop
        return outs, pose_logs

    def score_frames(self, frames, tracking_results, add_info=None, bgr=False, bbox_scale=None, with_smpl_params=None, fps=None):
        """Decoded frames + tracker output -> scores, all on the GPU (BASELINE config 5 without the detector).
        `with_smpl_params` (default: the render_mesh knob): also return the network's rotmat, betas and cam per track frame
        (and the add_info used), which render_overlay draws from.  `fps`: the video's frame rate, needed (ValueError without)
        only with the activity knob on.

        frames: uint8[F,H,W,3] (torch CUDA tensor or numpy); tracking_results: multi_person_tracker's dict
        {id: {'bbox': [n,4] (cx,cy,w,h), 'frames': [n]}}.  Does what base.py:53-73 (track filter + target
        selection), demo_dataset.py:58-74 (crop) and base.py:126-182 (pose, scores) do."""
        from poserisk_release_amd import tracks
        target = (None,) + tracks.target_track(tracking_results, len(frames), cfg.DATASET.min_frame_ratio)

        def shard(bboxes, fidx):
            # one process per GPU: this rank crops and scores its contiguous shard of the track
            world, rank = pl.world_and_rank()
            if world > 1:
                # the shard bounds and the gather's shapes follow from the track: a rank that selected another one (its own
                # tracker run, another file) would hang the collective or gather rows that are not its frames -- compare first
                import hashlib
                import torch.distributed as dist
                mine = (len(frames), len(fidx),
                        hashlib.sha256(np.ascontiguousarray(fidx).tobytes() + np.ascontiguousarray(bboxes).tobytes()).hexdigest())
                seen = [None] * world
                dist.all_gather_object(seen, mine)
                if any(s != seen[0] for s in seen):
                    raise RuntimeError(f"the ranks do not hold the same target track (frames, track length, digest per rank: "
                                       f"{[s[:2] + (s[2][:8],) for s in seen]}): run the front end on one rank and broadcast its "
                                       "output (Predictor.__call__ does), or pass every rank the same frames and tracking dict")
            return pl.shard_bounds(len(fidx), world, rank) + (len(fidx) if world > 1 else None,)
        return self._score_tracks(frames, [target], add_info, bgr, bbox_scale, shard,
                                  self.render_mesh if with_smpl_params is None else with_smpl_params, fps=fps)[0][0]

    def score_people(self, frames, tracking_results, add_info=None, bgr=False, bbox_scale=None, with_smpl_params=None, fps=None):
        """Decoded frames + tracker output -> the scores of EVERY person tracks.people_tracks keeps, in one pass over the model:
        {'people': [out_0, out_1, ...], 'ids': [...], 'frames_total': F}, in people_tracks order (element 0 is the person
        score_frames scores).  Each out_p holds what score_frames returns for that person alone -- result, joint_cam,
        debug_result, reba, rula, frames, bboxes -- bit for bit: a frame's bits do not depend on its batch
        (tests/test_encoder_batch_sweep.py), so the people share batches (_score_tracks).  With args.debug the dict also holds
        'pose_logs', each person's rows of the scorers' angle logs.  `with_smpl_params` (default: the people_mesh knob): every
        out_p also holds rotmat, betas, cam, add_info and bbox_scale, as score_frames(with_smpl_params=True) returns them for
        that person alone; render_people draws from them.  `fps`: as for score_frames.

        Not supported, by name: several ranks (hip_world_size / args.world_size > 1) and the render_mesh knob
        (pr_render_overlay draws one mesh per canvas)."""
        from poserisk_release_amd import tracks
        world, _ = pl.world_and_rank()
        if world > 1:
            raise NotImplementedError(f"score_people runs on one rank, this process group has {world}: persons='all' does not go "
                                      "with hip_world_size / args.world_size > 1")
        if self.render_mesh:
            raise NotImplementedError("score_people does not go with the render_mesh knob: pr_render_overlay draws one mesh per "
                                      "canvas (cfg.DATASET.render_mesh / args.render_mesh)")
        n_frames = len(frames)
        people = tracks.people_tracks(tracking_results, n_frames, cfg.DATASET.min_frame_ratio)
        if with_smpl_params is None:
            with_smpl_params = getattr(self, 'people_mesh', False)
        outs, pose_logs = self._score_tracks(frames, people, add_info, bgr, bbox_scale, with_smpl_params=bool(with_smpl_params), fps=fps)
        people_out = {'people': outs, 'ids': [pid for pid, _, _ in people], 'frames_total': n_frames}
        return dict(people_out, pose_logs=pose_logs) if self.debugging else people_out

    # ---- the mesh overlay (extends the --debug_frame mesh of base.py:273-282 to every track frame) -----------------
    def render_overlay(self, out, frames, title='REBA', bgr=False, alpha=0.6):
        """Yield (track frame numbers int[b], overlaid frames u8[b,H,W,3] CUDA) batch by batch: the fitted mesh of every
        track frame drawn over its video frame (poserisk_release_amd.render), parts coloured by the `title` scheme's
        risk levels ('REBA' / 'RULA'; None: one neutral colour).  `out` is what score_frames returned with the SMPL
        parameters.  The pose is rebuilt from the returned rotmat (ops.pose_to_euler's axis-angle: the root keeps the
        network's rotation, it is NOT overwritten as the scores' pose is), betas from the prediction, vertices from
        smpl_model.layer['neutral']; `frames` and the output share one channel order (`bgr`)."""
        from poserisk_release_amd import ops, render
        if 'rotmat' not in out:
            raise ValueError("render_overlay needs score_frames(..., with_smpl_params=True) (or the render_mesh knob)")
        scheme, faces, face_part, frames, dev, faces_dev = self._mesh_setup(frames, title)
        fidx, n = np.asarray(out['frames']), len(out['frames'])
        info = out.get('add_info') or default_information()
        for i in range(0, n, self.batch_size):
            j = min(i + self.batch_size, n)
            verts, rgb = self._posed_meshes(out['rotmat'][i:j], out['betas'][i:j], info, scheme, dev)
            img = render.overlay(frames, verts, faces_dev, out['cam'][i:j], out['bboxes'][i:j],
                                 scale=out.get('bbox_scale', cfg.DATASET.bbox_scale), frame_idx=fidx[i:j].astype(np.int32),
                                 face_part=face_part, part_rgb=rgb, alpha=alpha, bgr=bgr)
            yield fidx[i:j], img

    def _mesh_setup(self, frames, title):
        """What render_overlay and render_people share before their loops -> (scheme, the model's faces, face_part by the
        scheme, frames on the device, that device, the faces on it)."""
        from poserisk_release_amd import render
        faces = np.asarray(self.smpl_model.face)
        if faces.ndim != 2 or faces.shape[0] == 0:
            raise ValueError("the SMPL model has no faces to draw")
        scheme = None if title is None else str(title).upper()
        face_part = render.face_parts(self.smpl_model.layer['neutral'].th_weights.numpy(), faces, scheme)
        frames = self._on_device(frames)
        return scheme, faces, face_part, frames, frames.device, torch.as_tensor(faces.astype(np.int32), device=frames.device)

    def _posed_meshes(self, rotmat, betas, info, scheme, dev):
        """rotmat f32[n,24,3,3] + betas f32[n,10] (n <= batch_size) -> (vertices f32[n,V,3] on `dev`, part_rgb u8[n,P,3]): the
        meshes render_overlay and render_people draw and their parts' colours by the scheme's risk levels of each row."""
        from poserisk_release_amd import ops, render
        n = len(rotmat)
        aa, eul, _ = ops.pose_to_euler(torch.as_tensor(rotmat, device=dev))
        verts, _ = self.smpl_model.layer['neutral'](aa.reshape(n, 72), torch.as_tensor(betas, device=dev))
        if scheme is None:
            return verts, render.part_colours(np.zeros((n, 1)), None)
        packed = (ops.reba if scheme == 'REBA' else ops.rula)(eul, info[scheme]).cpu().numpy()
        return verts, render.part_colours(packed, scheme)

    def render_people(self, people_out, frames, title='REBA', bgr=False, alpha=0.6):
        """Yield (video frame numbers int[b], frames u8[b,H,W,3] CUDA) over ALL frames of the video, batch_size frames at a
        time: the fitted mesh of every scored person who is in the frame drawn over it, the people depth-tested against each
        other (poserisk_release_amd.render.overlay_people, pr_render_people); a frame nobody is in comes back as it is.
        `people_out` is what score_people returned with the SMPL parameters.  Meshes as in render_overlay, each person's parts
        coloured by that person's own risk levels of that frame; the meshes of a frame are ordered as tracks.people_tracks
        orders the people, and their depth steps come from render.people_z_step, the cameras' size on the screen."""
        from poserisk_release_amd import render
        outs = people_out['people']
        if any('rotmat' not in o for o in outs):
            raise ValueError("render_people needs score_people(..., with_smpl_params=True) (or the people_mesh knob)")
        scheme, faces, face_part, frames, dev, faces_dev = self._mesh_setup(frames, title)
        n_frames, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        if not outs:
            raise ValueError("render_people: nobody was scored")
        scale = outs[0].get('bbox_scale', cfg.DATASET.bbox_scale)
        info = outs[0].get('add_info') or default_information()
        # every (person, track frame) row is a mesh, person after person: a selection of rows keeps the people's order
        cat = lambda key: np.concatenate([np.asarray(o[key]) for o in outs])
        fidx, cam, bboxes, rotmat, betas = cat('frames'), cat('cam'), cat('bboxes'), cat('rotmat'), cat('betas')
        z_step = render.people_z_step(cam, bboxes, scale, H, W)
        for lo in range(0, n_frames, self.batch_size):
            hi = min(lo + self.batch_size, n_frames)
            sel = np.nonzero((fidx >= lo) & (fidx < hi))[0]
            verts, rgb = [], []
            for i in range(0, len(sel), self.batch_size):               # the SMPL layer takes batch_size rows a call
                v, c = self._posed_meshes(rotmat[sel[i:i + self.batch_size]], betas[sel[i:i + self.batch_size]], info, scheme, dev)
                verts.append(v)
                rgb.append(c)
            verts = torch.cat(verts) if verts else torch.zeros((0, int(faces.max()) + 1, 3), device=dev)
            img = render.overlay_people(frames, verts, faces_dev, cam[sel], bboxes[sel], (fidx[sel] - lo).astype(np.int32),
                                        np.arange(lo, hi, dtype=np.int32), z_step[sel], scale=scale, face_part=face_part,
                                        part_rgb=np.concatenate(rgb) if rgb else None, alpha=alpha, bgr=bgr)
            yield np.arange(lo, hi), img

    def _open_sink(self, output_path, name, frame_size, fps, bgr):
        """<output>/<name>: the sink of the gpu_video_codec knob (poserisk_release_amd/sinks.py) for frames of (height, width) =
        `frame_size`, with this Predictor's other knobs."""
        return sinks.open_sink(self.gpu_video_codec, osp.join(output_path, name), int(frame_size[1]), int(frame_size[0]), fps, bgr,
                               quality=self.gpu_video_quality, chroma=self.video_chroma, encoder=self.video_encoder,
                               encoder_ext=self.video_encoder_ext, matrix=_yuv_matrix())

    def write_mesh_overlay(self, out, frames, output_path, title='REBA', bgr=False, fps=30.0):
        """<output>/<TITLE>_mesh.mp4 where cv2 is importable, else <output>/<TITLE>_mesh/%09d.png (frame number) per track
        frame.  Returns the path written."""
        sink = self._open_sink(output_path, f"{title if title is not None else 'MESH'}_mesh", frames.shape[1:3], fps, bgr)
        return sinks.write_all(sink, self.render_overlay(out, frames, title, bgr))

    def _write_canvases(self, canvases, frames, output_path, name, bgr, fps):
        """<output>/<name> through the sink of the gpu_video_codec knob: `canvases` yields the canvases of `frames`' video batch
        by batch, one per video frame, numbered 0 .. n_frames - 1.  Returns the path written."""
        from poserisk_release_amd import video
        canvas_h, resize_w, panel_w = video.canvas_size(int(frames.shape[1]), int(frames.shape[2]))

        def batches():
            i = 0
            for batch in canvases:
                yield range(i, i + int(batch.shape[0])), batch
                i += int(batch.shape[0])
        return sinks.write_all(self._open_sink(output_path, name, (canvas_h, resize_w + panel_w), fps, bgr), batches())

    # ---- base.py:284-327 on the GPU (the gpu_video knob) ---------------------------------------------------------
    def write_gpu_video(self, out, frames, output_path, title, bgr=False, fps=30.0, mesh_sink=None):
        """`<TITLE>_video`: every frame of the video at 720 px wide with the target's box, beside the score panel, composed by
        poserisk_release_amd.video (pr_compose_video) from the arrays score_frames returned.  <output>/<TITLE>_video.mp4 where
        cv2 is importable (it only writes the container), else <output>/<TITLE>_video/%09d.png, one per video frame; with
        gpu_video_codec 'mjpeg' <output>/<TITLE>_video.avi, the canvases encoded on the GPU, whether or not cv2 is there; with
        'png' <output>/<TITLE>_video/%09d.png, encoded on the GPU (lossless), whether or not cv2 is there; with 'y4m'
        <output>/<TITLE>_video.y4m, or through the video_encoder knob's command <TITLE>_video.mp4 (sinks.Y4mSink).  With
        the render_mesh knob the track frames are the mesh-overlaid ones, the box over the mesh (`out` must then hold the SMPL
        parameters: render_overlay says so by name), and `mesh_sink(frame numbers, images)` receives every overlaid batch, so
        that the mesh output is written from the same rendering.  Returns the path written."""
        from poserisk_release_amd import video
        frames = self._on_device(frames)
        n_frames, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        _, scores, logs, _ = out[title.lower()]
        items = (self.reba if title.upper() == 'REBA' else self.rula).eval_items
        fidx = np.asarray(out['frames'])
        draw = video.draw_list(title, n_frames, out['bboxes'], (0, fidx, n_frames), scores, items, logs, video.canvas_size(H, W)[0])
        overlay = None
        if self.render_mesh:
            def overlay(lo, hi):
                sel = np.nonzero((fidx >= lo) & (fidx < hi))[0]
                if not sel.size:
                    return [], None
                some = dict(out, frames=fidx[sel], bboxes=out['bboxes'][sel])
                some.update({k: out[k][sel] for k in ('rotmat', 'betas', 'cam') if k in out})
                parts = list(self.render_overlay(some, frames, title, bgr))      # raises by name without the SMPL parameters
                numbers, images = np.concatenate([f for f, _ in parts]), torch.cat([img for _, img in parts])
                if mesh_sink is not None:
                    mesh_sink(numbers, images)
                return numbers, images
        return self._write_canvases(video.annotated_frames(frames, draw, self.batch_size, overlay=overlay), frames, output_path,
                                    title + '_video', bgr, fps)

    # ---- the persons='all' outputs (no counterpart in the reference, which describes one person) -----------------------------
    def write_people_video(self, people_out, frames, output_path, title, bgr=False, fps=30.0, mesh_sink=None):
        """`<TITLE>_people`: every frame of the video at 720 px wide with every scored person's box and `#<id> <score>` tag in
        the colour of that frame's action level, beside a panel that lists the people of the frame
        (poserisk_release_amd.video.people_draw_list, pr_compose_people), from what score_people returned.  Written through
        the sink of the gpu_video_codec knob, as write_gpu_video's.  With the people_mesh knob the image region is
        render_people's frame, boxes and tags over the meshes (`people_out` must then hold the SMPL parameters), and
        `mesh_sink(frame numbers, images)` receives every rendered batch, so that <TITLE>_people_mesh is written from the same
        rendering.  Returns the path written."""
        from poserisk_release_amd import video
        frames = self._on_device(frames)
        n_frames, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        scorer = self.reba if title.upper() == 'REBA' else self.rula
        people = []
        for pid, out in zip(people_out['ids'], people_out['people']):
            scores = out[title.lower()][1]
            acts = [scorer.action_level(s) for s in scores]
            people.append(dict(id=pid, frames=out['frames'], bboxes=out['bboxes'], scores=scores, levels=[a[0] for a in acts],
                               names=[a[1] for a in acts]))
        canvas_h, resize_w, _ = video.canvas_size(H, W)
        draw = video.people_draw_list(title, n_frames, people, canvas_h, resize_w, H, W, bgr=bgr)
        overlay = None
        if getattr(self, 'people_mesh', False):
            meshed = self.render_people(people_out, frames, title, bgr)       # batch_size frames a step, as people_frames asks

            def overlay(lo, hi):
                numbers, images = next(meshed)
                if numbers[0] != lo or numbers[-1] != hi - 1:
                    raise RuntimeError(f"render_people yielded frames {numbers[0]}..{numbers[-1]} where {lo}..{hi - 1} are composed")
                if mesh_sink is not None:
                    mesh_sink(numbers, images)
                return numbers, images
        return self._write_canvases(video.people_frames(frames, draw, self.batch_size, overlay=overlay), frames, output_path,
                                    title + '_people', bgr, fps)

    def _write_reports(self, out, folder, debug_folder, n_frames, pose_logs, after_plot=lambda title: None, after_txt=lambda title: None):
        """One scored person's files.  Into `folder`, per title scored: <TITLE>_score.png, then <title>_result.txt.  With args.debug
        into `debug_folder`: pose_log.csv (the debug_joints) first, and per title, last, <TITLE>_score_log.csv and <TITLE>_eval_pose_log.csv
        from pose_logs[<title>], rows of the scorer's angle log.  after_plot / after_txt: what __call__ writes in between (videos, mesh)."""
        from poserisk_release_amd import reports
        timestamp = (0, np.asarray(out['frames']), n_frames)           # base.py:130
        if self.debugging and self.debug_joints is not None:
            reports.save_pose_log_csv(debug_folder, timestamp, reports.pose_to_str(out['result']), self.debug_joints,
                                      self.smpl_model.joints_name_upper)
        for title, scorer in (('REBA', self.reba), ('RULA', self.rula)):
            if title.lower() not in out:
                continue
            final, scores, logs, (level, name) = out[title.lower()]
            reports.save_score_plot(folder, title, timestamp, scores)      # base.py:254-262
            after_plot(title)
            reports.write_result_txt(folder, title, final, level, name)
            after_txt(title)
            if self.debugging:
                reports.save_score_csv(debug_folder, title, timestamp, scores, scorer.eval_items, logs, pose_logs[title.lower()])

    def write_people_reports(self, people_out, output_path):
        """<output>/person_<id>/ per scored person -- reba_result.txt / rula_result.txt and <TITLE>_score.png, with args.debug the
        score, pose-evaluation and pose logs too, all by the method that writes the target's (_write_reports) -- and
        <output>/people.json.  Returns the list people.json holds."""
        plain = lambda v: v.item() if isinstance(v, np.generic) else v
        num = lambda v: None if v is None or np.isnan(v) else float(v)        # top-10 % of fewer than 10 frames is NaN: null
        n_frames, summary = people_out['frames_total'], []
        for p, (pid, out) in enumerate(zip(people_out['ids'], people_out['people'])):
            folder = osp.join(output_path, f'person_{pid}')
            os.makedirs(folder, exist_ok=True)
            self._write_reports(out, folder, folder, n_frames, people_out['pose_logs'][p] if self.debugging else None)
            fidx, boxes = np.asarray(out['frames']), np.asarray(out['bboxes'])
            entry = dict(id=plain(pid), first_frame=int(fidx.min()) if fidx.size else None, last_frame=int(fidx.max()) if fidx.size else None,
                         n_frames=int(fidx.size), mean_box_area=float((boxes[:, 2] * boxes[:, 3]).mean()) if fidx.size else None)
            for title in ('REBA', 'RULA'):
                if title.lower() in out:
                    final, _, _, (level, name) = out[title.lower()]
                    entry[title] = dict(avg=num(final[0]), top50=num(final[1]), top10=num(final[2]), max=num(final[3]), mode=num(final[4]),
                                        action_level=plain(level), action=name)
            summary.append(entry)
        with open(osp.join(output_path, 'people.json'), 'w') as f:
            json.dump({'frames_total': n_frames, 'people': summary}, f, indent=1)
        return summary

    def write_smooth_report(self, out, people_out, output_path):
        """<output>/smooth.json, written only when a smoothing knob is on: the parameters (in frames) and per scored person
        (the target alone, id null, without persons 'all') how many (row, joint) items stage 1 replaced by another frame's
        rotation and how many fell back in stage 2 (pr_smooth_tracks' replaced and status bits).  Returns what it holds."""
        from poserisk_release_amd import smooth
        plain = lambda v: v.item() if isinstance(v, np.generic) else v
        scored = list(zip(people_out['ids'], people_out['people'])) if people_out is not None else [(None, out)]
        people = []
        for pid, o in scored:
            replaced, fallbacks = smooth.counts(o['smooth']['status'], o['smooth']['replaced'])
            people.append(dict(id=plain(pid), n_frames=int(len(o['smooth']['status'])), replaced=replaced, fallbacks=fallbacks))
        report = dict(median_radius=int(out['smooth']['median_radius']), sigma=float(out['smooth']['sigma']), unit='frames',
                      gaussian_radius=smooth.gaussian_radius(float(out['smooth']['sigma'])), people=people)
        with open(osp.join(output_path, 'smooth.json'), 'w') as f:
            json.dump(report, f, indent=1)
        return report

    def write_activity_report(self, out, people_out, output_path):
        """<output>/activity.json, written only with the activity knob on: the parameters in seconds, degrees and frames, and
        per scored person (the target alone, id null, without persons 'all') the rows flagged per kind -- held, repeated,
        rapid, moved -- in all and per joint name, and the sum of each derived addend.  Returns what it holds."""
        from poserisk_release_amd import activity
        plain = lambda v: v.item() if isinstance(v, np.generic) else v
        scored = list(zip(people_out['ids'], people_out['people'])) if people_out is not None else [(None, out)]
        people = []
        for pid, o in scored:
            adds = np.asarray(o['activity']['adds']).reshape(-1, 4)
            people.append(dict(id=plain(pid), n_frames=int(len(adds)), **activity.counts(o['activity']['flags']),
                               adds={name: int(adds[:, c].sum()) for c, name in enumerate(activity.ADDS)}))
        report = dict(parameters={k: plain(v) for k, v in out['activity']['parameters'].items()}, joints=list(activity.JOINT_NAMES),
                      people=people)
        with open(osp.join(output_path, 'activity.json'), 'w') as f:
            json.dump(report, f, indent=1)
        return report

    # ---- base.py:273-282 ------------------------------------------------------------------------------------
    def visualize_joint_cam_mesh(self, debug_result, joint_cam, frames, output_path):
        """The --debug --debug_frame N outputs: `smpl_model.obj` (the frame's mesh in mm, zero betas, from the axis-angle
        with the root already overwritten, Q5) and `joint_3d.png`."""
        from poserisk_release_amd import reports
        idx = int(np.where(np.asarray(frames) == self.debug_frame)[0][0])
        pose = torch.as_tensor(debug_result[idx]).reshape(1, -1).float()
        verts, _ = self.smpl_model.layer['neutral'](pose, torch.zeros((1, 10)))
        mesh = verts.detach().cpu().numpy().astype(np.float32).reshape(-1, 3) * 1000
        reports.save_obj(mesh, self.smpl_model.face, osp.join(output_path, 'smpl_model.obj'))
        reports.save_joint_3d_plot(joint_cam[idx], self.smpl_model.skeleton, osp.join(output_path, 'joint_3d.png'),
                                   frame=self.debug_frame)

    # ---- main/run.py:31  predictor(args.input, args.info, args.output) -----------------------------------
    def _folder_sidecars(self, folder, frames=None):
        """What every frame folder carries beside its frames -> (fps, tracking): `fps.txt` (optional, 30.0 without it) and
        `tracking.pkl`; without that file and with cfg.TRACKER.weights set, the built-in tracker's dict for `frames`."""
        import pickle
        if frames is not None and self._tracker_weights() and not osp.isfile(osp.join(folder, 'tracking.pkl')):
            tracking = self.track_frames(frames, bgr=False)
        else:
            with open(osp.join(folder, 'tracking.pkl'), 'rb') as f:
                tracking = pickle.load(f)
        fps_file = osp.join(folder, 'fps.txt')
        fps = float(open(fps_file).read()) if osp.isfile(fps_file) else 30.0
        return fps, tracking

    def load_front_end(self, input_path, output_path, tracking_results=None):
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
            return (frames, False) + self._folder_sidecars(input_path, frames)
        if osp.isdir(input_path) and (osp.isfile(osp.join(input_path, 'tracking.pkl')) or self._tracker_weights()):
            from poserisk_release_amd import jpeg, png
            module, opts = jpeg, _jpeg_options()
            if png.list_frames(input_path) and not any(n.lower().endswith(('.jpg', '.jpeg')) for n in os.listdir(input_path)):
                module, opts = png, {}
            names = module.list_frames(input_path)
            if names:
                frames = self._decode_frames(module, [osp.join(input_path, n) for n in names], **opts)
                return (frames, False) + self._folder_sidecars(input_path, frames)
        not_mjpeg = None
        if osp.isfile(input_path):
            from poserisk_release_amd import mjpeg, y4m
            if mjpeg.is_avi(input_path):
                try:
                    reader = mjpeg.AviReader(input_path)
                except ValueError as e:
                    not_mjpeg = e                              # an AVI, but not one to read here: cv2 may still open it
                else:
                    return self._video_front_end(reader, input_path, output_path, tracking_results, **_jpeg_options())
            if y4m.is_y4m(input_path):
                with y4m.Reader(input_path) as reader:
                    return self._video_front_end(reader, input_path, output_path, tracking_results,
                                                 matrix=_yuv_matrix())
            if self.video_decoder:
                return self._decoder_front_end(input_path, output_path, tracking_results)
        try:
            import cv2
            from multi_person_tracker import MPT
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
        tracker = MPT(device=self.device, batch_size=8, display=False, detection_threshold=0.1, detector_type='yolo',
                      output_format='dict', yolo_img_size=416)
        tracking = tracker(image_path)
        frames = np.stack([cv2.imread(osp.join(image_path, '{0:09d}.jpg'.format(i))) for i in range(n)])
        shutil.rmtree(image_path, ignore_errors=True)
        return frames, True, fps, tracking

    def _decode_frames(self, module, paths, written_to=None, **opts):
        """`paths` (files, or their bytes) decoded by `module` (jpeg | png: decode_files with `opts`) -> the frames on the device.  The
        first bad frame raises RuntimeError naming its file -- for bytes written to a tracker's folder `written_to`, its number there."""
        frames, status = module.decode_files(paths, self.device, **opts)
        bad = module.bad_frames(paths, status, **{k: opts[k] for k in ('progressive',) if k in opts})
        if bad and written_to is not None:
            raise RuntimeError(f"{written_to!r}: frame {bad[0][0]} written for the tracker cannot be decoded: {bad[0][1]}")
        if bad:
            raise RuntimeError(f"{paths[bad[0][0]]!r} cannot be decoded: {bad[0][1]}"
                               + (f" (and {len(bad) - 1} more frames)" if len(bad) > 1 else ""))
        return frames

    def _video_front_end(self, reader, input_path, output_path, tracking_results=None, **opts):
        """load_front_end's cases 3, 3b and 3c: `reader` is the mjpeg.AviReader of `input_path` (`opts`: the JPEG options), or the
        y4m.Reader of `input_path` or of a decoder's standard output (`opts`: the colour matrix)."""
        from poserisk_release_amd import frontend
        frames, fps = frontend.read_video(reader, self.device, **_front_limits(), **opts)
        return self._tracking_for(frames, fps, input_path, output_path, tracking_results)

    def _decoder_front_end(self, input_path, output_path, tracking_results=None):
        """load_front_end's case 3c: self.video_decoder, with {input} replaced, runs as a child process whose standard output
        is read as YUV4MPEG2.  Never a shell and never this process's own program; the child is reaped whatever happens."""
        import shlex
        from poserisk_release_amd import _child, y4m
        if '{input}' not in self.video_decoder:
            raise ValueError(f"video_decoder {self.video_decoder!r} must be a command line containing {{input}}")
        child = _child.Child([a.replace('{input}', input_path) for a in shlex.split(self.video_decoder)],
                             f"{input_path!r}: the video decoder", feed=False)
        failure, read_to_the_end = None, False
        try:
            try:
                reader = y4m.Reader(child.pipe)
            except ValueError as e:
                failure = f"it wrote no YUV4MPEG2 stream header ({e})"
            else:
                try:
                    return_value = self._video_front_end(reader, input_path, output_path, tracking_results,
                                                         matrix=_yuv_matrix())
                    read_to_the_end = True
                except ValueError as e:                         # the stream broke off: the child's status says why
                    failure = str(e)
        finally:
            child.pipe.close()                  # a child still writing gets EPIPE and ends by itself; its status raises nothing
            child.finish(60 if read_to_the_end else 5, failure, raising=read_to_the_end or failure is not None)    # over another error
        return return_value

    # ---- the built-in tracker (cfg.TRACKER; off while its weights are '') --------------------------------------------------
    @staticmethod
    def _tracker_weights():
        return str(cfg.get('TRACKER', {}).get('weights', '') or '')

    def track_frames(self, frames, bgr=False):
        """frames u8[F,H,W,3] (device tensor or numpy) -> multi_person_tracker's dict, by this package's own detector
        (poserisk_release_amd.detector, YOLOv3 on the GPU) and tracker (poserisk_release_amd.sort).  No person found anywhere
        raises RuntimeError naming the threshold used."""
        from poserisk_release_amd import detector, sort
        t = cfg.TRACKER
        det = getattr(self, '_detector', None)
        key = (self._tracker_weights(), tuple(t.img_size), int(t.batch), str(t.get('precision', 'fp32')))
        detector.check_precision(key[3])        # 'fp32' | 'bf16', anything else raises naming the two
        if det is None or getattr(self, '_detector_key', None) != key:
            det = detector.Detector(key[0], img_size=key[1], device=self.device, max_batch=key[2], precision=key[3])
            self._detector, self._detector_key = det, key
        dets = det.detect(frames, bgr=bgr, conf_thres=float(t.conf_thres), nms_thres=float(t.nms_thres))
        tracking = sort.track_frames(dets, max_age=int(t.max_age), min_hits=int(t.min_hits), iou_thres=float(t.iou_thres))
        if not tracking:
            raise RuntimeError(f"the built-in tracker found no person track in {len(dets)} frames ({sum(len(d) for d in dets)} "
                               f"detections at conf_thres {float(t.conf_thres):g}, nms_thres {float(t.nms_thres):g}; a track needs "
                               f"{int(t.min_hits)} consecutive hits)")
        return tracking

    def _tracking_for(self, frames, fps, input_path, output_path, tracking_results=None):
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
        if self._tracker_weights():
            return frames, False, fps, self.track_frames(frames, bgr=False)
        try:
            from multi_person_tracker import MPT
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
            tracker = MPT(device=self.device, batch_size=8, display=False, detection_threshold=0.1, detector_type='yolo',
                          output_format='dict', yolo_img_size=416)
            tracking = tracker(image_path)
            frames = self._decode_frames(jpeg, files, written_to=image_path, **_jpeg_options())
        finally:
            shutil.rmtree(image_path, ignore_errors=True)
        return frames, False, fps, tracking

    def _front_end_on_rank0(self, input_path, output_path, world, rank, **given):
        """Several ranks (one per GPU): the front end writes, runs the tracker in and deletes <output>/tmp, so it runs on
        rank 0 ONLY and its output is broadcast -- every rank then shards the SAME track (a tracker run per rank may select
        different tracks; one rank's rmtree would delete JPEGs another rank is still reading).  The metadata goes as one
        pickled object, the frames as one uint8 tensor (on this rank's GPU with RCCL, on the host with gloo)."""
        import torch.distributed as dist
        meta, err = [None], None
        frames = None
        if rank == 0:
            try:
                frames, bgr, fps, tracking = self.load_front_end(input_path, output_path, **given)
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
            frames = torch.empty(m['shape'], dtype=torch.uint8, device=self.device if on_gpu else 'cpu')
        elif on_gpu:
            frames = frames.to(self.device)
        else:
            frames = frames.cpu()                    # gloo broadcasts host memory
        dist.broadcast(frames, src=0)
        return frames, m['bgr'], m['fps'], m['tracking']

    def __call__(self, input_path, info_path, output_path, frames=None, tracking_results=None, fps=30.0, bgr=False):
        """The reference's entry point (base.py:126-209) around the accelerated path: front end (given, found or
        the reference's own: `load_front_end`) -> crops, pose, scores on the GPU -> `reba_result.txt` /
        `rula_result.txt`, `<TITLE>_score.png`, `<TITLE>_video.mp4` (OpenCV drawing: only where cv2 is importable; with
        the gpu_video knob composed on the GPU instead, see write_gpu_video) and with `args.debug` the CSV logs under <output>/debug.  Returns the dict of `score_frames` plus `fps`.
        With the persons knob at 'all' all of that is written for the target from score_people's element 0 (the model runs
        once), then <output>/person_<id>/, <output>/people.json and, with gpu_video, <TITLE>_people (write_people_reports,
        write_people_video); the dict returned also holds 'people', what score_people returned."""
        from poserisk_release_amd import reports
        os.makedirs(output_path, exist_ok=True)
        world, rank = pl.world_and_rank()
        if frames is None or tracking_results is None:
            # tracking given without frames: a Motion-JPEG AVI input takes it (load_front_end, case 3); every other input
            # brings its own, as before
            given = {'tracking_results': tracking_results} if frames is None and tracking_results is not None else {}
            if world > 1:
                frames, bgr, fps, tracking_results = self._front_end_on_rank0(input_path, output_path, world, rank, **given)
            else:
                frames, bgr, fps, tracking_results = self.load_front_end(input_path, output_path, **given)
        add_info = _information(info_path if info_path and osp.isfile(str(info_path)) else None)      # base.py:140-142
        people_out = None
        if getattr(self, 'persons', 'target') == 'all':
            # everybody in one pass; the target is element 0, bit for bit what score_frames returns, so the model runs once
            people_out = self.score_people(frames, tracking_results, add_info, bgr=bgr, fps=fps)
            out = dict(people_out['people'][0])
            out['people'] = people_out
        else:
            out = self.score_frames(frames, tracking_results, add_info, bgr=bgr, fps=fps)
        out['fps'] = fps
        if rank != 0:
            # every rank holds all frames' results after the gather; the reports (result txt, plots, mp4, debug CSVs and
            # OBJ) are ONE set of files in <output>: rank 0 writes them, the others would race it on the same names
            return out
        if 'smooth' in out:                                        # only with a smoothing knob on
            self.write_smooth_report(out, people_out, output_path)
        if 'activity' in out:                                      # only with the activity knob on
            self.write_activity_report(out, people_out, output_path)
        fidx = out['frames']
        timestamp = (0, fidx, int(frames.shape[0]))                # base.py:130 (torch tensor or numpy: both have .shape)
        debug_path = osp.join(output_path, 'debug')
        if self.debugging:
            os.makedirs(debug_path, exist_ok=True)
        if self.debugging and self.debug_frame is not None and self.debug_frame >= 0:
            # base.py:128-135: the --debug_frame branch dumps that frame's mesh and 3-D skeleton and stops there
            self.visualize_joint_cam_mesh(out['debug_result'], out['joint_cam'], fidx, debug_path)
            if self.render_mesh:
                idx = int(np.where(np.asarray(fidx) == self.debug_frame)[0][0])
                one = dict(out, frames=fidx[idx:idx + 1], bboxes=out['bboxes'][idx:idx + 1], rotmat=out['rotmat'][idx:idx + 1],
                           betas=out['betas'][idx:idx + 1], cam=out['cam'][idx:idx + 1])
                title = 'REBA' if 'reba' in out else ('RULA' if 'rula' in out else None)
                for _, img in self.render_overlay(one, frames, title, bgr):
                    im = img[0].cpu().numpy()
                    sinks.save_png(osp.join(debug_path, 'mesh_overlay.png'), im[..., ::-1] if bgr else im)
            print("\n Debug files are saved in : ", debug_path)
            return out
        show = getattr(self, 'visualize', True)
        on_gpu = show and self.gpu_video
        if on_gpu:
            frames = torch.as_tensor(frames).to(self.device)       # one upload for both titles' videos (and the mesh)

        def with_mesh_sink(name, write):                           # one rendering of the meshes feeds the video and <output>/<name>
            mesh = self._open_sink(output_path, name, frames.shape[1:3], fps, bgr)
            try:
                write(mesh.put)
            except BaseException:
                mesh.abort()                    # the video's error stands; a mesh encoder child is reaped all the same
                raise
            mesh.close()

        def videos(title):                                         # base.py:156,173: behind the title's plot
            if on_gpu:
                if self.render_mesh:                # one rendering of the mesh feeds both outputs
                    with_mesh_sink(title + '_mesh', lambda put: self.write_gpu_video(out, frames, output_path, title, bgr, fps, mesh_sink=put))
                else:
                    self.write_gpu_video(out, frames, output_path, title, bgr, fps)
            elif show:                                             # ... (OpenCV only)
                _, scores, logs, _ = out[title.lower()]
                fr = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)   # once, host side
                video = reports.write_annotated_video(output_path, title, fr if bgr else fr[..., ::-1], out['bboxes'], timestamp, fps,
                                                      scores, (self.reba if title == 'REBA' else self.rula).eval_items, logs)
                if video is None and not getattr(self, '_warned_no_cv2', False):
                    print("OpenCV (cv2) is not importable: the annotated mp4 is skipped, all other outputs are written")
                    self._warned_no_cv2 = True

        def mesh_alone(title):                                     # behind the title's result txt
            if self.render_mesh and not on_gpu:                    # with both knobs videos() has written the mesh
                self.write_mesh_overlay(out, frames, output_path, title, bgr, fps)
        # the scorers' whole angle logs, as the reference writes them (Q19: they are never cleared)
        self._write_reports(out, output_path, debug_path, timestamp[2], {'reba': self.reba.log, 'rula': self.rula.log}, videos, mesh_alone)
        if people_out is not None:
            self.write_people_reports(people_out, output_path)
            people_mesh = getattr(self, 'people_mesh', False)
            if on_gpu:
                for title in ('REBA', 'RULA'):
                    if title.lower() not in out:
                        continue
                    if people_mesh:                     # one rendering of the meshes feeds both outputs, as in videos()
                        with_mesh_sink(title + '_people_mesh',
                                       lambda put: self.write_people_video(people_out, frames, output_path, title, bgr, fps, mesh_sink=put))
                    else:
                        self.write_people_video(people_out, frames, output_path, title, bgr, fps)
            elif show:
                print("The people video (<TITLE>_people) is composed on the GPU only: it needs the gpu_video knob and is skipped")
                if people_mesh:
                    print("The people mesh (<TITLE>_people_mesh) is drawn beside it: it needs the gpu_video knob too and is skipped")
        return out
