"""Mirror of the hot-path half of lib/core/base.py::Predictor.

    predictor = Predictor(args)                                       main/run.py:31
    result, joint_cam, images, debug_result = predictor.get_pose_estimation_results(loader)   base.py:126
    reba_results = predictor.reba(result, joint_cam, add_info)        base.py:151
    final, scores, logs = predictor.post_processing(reba_results, ...)  base.py:153

`get_pose_estimation_results` is the reference's loop (base.py:211-240) with the per-frame Python
removed: every batch is one `pr_frames_forward` call on the GPU, results stay on the device until the
end of the loop, and with `torch.distributed` initialised every rank takes a contiguous frame shard and
the per-frame records are all-gathered once.  This file holds the Predictor's construction, its knobs and
its scoring.  Where `__call__`'s frames and tracking come from (base.py:47-74, outside the accelerated path:
DESIGN.md section 7) is core/front_end.py, what it writes once the scores are there is core/outputs.py; the
Predictor's methods of those names are their functions.
"""
import json
import os
import os.path as osp

import numpy as np
import torch

from poserisk_release_amd import pipeline as pl
from poserisk_release_amd import synth
from poserisk_release_amd.hmr import hmr

from core import front_end, outputs
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


def _video_output_knobs(args):
    """-> (gpu_video_codec, video_encoder, video_encoder_ext, video_chroma, gpu_video_quality), cross-checked: an encoder command
    needs its {output}, is fed YUV4MPEG2 and so implies the 'y4m' codec."""
    codec = outputs.known_codec(str(_knob(args, 'video_codec', 'gpu_video_codec', '')))
    encoder = str(_knob(args, 'video_encoder', 'video_encoder', ''))
    if encoder:
        if '{output}' not in encoder:
            raise ValueError(f"video_encoder {encoder!r} must be a command line containing {{output}}")
        if codec not in ('', 'y4m'):
            raise ValueError(f"video_encoder is fed YUV4MPEG2: it goes with gpu_video_codec 'y4m' (or ''), not {codec!r}")
        codec = 'y4m'
    return (codec, encoder, str(_knob(args, 'video_encoder_ext', 'video_encoder_ext', '.mp4')),
            str(cfg.DATASET.get('video_chroma', '420mpeg2') or '420mpeg2'), int(cfg.DATASET.get('gpu_video_quality', 90)))


def track_start(people):
    """people [(id, bboxes, frame indices)] -> i64[len + 1]: where each person's rows start in the concatenation (and its end)."""
    return np.cumsum([0] + [len(f) for _, _, f in people]).astype(np.int64)


def _valid_rotations(status, where):
    """A non-zero rotation status (device i32[n]) raises, naming its rows: the reference aborts on these (coord_utils.py:70,91)."""
    status = status.cpu().numpy()
    if np.any(status != 0):
        raise AssertionError(f"invalid rotation {where} {np.nonzero(status)[0].tolist()}")


class Predictor:
    # what a Predictor that never ran __init__ (the CPU tests build such) answers for the knobs its methods read; __init__ sets them from
    # args and cfg, except `visualize`: main/run.py's --visualize is ignored, as the reference ignores it
    persons = 'target'
    people_mesh = False
    render_mesh = False
    gpu_video = False
    smooth_median_radius = 0
    smooth_sigma = 0.0
    activity = None
    visualize = True
    _detector = None                    # front_end.track_frames' detector ...
    _detector_key = None                # ... and the cfg.TRACKER values it was built from
    _warned_no_cv2 = False

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
        self.lanes = int(getattr(args, 'lanes', None) or cfg.DATASET.get('hip_lanes', 2))
        self._pipe = None
        debug = bool(getattr(args, 'debug', False))
        self.reba, self.rula = REBA(debug), RULA(debug)
        scores = str(getattr(args, 'type', 'REBA,RULA')).replace(' ', '').upper().split(',')
        self.run_reba = 'REBA' in scores
        self.run_rula = 'RULA' in scores
        self.debugging = debug
        self.debug_frame = getattr(args, 'debug_frame', -1)
        # the knobs of the MI355X path: args.<name>, else cfg's (core/config.py's docstring says what each one does)
        self.render_mesh = bool(_knob(args, 'render_mesh', 'render_mesh', False))
        self.gpu_video = bool(_knob(args, 'gpu_video', 'gpu_video', False))
        self.persons = str(_knob(args, 'persons', 'persons', 'target'))
        if self.persons not in ('target', 'all'):
            raise ValueError(f"persons {self.persons!r} is not known: 'target' or 'all' (cfg.DATASET.persons / args.persons)")
        self.people_mesh = bool(_knob(args, 'people_mesh', 'people_mesh', False))
        if self.people_mesh and self.persons != 'all':
            raise ValueError(f"people_mesh draws the people that persons 'all' scores, but persons is {self.persons!r} "
                             "(cfg.DATASET.people_mesh / args.people_mesh, cfg.DATASET.persons / args.persons)")
        from poserisk_release_amd.smooth import check_parameters
        self.smooth_median_radius, self.smooth_sigma = check_parameters(_knob(args, 'smooth_median_radius', 'smooth_median_radius', 0),
                                                                        _knob(args, 'smooth_sigma', 'smooth_sigma', 0.0))
        self.activity = self._activity_knob(args)           # None (off), or cfg.ACTIVITY's parameters
        (self.gpu_video_codec, self.video_encoder, self.video_encoder_ext, self.video_chroma,
         self.gpu_video_quality) = _video_output_knobs(args)
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
        _valid_rotations(st, "in frames")
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
        sm = smooth.smooth_tracks(torch.as_tensor(smpl['rotmat'], device=dev), np.asarray(fidx, np.int64), track_start(people),
                                  median_radius, sigma, betas=torch.as_tensor(smpl['betas'], device=dev),
                                  cam=torch.as_tensor(smpl['cam'], device=dev))
        aa, eul, st = ops.pose_to_euler(sm['rotmat'])
        n = aa.shape[0]
        joint_cam = torch.empty((n, 24, 3), dtype=torch.float32, device=dev)
        for lo in range(0, n, self.batch_size):                     # the SMPL layer takes batch_size rows a call
            layer.joint_cam(aa[lo:lo + self.batch_size], out=joint_cam[lo:lo + self.batch_size])
        _valid_rotations(st, "after smoothing in rows")
        smpl.update({k: sm[k].cpu().numpy() for k in ('rotmat', 'betas', 'cam')})
        flags = {k: sm[k].cpu().numpy() for k in ('status', 'replaced')}
        return eul.cpu().numpy(), joint_cam.cpu().numpy(), aa.cpu().numpy(), flags

    def _activity_rows(self, rotmat, people, fidx, fps, parameters):
        """The activity knob's half of _score_tracks: ONE activity.activity_tracks call over everybody's rows of `rotmat` (host
        f32[n,24,3,3], person after person; windows on the frame numbers `fidx`, never across people) -> (flags i32[n,4],
        adds i32[n,4], the parameters in seconds and frames), host arrays."""
        from poserisk_release_amd import activity
        dev = self.smpl_model.layer['neutral'].device
        act = activity.activity_tracks(torch.as_tensor(rotmat, device=dev), np.asarray(fidx, np.int64), track_start(people), fps,
                                       **parameters)
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
        deriving = self.activity
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
        smooth_m, smooth_sigma = self.smooth_median_radius, self.smooth_sigma
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
            with_smpl_params = self.people_mesh
        outs, pose_logs = self._score_tracks(frames, people, add_info, bgr, bbox_scale, with_smpl_params=bool(with_smpl_params), fps=fps)
        people_out = {'people': outs, 'ids': [pid for pid, _, _ in people], 'frames_total': n_frames}
        return dict(people_out, pose_logs=pose_logs) if self.debugging else people_out

    # ---- the public names of what core/front_end.py and core/outputs.py hold: their functions take the predictor first ----------
    load_front_end = front_end.load_front_end
    track_frames = front_end.track_frames
    render_overlay = outputs.render_overlay
    render_people = outputs.render_people
    write_mesh_overlay = outputs.write_mesh_overlay
    write_gpu_video = outputs.write_gpu_video
    write_people_video = outputs.write_people_video
    write_people_reports = outputs.write_people_reports
    write_smooth_report = outputs.write_smooth_report
    write_activity_report = outputs.write_activity_report
    visualize_joint_cam_mesh = outputs.visualize_joint_cam_mesh

    # ---- main/run.py:31  predictor(args.input, args.info, args.output) -----------------------------------
    def __call__(self, input_path, info_path, output_path, frames=None, tracking_results=None, fps=30.0, bgr=False):
        """The reference's entry point (base.py:126-209) around the accelerated path: front end (given, found or
        the reference's own: `load_front_end`) -> crops, pose, scores on the GPU -> `reba_result.txt` /
        `rula_result.txt`, `<TITLE>_score.png`, `<TITLE>_video.mp4` (OpenCV drawing: only where cv2 is importable; with
        the gpu_video knob composed on the GPU instead, see write_gpu_video) and with `args.debug` the CSV logs under <output>/debug.  Returns the dict of `score_frames` plus `fps`.
        With the persons knob at 'all' all of that is written for the target from score_people's element 0 (the model runs
        once), then <output>/person_<id>/, <output>/people.json and, with gpu_video, <TITLE>_people (write_people_reports,
        write_people_video); the dict returned also holds 'people', what score_people returned."""
        os.makedirs(output_path, exist_ok=True)
        world, rank = pl.world_and_rank()
        if frames is None or tracking_results is None:
            # tracking given without frames: a Motion-JPEG AVI input takes it (load_front_end, case 3); every other input
            # brings its own, as before
            given = {'tracking_results': tracking_results} if frames is None and tracking_results is not None else {}
            if world > 1:
                frames, bgr, fps, tracking_results = front_end.load_on_rank0(self, input_path, output_path, rank, **given)
            else:
                frames, bgr, fps, tracking_results = self.load_front_end(input_path, output_path, **given)
        add_info = _information(info_path if info_path and osp.isfile(str(info_path)) else None)      # base.py:140-142
        people_out = None
        if self.persons == 'all':
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
        outputs.write_outputs(self, out, people_out, frames, output_path, bgr, fps)
        return out
