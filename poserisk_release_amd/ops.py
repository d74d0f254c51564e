"""Thin torch-tensor wrappers over the stand-alone C-ABI kernels (rotation conversions, scorers,
the stand-alone conv used by parity tests and tile tuning)."""
import numpy as np
import torch

from . import _lib


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _need_cuda(t, name):
    if t.device.type != "cuda":
        raise _lib.PoseRiskHipError(f"{name}: tensor must be on the GPU (no CPU fallback)")


def _out(out, shape, dt, dev):
    """The output tensor: a fresh one, or the caller's (e.g. a view into a larger buffer with guard rows behind it)."""
    if out is None:
        return torch.empty(shape, dtype=dt, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != dt or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous {dt} tensor of shape {tuple(shape)} on {dev}")
    return out


def _outs(out, n):
    """A wrapper's `out=` for n outputs: None, or one tensor per output in the order they are returned."""
    if out is None:
        return (None,) * n
    if isinstance(out, torch.Tensor) or len(out) != n:
        raise ValueError(f"out must be a sequence of {n} tensors")
    return tuple(out)


def rot6d_to_rotmat(pose6d, out=None):
    """SPIN utils/geometry.py::rot6d_to_rotmat.  f32[N,144] -> f32[N,24,3,3]."""
    _need_cuda(pose6d, "rot6d_to_rotmat")
    p = pose6d.contiguous().float()
    N = p.shape[0]
    out = _out(out, (N, 24, 3, 3), torch.float32, p.device)
    _lib.check(_lib.load().pr_rot6d_to_rotmat(p.data_ptr(), N, out.data_ptr(), _stream(p.device)), "pr_rot6d_to_rotmat")
    return out


def pose_to_euler(rotmat, out=None):
    """rot_to_angle + axis_angle_to_euler_angle (lib/utils/coord_utils.py:24-30, 83-95) for a batch.
    f32[N,24,3,3] -> (axis_angle f32[N,24,3], euler_deg f64[N,24,3], status int32[N]); out: those three, to write into."""
    _need_cuda(rotmat, "pose_to_euler")
    r = rotmat.contiguous().float()
    N = r.shape[0]
    aa, eul, st = _outs(out, 3)
    aa = _out(aa, (N, 24, 3), torch.float32, r.device)
    eul = _out(eul, (N, 24, 3), torch.float64, r.device)
    st = _out(st, (N,), torch.int32, r.device)
    _lib.check(_lib.load().pr_pose_to_euler(r.data_ptr(), N, aa.data_ptr(), eul.data_ptr(), st.data_ptr(),
                                            _stream(r.device)), "pr_pose_to_euler")
    return aa, eul, st


def axis_angle_to_euler(axis_angle, out=None):
    """axis_angle_to_euler_angle (lib/utils/coord_utils.py:83-95) for a batch.
    f32[N,24,3] -> (euler_deg f64[N,24,3], status int32[N]); out: those two, to write into."""
    _need_cuda(axis_angle, "axis_angle_to_euler")
    a = axis_angle.contiguous().float()
    N = a.shape[0]
    eul, st = _outs(out, 2)
    eul = _out(eul, (N, 24, 3), torch.float64, a.device)
    st = _out(st, (N,), torch.int32, a.device)
    _lib.check(_lib.load().pr_axis_angle_to_euler(a.data_ptr(), N, eul.data_ptr(), st.data_ptr(), _stream(a.device)),
               "pr_axis_angle_to_euler")
    return eul, st


def _addend_rows(rows, shape, dev, name):
    """A scorer's per-row addends (tensor or array of integers) -> a contiguous int32 tensor of `shape` on `dev`."""
    rows = torch.as_tensor(rows)
    if rows.dtype not in (torch.int32, torch.int64) or tuple(rows.shape) != tuple(shape):
        raise ValueError(f"{name}: rows must be integers of shape {tuple(shape)}, got {rows.dtype} {tuple(rows.shape)}")
    return rows.to(dev, torch.int32).contiguous()


def reba(euler_deg, info, out=None, rows=None):
    """REBA.__call__ arithmetic (lib/utils/reba.py:50-81).  f64[N,24,3] -> int32[N,10].
    rows: None, or int[N]: row f's value is added to info's Activity_Score (pr_reba_rows; activity.activity_tracks derives it)."""
    _need_cuda(euler_deg, "reba")
    e = euler_deg.contiguous().double()
    N = e.shape[0]
    out = _out(out, (N, 10), torch.int32, e.device)
    s = _lib.reba_info_struct(info)
    if rows is None:
        _lib.check(_lib.load().pr_reba(e.data_ptr(), N, s, out.data_ptr(), _stream(e.device)), "pr_reba")
    else:
        rows = _addend_rows(rows, (N,), e.device, "reba")
        _lib.check(_lib.load().pr_reba_rows(e.data_ptr(), N, s, rows.data_ptr() if N else None, out.data_ptr(), _stream(e.device)),
                   "pr_reba_rows")
    return out


def rula(euler_deg, info, out=None, rows=None):
    """RULA.__call__ arithmetic (lib/utils/rula.py:66-98).  f64[N,24,3] -> int32[N,12].
    rows: None, or int[N,3]: row f's values are added to info's A_Muscle_use_L, A_Muscle_use_R and B_Muscle_use (pr_rula_rows)."""
    _need_cuda(euler_deg, "rula")
    e = euler_deg.contiguous().double()
    N = e.shape[0]
    out = _out(out, (N, 12), torch.int32, e.device)
    s = _lib.rula_info_struct(info)
    if rows is None:
        _lib.check(_lib.load().pr_rula(e.data_ptr(), N, s, out.data_ptr(), _stream(e.device)), "pr_rula")
    else:
        rows = _addend_rows(rows, (N, 3), e.device, "rula")
        _lib.check(_lib.load().pr_rula_rows(e.data_ptr(), N, s, rows.data_ptr() if N else None, out.data_ptr(), _stream(e.device)),
                   "pr_rula_rows")
    return out


def _device_index(t):
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _precision(precision):
    """The library's precision flag and the tensors' dtype."""
    return (1, torch.bfloat16) if precision == "bf16" else (0, torch.float32)


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if shape is None else a.reshape(shape)


def _ptr(a):
    """The data pointer of a numpy array or a tensor; None stays None (an optional argument)."""
    return None if a is None else a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def _timed(call, name, y, repeats):
    """A stand-alone entry with a `repeats` argument: call(ms) -> status.  Returns (y, ms_per_launch or None)."""
    ms = np.zeros(1, np.float32)
    _lib.check(call(ms.ctypes.data), name)
    return y, (float(ms[0]) if repeats > 0 else None)


def conv2d_nhwc(x, w_oihw, bias=None, residual=None, stride=1, pad=0, relu=False, tile_cfg=-1, repeats=0,
                precision="fp32", out=None):
    """Stand-alone conv on NHWC (test / tuning entry).  x [B,H,W,Cin] CUDA (f32, or bf16 with
    precision="bf16"), w numpy OIHW.  Returns (y [B,Ho,Wo,Cout] in x's dtype, ms_per_launch or None)."""
    _need_cuda(x, "conv2d_nhwc")
    bf, dt = _precision(precision)
    x = x.contiguous().to(dt)
    B, H, W, Cin = x.shape
    w = _f32(w_oihw)
    Cout, Cin_real, KH, KW = w.shape
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    y = _out(out, (B, Ho, Wo, Cout), dt, x.device)
    b = _f32(bias) if bias is not None else None
    res = residual.contiguous().to(dt) if residual is not None else None
    return _timed(lambda ms: _lib.load().pr_conv2d_nhwc(
        _device_index(x), x.data_ptr(), w.ctypes.data, _ptr(b), _ptr(res), y.data_ptr(), B, H, W, Cin, Cin_real, Cout, KH, KW,
        stride, pad, int(relu), tile_cfg, bf, repeats, ms, _stream(x.device)), "pr_conv2d_nhwc", y, repeats)


def det_conv_nhwc(x, packed, cout, ksize, stride=1, leaky=True, residual=None, out=None):
    """The detector's convolution alone (pr_det_conv_nhwc, csrc/det_conv.hip): x f32[B,H,W,Cin] CUDA, `packed` ONE convolution in
    pr_det_fold_pack's layout on the device (bias[cout_pad], then w[cout_pad][kpad]) -> f32[B,Ho,Wo,cout] = leaky(conv + b)
    [+ residual]; padding ksize // 2.  Asynchronous; allocates nothing with `out` given."""
    _need_cuda(x, "det_conv_nhwc")
    B, H, W, Cin = x.shape
    pad = ksize // 2
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    y = _out(out, (B, Ho, Wo, cout), torch.float32, x.device)
    _lib.check(_lib.load().pr_det_conv_nhwc(x.data_ptr(), packed.data_ptr(), residual.data_ptr() if residual is not None else None,
                                            y.data_ptr(), B, H, W, Cin, int(cout), int(ksize), int(stride), int(bool(leaky)),
                                            _stream(x.device)), "pr_det_conv_nhwc")
    return y


def det_conv_nhwc_bf16(x, packed, cout, ksize, stride=1, leaky=True, residual=None, out_dtype=torch.bfloat16, out=None):
    """The detector's bf16 convolution alone (pr_det_conv_nhwc_bf16, csrc/det_conv_bf16.hip): x bf16[B,H,W,Cin] CUDA (Cin a
    multiple of 8), `packed` ONE convolution as bytes on the device (bias f32[cout_pad], then w bf16[cout_pad][kpad]), residual
    bf16 -> out_dtype (torch.bfloat16 | torch.float32) [B,Ho,Wo,cout] = round(leaky(conv + b) [+ residual]), rounded once."""
    _need_cuda(x, "det_conv_nhwc_bf16")
    if x.dtype != torch.bfloat16 or (residual is not None and residual.dtype != torch.bfloat16) or not x.is_contiguous():
        raise ValueError("det_conv_nhwc_bf16: x and residual must be contiguous torch.bfloat16 tensors")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"det_conv_nhwc_bf16: out_dtype {out_dtype} unknown: torch.bfloat16 or torch.float32")
    B, H, W, Cin = x.shape
    pad = ksize // 2
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    y = _out(out, (B, Ho, Wo, cout), out_dtype, x.device)
    _lib.check(_lib.load().pr_det_conv_nhwc_bf16(x.data_ptr(), packed.data_ptr(), residual.data_ptr() if residual is not None else None,
                                                 y.data_ptr(), B, H, W, Cin, int(cout), int(ksize), int(stride), int(bool(leaky)),
                                                 int(out_dtype == torch.float32), _stream(x.device)), "pr_det_conv_nhwc_bf16")
    return y


def conv1x1_dual_nhwc(x1, w1, x2, w2, bias=None, stride2=1, relu=False, tile_cfg=-1, precision="fp32", out=None):
    """relu(x1*W1 + x2[::stride2, ::stride2]*W2 + bias) as one dual-source GEMM (a first Bottleneck's conv3 with its
    downsample branch summed in).  x1 [B,Ho,Wo,C1], x2 [B,H2,W2,C2] CUDA, w1 [Cout,C1], w2 [Cout,C2] numpy."""
    _need_cuda(x1, "conv1x1_dual_nhwc")
    bf, dt = _precision(precision)
    x1, x2 = x1.contiguous().to(dt), x2.contiguous().to(dt)
    B, Ho, Wo, C1 = x1.shape
    _, H2, W2, C2 = x2.shape
    w1, w2 = _f32(w1, (-1, C1)), _f32(w2, (-1, C2))
    Cout = w1.shape[0]
    y = _out(out, (B, Ho, Wo, Cout), dt, x1.device)
    b = _f32(bias) if bias is not None else None
    _lib.check(_lib.load().pr_conv1x1_dual_nhwc(
        _device_index(x1), x1.data_ptr(), w1.ctypes.data, x2.data_ptr(), w2.ctypes.data, _ptr(b),
        y.data_ptr(), B, Ho, Wo, C1, H2, W2, C2, stride2, Cout, int(relu), tile_cfg, bf,
        _stream(x1.device)), "pr_conv1x1_dual_nhwc")
    return y


def conv3x3_conv1x1_nhwc(x, w2, b2, w3, b3, residual=None, relu=True, precision="fp32", out=None):
    """relu?(relu(conv3x3(x, w2) + b2) * w3^T + b3 + residual) in one kernel (a layer1 Bottleneck's conv2 + conv3).
    x [B,H,W,Cin] CUDA (f32, or bf16 with precision="bf16"), w2 [64,Cin,3,3], w3 [N3,64] numpy -> [B,H,W,N3]."""
    _need_cuda(x, "conv3x3_conv1x1_nhwc")
    bf, dt = _precision(precision)
    x = x.contiguous().to(dt)
    B, H, W, Cin = x.shape
    w2, w3, b2, b3 = _f32(w2), _f32(w3, (-1, 64)), _f32(b2), _f32(b3)
    N3 = w3.shape[0]
    res = residual.contiguous().to(dt) if residual is not None else None
    y = _out(out, (B, H, W, N3), dt, x.device)
    _lib.check(_lib.load().pr_conv3x3_conv1x1_nhwc(
        _device_index(x), x.data_ptr(), w2.ctypes.data, b2.ctypes.data, w3.ctypes.data, b3.ctypes.data,
        _ptr(res), y.data_ptr(), B, H, W, Cin, N3, int(relu), bf, _stream(x.device)), "pr_conv3x3_conv1x1_nhwc")
    return y


def conv3x3_wino64_nhwc(x, w2, b2, w3=None, b3=None, residual=None, relu=True, form=5, out=None):
    """A layer1 conv2 (64 -> 64, 3x3 / stride 1 / pad 1, fp32) as Winograd F(4x4,3x3) in one launch, alone --
    relu?(conv3x3(x, w2) + b2) -> [B,H,W,64] -- or, with w3 [N3,64] / b3, with conv3 behind it as conv3x3_conv1x1_nhwc:
    relu?(relu(conv3x3(x, w2) + b2) * w3^T + b3 + residual) -> [B,H,W,N3].  form 4 or 5 (the interpolation points).
    Other channel counts are refused by the library."""
    _need_cuda(x, "conv3x3_wino64_nhwc")
    x = x.contiguous().float()
    B, H, W, Cin = x.shape
    w2, b2 = _f32(w2), _f32(b2)
    Cout = w2.shape[0]
    fused = w3 is not None
    w3, b3 = (_f32(w3, (-1, 64)), _f32(b3)) if fused else (None, None)
    N3 = w3.shape[0] if fused else 0
    res = residual.contiguous().float() if residual is not None else None
    y = _out(out, (B, H, W, N3 if fused else Cout), torch.float32, x.device)
    _lib.check(_lib.load().pr_conv3x3_wino64_nhwc(
        _device_index(x), x.data_ptr(), w2.ctypes.data, b2.ctypes.data, _ptr(w3), _ptr(b3), _ptr(res), y.data_ptr(), B, H, W,
        Cin, Cout, N3, int(relu), int(relu), form, _stream(x.device)), "pr_conv3x3_wino64_nhwc")
    return y


def _bottleneck(planes, first, name, x, w1, b1, w2, b2, w3, b3, wd, bd, repeats, out):
    """The three whole-Bottleneck wrappers: `planes` channels inside, 4 * planes out, the same in (a first block: planes)."""
    _need_cuda(x, name)
    x = x.contiguous().to(torch.bfloat16)
    B, H, W, C = x.shape
    P, cin = planes, planes if first else 4 * planes
    if C != cin:
        raise ValueError(f"{name}: {cin} input channels expected, got {C}")
    w = [_f32(w1, (P, C)), _f32(b1, (P,)), _f32(w2, (P, P, 3, 3)), _f32(b2, (P,)), _f32(w3, (4 * P, P)), _f32(b3, (4 * P,))]
    if planes == 64:      # the only entry with a downsample branch in its signature
        w += [_f32(wd, (4 * P, P)), _f32(bd, (4 * P,))] if first else [None, None]
    y = _out(out, (B, H, W, 4 * P), torch.bfloat16, x.device)
    entry = getattr(_lib.load(), f"pr_{name}")
    return _timed(lambda ms: entry(_device_index(x), x.data_ptr(), *map(_ptr, w), y.data_ptr(), B, H, W, repeats, ms,
                                   _stream(x.device)), f"pr_{name}", y, repeats)


def bottleneck_nhwc(x, w1, b1, w2, b2, w3, b3, wd=None, bd=None, repeats=0, out=None):
    """A whole layer1 Bottleneck (conv1 1x1 -> conv2 3x3 -> conv3 1x1 + identity, ReLU after each; BatchNorm folded by
    the caller) in one persistent bf16 kernel.  Without `wd`: x bf16 [B,H,W,256] CUDA, w1 [64,256], identity = x.  With
    `wd` [256,64] / `bd` [256] (the stage's first block): x bf16 [B,H,W,64], w1 [64,64], identity = the downsample branch.
    w2 [64,64,3,3], w3 [256,64] numpy.  Returns (y bf16 [B,H,W,256], ms_per_launch or None)."""
    return _bottleneck(64, wd is not None, "bottleneck_nhwc", x, w1, b1, w2, b2, w3, b3, wd, bd, repeats, out)


def bottleneck128_nhwc(x, w1, b1, w2, b2, w3, b3, repeats=0, out=None):
    """A whole layer2 Bottleneck (plain block: conv1 1x1 512 -> 128, conv2 3x3, conv3 1x1 128 -> 512 + identity, ReLU after
    each; BatchNorm folded by the caller) in one persistent bf16 kernel.  x bf16 [B,H,W,512] CUDA (W <= 31), w1 [128,512],
    w2 [128,128,3,3], w3 [512,128] numpy.  Returns (y bf16 [B,H,W,512], ms_per_launch or None)."""
    return _bottleneck(128, False, "bottleneck128_nhwc", x, w1, b1, w2, b2, w3, b3, None, None, repeats, out)


def bottleneck256_nhwc(x, w1, b1, w2, b2, w3, b3, repeats=0, out=None):
    """A whole layer3 Bottleneck (plain block: conv1 1x1 1024 -> 256, conv2 3x3, conv3 1x1 256 -> 1024 + identity, ReLU after
    each; BatchNorm folded by the caller) in one bf16 kernel, one frame per workgroup.  x bf16 [B,H,W,1024] CUDA (H W <= 224),
    w1 [256,1024], w2 [256,256,3,3], w3 [1024,256] numpy.  Returns (y bf16 [B,H,W,1024], ms_per_launch or None)."""
    return _bottleneck(256, False, "bottleneck256_nhwc", x, w1, b1, w2, b2, w3, b3, None, None, repeats, out)


def stem_pool_nhwc(x, w, bias, repeats=0, out=None):
    """The bf16 encoder's stem in one kernel: 4x4 / stride-1 convolution (window rows y-2 .. y+1, i.e. padding 2 with the
    last row and column of the padded result dropped) over x bf16 [B,H,H,16] CUDA + bias + ReLU + MaxPool2d(3, 2, 1).
    w [64,16,4,4], bias [64] numpy.  Returns (y bf16 [B,H/2,H/2,64], ms_per_launch or None)."""
    _need_cuda(x, "stem_pool_nhwc")
    x = x.contiguous().to(torch.bfloat16)
    B, H, W, C = x.shape
    if C != 16 or H != W or H % 2:
        raise ValueError("stem_pool_nhwc: x must be [B,H,H,16] with even H")
    w, b = _f32(w, (64, 16, 4, 4)), _f32(bias, (64,))
    y = _out(out, (B, H // 2, H // 2, 64), torch.bfloat16, x.device)
    return _timed(lambda ms: _lib.load().pr_stem_pool_nhwc(
        _device_index(x), x.data_ptr(), w.ctypes.data, b.ctypes.data, y.data_ptr(), B, H, repeats, ms, _stream(x.device)),
        "pr_stem_pool_nhwc", y, repeats)


def stem_pool_f32_nhwc(x, w, bias, repeats=0, out=None):
    """The fp32 encoder's stem in one kernel: 4x4 / stride-1 convolution (window rows y-2 .. y+1) over the space-to-depth
    image x f32 [B,112,112,12] CUDA + bias + ReLU + MaxPool2d(3, 2, 1).  w [64,12,4,4], bias [64] numpy.
    Returns (y f32 [B,56,56,64], ms_per_launch or None)."""
    _need_cuda(x, "stem_pool_f32_nhwc")
    x = x.contiguous().float()
    if tuple(x.shape[1:]) != (112, 112, 12):
        raise ValueError(f"stem_pool_f32_nhwc: x must be [B,112,112,12], got {tuple(x.shape)}")
    B = x.shape[0]
    w, b = _f32(w, (64, 12, 4, 4)), _f32(bias, (64,))
    y = _out(out, (B, 56, 56, 64), torch.float32, x.device)
    return _timed(lambda ms: _lib.load().pr_stem_pool_f32_nhwc(
        _device_index(x), x.data_ptr(), w.ctypes.data, b.ctypes.data, y.data_ptr(), B, repeats, ms, _stream(x.device)),
        "pr_stem_pool_f32_nhwc", y, repeats)


def crop_frames(frames, bboxes, frame_idx=None, scale=1.2, bgr=False, return_status=False, out=None):
    """GPU form of CropDataset.__getitem__ (data/demo_dataset.py:58-74) for a whole batch.
    frames u8[F,H,W,3] CUDA, bboxes f32[N,4] (cx,cy,w,h), frame_idx int32[N] or None -> f32[N,3,224,224].
    A host-side `frame_idx` is range-checked here (ValueError); one that already lives on the GPU is checked by
    the kernel, which zero-fills such crops and flags them in the int32[N] status (`return_status=True`).
    out: the crops tensor to write into, or (crops, status) with `return_status`."""
    _need_cuda(frames, "crop_frames")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("frames must be uint8 [F,H,W,3]")
    frames = frames.contiguous()
    bb = torch.as_tensor(bboxes, dtype=torch.float32).to(frames.device).contiguous()
    N = bb.shape[0]
    if frame_idx is None:
        if N > frames.shape[0]:
            raise ValueError(f"{N} boxes for {frames.shape[0]} frames without a frame index")
    else:
        if not (isinstance(frame_idx, torch.Tensor) and frame_idx.device.type == "cuda"):
            host = np.asarray(frame_idx).reshape(-1)
            if host.shape[0] != N:
                raise ValueError(f"{host.shape[0]} frame indices for {N} boxes")
            if N and (int(host.min()) < 0 or int(host.max()) >= frames.shape[0]):
                raise ValueError(f"frame index out of range: {int(host.min())}..{int(host.max())} with "
                                 f"{frames.shape[0]} frames")
    if bb.dim() != 2 or bb.shape[1] != 4:
        raise ValueError(f"bboxes must be [N,4] (cx,cy,w,h), got {tuple(bb.shape)}")
    idx = None
    if frame_idx is not None:
        # the kernel reads frame_idx[n] for every n < N before it range-checks the VALUE: the array itself must hold N ints
        idx = torch.as_tensor(frame_idx).to(frames.device)
        if idx.dim() != 1 or idx.numel() != N:
            raise ValueError(f"frame_idx must be a vector of {N} frame indices, got shape {tuple(idx.shape)}")
        if idx.dtype.is_floating_point or idx.dtype == torch.bool:
            raise ValueError(f"frame_idx must hold integers, got {idx.dtype}")
        idx = idx.to(torch.int32).contiguous()
    out, status = _outs(out, 2) if return_status else (out, None)
    out = _out(out, (N, 3, 224, 224), torch.float32, frames.device)
    status = _out(status, (N,), torch.int32, frames.device) if return_status else None
    F, H, W, _ = frames.shape
    _lib.check(_lib.load().pr_crop_frames(frames.data_ptr(), F, H, W, int(bool(bgr)),
                                          idx.data_ptr() if idx is not None else None, bb.data_ptr(), N,
                                          float(scale), out.data_ptr(),
                                          status.data_ptr() if status is not None else None,
                                          _stream(frames.device)), "pr_crop_frames")
    return (out, status) if return_status else out
