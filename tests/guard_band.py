"""Guard bands around test tensors: does a kernel stay inside the tensors it was given?  (A helper module, not a conftest;
it works on any device, tests/test_guard_band_cpu.py exercises it on the CPU.)

The parity tests hand every kernel fresh torch allocations.  The caching allocator rounds sizes up and hands out pooled
blocks, so a store a few rows past the end lands in slack or in a dead tensor and a read past the end returns some finite
stale number: neither is noticed.  Here a tensor is a view into the middle of a larger allocation (an "arena") whose two
guard regions, in front of and behind the view, hold a known fill:

  inputs    NaN (fp32 / bf16 / fp64), 255 (uint8 frames), 0x7fffffff (int32 indices): a value read from a guard and used
            poisons the output (NaN), saturates a pixel, or is an index far out of range;
  outputs   a canary no kernel can legitimately produce (-12345.0; bf16: the nearest representable, -12352.0; 0x5A for
            uint8; -7 for int32): a guard that no longer holds it was written, an output element that still holds it was not.

A guard is max(one frame [H, W, C] of the tensor -- for tensors without a frame axis, one row --, 4 KiB), rounded up to a
multiple of 256 bytes: a kernel that is one whole frame or one halo row off still lands in it, and the view keeps the
256-byte alignment of a torch allocation (pointer alignment is not what this tests; no kernel gets a less-aligned pointer).

What the fence cannot see, by construction:
  * the library's own workspaces, which the handles hipMalloc themselves: they cannot be fenced from outside.  The
    INTERNAL fence does that from inside (POSERISK_FENCE=1 | 2, csrc/fence.h, pr_fence_check; DESIGN.md 4.1;
    tests/test_internal_fence_gpu.py): every allocation of the library's own between 0xFF guards, tensors in the buffers
    that are sized as a maximum placed head- or tail-aligned.  What remains invisible to both fences:
  * a buffer the internal fence leaves head-aligned in both modes (the split-K tickets; the max_batch-sized regressor and
    SMPL workspaces unless max_batch == B): an access behind its tensor lands in the buffer's own slack;
  * an out-of-tensor READ whose value is discarded before it reaches an output (masked, multiplied away by a select, or
    dropped with a row >= M): only a value that takes part in an output shows;
  * an access further away than the guard (a wild pointer rather than an off-by-a-row).
"""
import math

import torch

CANARY_FLOAT = -12345.0
CANARY_U8 = 0x5A
CANARY_I32 = -7
MIN_GUARD_BYTES = 4096
ALIGN = 256


def input_fill(dtype):
    """The guard fill around an input of `dtype`."""
    if dtype.is_floating_point:
        return float("nan")
    return {torch.uint8: 255, torch.int32: 0x7fffffff}[dtype]


def canary(dtype):
    """The guard fill (and initial content) of an output of `dtype`."""
    if dtype.is_floating_point:
        return CANARY_FLOAT
    return {torch.uint8: CANARY_U8, torch.int32: CANARY_I32}[dtype]


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def guard_bytes(shape, dtype):
    """max(one frame / one row of the tensor, 4 KiB), rounded up to a multiple of 256 bytes."""
    unit = math.prod(tuple(shape)[1:]) * _itemsize(dtype)
    return (max(unit, MIN_GUARD_BYTES) + ALIGN - 1) // ALIGN * ALIGN


def arena(shape, dtype, device, fill):
    """-> (big, view): `view`, a contiguous tensor of `shape`, in the middle of the 1-D allocation `big`, with
    guard_bytes(shape, dtype) of `fill` in front of it and behind it (the view itself starts out as `fill` too)."""
    shape = tuple(int(s) for s in shape)
    g = guard_bytes(shape, dtype) // _itemsize(dtype)
    n = math.prod(shape)
    big = torch.full((g + n + g,), fill, dtype=dtype, device=device)
    view = big[g:g + n].view(shape)
    big.guard_elems, big.guard_fill = g, fill
    assert view.is_contiguous() and view.data_ptr() == big.data_ptr() + g * _itemsize(dtype)
    return big, view


def _touched(region, fill):
    """Indices of the elements of the 1-D `region` whose bits are not those of `fill`."""
    size = region.element_size()
    pattern = torch.full((1,), fill, dtype=region.dtype, device=region.device).view(torch.uint8)
    diff = (region.view(torch.uint8).view(-1, size) != pattern).any(dim=1)
    return torch.nonzero(diff).flatten()


def assert_guards_intact(big, view, what):
    """Both guard regions of arena(...)'s `big` are bit for bit their fill; the failure names the side, the first and last
    touched element relative to the view (in front: -1 is the element before view[0]; behind: +0 is the element after
    the view's last) and how many elements changed."""
    g, n = big.guard_elems, view.numel()
    assert big.numel() == g + n + g and view.data_ptr() == big.data_ptr() + g * big.element_size(), f"{what}: not its arena"
    problems = []
    front = _touched(big[:g], big.guard_fill)
    if front.numel():
        problems.append(f"guard IN FRONT of the tensor touched: {front.numel()} elements, first at {int(front[0]) - g}, "
                        f"last at {int(front[-1]) - g} (elements relative to the tensor's first)")
    back = _touched(big[g + n:], big.guard_fill)
    if back.numel():
        problems.append(f"guard BEHIND the tensor touched: {back.numel()} elements, first at +{int(back[0])}, "
                        f"last at +{int(back[-1])} (elements past the tensor's last)")
    assert not problems, f"{what} {tuple(view.shape)} {view.dtype}: " + "; ".join(problems)


def guarded_input(t, device=None):
    """`t`'s values in a view of an arena whose guards hold input_fill(t.dtype) -> (big, view)."""
    device = t.device if device is None else torch.device(device)
    big, view = arena(t.shape, t.dtype, device, input_fill(t.dtype))
    view.copy_(t)
    return big, view


def run_guarded(fn, inputs, outputs, device=None, mutated=(), may_hold_canary=(), nan_expected=None):
    """Run `fn` once with every tensor in an arena and check that it stayed inside them.

    inputs   {name: tensor}: each is copied into a view whose guards hold NaN / 255 / 0x7fffffff.  Give each in the dtype
             the kernel reads: a wrapper that converts (.float(), .to(bf16)) or re-lays a tensor out makes a copy outside the
             arena, which would defeat the guard -- so the views are checked to be contiguous already (`.contiguous()` returns
             the view itself, same data_ptr), and `fn` must pass them on as they are.
    outputs  {name: (shape, dtype)}: each is a view, initially all canary, whose guards hold the canary.
    fn(ins, outs) gets the two dicts of views and passes the outputs as the wrappers' `out=`.

    Afterwards: all guards intact (inputs' too: a kernel must not write around its inputs either); no input changed, except
    those named in `mutated`; no NaN and no surviving canary anywhere in the outputs (names in `may_hold_canary` are exempt
    from the canary check: an integer output whose legitimate values include it).  nan_expected {name: bool array of the
    output's shape}: where a case plants NaNs in its inputs, the elements whose reference is NaN -- a NaN anywhere else still
    fails.  -> {name: output view}."""
    ins, outs, arenas = {}, {}, []
    for name, t in inputs.items():
        big, view = guarded_input(t, device)
        assert view.contiguous().data_ptr() == view.data_ptr() == big.data_ptr() + big.guard_elems * big.element_size()
        ins[name] = view
        arenas.append((f"input {name}", big, view, view.clone()))
    for name, (shape, dtype) in outputs.items():
        dev = device if device is not None else next(iter(ins.values())).device
        big, view = arena(shape, dtype, dev, canary(dtype))
        outs[name] = view
        arenas.append((f"output {name}", big, view, None))
    fn(ins, outs)
    if any(v.device.type == "cuda" for v in outs.values()):
        torch.cuda.synchronize()
    for what, big, view, before in arenas:
        assert_guards_intact(big, view, what)
        name = what.split(" ", 1)[1]
        if before is not None:
            if name not in mutated:
                same = view.view(torch.uint8) == before.view(torch.uint8) if view.dim() else view == before
                assert bool(same.all()), f"{what}: the kernel wrote into its input ({int((~same).sum())} bytes changed)"
            continue
        if view.dtype.is_floating_point:
            nan = torch.isnan(view)
            if nan_expected is not None and name in nan_expected:
                nan &= ~torch.as_tensor(nan_expected[name], device=view.device).reshape(view.shape)
            assert not bool(nan.any()), (f"{what}: {int(nan.sum())} NaN, first at flat element {int(torch.nonzero(nan.flatten())[0])}"
                                         " -- a value from an input's NaN guard (a read outside an input tensor) reached the output")
        if name not in may_hold_canary:
            left = view == torch.full((), canary(view.dtype), dtype=view.dtype, device=view.device)
            assert not bool(left.any()), (f"{what}: {int(left.sum())} elements UNWRITTEN (still the canary), first at flat element "
                                          f"{int(torch.nonzero(left.flatten())[0])}")
    return outs
