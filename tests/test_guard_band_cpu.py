"""The guard-band harness (tests/guard_band.py) on the CPU: a correct fake kernel passes, and each of four broken ones --
a store behind the output, a store in front of it, a read past the end of an input, an output element left unwritten -- is
caught with a message that says what happened and on which side.  This is what shows the fence can catch something."""
import pytest
import torch

import guard_band as gb

SHAPE = (3, 5, 4)      # 60 elements: rows of 20


def _flat(view, offset, n):
    """n elements of view's storage from `offset` elements relative to view[0] (may reach outside the view)."""
    return view.as_strided((n,), (1,), view.storage_offset() + offset)


def _scale_correct(ins, outs):
    torch.mul(ins["x"], 2.0, out=outs["y"])


def _writes_one_behind(ins, outs):
    _scale_correct(ins, outs)
    _flat(outs["y"], outs["y"].numel(), 1).fill_(1.0)


def _writes_one_in_front(ins, outs):
    _scale_correct(ins, outs)
    _flat(outs["y"], -1, 1).fill_(1.0)


def _reads_one_past_the_input(ins, outs):
    _scale_correct(ins, outs)
    n = ins["x"].numel()
    outs["y"].view(-1)[n - 1] += 0.0 * _flat(ins["x"], n, 1)[0]      # "weight 0": a NaN still poisons the sum


def _leaves_one_unwritten(ins, outs):
    y = outs["y"].view(-1)
    torch.mul(ins["x"].view(-1)[:-1], 2.0, out=y[:-1])


def _run(fn, dtype=torch.float32):
    x = torch.arange(60, dtype=torch.float32).reshape(SHAPE).to(dtype) + 1
    return x, gb.run_guarded(fn, {"x": x}, {"y": (SHAPE, dtype)}, device="cpu")["y"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_a_correct_kernel_passes(dtype):
    x, y = _run(_scale_correct, dtype)
    assert torch.equal(y, x * 2)


@pytest.mark.parametrize("fn,words", [
    (_writes_one_behind, ["output y", "BEHIND", "1 elements", "first at +0", "last at +0"]),
    (_writes_one_in_front, ["output y", "IN FRONT", "1 elements", "first at -1", "last at -1"]),
    (_reads_one_past_the_input, ["output y", "NaN", "first at flat element 59", "read outside an input"]),
    (_leaves_one_unwritten, ["output y", "UNWRITTEN", "1 elements", "first at flat element 59"]),
], ids=["store_behind", "store_in_front", "read_past_input", "unwritten"])
def test_broken_kernels_are_caught(fn, words):
    with pytest.raises(AssertionError) as e:
        _run(fn)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_a_store_around_an_input_is_caught_too():
    def bad(ins, outs):
        _scale_correct(ins, outs)
        _flat(ins["x"], -3, 2).fill_(0.0)

    with pytest.raises(AssertionError, match=r"input x .*IN FRONT.*2 elements, first at -3, last at -2"):
        _run(bad)

    def overwrites_input(ins, outs):
        _scale_correct(ins, outs)
        ins["x"].view(-1)[7] = 0.0

    with pytest.raises(AssertionError, match="input x: the kernel wrote into its input"):
        _run(overwrites_input)
    gb.run_guarded(overwrites_input, {"x": torch.ones(SHAPE)}, {"y": (SHAPE, torch.float32)}, device="cpu", mutated=("x",))


def test_a_planted_nan_passes_only_where_it_is_expected():
    x = torch.arange(60, dtype=torch.float32).reshape(SHAPE) + 1
    x[1, 2, 3] = float("nan")
    run = lambda fn, mask: gb.run_guarded(fn, {"x": x}, {"y": (SHAPE, torch.float32)}, device="cpu", nan_expected={"y": mask})["y"]
    y = run(_scale_correct, torch.isnan(x).numpy())
    assert torch.equal(torch.isnan(y), torch.isnan(x))
    with pytest.raises(AssertionError, match="1 NaN, first at flat element 31"):      # the planted one, with no mask for it
        run(_scale_correct, torch.zeros(SHAPE, dtype=torch.bool).numpy())
    with pytest.raises(AssertionError, match="1 NaN, first at flat element 59"):      # the guard's NaN is not excused by the mask
        run(_reads_one_past_the_input, torch.isnan(x).numpy())


def test_guard_sizes_and_fills():
    # one frame, at least 4 KiB, in multiples of 256 bytes
    assert gb.guard_bytes((2, 9, 9, 64), torch.float32) == 9 * 9 * 64 * 4
    assert gb.guard_bytes((2, 5, 5, 96), torch.bfloat16) == 4864            # 4800 -> next multiple of 256
    assert gb.guard_bytes((7, 144), torch.float32) == 4096                  # a row of 576 bytes: the floor
    assert gb.guard_bytes((5,), torch.int32) == 4096
    assert gb.guard_bytes((2, 37, 53, 3), torch.uint8) == 5888              # 5883 -> 5888
    for dtype, fill in [(torch.float32, gb.CANARY_FLOAT), (torch.bfloat16, gb.CANARY_FLOAT), (torch.uint8, 0x5A), (torch.int32, -7)]:
        big, view = gb.arena((3, 7), dtype, "cpu", gb.canary(dtype))
        g = big.guard_elems
        assert g * big.element_size() == 4096 and big.numel() == 2 * g + 21
        assert view.data_ptr() - big.data_ptr() == 4096 and view.is_contiguous() and view.shape == (3, 7)
        assert bool((big == torch.full((), fill, dtype=dtype)).all())
        gb.assert_guards_intact(big, view, "fresh")
    assert float(torch.full((), gb.CANARY_FLOAT, dtype=torch.bfloat16)) == -12352.0      # the nearest bf16
    big, view = gb.arena((4, 3), torch.float64, "cpu", gb.input_fill(torch.float64))
    assert bool(torch.isnan(big).all())
    gb.assert_guards_intact(big, view, "NaN guards compare by bits")
    big[0] = -float("nan")                                                   # another NaN: other bits, so it counts as touched
    with pytest.raises(AssertionError, match="IN FRONT"):
        gb.assert_guards_intact(big, view, "sign bit of a NaN")
    assert gb.input_fill(torch.uint8) == 255 and gb.input_fill(torch.int32) == 0x7fffffff


def test_integer_outputs():
    def copy(ins, outs):
        outs["s"].copy_(ins["i"] % 5)

    idx = torch.tensor([0, 7, -2, 2], dtype=torch.int32)
    assert gb.run_guarded(copy, {"i": idx}, {"s": ((4,), torch.int32)}, device="cpu")["s"].tolist() == [0, 2, 3, 2]

    def skips_last(ins, outs):
        outs["s"][:3].copy_(ins["i"][:3])

    with pytest.raises(AssertionError, match="output s: 1 elements UNWRITTEN"):
        gb.run_guarded(skips_last, {"i": idx}, {"s": ((4,), torch.int32)}, device="cpu")
