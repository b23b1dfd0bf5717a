"""The guarded output arena of the raw-ABI tests (tests/abi_arena.py) on CPU
tensors: an overwritten guard word is reported, written and untouched payload
elements are told apart, payloads are 16-byte aligned."""
import numpy as np
import pytest
import torch

from tests.abi_arena import GUARD_BYTES, PATTERNS, Arena, all_written, bits, untouched


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.uint8])
def test_payload_is_aligned_and_filled(dtype):
    ar = Arena("cpu")
    views = [ar.alloc(shape, dtype) for shape in ((3, 5), (1,), (7, 1, 2), 0)]
    for v in views:
        assert v.data_ptr() % 16 == 0
        assert bool(untouched(v).all()) and v.is_contiguous()
    assert views[0].shape == (3, 5) and views[3].numel() == 0
    ar.check_guards()
    if dtype == torch.float32:
        assert bool(torch.isnan(views[0]).all())          # a quiet NaN: arithmetic on it shows


def test_written_and_untouched_elements_are_told_apart():
    ar = Arena("cpu")
    v = ar.alloc((4, 6))
    assert not all_written(v)
    v[1, 2] = 0.0
    v[3] = float("nan")                                   # another NaN is a written value
    u = untouched(v)
    assert not bool(u[1, 2]) and not bool(u[3].any())
    assert int(u.sum()) == 24 - 1 - 6
    assert bool(untouched(v, (slice(None), 0))[:3].all())
    v[:] = 1.0
    assert all_written(v)
    m = ar.alloc((5,), torch.uint8)
    m[:4] = torch.tensor([0, 1, 1, 0], dtype=torch.uint8)
    assert untouched(m).tolist() == [False, False, False, False, True]
    ar.check_guards()


def test_put_copies_and_keeps_guards():
    ar = Arena("cpu")
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    v = ar.put(a, "h")
    assert np.array_equal(v.numpy(), a) and all_written(v)
    ar.check_guards()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.uint8])
@pytest.mark.parametrize("side", ["front", "back"])
def test_overwritten_guard_word_is_reported(dtype, side):
    ar = Arena("cpu")
    ar.alloc((2, 2), dtype, "first")
    v = ar.alloc((3,), dtype, "victim")
    # the whole allocation behind the payload view: one element past either end
    g = GUARD_BYTES // v.element_size()
    whole = v.as_strided((g + 3 + g,), (1,), v.storage_offset() - g)
    assert bool((bits(whole) == PATTERNS[dtype]).all())
    whole[g - 1 if side == "front" else g + 3] = 0
    with pytest.raises(AssertionError, match=f"victim: 1 {side} guard"):
        ar.check_guards()


OFFSETS = [(torch.float32, 4), (torch.float32, 8), (torch.float32, 12), (torch.int32, 4),
           (torch.int32, 8), (torch.float64, 8), (torch.int64, 8), (torch.uint8, 1),
           (torch.uint8, 2), (torch.uint8, 3)]


@pytest.mark.parametrize("dtype,offset", OFFSETS)
def test_offset_payload_starts_that_many_bytes_past_a_16_byte_boundary(dtype, offset):
    ar = Arena("cpu")
    views = [ar.alloc(shape, dtype, offset=offset) for shape in ((3, 5), (1,), 0)]
    views.append(ar.put(np.arange(6).astype(views[0].numpy().dtype).reshape(2, 3), offset=offset))
    base = ar.alloc((4,), dtype)                          # the default: on the boundary
    assert base.data_ptr() % 16 == 0
    for v in views:
        assert (v.numel() == 0 or v.data_ptr() % 16 == offset) and v.is_contiguous()
    assert bool(untouched(views[0]).all()) and views[0].shape == (3, 5) and views[2].numel() == 0
    assert views[3].flatten().tolist() == list(range(6)) and all_written(views[3])
    ar.check_guards()


def test_offset_must_be_a_multiple_of_the_element_size_below_16():
    ar = Arena("cpu")
    for dtype, bad in ((torch.float32, 2), (torch.float32, 16), (torch.float64, 4),
                       (torch.int64, 12), (torch.uint8, -1)):
        with pytest.raises(AssertionError):
            ar.alloc((3,), dtype, offset=bad)


@pytest.mark.parametrize("dtype,offset", OFFSETS)
@pytest.mark.parametrize("side", ["front", "back"])
def test_overwritten_guard_word_of_an_offset_payload_is_reported(dtype, offset, side):
    """The element just before an offset payload (inside the bytes the offset
    added to the front guard) and the one just past its end."""
    ar = Arena("cpu")
    v = ar.alloc((3,), dtype, "victim", offset=offset)
    near = v.as_strided((5,), (1,), v.storage_offset() - 1)
    assert bits(near)[0] == PATTERNS[dtype] and bits(near)[4] == PATTERNS[dtype]
    near[0 if side == "front" else 4] = 0
    with pytest.raises(AssertionError, match=f"victim: 1 {side} guard"):
        ar.check_guards()
