"""The package's device-call layer (_device.py) on CPU tensors: what tensor / lengths hand on and what they refuse, and the per-shape
buffer sets of buffers.  No library call is made; call itself needs a device (tests/test_gpu_manual.py captures one in a graph)."""
import numpy as np
import pytest
import torch

from taco_amd import _device as D

CPU = torch.device("cpu")


def test_tensor_hands_on_what_already_conforms():
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    y = D.tensor(x, CPU, torch.float32, "x", ("B", ("T", 4)))
    assert y is x or (y.data_ptr() == x.data_ptr() and y.shape == x.shape)
    i = torch.arange(3, dtype=torch.int32)
    assert D.lengths(i, CPU, 3, "frames").data_ptr() == i.data_ptr()


def test_tensor_converts_dtype_and_contiguity():
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    y = D.tensor(a, CPU, torch.float32, "a")
    assert y.dtype == torch.float32 and y.is_contiguous() and np.array_equal(y.numpy(), a.astype(np.float32))
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()                     # [4, 3], strided
    y = D.tensor(t, CPU, torch.float32, "t")
    assert y.is_contiguous() and y.data_ptr() != t.data_ptr() and torch.equal(y, t)
    y = D.tensor([[1, 2], [3, 4]], CPU, torch.int32, "list")
    assert y.dtype == torch.int32 and y.tolist() == [[1, 2], [3, 4]]


def test_tensor_picks_the_inputs_own_dtype_out_of_a_tuple():
    kinds = (torch.float32, torch.int16)
    i16 = torch.zeros(5, dtype=torch.int16)
    assert D.tensor(i16, CPU, kinds, "pcm").data_ptr() == i16.data_ptr()            # among them: kept
    assert D.tensor(torch.zeros(5, dtype=torch.float32), CPU, kinds, "pcm").dtype == torch.float32
    assert D.tensor(np.zeros(5, np.float64), CPU, kinds, "pcm").dtype == torch.float32      # not among them: the first


def test_tensor_refuses_a_wrong_rank_or_fixed_size_with_the_audio_text():
    x = torch.zeros((2, 7, 5))
    assert D.tensor(x, CPU, torch.float32, "linear", ("B", "T", ("num_freq", 5))) is x
    with pytest.raises(Exception) as e:
        D.tensor(x, CPU, torch.float32, "linear", ("B", "T", ("num_freq", 9)))
    assert type(e.value) is Exception and str(e.value) == "linear must be [B, T, num_freq = 9], got shape (2, 7, 5)"
    with pytest.raises(Exception) as e:
        D.tensor(x[0], CPU, torch.float32, "linear", ("B", "T", ("num_freq", 5)))
    assert type(e.value) is Exception and str(e.value) == "linear must be [B, T, num_freq = 5], got shape (7, 5)"
    with pytest.raises(Exception) as e:
        D.lengths(np.zeros(4, np.int64), CPU, 3, "frames")
    assert type(e.value) is Exception and str(e.value) == "frames must be [B = 3], got shape (4,)"
    assert D.tensor(x[0], CPU, torch.float32, "linear").shape == (7, 5)             # dims None: the caller checks


def test_lengths_of_none_is_none():
    assert D.lengths(None, CPU, 3, "frames") is None
    v = D.lengths([1, 2, 3], CPU, 3, "frames")
    assert v.dtype == torch.int32 and v.tolist() == [1, 2, 3]


def test_buffers_keeps_one_set_per_key_and_only_ever_adds_to_it():
    cache = {}
    key = ("cpu", "dtw", 2, 5)
    first = D.buffers(cache, key, dist=((2,), torch.float32), ws=((0,), torch.uint8))
    assert first["dist"].shape == (2,) and first["dist"].dtype == torch.float32 and first["ws"].numel() == 0
    ptrs = {k: (v, v.data_ptr()) for k, v in first.items()}
    again = D.buffers(cache, key, dist=((2,), torch.float32), ws=((0,), torch.uint8))
    assert again is first and all(again[k] is t and t.data_ptr() == p for k, (t, p) in ptrs.items())      # the same tensors
    more = D.buffers(cache, key, dist=((2,), torch.float32), path=((2, 9, 2), torch.int32))               # a new name joins the set
    assert more is first and more["path"].shape == (2, 9, 2) and more["path"].dtype == torch.int32
    assert all(more[k] is t and t.data_ptr() == p for k, (t, p) in ptrs.items())                          # and replaces nothing
    other = D.buffers(cache, ("cpu", "dtw", 3, 5), dist=((3,), torch.float32))
    assert other is not first and other["dist"].shape == (3,) and other["dist"].data_ptr() != first["dist"].data_ptr()
    assert "path" not in other and len(cache) == 2
