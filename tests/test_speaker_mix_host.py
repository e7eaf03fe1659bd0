"""Speaker mixtures, the host side: taco_amd.speaker_weights on every accepted and every rejected form, the five *_mix symbols of
the library and their ctypes prototypes, and the Synthesizer no longer refusing a dict."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

MIX = ["taco_forward_infer_mix", "taco_plan_create_mix", "taco_encoder_forward_mix", "taco_decoder_forward_mix",
       "taco_postnet_forward_mix"]


def _sw(*a):
    import taco_amd
    return taco_amd.speaker_weights(*a)


def test_a_dict_is_one_mixture_for_every_row():
    w = _sw({0: 0.7, 2: 0.3}, 3, 4)
    assert w.dtype == np.float32 and w.shape == (4, 3) and w.flags["C_CONTIGUOUS"]
    assert np.array_equal(w, np.tile(np.array([[0.7, 0, 0.3]], np.float32), (4, 1)))
    # weights are used as given: not normalised, any sign
    assert np.array_equal(_sw({1: 2.5, 0: -0.5}, 2, 1), np.array([[-0.5, 2.5]], np.float32))
    assert np.array_equal(_sw({np.int64(1): np.float32(1)}, 2, 2), np.array([[0, 1], [0, 1]], np.float32))


def test_a_list_of_ints_and_dicts_is_per_row():
    w = _sw([0, {0: .5, 1: .5}, 1, np.int32(2)], 3, 4)
    assert w.dtype == np.float32
    assert np.array_equal(w, np.array([[1, 0, 0], [.5, .5, 0], [0, 1, 0], [0, 0, 1]], np.float32))
    assert np.array_equal(_sw((1, 0), 2, 2), np.array([[0, 1], [1, 0]], np.float32))


def test_an_array_of_the_right_shape_passes_through():
    a = np.array([[.25, .75], [1, 0], [0, 0]], np.float64)
    w = _sw(a, 2, 3)
    assert w.dtype == np.float32 and np.array_equal(w, a.astype(np.float32))
    assert np.array_equal(_sw(a.tolist(), 2, 3), w)                     # nested lists of numbers are an array
    assert np.array_equal(_sw(np.eye(2, dtype=np.int64), 2, 2), np.eye(2, dtype=np.float32))
    import torch
    assert np.array_equal(_sw(torch.tensor(a), 2, 3), w)


@pytest.mark.parametrize("spec,ns,batch", [
    ({}, 3, 2),                                         # an empty mixture
    ({3: 1.0}, 3, 2), ({-1: 1.0}, 3, 2),                # ids outside [0, num_speakers)
    ([0, 3], 3, 2), ([0, {0: .5, 5: .5}], 3, 2),
    ({0: float("nan")}, 3, 2), ({0: float("inf")}, 3, 2), ({0: 1e39}, 3, 2),      # not finite (as float32)
    ([0, {1: float("-inf")}], 3, 2),
    ([0, 1, 2], 3, 2), ([0], 3, 2), ([], 3, 2),         # a wrong length
    ({0.5: 1.0}, 3, 2), ({"0": 1.0}, 3, 2), ({True: 1.0}, 3, 2),       # ids that are not integers
    (np.ones((2, 4), np.float32), 3, 2), (np.ones((3, 3), np.float32), 3, 2), (np.ones((3,), np.float32), 3, 3),      # a wrong shape
    (np.ones((2, 3, 1), np.float32), 3, 2),
    (np.array([[1, np.nan, 0], [0, 0, 1]], np.float32), 3, 2), (np.array([[1, 1e39, 0], [0, 0, 1]], np.float64), 3, 2),
    (np.array([["a", "b", "c"]] * 2), 3, 2), (None, 3, 2), ("0", 3, 1),
    ({0: 1.0}, 0, 2), ({0: 1.0}, 3, 0),
])
def test_rejected_forms_raise(spec, ns, batch):
    with pytest.raises(ValueError):
        _sw(spec, ns, batch)


def test_the_library_exports_the_mix_entry_points_and_the_prototypes_carry_them():
    from taco_amd import _lib
    lib = _lib.load_library()
    assert lib.taco_abi_version() == 1                  # additive: the version stays
    for name in MIX:
        base = name[:-len("_mix")]
        assert name in _lib.PROTOTYPES and _lib.PROTOTYPES[name] == _lib.PROTOTYPES[base], name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(_lib.PROTOTYPES[name][1])
    # without a model nothing can be mixed: an error with a message, no crash
    z = C.c_void_p(0)
    assert lib.taco_forward_infer_mix(z, z, z, z, z, 1, 1, 1, z, z, z, z, z, z, 0) == _lib.TACO_ERR_ARG
    assert lib.taco_last_error()
    assert lib.taco_postnet_forward_mix(z, z, z, z, 1, 1, z, z, z, 0) == _lib.TACO_ERR_ARG


@pytest.mark.parametrize("B", [8, 96])
def test_a_null_model_is_refused_the_same_way_at_any_batch_size(B):
    """The forward and the three stage entries, with ids and with weights: arguments are validated before the batch is split into passes, so a
    null model is TACO_ERR_ARG ("null model") at 96 rows as at 8 -- and before any HIP call (there is no device to set)."""
    from taco_amd import _lib
    lib = _lib.load_library()
    z = C.c_void_p(0)
    for sfx in ("", "_mix"):
        calls = [(getattr(lib, "taco_forward_infer" + sfx), (z, z, z, z, z, B, 5, 3, z, z, z, z, z, z, 0)),
                 (getattr(lib, "taco_encoder_forward" + sfx), (z, z, z, z, z, B, 5, z, z, 0)),
                 (getattr(lib, "taco_decoder_forward" + sfx), (z, z, z, z, B, 5, 3, z, z, z, z, z, z, z, 0)),
                 (getattr(lib, "taco_postnet_forward" + sfx), (z, z, z, z, B, 5, z, z, z, 0))]
        for fn, a in calls:
            assert fn(*a) == _lib.TACO_ERR_ARG, (fn.__name__, B)
            assert lib.taco_last_error() == b"null model", (fn.__name__, B, lib.taco_last_error())


def test_the_header_declares_each_mix_entry_point_with_its_namesakes_arguments():
    import os
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "taco_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)

    def args(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    for name in MIX:
        mine, base = args(name), args(name[:-len("_mix")])
        assert len(mine) == len(base)
        diff = [(a, b) for a, b in zip(mine, base) if a != b]
        assert diff == [("const float* d_speaker_weights", "const int32_t* d_speaker_id")], (name, diff)


def test_the_synthesizer_routes_dicts_instead_of_refusing_them():
    import taco_amd
    src = inspect.getsource(taco_amd.synthesizer)
    assert "not supported" not in src
    assert not re.search(r"raise[^\n]*dict", src)
    s = taco_amd.Synthesizer()
    s.num_speakers = 3
    assert np.array_equal(s._speaker_feed({0: .5, 2: .5}, 2)["speaker_weights"], np.array([[.5, 0, .5]] * 2, np.float32))
    assert np.array_equal(s._speaker_feed([0, {1: 1.0}], 2)["speaker_weights"], np.array([[1, 0, 0], [0, 1, 0]], np.float32))
    for ids in (None, [0, 1], np.array([2, 1], np.int32)):        # an all-int list keeps going down the id path unchanged
        feed = s._speaker_feed(ids, 2)
        assert list(feed) == ["speaker_id"] and feed["speaker_id"] is ids
    for name in ("run", "encoder", "decoder", "postnet"):
        assert "speaker_weights" in inspect.signature(getattr(taco_amd.Tacotron, name)).parameters, name
    assert "speaker_weights" in inspect.signature(taco_amd.tacotron.PlanPool.submit).parameters
