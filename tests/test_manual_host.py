"""Second-pass manual alignments on the device (taco_manual_alignments, synthesizer.py:171-205), the host side: the symbol, its ctypes
prototype and its declaration, every argument error (all returned before any HIP call, so they work without a GPU), and the new
keyword on the two Python entry points.  The kernel itself is held to NumPy in tests/test_gpu_manual.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from taco_amd import _lib

NAME = "taco_manual_alignments"
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "taco_abi.h")


def test_the_library_exports_the_symbol_and_the_prototype_carries_it():
    lib = _lib.load_library()
    assert lib.taco_abi_version() == 1                  # additive: the version stays
    assert NAME in _lib.PROTOTYPES
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]


def test_the_header_declares_it_directly_after_the_attention_trim():
    text = open(HEADER).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(([^;]*)\)\s*;" % NAME, text, flags=re.S)
    assert m, "not declared"
    comment = re.sub(r"\s+", " ", m.group(1))
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    assert args == ["void* hip_stream", "const float* d_alignments", "int B", "int T_in", "int n_steps", "int mode", "float* d_manual"]
    # the comment cites the reference lines and states the axis, the tie rule and that mode 2 is refused
    assert "synthesizer.py:171-205" in comment and "DECODER steps" in comment and "first index of the maximum" in comment
    assert "NaN" in comment and "mode 2" in comment and "np.pow" in comment and "TACO_ERR_UNSUPPORTED" in comment
    bare = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    order = [x.group(1) for x in re.finditer(r"\b(?:int|void|size_t)\s+(taco_\w+)\s*\(", bare)]
    assert order[order.index("taco_attention_trim") + 1] == NAME


def test_argument_errors_return_before_any_device_call():
    """Dummy non-null addresses stand in for device memory: validation rejects every one of these calls before it is touched."""
    lib = _lib.load_library()
    A, O = 1 << 20, 1 << 24                                           # 16 MiB apart: disjoint for every size used here

    def call(a=A, o=O, B=2, T_in=3, n=5, mode=1):
        rc = lib.taco_manual_alignments(None, C.c_void_p(a) if a else None, B, T_in, n, mode, C.c_void_p(o) if o else None)
        return rc, lib.taco_last_error()

    for kw in (dict(a=0), dict(o=0), dict(a=0, o=0)):
        rc, msg = call(**kw)
        assert rc == _lib.TACO_ERR_ARG and b"null" in msg, kw
    for kw in (dict(B=0), dict(T_in=0), dict(n=0), dict(B=-1), dict(T_in=-7), dict(n=-2 ** 31)):
        rc, msg = call(**kw)
        assert rc == _lib.TACO_ERR_ARG and b">= 1" in msg, kw
    nbytes = 2 * 3 * 5 * 4
    for a, o in ((A, A), (A, A + 4), (A + 4, A), (A, A + nbytes - 4), (A + nbytes - 4, A)):
        for mode in (1, 3):
            rc, msg = call(a=a, o=o, mode=mode)
            assert rc == _lib.TACO_ERR_ARG and b"overlap" in msg, (a, o, mode)
    rc, msg = call(mode=2)
    assert rc == _lib.TACO_ERR_UNSUPPORTED and b"np.pow" in msg and b"synthesizer.py:181-188" in msg
    for mode in (0, -1, 4, 2 ** 31 - 1):
        rc, msg = call(mode=mode)
        assert rc == _lib.TACO_ERR_ARG and b"manual_attention_mode" in msg, mode
    # buffers that touch but do not overlap get past the overlap check (here they end at the mode check: still no device call)
    for a, o in ((A, A + nbytes), (A + nbytes, A)):
        rc, msg = call(a=a, o=o, mode=2)
        assert rc == _lib.TACO_ERR_UNSUPPORTED
    # sizes whose byte count does not fit 64 bits are not mistaken for small ones
    rc, msg = call(a=A, o=O, B=2 ** 31 - 1, T_in=2 ** 31 - 1, n=2 ** 31 - 1, mode=1)
    assert rc == _lib.TACO_ERR_ARG and b"overlap" in msg


def test_the_python_entry_points_take_manual_attention_mode():
    import taco_amd
    for fn in (taco_amd.Tacotron.run, taco_amd.Synthesizer.synthesize_audio, taco_amd.Synthesizer.synthesize):
        p = inspect.signature(fn).parameters
        assert "manual_attention_mode" in p and p["manual_attention_mode"].default == 0, fn
    p = inspect.signature(taco_amd.Tacotron.manual_alignments_from).parameters
    assert list(p)[1:] == ["alignments", "mode", "out"] and p["out"].default is None


def test_mode_2_and_a_double_request_raise_before_the_model_is_touched():
    """Both refusals come before the first forward, so a Synthesizer without a model shows them."""
    import pytest
    import taco_amd
    from taco_amd.synthesizer import manual_alignments_of
    with pytest.raises(Exception) as host:
        manual_alignments_of(np.zeros((1, 2, 2), np.float32), 2)
    m = taco_amd.Tacotron()
    m._handle = object()                                              # stands in for a built model: mode 2 is refused before it is used
    with pytest.raises(Exception) as e:
        m.run(inputs=np.zeros((1, 2), np.int32), input_lengths=np.ones((1,), np.int32), manual_attention_mode=2)
    assert str(e.value) == str(host.value) and type(e.value) is Exception
    with pytest.raises(Exception) as e:
        m.manual_alignments_from(None, 2)
    assert str(e.value) == str(host.value)
    m._handle = None
    s = taco_amd.Synthesizer()
    with pytest.raises(_lib.TacoError) as e:
        s.synthesize_audio(tokens=np.array([[5, 1]]), manual_attention_mode=1, manual_alignments=np.zeros((1, 1, 2), np.float32))
    assert e.value.code == _lib.TACO_ERR_ARG
