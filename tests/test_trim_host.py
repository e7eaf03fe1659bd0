"""Host side of the silence trim (taco_wav_trim; librosa.effects.trim of synthesizer.py:266-269): the float64 restatement
tests/trim_reference.py against itself -- the long route (np.pad, frames, rfft, mean |S|^2) equals the three-sum Parseval form the
kernel uses -- its edge cases, and the C entry point's exports, workspace size and argument checks, which return before any device
call.  UNPINNED on librosa (see tests/trim_reference.py).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import trim_reference as R
from taco_amd import _lib


@pytest.mark.parametrize("N,hop", [(64, 8), (5120, 256)])
def test_rfft_route_equals_the_parseval_form(N, hop):
    rs = np.random.RandomState(N)
    y = rs.randn(3 * N + 7) + 0.3                           # an offset: the DC term is not small
    a, b = R.frame_mse(y, N, hop), R.parseval_mse(y, N, hop)
    d = float(np.abs(a - b).max() / np.abs(a).max())
    print("N %d: rfft route vs Parseval form, max relative difference %.3g over %d frames" % (N, d, len(a)))
    assert a.shape == b.shape == (1 + len(y) // hop,)
    assert d < 1e-12
    c = R.frame_mse(y, N, hop, drop_dc_nyquist=True)        # the control form differs by far more than that
    assert float(np.abs(a - c).max() / np.abs(a).max()) > 1e-3


@pytest.mark.parametrize("N,hop", [(64, 8), (80, 20), (5120, 256)])
def test_frame_count(N, hop):
    for n in (2, hop - 1, hop, hop + 1, 7 * hop - 1, 7 * hop, 7 * hop + 1):
        if n >= 2:
            assert R.frames_of(np.zeros(n), N, hop).shape == (1 + n // hop, N)
            assert R.trim(np.ones(n), 50, N, hop)[1].shape == (1 + n // hop,)


@pytest.mark.parametrize("n,N,hop", [(1500, 5120, 256), (9, 64, 8), (2, 64, 8)])
def test_a_row_shorter_than_half_a_frame_is_reflected_repeatedly(n, N, hop):
    y = np.random.RandomState(n).randn(n)
    fr = R.frames_of(y, N, hop)
    P = 2 * (n - 1)
    for t in (0, fr.shape[0] - 1):                           # the index map the kernel uses: period 2(n - 1)
        j = (np.arange(N) + t * hop - N // 2) % P
        assert np.array_equal(fr[t], y[np.where(j < n, j, P - j)])
    for energy in R.ENERGIES:
        index, db, margin = R.trim(y, 50, N, hop, energy)
        assert index.tolist() == [0, n] and np.isfinite(db).all() and db.max() == 0.0


def test_all_zero_and_degenerate_rows():
    for energy in R.ENERGIES:
        index, db, margin = R.trim(np.zeros(300), 50, 64, 8, energy)       # every frame clamps to 1e-10: db = 0 > -top_db
        assert index.tolist() == [0, 300] and np.all(db == 0.0) and margin == 50.0
    assert R.trim(np.zeros(1))[0].tolist() == [0, 1] and R.trim(np.zeros(0))[0].tolist() == [0, 0]


def test_the_two_energy_conventions_differ_on_the_burst_signal():
    x = R.burst_rows(40000, [40000], [(0.25, 0.65)], seed=0)[0]
    a, b = R.trim(x, 50, 5120, 256, "spectral"), R.trim(x, 50, 5120, 256, "time")
    print("burst on [10000, 26000) of 40000 at 5120/256/50 dB: spectral %s, time-domain %s" % (a[0].tolist(), b[0].tolist()))
    assert a[0].tolist() != b[0].tolist()
    assert b[0][0] <= a[0][0] and a[0][1] <= b[0][1]        # the Hann window narrows the frame: the spectral cut is the tighter one


def test_library_exports_the_trim_entry_points():
    lib = _lib.load_library()
    for name in ("taco_wav_trim", "taco_wav_trim_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert (_lib.TACO_TRIM_SPECTRAL, _lib.TACO_TRIM_TIME) == (0, 1)


def test_workspace_bytes_positive_and_monotone():
    lib = _lib.load_library()
    ws = lambda B, L, N=5120, hop=256: int(lib.taco_wav_trim_workspace_bytes(B, L, N, hop))
    assert ws(1, 2) > 0
    assert ws(1, 40000) >= 4 * (1 + 40000 // 256)
    for B in (1, 2, 7, 32):
        assert ws(B + 1, 40000) >= ws(B, 40000) > 0
    for L in (2, 255, 256, 40000, 153300):
        assert ws(4, 2 * L) >= ws(4, L) > 0
    assert ws(32, 153300) > ws(1, 153300) and ws(4, 153300) > ws(4, 1000)
    assert ws(4, 1000, 64, 8) >= 4 * 4 * (1 + 1000 // 8)


def test_argument_errors_return_before_any_device_call():
    """Dummy non-null addresses stand in for device memory: validation rejects every one of these calls before it is touched."""
    lib = _lib.load_library()
    d = C.c_void_p(4096)
    big = 1 << 20

    def call(wav=d, ns=None, B=2, L=1000, top_db=50.0, N=64, hop=8, energy=_lib.TACO_TRIM_SPECTRAL, index=d, db=None, ws=d, ws_bytes=big):
        return lib.taco_wav_trim(None, wav, ns, B, L, top_db, N, hop, energy, index, db, ws, ws_bytes)

    assert call(hop=0) == _lib.TACO_ERR_ARG and call(hop=-3) == _lib.TACO_ERR_ARG
    assert call(N=1) == _lib.TACO_ERR_ARG and call(N=0) == _lib.TACO_ERR_ARG
    assert call(energy=2) == _lib.TACO_ERR_ARG and call(energy=-1) == _lib.TACO_ERR_ARG
    assert call(wav=None) == _lib.TACO_ERR_ARG
    assert call(index=None) == _lib.TACO_ERR_ARG
    assert call(ws=None) == _lib.TACO_ERR_ARG
    assert call(B=0) == _lib.TACO_ERR_ARG and call(L=0) == _lib.TACO_ERR_ARG
    need = int(lib.taco_wav_trim_workspace_bytes(2, 1000, 64, 8))
    assert call(ws_bytes=need - 1) == _lib.TACO_ERR_ARG and call(ws_bytes=0) == _lib.TACO_ERR_ARG
    assert b"workspace" in lib.taco_last_error()
    assert call(N=65) == _lib.TACO_ERR_UNSUPPORTED and call(N=5121, hop=256) == _lib.TACO_ERR_UNSUPPORTED      # odd
    assert call(N=8194, hop=256) == _lib.TACO_ERR_UNSUPPORTED                                                  # frame + window past the LDS limit
    assert call(N=16386, hop=256, energy=_lib.TACO_TRIM_TIME) == _lib.TACO_ERR_UNSUPPORTED
    assert b"LDS" in lib.taco_last_error()
