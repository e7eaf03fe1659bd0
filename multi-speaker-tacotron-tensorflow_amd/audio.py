"""Spectrogram -> waveform on the GPU: `inv_spectrogram` of the reference's audio/__init__.py:54-56 (denormalise, dB -> amplitude,
^power, Griffin-Lim with librosa-semantics STFT/ISTFT, inverse pre-emphasis), the step synthesizer.py:264 runs on the CPU for
every utterance -- and waveform -> the linear and mel targets training consumes: `spectrogram` / `melspectrogram` of
audio/__init__.py:48-51,64-67, which datasets/generate_data.py:151-158 runs on the CPU for every corpus file (class Spectrogram).
The reference's two other vocoders are here as well: `inv_spectrogram_tensorflow` (:59-61,87-96, the deterministic Griffin-Lim of its
inference graph, GriffinLim(flavor="tensorflow")) and `inv_melspectrogram` (:70-72,136-140, GriffinLim.inv_melspectrogram).  With them
every arithmetic function of the reference's audio/__init__.py runs on the device.
All arithmetic is in libtaco_hip (taco_gl_*, taco_spec_*); PyTorch holds the buffers.  The host computations are the mel filter
bank (mel_basis) and its pseudo-inverse (inv_mel_basis), built once in float64 and uploaded.
Recordings reach the model's sample rate through class Resampler (taco_resample_*, taco_wav_resample): librosa.core.load's and
resample_audio's band-limited sinc interpolation (audio/__init__.py:12-20,30-32), whose one host computation is the Kaiser-windowed
half filter (kaiser_window).
Every public method reaches the library through the package's one marshalling layer (_device.py): tensor / lengths (inputs onto the
device, shape checks), workspace (the handle's scratch memory) and call (device, stream, pointers, status)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._device import STREAM, Handle, call, lengths, tensor, workspace


def hz_to_mel(f):
    """Slaney's scale (librosa.hz_to_mel, htk=False): linear below 1 kHz (200/3 Hz per mel), logarithmic above (27 mels per factor 6.4)."""
    f = np.asarray(f, np.float64)
    lin = f / (200.0 / 3)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / (np.log(6.4) / 27.0), lin)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (np.maximum(m, 15.0) - 15.0)), (200.0 / 3) * m)


def mel_basis(hparams):
    """The filter bank of the reference's _build_mel_basis (audio/__init__.py:142-144): librosa.filters.mel(sample_rate, n_fft,
    n_mels=num_mels) with librosa's defaults -- fmin 0, fmax sample_rate/2, Slaney's mel scale (htk=False), Slaney's area
    normalisation -- restated in NumPy float64 from librosa's documented algorithm (0.5/0.6 era): num_mels + 2 points evenly spaced
    in mels, and on the grid of bin frequencies the triangle max(0, min(rising ramp, falling ramp)) times 2 / (its width in Hz).
    Returns [num_mels, num_freq].  UNPINNED on librosa itself (this project does not depend on it and no test runs it): it is held by an
    independently written per-filter formulation (tests/spec_reference.py, tests/test_spec_host.py) and by the scale's known
    points.  Whether librosa of that era returned float32 or float64 is unknown as well; this stays float64 and is cast to float32
    at upload."""
    g = lambda k, d: getattr(hparams, k, d)
    sr, num_freq, n_mels = float(g("sample_rate", 24000)), int(g("num_freq", 1025)), int(g("num_mels", 80))
    fftfreqs = np.linspace(0.0, sr / 2, num_freq)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    return weights * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]


def inv_mel_basis(hparams):
    """The reference's _inv_mel_basis (audio/__init__.py:136-140): np.linalg.pinv(_build_mel_basis()), [num_freq, num_mels], float64
    (cast to float32 at upload).  The filter bank has full row rank, so mel_basis . inv_mel_basis = I.  As UNPINNED on librosa as
    mel_basis is."""
    return np.linalg.pinv(mel_basis(hparams))


def c_audio_hparams(hparams):
    g = lambda k, d: getattr(hparams, k, d)
    return _lib.TacoAudioHParams(
        num_freq=int(g("num_freq", 1025)), sample_rate=int(g("sample_rate", 24000)), griffin_lim_iters=int(g("griffin_lim_iters", 60)),
        frame_length_ms=float(g("frame_length_ms", 50)), frame_shift_ms=float(g("frame_shift_ms", 12.5)),
        preemphasis=float(g("preemphasis", 0.97)), min_level_db=float(g("min_level_db", -100)), ref_level_db=float(g("ref_level_db", 20)),
        power=float(g("power", 1.5)))


def num_frames(hparams, n_samples):
    """Frames of spectrogram(y) for n_samples samples: 1 + n_samples // hop (taco_spec_num_frames; host arithmetic, no GPU needed)."""
    hp = c_audio_hparams(hparams)
    return int(_lib.load_library().taco_spec_num_frames(C.byref(hp), int(n_samples)))


_ENERGY = {"spectral": _lib.TACO_TRIM_SPECTRAL, "time": _lib.TACO_TRIM_TIME}      # frame energies of trim / split


def _energy(name):
    if name not in _ENERGY:
        raise _lib.TacoError(_lib.TACO_ERR_ARG, "energy must be one of %s, got %r" % (sorted(_ENERGY), name))
    return _ENERGY[name]


def pcm_frame_of_ms(j, sample_rate):
    """The frame at which millisecond j starts: floor(j * sr / 1000), pydub's int(j * (sr / 1000.0)) (include/taco_abi.h)"""
    return int(j) * int(sample_rate) // 1000


def pcm_len_ms(n, sample_rate):
    """Milliseconds of n frames: pydub's len(AudioSegment) = round(1000 * (n / sr)), Python's round (half to even)"""
    return int(round(1000.0 * (int(n) / float(sample_rate))))


def pcm_threshold(silence_thresh):
    """The integer bound k = floor(10^(dB/20) * 32768) of taco_pcm_nonsilent: audioop.rms returns an integer, so pydub's rms <= thresh
    is rms <= k.  No rms passes 32768, so a larger k means what 32768 does."""
    return int(min(np.floor(10 ** (float(silence_thresh) / 20) * 32768.0), 32768.0))


class GriffinLim(Handle):
    """flavor "librosa" (default): the handle of inv_spectrogram / inv_melspectrogram and of everything Spectrogram adds.  "tensorflow":
    the handle of inv_spectrogram_tensorflow (tf.contrib.signal's uncentred STFT; the librosa-flavour methods raise TacoError on it).
    pcm16, trim, split, remove_breath, nonsilent, range_sumsq, apply_gains, set_inv_mel_basis and mel_to_linear work on either, and
    so does the momentum of Fast Griffin-Lim (set_momentum; not in the reference, off by default); convergence is librosa-flavour."""
    _destroy = "taco_gl_destroy"

    def __init__(self, hparams, device="cuda:0", flavor="librosa", momentum=0.0):
        """momentum: Fast Griffin-Lim (set_momentum); 0, the default, is the reference's loop."""
        self.hp = c_audio_hparams(hparams)
        self.hparams = hparams
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.TacoError(_lib.TACO_ERR_ARG, "GriffinLim runs on a GPU (got %s); there is no CPU fallback" % device)
        if flavor not in ("librosa", "tensorflow"):
            raise _lib.TacoError(_lib.TACO_ERR_ARG, "flavor must be 'librosa' or 'tensorflow', got %r" % (flavor,))
        self.flavor = flavor
        self._lib = _lib.load_library()
        self._h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        create = self._lib.taco_gl_create_tf if flavor == "tensorflow" else self._lib.taco_gl_create
        _lib.check(create(C.byref(self.hp), idx, C.byref(self._h)))
        self._ws = None
        self._inv_mels = 0
        if momentum:
            self.set_momentum(momentum)

    def set_momentum(self, momentum):
        """Fast Griffin-Lim (Perraudin, Balazs, Sondergaard 2013) in the loop of all three vocoders: every iteration projects
        stft(y) - c * (the estimate before it), c = momentum / (1 + momentum).  0 <= momentum <= 1; 0 is the reference's loop, bit
        for bit; 0.99 is librosa.griffinlim's default.  Stays set until changed.  A non-zero value adds one estimate buffer to the
        loop's workspace: every vocoder call asks the library for its size after the momentum is set."""
        _lib.check(self._lib.taco_gl_set_momentum(self._h, float(momentum)))

    @property
    def momentum(self):
        return float(self._lib.taco_gl_momentum(self._h))

    def _momentum(self, momentum):
        """The momentum keyword of the vocoder methods: None keeps the handle's value, a value is set and stays set"""
        if momentum is not None:
            self.set_momentum(momentum)

    def num_samples(self, T):
        return int(self._lib.taco_gl_num_samples(self._h, T))

    def min_frames(self):
        return int(self._lib.taco_gl_min_frames(self._h))

    def inv_spectrogram(self, linear, init_uniform=None, seed=0, iters=None, momentum=None):
        """linear [B, T, num_freq] (model layout; numpy or tensor) -> waveforms [B, hop*(T-1)] (device tensor).
        init_uniform [B, T, num_freq] in [0,1) replaces the reference's np.random.rand initial phases (default: hash of seed).
        momentum: None keeps the handle's (set_momentum); a value is set for this call and stays set."""
        return self.inv_spectrogram_rows(linear, None, init_uniform, seed, iters, momentum)[0]

    def inv_spectrogram_rows(self, linear, frames, init_uniform=None, seed=0, iters=None, momentum=None):
        """Per utterance length (synthesizer.py:242-264: `inv_spectrogram(wav[:spec_end_idx].T)`): linear [B, T, num_freq], frames [B]
        (a device int32 tensor is used as it is and never read on the host -- Synthesizer.attention_trim's kernel output; host data is
        uploaded; None: all T) -> (wav [B, hop*(T-1)], num_samples [B] int32), device tensors.  Row b holds the waveform of its first
        frames[b] frames (clamped to [min_frames(), T]) in its first num_samples[b] samples and zeros after.  momentum as inv_spectrogram."""
        return self._vocode_rows(self._lib.taco_gl_inv_spectrogram_rows, linear, "linear", ("num_freq", self.hp.num_freq), frames, init_uniform, seed, iters,
                                 momentum)

    def _vocode_rows(self, fn, x, what, width, frames, init_uniform, seed, iters, momentum=None):
        """The librosa-flavour vocoders: fn is the entry point, x [B, T, width[1]] its input, named `what` and its last dimension width[0] in errors"""
        dev = self.device
        x = tensor(x, dev, torch.float32, what, ("B", "T", width))
        B, T, _ = x.shape
        u = None if init_uniform is None else tensor(init_uniform, dev, torch.float32, "init_uniform", (("B", B), ("T", T), ("num_freq", self.hp.num_freq)))
        fr = lengths(frames, dev, B, "frames")
        self._momentum(momentum)      # before the size is asked for: the workspace depends on it
        ws = workspace(self, self._lib.taco_gl_rows_workspace_bytes(self._h, B, T))
        wav = torch.empty((B, self.num_samples(T)), dtype=torch.float32, device=dev)
        ns = torch.empty((B,), dtype=torch.int32, device=dev)
        call(dev, fn, self._h, STREAM, x, fr, u, C.c_ulonglong(int(seed)), B, T, -1 if iters is None else int(iters), wav, ns, ws, ws.numel())
        return wav, ns

    def tf_num_samples(self, T):
        return int(self._lib.taco_gl_tf_num_samples(self._h, T))

    def inv_spectrogram_tensorflow(self, linear, frames=None, iters=None, momentum=None):
        """inv_spectrogram_tensorflow of audio/__init__.py:59-61,87-96 (the reference's Synthesizer.wav_output, synthesizer.py:53-54) on
        a flavor="tensorflow" handle: linear [B, T, num_freq], frames [B] (a device int32 tensor is used as it is; None: all T; clamped
        to [1, T]) -> (wav [B, hop*(T-1) + win], num_samples [B] int32), device tensors.  Zero initial phase, est / max(1e-8, |est|), no
        inverse pre-emphasis: the same spectrogram always gives the same samples.  Row b is the vocoding of linear[b, :frames[b]] in
        its first hop*(frames[b]-1) + win samples, zeros after.  UNPINNED on TensorFlow: tf.contrib.signal.stft / inverse_stft restated
        (include/taco_abi.h), checked against tests/vocoder_reference.py, not against TensorFlow.  momentum as inv_spectrogram."""
        dev = self.device
        x = tensor(linear, dev, torch.float32, "linear", ("B", "T", ("num_freq", self.hp.num_freq)))
        B, T, _ = x.shape
        fr = lengths(frames, dev, B, "frames")
        self._momentum(momentum)      # before the size is asked for: the workspace depends on it
        ws = workspace(self, self._lib.taco_gl_tf_workspace_bytes(self._h, B, T))
        wav = torch.empty((B, self.tf_num_samples(T)), dtype=torch.float32, device=dev)
        ns = torch.empty((B,), dtype=torch.int32, device=dev)
        call(dev, self._lib.taco_gl_inv_spectrogram_tf, self._h, STREAM, x, fr, B, T, -1 if iters is None else int(iters), wav, ns, ws, ws.numel())
        return wav, ns

    def set_inv_mel_basis(self, inv=None):
        """Uploads the pseudo-inverse of the mel filter bank, [num_freq, num_mels]; None: inv_mel_basis(hparams)."""
        b = np.ascontiguousarray(np.asarray(inv_mel_basis(self.hparams) if inv is None else inv), dtype=np.float32)
        if b.ndim != 2 or b.shape[0] != self.hp.num_freq:
            raise Exception("inv must be [num_freq = %d, num_mels], got %s" % (self.hp.num_freq, b.shape))
        _lib.check(self._lib.taco_gl_set_inv_mel_basis(self._h, b.ctypes.data_as(C.c_void_p), b.shape[1]))
        self._inv_mels = int(b.shape[1])

    @property
    def inv_mels(self):
        """Filters of the inverse basis in use; 0: set_inv_mel_basis has not been called"""
        return self._inv_mels

    def _need_inv_mels(self):
        if not self._inv_mels:
            raise _lib.TacoError(_lib.TACO_ERR_STATE, "the mel vocoder needs the inverse basis: call set_inv_mel_basis first")
        return self._inv_mels

    def mel_to_linear(self, mel):
        """_mel_to_linear(_db_to_amp(_denormalize(mel))) of audio/__init__.py:71,136-140: mel [B, T, num_mels] (normalised, as the model's
        mel_outputs) -> linear magnitudes [B, T, num_freq] (device tensor), floored at 1e-10, before ^power."""
        x = tensor(mel, self.device, torch.float32, "mel", ("B", "T", ("num_mels", self._need_inv_mels())))
        B, T, _ = x.shape
        out = torch.empty((B, T, self.hp.num_freq), dtype=torch.float32, device=self.device)
        call(self.device, self._lib.taco_gl_mel_to_linear, self._h, STREAM, x, B, T, out)
        return out

    def inv_melspectrogram(self, mel, frames=None, init_uniform=None, seed=0, iters=None, momentum=None):
        """inv_melspectrogram of audio/__init__.py:70-72 per utterance length: mel [B, T, num_mels] -> (wav [B, hop*(T-1)], num_samples [B]
        int32), device tensors; frames, init_uniform, seed, iters and momentum as inv_spectrogram_rows."""
        return self._vocode_rows(self._lib.taco_gl_inv_melspectrogram_rows, mel, "mel", ("num_mels", self._need_inv_mels()), frames, init_uniform, seed, iters,
                                 momentum)

    _TARGET_KINDS = {"normalised": 0, "magnitude": 1}

    def convergence(self, target, wav, frames=None, kind="normalised"):
        """Spectral convergence || |stft(y)| - S || / || S || per utterance (taco_gl_convergence): how consistent the phases of a
        vocoder's output are with the magnitudes it was made from, at any momentum and iteration count.  wav [B, hop*(T-1)] is the
        output rectangle of inv_spectrogram(_rows) / inv_melspectrogram, frames [B] the vector that call was given (None: all T).
        target [B, T, num_freq]: kind "normalised", the linear spectrogram the vocoder took; kind "magnitude", the magnitudes
        themselves -- for the mel vocoder mel_to_linear(mel) ** hparams.power.  Returns a device tensor [B]; 0 for a silent target.
        librosa flavour only."""
        if kind not in self._TARGET_KINDS:
            raise _lib.TacoError(_lib.TACO_ERR_ARG, "kind must be one of %s, got %r" % (sorted(self._TARGET_KINDS), kind))
        dev = self.device
        x = tensor(target, dev, torch.float32, "target", ("B", "T", ("num_freq", self.hp.num_freq)))
        B, T, _ = x.shape
        y = tensor(wav, dev, torch.float32, "wav", (("B", B), ("hop*(T-1)", self.num_samples(T))))
        fr = lengths(frames, dev, B, "frames")
        ws = workspace(self, self._lib.taco_gl_convergence_workspace_bytes(self._h, B, T))
        sc = torch.empty((B,), dtype=torch.float32, device=dev)
        call(dev, self._lib.taco_gl_convergence, self._h, STREAM, x, self._TARGET_KINDS[kind], fr, y, B, T, sc, ws, ws.numel())
        return sc

    def pcm16(self, wav, num_samples=None):
        """save_audio's scaling (audio/__init__.py:23-24) per row: wav [B, L] float32, num_samples [B] (None: L) -> int16 [B, L] (device
        tensor); row b is x * 32767 / max(0.01, max|x[:num_samples[b]]|) truncated, zeros past num_samples[b]."""
        x = tensor(wav, self.device, torch.float32, "wav", ("B", "L"))
        B, L = x.shape
        ns = lengths(num_samples, self.device, B, "num_samples")
        pcm = torch.empty((B, L), dtype=torch.int16, device=self.device)
        call(self.device, self._lib.taco_wav_to_pcm16, STREAM, x, ns, B, L, pcm)
        return pcm

    def trim(self, wav, num_samples=None, top_db=60, frame_length=2048, hop_length=512, energy="spectral", return_db=False):
        """librosa.effects.trim's index per row (synthesizer.py:266-269 calls it with top_db=50, frame_length=5120, hop_length=256; the
        defaults here are librosa's): wav [B, L] float32, num_samples [B] (a device int32 tensor is used as it is; None: L) -> index
        [B, 2] int32 (device tensor), row b = [start, end] of the non-silent part of its first num_samples[b] samples; with return_db
        also the frames' dB below the loudest frame, [B, 1 + L // hop_length], zeros past a row's own 1 + n_b // hop_length frames.
        energy "spectral" is librosa 0.5.x (the reference's pin: mean of the one-sided |stft|^2, Hann window), "time" librosa >= 0.6
        (mean square of the unwindowed frame).  UNPINNED on librosa: a restatement of the documented algorithm (include/taco_abi.h,
        taco_wav_trim), checked against tests/trim_reference.py, not against librosa."""
        dev = self.device
        x = tensor(wav, dev, torch.float32, "wav", ("B", "L"))
        B, L = x.shape
        ns = lengths(num_samples, dev, B, "num_samples")
        mode, frame_length, hop_length = _energy(energy), int(frame_length), int(hop_length)
        ws = workspace(self, self._lib.taco_wav_trim_workspace_bytes(B, L, frame_length, hop_length))
        index = torch.empty((B, 2), dtype=torch.int32, device=dev)
        db = torch.empty((B, 1 + L // max(hop_length, 1)), dtype=torch.float32, device=dev) if return_db else None
        call(dev, self._lib.taco_wav_trim, STREAM, x, ns, B, L, float(top_db), frame_length, hop_length, mode, index, db, ws, ws.numel())
        return (index, db) if return_db else index

    def split(self, wav, num_samples=None, top_db=60, frame_length=2048, hop_length=512, energy="spectral", max_intervals=None, return_db=False):
        """librosa.effects.split per row (audio/silence.py:44-45 calls it with top_db=40, frame_length=1024, hop_length=256, remove_breath
        with 40 / 128 / 32; the defaults here are librosa's): wav [B, L] float32, num_samples [B] (a device int32 tensor is used as it
        is; None: L) -> (intervals [B, M, 2], counts [B]), device int32 tensors: row b's maximal runs of non-silent frames in order as
        [start, end) in samples, counts[b] of them, exact zeros after; with return_db also the frames' dB as `trim` returns them.  M =
        max_intervals, by default (Fmax + 1) // 2 with Fmax = 1 + L // hop_length, the most runs Fmax frames can hold, so the table
        never overflows; with a smaller M counts still holds the true number and the first M runs are written.  Frames, energies and
        the threshold are `trim`'s: intervals[b, 0, 0] and intervals[b, counts[b] - 1, 1] are its index.  UNPINNED on librosa
        (include/taco_abi.h, taco_wav_split), checked against tests/split_reference.py, not against librosa."""
        dev = self.device
        x = tensor(wav, dev, torch.float32, "wav", ("B", "L"))
        B, L = x.shape
        ns = lengths(num_samples, dev, B, "num_samples")
        mode, frame_length, hop_length = _energy(energy), int(frame_length), int(hop_length)
        fmax = 1 + L // max(hop_length, 1)
        M = (fmax + 1) // 2 if max_intervals is None else int(max_intervals)
        ws = workspace(self, self._lib.taco_wav_split_workspace_bytes(B, L, frame_length, hop_length))
        intervals = torch.empty((B, max(M, 1), 2), dtype=torch.int32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        db = torch.empty((B, fmax), dtype=torch.float32, device=dev) if return_db else None
        call(dev, self._lib.taco_wav_split, STREAM, x, ns, B, L, float(top_db), frame_length, hop_length, mode, M, intervals, counts, db, ws,
              ws.numel())
        return (intervals, counts, db) if return_db else (intervals, counts)

    def remove_breath(self, wav, num_samples=None, top_db=40, frame_length=128, hop_length=32, threshold=0.05, energy="spectral", return_info=False):
        """remove_breath of audio/silence.py:21-31 per row of a rectangle (the defaults are its constants): `split` at 128 / 32, then
        every interval whose mean |x| lies more than `threshold` below the row's -- re-evaluated after every mute, as the reference
        mutes in place -- is set to zero.  wav [B, L], num_samples [B] or None -> the muted waveforms [B, L] (a new device tensor:
        bits of the input outside the muted intervals, zeros past num_samples[b]); with return_info also (intervals, counts, muted
        [B, M] int32, abs_mean [B, 1 + M] float32: the row's mean before any mute, then each interval's)."""
        dev = self.device
        x = tensor(wav, dev, torch.float32, "wav", ("B", "L"))
        B, L = x.shape
        ns = lengths(num_samples, dev, B, "num_samples")
        intervals, counts = self.split(x, ns, top_db=top_db, frame_length=frame_length, hop_length=hop_length, energy=energy)
        M = intervals.shape[1]
        out = torch.empty_like(x)
        muted = torch.empty((B, M), dtype=torch.int32, device=dev) if return_info else None
        mean = torch.empty((B, 1 + M), dtype=torch.float32, device=dev) if return_info else None
        call(dev, self._lib.taco_wav_breath_mute, STREAM, x, ns, B, L, intervals, counts, M, float(threshold), out, muted, mean)
        return (out, (intervals, counts, muted, mean)) if return_info else out

    def _pcm(self, pcm):
        """int16 [B, L] (one channel) or [B, L, channels] interleaved, numpy or tensor -> a contiguous [B, L, channels] device tensor"""
        x = pcm if torch.is_tensor(pcm) else torch.as_tensor(np.asarray(pcm))
        if x.dtype != torch.int16:
            raise _lib.TacoError(_lib.TACO_ERR_ARG, "pcm must be int16 (16-bit PCM, as pydub's AudioSegment holds it), got %s: pcm16 turns a float "
                                 "waveform into it" % (x.dtype,))
        if x.dim() not in (2, 3):
            raise Exception("pcm must be [B, L] or [B, L, channels], got shape %s" % (tuple(x.shape),))
        x = x.to(self.device).contiguous()
        return x.unsqueeze(2) if x.dim() == 2 else x

    def nonsilent(self, pcm, num_frames=None, sample_rate=None, min_silence_len=1000, silence_thresh=-16, max_ranges=None, return_window_sumsq=False,
                  return_energy=False):
        """pydub.silence.detect_nonsilent (seek_step=1) per row (audio/silence.py:90-92 calls it with min_silence_len=100,
        silence_thresh=-40, app.py:34-35 with 300 / -50; the defaults here are pydub's): pcm int16 [B, L] or [B, L, channels] interleaved
        (a float input is refused: see pcm16), num_frames [B] (a device int32 tensor is used as it is; None: L), sample_rate (None:
        hparams.sample_rate) -> (ranges [B, R, 2], counts [B], len_ms [B]), device int32 tensors: row b's non-silent ranges in
        milliseconds in order, counts[b] of them, exact zeros after, and the row's length in milliseconds.  R = max_ranges, by default
        Mmax // (min_silence_len + 1) + 2, the most ranges Mmax = pcm_len_ms(L) milliseconds can hold; with a smaller R counts still
        holds the true number and the first R ranges are written.  return_window_sumsq: also every window's sum of squares, int64
        [B, Mmax], zeros past a row's own windows; return_energy: also the per-millisecond sums of squares int64 [B, Mmax] range_sumsq
        takes (the call then works in a workspace of its own, which the tensor keeps alive; entries at or past a row's len_ms are
        not written).  The threshold reaches the device as the integer k = pcm_threshold(silence_thresh).  UNPINNED on pydub
        (include/taco_abi.h, taco_pcm_nonsilent), checked against tests/pydub_reference.py and the standard library's audioop."""
        dev = self.device
        x = self._pcm(pcm)
        B, L, ch = x.shape
        sr = int(getattr(self.hparams, "sample_rate", 24000) if sample_rate is None else sample_rate)
        W = int(min_silence_len)
        nf = lengths(num_frames, dev, B, "num_frames")
        mmax = pcm_len_ms(L, sr) if sr >= 1 and L >= 1 else 0
        R = mmax // (max(W, 1) + 1) + 2 if max_ranges is None else int(max_ranges)
        nbytes = self._lib.taco_pcm_nonsilent_workspace_bytes(B, L, sr)
        ws = torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=dev) if return_energy else workspace(self, max(nbytes, 8))
        ranges = torch.empty((B, max(R, 1), 2), dtype=torch.int32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        len_ms = torch.empty((B,), dtype=torch.int32, device=dev)
        wss = torch.empty((B, mmax), dtype=torch.int64, device=dev) if return_window_sumsq else None
        call(dev, self._lib.taco_pcm_nonsilent, STREAM, x, nf, B, L, ch, sr, W, pcm_threshold(silence_thresh), R, ranges, counts, len_ms, wss, ws,
              ws.numel())
        out = (ranges, counts, len_ms)
        if return_window_sumsq:
            out += (wss,)
        if return_energy:
            out += (ws[:B * mmax * 8].view(torch.int64).view(B, mmax),)
        return out

    def range_sumsq(self, energy, ranges, counts, L, channels, num_frames=None, sample_rate=None):
        """The exact sum of squares and the number of samples of every range of a table in milliseconds: energy int64 [B, Mmax] as
        `nonsilent(..., return_energy=True)` of a rectangle of L frames returned it, ranges int32 [B, R, 2], counts [B] -> (sumsq, samples),
        int64 [B, R] device tensors, zeros at and past counts[b] (taco_pcm_range_sumsq)."""
        dev = self.device
        sr = int(getattr(self.hparams, "sample_rate", 24000) if sample_rate is None else sample_rate)
        L, channels = int(L), int(channels)
        ranges = tensor(ranges, dev, torch.int32, "ranges", ("B", "R", ("2", 2)))
        B, R, _ = ranges.shape
        mmax = pcm_len_ms(L, sr) if sr >= 1 and L >= 1 else 0
        energy = tensor(energy, dev, torch.int64, "energy", (("B", B), ("Mmax", mmax)))
        counts = lengths(counts, dev, B, "counts")
        nf = lengths(num_frames, dev, B, "num_frames")
        sumsq = torch.empty((B, R), dtype=torch.int64, device=dev)
        samples = torch.empty((B, R), dtype=torch.int64, device=dev)
        call(dev, self._lib.taco_pcm_range_sumsq, STREAM, energy if mmax else sumsq, nf, B, L, channels, sr, ranges, counts, R, sumsq, samples)
        return sumsq, samples

    def apply_gains(self, pcm, ranges, counts, gains, num_frames=None, sample_rate=None):
        """audioop.mul per range and the cut of app.py's amplify: pcm int16 [B, L(, channels)], ranges int32 [B, R, 2] in milliseconds
        and in order, counts [B], gains float64 [B, R] -> (out int16 [B, L_out, channels], out_frames [B] int32), device tensors: row b
        holds the frames from its first range's start to its end in milliseconds, a sample inside range k as clip(floor(x * gains[b,
        k])), a sample between ranges unchanged, zeros after out_frames[b]; L_out = pcm_frame_of_ms(pcm_len_ms(L)) (taco_pcm_apply_gains)."""
        dev = self.device
        x = self._pcm(pcm)
        B, L, ch = x.shape
        sr = int(getattr(self.hparams, "sample_rate", 24000) if sample_rate is None else sample_rate)
        ranges = tensor(ranges, dev, torch.int32, "ranges", (("B", B), "R", ("2", 2)))
        R = ranges.shape[1]
        counts = lengths(counts, dev, B, "counts")
        gains = tensor(gains, dev, torch.float64, "gains", (("B", B), ("R", R)))
        nf = lengths(num_frames, dev, B, "num_frames")
        L_out = max(1, pcm_frame_of_ms(pcm_len_ms(L, sr), sr)) if sr >= 1 else 1
        out = torch.empty((B, L_out, ch), dtype=torch.int16, device=dev)
        on = torch.empty((B,), dtype=torch.int32, device=dev)
        call(dev, self._lib.taco_pcm_apply_gains, STREAM, x, nf, B, L, ch, sr, ranges, counts, R, gains, out, L_out, on)
        return out, on


class Spectrogram(GriffinLim):
    """Waveform -> training targets on the GPU, on the handle (windowed-DFT pack, slots, workspace) of GriffinLim.
    basis: "slaney" (default) uploads mel_basis(hparams); an array [num_mels, num_freq] uploads that; None uploads nothing, and mel
    outputs raise TacoError until set_mel_basis is called."""

    def __init__(self, hparams, device="cuda:0", basis="slaney"):
        super(Spectrogram, self).__init__(hparams, device)
        if basis is not None:
            self.set_mel_basis(mel_basis(hparams) if isinstance(basis, str) else basis)

    def set_mel_basis(self, basis):
        b = np.ascontiguousarray(np.asarray(basis), dtype=np.float32)
        if b.ndim != 2 or b.shape[1] != self.hp.num_freq:
            raise Exception("basis must be [num_mels, num_freq = %d], got %s" % (self.hp.num_freq, b.shape))
        _lib.check(self._lib.taco_gl_set_mel_basis(self._h, b.ctypes.data_as(C.c_void_p), b.shape[0]))

    @property
    def num_mels(self):
        return int(self._lib.taco_spec_num_mels(self._h))

    def num_frames(self, n_samples):
        return int(self._lib.taco_spec_num_frames(C.byref(self.hp), int(n_samples)))

    def targets(self, wav, num_samples=None, mel=True, out=None):
        """wav [B, Lmax] (numpy or tensor), num_samples [B] (a device int32 tensor is used as it is; host data is uploaded; None:
        all Lmax) -> (linear [B, Tmax, num_freq], mel [B, Tmax, num_mels] or None with mel=False, num_frames [B] int32), device
        tensors, Tmax = 1 + Lmax // hop.  Row b holds its own 1 + n_b // hop frames and exact zeros after.  out = (linear, mel,
        num_frames): contiguous device tensors of exactly those shapes that are written in place and returned (nothing is allocated
        once the workspace has its size)."""
        dev = self.device
        x = tensor(wav, dev, torch.float32, "wav", ("B", "Lmax"))
        B, L = x.shape
        ns = lengths(num_samples, dev, B, "num_samples")
        ws = workspace(self, self._lib.taco_spec_workspace_bytes(self._h, B, L))
        T = self.num_frames(L)
        if mel and not self.num_mels:
            raise _lib.TacoError(_lib.TACO_ERR_STATE, "the mel output needs a filter bank: call set_mel_basis first (or pass mel=False)")
        if out is not None:
            lin, m, nf = out
            want = [(lin, (B, T, self.hp.num_freq), torch.float32), (nf, (B,), torch.int32)] + ([(m, (B, T, self.num_mels), torch.float32)] if mel else [])
            for t, shape, dt in want:
                if not (torch.is_tensor(t) and t.is_cuda and tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous()):
                    raise Exception("out= wants contiguous %s tensors [B, Tmax, num_freq] / [B, Tmax, num_mels] / [B] on %s; expected shape %s" % (dt, dev, shape))
            m = m if mel else None
        else:
            lin = torch.empty((B, T, self.hp.num_freq), dtype=torch.float32, device=dev)
            m = torch.empty((B, T, self.num_mels), dtype=torch.float32, device=dev) if mel else None
            nf = torch.empty((B,), dtype=torch.int32, device=dev)
        call(dev, self._lib.taco_spec_targets, self._h, STREAM, x, ns, B, L, lin, m, nf, ws, ws.numel())
        return lin, m, nf

    def spectrogram(self, y):
        """The reference's spectrogram(y): one 1-D waveform -> [num_freq, T] (device tensor)."""
        return self.targets(torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).reshape(1, -1), mel=False)[0][0].t()

    def melspectrogram(self, y):
        """The reference's melspectrogram(y): one 1-D waveform -> [num_mels, T] (device tensor)."""
        return self.targets(torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).reshape(1, -1))[1][0].t()

    def process(self, wavs):
        """A list of 1-D waveforms of any lengths, as ONE batch -> a list of {"linear": [T_b, num_freq], "mel": [T_b, num_mels]},
        float32 NumPy arrays cut to each row's own frames (what generate_data.py:156-158 stores per file)."""
        wavs = [np.asarray(w, np.float32).reshape(-1) for w in wavs]
        n = np.array([len(w) for w in wavs], np.int32)
        x = np.zeros((len(wavs), int(n.max())), np.float32)
        for b, w in enumerate(wavs):
            x[b, :len(w)] = w
        lin, m, nf = self.targets(x, n)
        lin, m, nf = lin.cpu().numpy(), m.cpu().numpy(), nf.cpu().numpy()
        return [{"linear": lin[b, :nf[b]].copy(), "mel": m[b, :nf[b]].copy()} for b in range(len(wavs))]


def kaiser_window(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596):
    """The half window of resampy's sinc_window(num_zeros, precision, kaiser(beta), rolloff) in float64 (the defaults are
    'kaiser_best'): with num_table = 2**precision and n = num_table * num_zeros, half[i] = rolloff * sinc(rolloff * i / num_table) *
    kaiser(2n + 1, beta)[n + i], i = 0..n.  UNPINNED on resampy: restated from its documented algorithm, not run against it."""
    num_table = 2 ** int(precision)
    n = num_table * int(num_zeros)
    return rolloff * np.sinc(rolloff * (np.arange(n + 1) / num_table)) * np.kaiser(2 * n + 1, beta)[n:]


# resampy's named filters as arguments of kaiser_window.  kaiser_best is the reference's (librosa 0.5.1's default res_type; the
# constants are those of the issue that introduced this path).  kaiser_fast's constants are RECALLED from resampy's documentation and
# were not verified against it here.
FILTERS = {"kaiser_best": dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596),
           "kaiser_fast": dict(num_zeros=16, precision=9, beta=8.555504641634386, rolloff=0.85)}



class Resampler(Handle):
    """Recordings at orig_sr -> target_sr on the GPU, as librosa.core.resample(y, orig_sr, target_sr) with resampy's sinc interpolation
    does, but with every output at its exact position t * orig_sr / target_sr (include/taco_abi.h says where resampy 0.2.0's
    accumulated position differs).  filter: a name in FILTERS, a dict of kaiser_window's arguments, or a float64 half window (then
    num_table = entries per zero crossing is required).  UNPINNED on resampy and librosa; held by tests/resample_reference.py.
    The handle is made without a device; the filter bank is uploaded by the first `resample`."""
    _destroy = "taco_resample_destroy"

    def __init__(self, orig_sr, target_sr, filter="kaiser_best", num_table=None, device="cuda:0"):
        self.orig_sr, self.target_sr = int(orig_sr), int(target_sr)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.TacoError(_lib.TACO_ERR_ARG, "Resampler runs on a GPU (got %s); there is no CPU fallback" % device)
        if isinstance(filter, str):
            if filter not in FILTERS:
                raise _lib.TacoError(_lib.TACO_ERR_ARG, "filter must be one of %s, a dict or a half window, got %r" % (sorted(FILTERS), filter))
            filter = FILTERS[filter]
        if isinstance(filter, dict):
            half, table = kaiser_window(**filter), 2 ** int(filter.get("precision", 9))
        else:
            if num_table is None:
                raise _lib.TacoError(_lib.TACO_ERR_ARG, "a half window needs num_table, its entries per zero crossing")
            half, table = filter, num_table
        half = np.ascontiguousarray(np.asarray(half, np.float64).reshape(-1))
        self.num_table = int(table if num_table is None else num_table)
        self._lib = _lib.load_library()
        self._h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self._lib.taco_resample_create(self.orig_sr, self.target_sr, half.ctypes.data_as(C.c_void_p), len(half), self.num_table, idx,
                                                  C.byref(self._h)))

    def out_len(self, n):
        """int(ceil(n * ratio)): samples librosa.core.resample returns for n (fix_length)"""
        return int(self._lib.taco_resample_out_len(self._h, int(n)))

    def computed_len(self, n):
        """int(n * ratio): samples resampy computes; out_len(n) - computed_len(n) in {0, 1} trailing zeros follow"""
        return int(self._lib.taco_resample_computed_len(self._h, int(n)))

    @property
    def phases(self):
        return int(self._lib.taco_resample_phases(self._h))

    @property
    def taps(self):
        return int(self._lib.taco_resample_taps(self._h))

    @property
    def left_taps(self):
        return int(self._lib.taco_resample_left_taps(self._h))

    @property
    def tile(self):
        return int(self._lib.taco_resample_tile(self._h))

    def bank(self):
        """The fp32 filter bank [phases, taps] (NumPy): entry j of row r weighs x[n - (left_taps - 1) + j]."""
        b = np.empty((self.phases, self.taps), np.float32)
        _lib.check(self._lib.taco_resample_bank(self._h, b.ctypes.data_as(C.c_void_p)))
        return b

    def resample(self, wav, num_samples=None, channels=1):
        """wav [B, L] (channels = 1) or [B, L, channels] interleaved, float32 or int16 (16-bit PCM, taken as s / 32768; any other dtype
        is converted to float32); num_samples [B] (a device int32 tensor is used as it is; host data is uploaded; None: L) ->
        (out [B, out_len(L)] float32, out_samples [B] int32), device tensors.  More than one channel is averaged (librosa.to_mono).
        Row b holds its computed_len(n_b) outputs, exact zeros after, and out_samples[b] = out_len(n_b)."""
        dev = self.device
        x = tensor(wav, dev, (torch.float32, torch.int16), "wav")
        channels = int(channels)
        if x.dim() == 3 and channels == 1:
            channels = int(x.shape[2])
        if x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[2] != channels) or (x.dim() == 2 and x.shape[1] % max(channels, 1)):
            raise Exception("wav must be [B, L] or [B, L, channels = %d], got shape %s" % (channels, tuple(x.shape)))
        B, L = int(x.shape[0]), int(x.shape[1]) // (channels if x.dim() == 2 else 1)
        ns = lengths(num_samples, dev, B, "num_samples")
        L_out = self.out_len(L)
        out = torch.empty((B, L_out), dtype=torch.float32, device=dev)
        on = torch.empty((B,), dtype=torch.int32, device=dev)
        fmt = _lib.TACO_WAV_PCM16 if x.dtype == torch.int16 else _lib.TACO_WAV_F32
        call(dev, self._lib.taco_wav_resample, self._h, STREAM, x, fmt, channels, ns, B, L, out, L_out, on)
        return out, on
