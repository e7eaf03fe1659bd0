"""`Synthesizer` -- the inference driver of the reference (synthesizer.py:23-207), re-hosted.

Kept: load() / synthesize() / close() names and arguments; token -> input_lengths rule
(synthesizer.py:120); default speaker id zeros (:43-44); speaker mixtures (`speaker_ids` a dict {id: weight},
:153-164 -- a branch that never ran in the reference; its intent, the sum of weight * speaker_embed_table[id], is served by the
library's _mix entry points); the (linear_outputs, alignments) fetch pair
(:122-126,166-167); manual-attention second pass for modes 1 and 3 (:171-205; its alignments are built on the device from the
first pass's, Tacotron.run(manual_attention_mode=); mode 2 is broken in the reference: np.pow does not exist); text -> ids with the Korean normaliser (text.py, korean.py); the attention trim
(:242-262, device kernel) and, with vocode=True, the spectrogram -> waveform step on the GPU (audio.py),
followed by the silence trim of librosa_trim=True (:266-269, device kernels; without vocode there is no audio and it is a no-op).
Out of scope: plots, wav / npy file output, sentence concatenation -- `synthesize` returns the model
outputs as numpy arrays (and keeps `spec_end_idx` / `wavs` as attributes) instead."""
import glob
import os
import re

import numpy as np
import torch

from ._device import STREAM, call
from .hparams import hparams, load_hparams, EOS_ID
from .tacotron import create_model, speaker_weights
from .weights import load_weights


def get_most_recent_checkpoint(checkpoint_dir, checkpoint_step=None):
    """synthesizer.py:289-299: `model.ckpt-<step>.safetensors` packs written here, or the reference's own TensorFlow
    checkpoints (`model.ckpt-<step>.index` + `.data-*`, read by tf_checkpoint.py without TensorFlow)."""
    if checkpoint_step is None:
        paths = glob.glob(os.path.join(checkpoint_dir, "*.safetensors")) + glob.glob(os.path.join(checkpoint_dir, "model.ckpt-*.index"))
        if not paths:
            raise Exception(" [!] No checkpoint found in {}".format(checkpoint_dir))
        def step_of(p):
            m = re.search(r"ckpt-(\d+)", os.path.basename(p))
            return int(m.group(1)) if m else -1
        return max(paths, key=step_of)
    st = os.path.join(checkpoint_dir, "model.ckpt-{}.safetensors".format(checkpoint_step))
    return st if os.path.exists(st) or not os.path.exists(st[:-len("safetensors")] + "index") else st[:-len("safetensors")] + "index"


def manual_alignments_of(alignments, mode):
    """The alignments the reference feeds to its second pass (synthesizer.py:171-205) from the first pass's `alignments` [N, T_in, T_dec]:
    [N, T_dec, T_in] (the layout of the `manual_alignments` placeholder, rnn_wrappers.py:313-317).
      mode 1 ("argmax one hot", :173-179): zeros, and for every ENCODER position e a one at the decoder step where e was attended most --
             the reference takes `alignments[idx].argmax(1)`, the argmax over decoder steps, and writes `new[(argmax, range(E))] = 1`; a
             decoder step can therefore end up with no one at all, or with several.  Reproduced as it stands.
      mode 3 ("prunning", :189-195): the same ones written into a copy of the transposed alignments instead of into zeros.
      mode 2 calls np.pow, which does not exist (:181-188): the reference raises AttributeError there; so does this (as an Exception).
    Pinned on the reference's own code: tests/golden/manual_vectors.npz (tools/make_reference_vectors.py)."""
    alignments = np.asarray(alignments)
    if mode == 2:
        raise Exception("manual_attention_mode 2 is broken in the reference (np.pow, synthesizer.py:181-188)")
    alignments_T = np.transpose(alignments, [0, 2, 1])                                   # [N, D, E]
    new_alignments = np.zeros_like(alignments_T) if mode == 1 else alignments_T.copy()
    for idx in range(len(alignments)):
        argmax = alignments[idx].argmax(1)                                               # [E]: decoder step of every encoder position
        new_alignments[idx][(argmax, np.arange(len(argmax)))] = 1
    return new_alignments


class Synthesizer(object):
    # text -> ids ending in EOS (text/__init__.py:23-58): jamo tokeniser of text.py; the reference's Korean number / abbreviation
    # normaliser is not part of it -- assign a callable that includes one if the input needs it
    text_to_sequence = None

    def close(self):
        if getattr(self, "model", None) is not None:
            self.model.close()
            self.model = None

    def load(self, checkpoint_path, num_speakers=2, checkpoint_step=None, model_name='tacotron', device=None):
        self.num_speakers = num_speakers
        if os.path.isdir(checkpoint_path):
            load_path = checkpoint_path
            checkpoint_path = get_most_recent_checkpoint(checkpoint_path, checkpoint_step)
        else:
            load_path = os.path.dirname(checkpoint_path)
        self.hparams = hparams.copy()
        load_hparams(self.hparams, load_path)
        self.model = create_model(self.hparams)
        if checkpoint_path.endswith(".index") or os.path.exists(checkpoint_path + ".index"):      # a TensorFlow checkpoint of the reference
            from .tf_checkpoint import import_tf_checkpoint
            prefix = checkpoint_path[:-len(".index")] if checkpoint_path.endswith(".index") else checkpoint_path
            self.model.load_weights(import_tf_checkpoint(prefix, self.hparams, num_speakers))
        else:
            self.model.load_weights(load_weights(checkpoint_path))
        self.model.initialize(None, None, self.num_speakers, None, device=device)   # placeholders (:39-52)
        return self

    def _token_rows(self, texts, tokens):
        """texts (through the tokeniser) or ready token rows -> [N, T_in] array"""
        if type(texts) == str:
            texts = [texts]
        if texts is not None and tokens is None:
            if self.text_to_sequence is None:
                # text/__init__.py:23-58 with the korean cleaner: normalise (numbers, units, Latin letters), decompose, append EOS
                from .text import text_to_sequence as _t2s
                from .korean import KoreanNormalizer
                if getattr(self, "normalizer", None) is None:
                    self.normalizer = KoreanNormalizer()
                sequences = [_t2s(text, normalizer=self.normalizer) for text in texts]
            else:
                sequences = [self.text_to_sequence(text) for text in texts]
            if len(set(len(x) for x in sequences)) > 1:            # the reference needs equal lengths here (App. C); pad like the feeder
                from .text import pad_token_rows
                sequences = pad_token_rows(sequences)
        elif tokens is not None:
            sequences = tokens
        else:
            raise Exception("either texts or tokens is required")
        sequences = np.asarray(sequences)
        if sequences.ndim != 2:
            raise Exception("token rows must have equal length (pre-pad with 0 as eval.py / train.py:27-40 do)")
        return sequences

    def _speaker_feed(self, speaker_ids, batch):
        """`speaker_ids` -> the model's speaker feed.  A dict {id: weight} (the reference's form, synthesizer.py:153-164: one mixture
        for every row) or a list with a dict among its items (per row: an int or a dict) blends trained speakers and goes through
        speaker_weights(); anything else -- None, an all-int list, an array -- is speaker ids as before."""
        if isinstance(speaker_ids, dict) or (isinstance(speaker_ids, (list, tuple)) and any(isinstance(v, dict) for v in speaker_ids)):
            return {"speaker_weights": speaker_weights(speaker_ids, self.num_speakers, batch)}
        return {"speaker_id": speaker_ids}

    def synthesize(self, texts=None, tokens=None, base_path=None, paths=None, speaker_ids=None,
                   start_of_sentence=None, end_of_sentence=True, pre_word_num=0, post_word_num=0,
                   pre_surplus_idx=0, post_surplus_idx=1, use_short_concat=False,
                   manual_attention_mode=0, base_alignment_path=None, librosa_trim=False,
                   attention_trim=True, manual_alignments=None, vocode=False):
        sequences = self._token_rows(texts, tokens)
        input_lengths = np.argmax(sequences == EOS_ID, 1).astype(np.int32)             # synthesizer.py:120
        speaker = self._speaker_feed(speaker_ids, len(sequences))
        if manual_alignments is None and base_alignment_path is not None:               # :134-150
            alignment_path = os.path.join(base_alignment_path, os.path.basename(base_path))
            loaded = [np.load("{}.{}.npy".format(alignment_path, idx)) for idx in range(len(sequences))]
            manual_alignments = np.transpose(loaded, [0, 2, 1])
        # manual_attention_mode > 0 (:171-205): the second pass runs inside run(), its alignments built on the device from the first
        # pass's (k_manual_alignments; manual_alignments_of above is the host restatement).  Only the pass that is returned is downloaded
        linear, alignments = self.model.run(
            inputs=sequences.astype(np.int32), input_lengths=input_lengths, **speaker,
            manual_alignments=manual_alignments, is_manual_attention=manual_alignments is not None,
            manual_attention_mode=manual_attention_mode)
        linear, alignments = linear.cpu().numpy(), alignments.cpu().numpy()
        # attention_trim (:242-262): frames to keep per utterance, from the argmax walk over the alignments (device kernel)
        self.spec_end_idx = None
        if attention_trim and end_of_sentence:
            self.spec_end_idx = self.attention_trim_end(alignments, [len(seq) for seq in sequences])
        # plot_graph_and_save_audio (:264): wav = wav[:spec_end_idx]; audio_out = inv_spectrogram(wav.T) -- on the GPU, whole batch at once
        # librosa_trim (:266-269): audio_out[:index[-1]] of librosa.effects.trim(audio_out, frame_length=5120, hop_length=256, top_db=50), on
        # the GPU.  It acts on the audio, so without vocode there is nothing to cut and the flag is a no-op
        self.wavs = None
        self.trim_index = None
        if vocode:
            self.wavs = self.inv_spectrogram(linear, self.spec_end_idx, librosa_trim=librosa_trim and end_of_sentence)
        return linear, alignments

    def synthesize_audio(self, texts=None, tokens=None, speaker_ids=None, end_of_sentence=True, attention_trim=True,
                         manual_alignments=None, seed=0, iters=None, pcm=True, librosa_trim=False, vocoder="griffin_lim",
                         manual_attention_mode=0, momentum=None, return_convergence=False, rate=None, token_stretch=None, pitch=None,
                         return_durations=False, formant=None, envelope_order=None):
        """The reference's synthesize -> plot_graph_and_save_audio chain up to the samples save_audio writes (synthesizer.py:119-126,
        242-264; audio/__init__.py:22-25), everything between the token upload and the audio download on the device: the forward, the
        attention trim on the device alignments, Griffin-Lim on every utterance's own frames read from the trim kernel's output, the
        scaling to 16-bit PCM.  Returns a list of 1-D arrays, int16 (pcm) or float32, each cut to its own length; `spec_end_idx` is set
        as by `synthesize`.  Frame counts below GriffinLim.min_frames() are raised to it (include/taco_abi.h).  `seed` picks the
        initial phases (the reference draws np.random.rand).  Copies to the host: the audio buffer and two [N] int vectors.
        librosa_trim (with end_of_sentence; synthesizer.py:266-269): the silence trim librosa.effects.trim(audio_out, frame_length=5120,
        hop_length=256, top_db=50) runs on the device between Griffin-Lim and the scaling (GriffinLim.trim; UNPINNED on librosa, the
        0.5.x energy convention of the reference's pin); its `end` replaces the row's sample count for the PCM peak and for the cut
        (the reference cuts the tail only), and `trim_index` [N, 2] (start, end) is downloaded in place of the sample counts.  Off
        (the default): `trim_index` is None and nothing else changes.
        vocoder: "griffin_lim" (default) is inv_spectrogram as above.  "tensorflow" runs model.linear_outputs through
        inv_spectrogram_tensorflow (audio/__init__.py:59-61), the reference's Synthesizer.wav_output (synthesizer.py:53-54), with the
        attention trim's frame counts: deterministic, `seed` is not used.  "mel" runs model.mel_outputs -- what the decoder produced
        before the post-net -- through inv_melspectrogram (:70-72).  Both UNPINNED (include/taco_abi.h).  pcm, librosa_trim and the
        returned list behave the same for all three; any other name raises TacoError(TACO_ERR_ARG).
        manual_attention_mode 1 or 3 (synthesizer.py:171-205): the two-pass synthesis of `synthesize`, still without leaving the device
        -- forward, the second pass's alignments from the first pass's (Tacotron.manual_alignments_from), second forward -- and the trim,
        the vocoder and the PCM step then run on the second pass.  It excludes an explicit `manual_alignments` (TacoError(TACO_ERR_ARG));
        mode 2 raises as manual_alignments_of does.
        momentum: Fast Griffin-Lim in whichever vocoder runs (GriffinLim.set_momentum; not in the reference).  None keeps the
        vocoder handle's value, 0 unless an earlier call set one; a value is set and stays set.
        return_convergence: `convergence` is set to a float32 array [N], each utterance's spectral convergence || |stft(y)| - S || /
        || S || over its own frames (GriffinLim.convergence), measured on the device on the vocoder's output before any librosa_trim;
        for "griffin_lim" and "mel" -- with "tensorflow" it raises TacoError(TACO_ERR_ARG).  Off (the default): `convergence` is None.
        rate, token_stretch, pitch (prosody.py; not in the reference): how the sentence is spoken, applied to the spectrogram between the
        attention trim and the vocoder (prosody.warp_map, prosody.warp) -- to `linear` for "griffin_lim" and "tensorflow", to the mel outputs
        for "mel".  rate: a scalar or one value per row, > 1 is faster (row_stretch = float32(1 / rate)).  token_stretch: per row a sequence
        of duration multipliers, one per token (a flat sequence serves a single row); shorter rows are padded with 1; every decoder step
        takes the multiplier of the token it attends most to.  pitch: semitones, a scalar or one value per row, a scale of the bin axis
        (prosody.semitones_to_scale), so formants move with it; with vocoder="mel" it raises TacoError(TACO_ERR_ARG): the mel axis is not
        linear in frequency.  The vocoder receives the warped frame counts, kept in `warped_frames` [N]; `spec_end_idx` keeps meaning the
        trim's frame counts.  return_durations: `token_frames` [N, T_in] is set, the trimmed frames attributed to each token -- the model's
        own durations.  Values that are not finite and positive (rate, token_stretch) or finite (pitch), and sequences longer than the batch
        or the token rows, raise TacoError(TACO_ERR_ARG) before the model runs.  With all four at their defaults nothing of this runs:
        `warped_frames` and `token_frames` are None.
        formant, envelope_order (prosody.warp_formant; not in the reference): formant is in semitones, a scalar or one value per row.  With it
        given (0.0 included) the spectrogram goes through taco_spec_warp_formant in place of taco_spec_warp: every frame is split into its
        spectral envelope (the low-quefrency part of its cepstrum, envelope_order + 1 coefficients; None: prosody.default_order(sample_rate),
        2 ms) and the excitation, the envelope's bin axis is scaled by semitones_to_scale(formant) and the excitation's by
        semitones_to_scale(pitch) (None: 0 semitones).  pitch=3, formant=0 raises the pitch and keeps the voice; formant=-2 alone darkens the
        voice at the same pitch.  Without rate or token_stretch the time map is the identity.  Refused like pitch: vocoder="mel", values
        that are not finite, more values than rows; envelope_order without formant, or below 0.  With formant=None nothing of this runs."""
        from . import _lib
        if manual_attention_mode > 0 and manual_alignments is not None:
            raise _lib.TacoError(_lib.TACO_ERR_ARG, "manual_attention_mode builds the second pass's alignments itself: it cannot be "
                                 "combined with manual_alignments")
        if vocoder not in ("griffin_lim", "tensorflow", "mel"):
            raise _lib.TacoError(_lib.TACO_ERR_ARG, "vocoder must be 'griffin_lim', 'tensorflow' or 'mel', got %r" % (vocoder,))
        if return_convergence and vocoder == "tensorflow":
            raise _lib.TacoError(_lib.TACO_ERR_ARG, "return_convergence serves the librosa-flavour vocoders 'griffin_lim' and 'mel', not 'tensorflow'")
        sequences = self._token_rows(texts, tokens)
        input_lengths = np.argmax(sequences == EOS_ID, 1).astype(np.int32)             # synthesizer.py:120
        speaker = self._speaker_feed(speaker_ids, len(sequences))
        formant_scale = self._formant_args(len(sequences), formant, envelope_order, vocoder)
        stretch = self._prosody_args(len(sequences), sequences.shape[1], rate, token_stretch, pitch if formant is None or pitch is not None else 0.0, vocoder)
        linear, alignments = self.model.run(
            inputs=sequences.astype(np.int32), input_lengths=input_lengths, **speaker,
            manual_alignments=manual_alignments, is_manual_attention=manual_alignments is not None,
            manual_attention_mode=manual_attention_mode)
        frames = None
        if attention_trim and end_of_sentence:
            frames = self._attention_trim_device(alignments, [len(seq) for seq in sequences])
        trimmed = frames
        self.warped_frames = self.token_frames = None
        mel = None
        if vocoder == "mel":
            mel = self.model.mel_outputs                       # [N, steps, r * num_mels] or [N, frames, num_mels]: the same memory
            mel = mel.reshape(mel.shape[0], -1, self.hparams.num_mels)
        if stretch is not None:                                # rate / token_stretch / pitch: warp what the vocoder reads, hand it the new frame counts
            from . import prosody
            row_stretch, tok_stretch, freq_scale = stretch
            r, T = self.hparams.reduction_factor, linear.shape[1]
            if frames is None and row_stretch is None and tok_stretch is None:      # pitch / formant alone with the trim off: the batch size has to come from somewhere
                row_stretch = np.ones(len(sequences), np.float32)
            wmap = prosody.warp_map(frames, T, r, alignments if tok_stretch is not None or return_durations else None, row_stretch, tok_stretch,
                                    out_cap=prosody.out_frames_bound(T, row_stretch, tok_stretch), return_token_frames=return_durations)
            if vocoder == "mel":
                mel, frames = prosody.warp(mel, trimmed, wmap)
            elif formant_scale is not None:
                order = prosody.default_order(self.hparams.sample_rate) if envelope_order is None else int(envelope_order)
                linear, frames = prosody.warp_formant(linear, trimmed, wmap, freq_scale, formant_scale, order=min(order, linear.shape[2] - 2))
            else:
                linear, frames = prosody.warp(linear, trimmed, wmap, freq_scale)
            self.warped_frames = frames.cpu().numpy()
            tokf = wmap.token_frames
        elif return_durations:
            from . import prosody
            tokf = prosody.token_frames(alignments, frames, self.hparams.reduction_factor)
        if return_durations:
            self.token_frames = tokf.cpu().numpy()
        if vocoder == "tensorflow":
            gl = self._griffin_lim_tf()
            wav, num_samples = gl.inv_spectrogram_tensorflow(linear, frames, iters=iters, momentum=momentum)
        elif vocoder == "mel":
            gl = self._griffin_lim()
            if not gl.inv_mels:
                gl.set_inv_mel_basis()
            wav, num_samples = gl.inv_melspectrogram(mel, frames, seed=seed, iters=iters, momentum=momentum)
            sc = gl.convergence(gl.mel_to_linear(mel) ** float(gl.hp.power), wav, frames, kind="magnitude") if return_convergence else None
        else:
            gl = self._griffin_lim()
            wav, num_samples = gl.inv_spectrogram_rows(linear, frames, seed=seed, iters=iters, momentum=momentum)
            sc = gl.convergence(linear, wav, frames) if return_convergence else None
        self.convergence = sc.cpu().numpy() if return_convergence else None
        index = None
        if librosa_trim and end_of_sentence:
            index = gl.trim(wav, num_samples, **self.LIBROSA_TRIM)
            num_samples = index[:, 1].contiguous()
        audio = gl.pcm16(wav, num_samples) if pcm else wav
        self.spec_end_idx = None if trimmed is None else trimmed.cpu().numpy()
        audio = audio.cpu().numpy()
        self.trim_index = None if index is None else index.cpu().numpy()
        return [a[:n] for a, n in zip(audio, num_samples.cpu().numpy() if index is None else self.trim_index[:, 1])]

    @staticmethod
    def _prosody_args(N, T_in, rate, token_stretch, pitch, vocoder):
        """synthesize_audio's rate / token_stretch / pitch -> (row_stretch [N] or None, token_stretch [N, T_in] or None, freq_scale [N] or
        None) as float32 host arrays, or None when all three are at their defaults.  Every refusal is a TacoError(TACO_ERR_ARG)."""
        from . import _lib
        from .prosody import semitones_to_scale

        def bad(msg):
            return _lib.TacoError(_lib.TACO_ERR_ARG, msg)

        def per_row(v, what, positive):
            try:
                a = np.asarray(v, np.float64)
            except (TypeError, ValueError):
                raise bad("%s must be a number or one number per row" % what)
            if a.ndim > 1 or (a.ndim == 1 and len(a) != N):
                raise bad("%s must be a scalar or one value per row (%d), got shape %s" % (what, N, a.shape))
            if not np.isfinite(a).all() or (positive and not (a > 0).all()):
                raise bad("%s must be finite%s, got %r" % (what, " and > 0" if positive else "", v))
            return np.broadcast_to(a, (N,))

        if rate is None and token_stretch is None and pitch is None:
            return None
        if pitch is not None and vocoder == "mel":
            raise bad("pitch scales a linear frequency axis: it serves the vocoders 'griffin_lim' and 'tensorflow', not 'mel'")
        row = None if rate is None else (1.0 / per_row(rate, "rate", True)).astype(np.float32)
        scale = None if pitch is None else semitones_to_scale(per_row(pitch, "pitch", False))
        tok = None
        if token_stretch is not None:
            rows = list(token_stretch)
            if rows and np.ndim(rows[0]) == 0:                 # a flat sequence: the one row of a batch of one
                if N != 1:
                    raise bad("token_stretch must hold one sequence per row; a flat sequence serves a batch of one, this one has %d rows" % N)
                rows = [rows]
            if len(rows) > N:
                raise bad("token_stretch has %d rows, the batch has %d" % (len(rows), N))
            tok = np.ones((N, T_in), np.float32)
            for i, row_i in enumerate(rows):
                try:
                    a = np.asarray(row_i, np.float64)
                except (TypeError, ValueError):
                    raise bad("token_stretch row %d is not a sequence of numbers" % i)
                if a.ndim != 1 or len(a) > T_in:
                    raise bad("token_stretch row %d has shape %s, the token rows have %d tokens" % (i, a.shape, T_in))
                if not np.isfinite(a).all() or not (a > 0).all():
                    raise bad("token_stretch must be finite and > 0, row %d is %r" % (i, row_i))
                tok[i, :len(a)] = a
        return row, tok, scale

    @staticmethod
    def _formant_args(N, formant, envelope_order, vocoder):
        """synthesize_audio's formant / envelope_order -> formant_scale [N] float32, or None without formant.  Every refusal is a
        TacoError(TACO_ERR_ARG)."""
        from . import _lib
        from .prosody import semitones_to_scale

        def bad(msg):
            return _lib.TacoError(_lib.TACO_ERR_ARG, msg)

        if formant is None:
            if envelope_order is not None:
                raise bad("envelope_order belongs to formant: without it no envelope is formed")
            return None
        if vocoder == "mel":
            raise bad("formant scales a linear frequency axis: it serves the vocoders 'griffin_lim' and 'tensorflow', not 'mel'")
        try:
            a = np.asarray(formant, np.float64)
        except (TypeError, ValueError):
            raise bad("formant must be a number or one number per row")
        if a.ndim > 1 or (a.ndim == 1 and len(a) != N):
            raise bad("formant must be a scalar or one value per row (%d), got shape %s" % (N, a.shape))
        if not np.isfinite(a).all():
            raise bad("formant must be finite, got %r" % (formant,))
        if envelope_order is not None and (isinstance(envelope_order, bool) or not isinstance(envelope_order, (int, np.integer)) or envelope_order < 0):
            raise bad("envelope_order must be an integer >= 0, got %r" % (envelope_order,))
        return semitones_to_scale(np.broadcast_to(a, (N,)))

    LIBROSA_TRIM = dict(top_db=50, frame_length=5120, hop_length=256)      # synthesizer.py:267-268

    def _griffin_lim(self):
        from .audio import GriffinLim
        if getattr(self, "_gl", None) is None:
            self._gl = GriffinLim(self.hparams, device=str(self.model.device))
        return self._gl

    def _griffin_lim_tf(self):
        from .audio import GriffinLim
        if getattr(self, "_gl_tf", None) is None:
            self._gl_tf = GriffinLim(self.hparams, device=str(self.model.device), flavor="tensorflow")
        return self._gl_tf

    def inv_spectrogram(self, linear, spec_end_idx=None, librosa_trim=False):
        """audio/__init__.py:54-56 for a batch [N, T, num_freq]; returns a list of 1-D float32 arrays (each cut to the samples its
        own frames produce when spec_end_idx is given: Griffin-Lim runs on the padded batch, frames past the end are silence-level).
        librosa_trim: each row is then cut to the `end` of GriffinLim.trim on those samples (synthesizer.py:266-269) and
        `trim_index` [N, 2] is set."""
        self._griffin_lim()
        x = np.array(linear, np.float32, copy=True)
        if spec_end_idx is not None:
            for i, e in enumerate(spec_end_idx):
                x[i, int(e):] = 0.0                       # normalised 0 = min_level_db: the reference would not have synthesised these frames
        dwav = self._gl.inv_spectrogram(x)
        wav = dwav.cpu().numpy()
        hop = self._gl.num_samples(2)
        ends = [wav.shape[1]] * len(wav) if spec_end_idx is None else [hop * max(int(e) - 1, 1) for e in spec_end_idx]
        if librosa_trim:
            self.trim_index = self._gl.trim(dwav, np.asarray(ends, np.int32), **self.LIBROSA_TRIM).cpu().numpy()
            ends = self.trim_index[:, 1]
        if spec_end_idx is None and not librosa_trim:
            return [w for w in wav]
        return [w[:int(e)] for w, e in zip(wav, ends)]

    def attention_trim_end(self, alignments, sequence_lengths):
        """spec_end_idx = reduction_factor * j + 3 per utterance (synthesizer.py:242-262); alignments [N, T_in, T_dec]."""
        return self._attention_trim_device(alignments, sequence_lengths).cpu().numpy()

    def _attention_trim_device(self, alignments, sequence_lengths):
        m = self.model
        al = m._as_dev(alignments, torch.float32)
        sl = m._as_dev(np.asarray(sequence_lengths, np.int32), torch.int32)
        N, T_in, n = al.shape
        out = torch.zeros((N,), dtype=torch.int32, device=al.device)
        call(al.device, m._lib.taco_attention_trim, STREAM, al, sl, N, T_in, n, self.hparams.reduction_factor, out)
        return out
