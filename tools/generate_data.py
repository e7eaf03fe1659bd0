#!/usr/bin/env python
"""Waveforms -> the `.npz` training examples that feeder.NpzSource replays: what the reference's datasets/generate_data.py:144-161
(_process_utterance) writes per corpus file -- "linear" [T, num_freq], "mel" [T, num_mels] (float32, spectrogram(wav).T and
melspectrogram(wav).T), "tokens", "loss_coeff" -- with the two spectrograms computed on the GPU (taco_amd.Spectrogram) instead of
librosa on the CPU.  Waveforms are in-memory arrays or `.npy` files of float samples at hparams.sample_rate -- or, with --orig-sr N,
at N Hz (float, or int16 PCM; [n] or [n, channels]): each is then resampled to hparams.sample_rate on the device first
(taco_amd.Resampler, what librosa.core.load does on the CPU); decoding audio files stays outside.  Utterances are sorted by length and analysed `batch` at a time, so a batch's rows are padded to a
neighbour's length, not the corpus maximum.

    python tools/generate_data.py OUT_DIR a.npy b.npy ... [--tokens tokens.npy ...] [--loss-coeff 1.0] [--batch 32] [--orig-sr N]

(--tokens: one `.npy` of token ids per waveform, in order; without it an empty token array is stored)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def resample_all(data, orig_sr, hparams, device="cuda:0"):
    """Recordings at orig_sr ([n] or [n, channels]; int16 is 16-bit PCM) -> float32 [n'] NumPy arrays at hparams.sample_rate, one device
    call per recording (rows of one call share a dtype and a channel count; recordings need not)."""
    import taco_amd
    rs = taco_amd.Resampler(orig_sr, int(getattr(hparams, "sample_rate", 24000)), device=device)
    out = []
    for a in data:
        a = np.asarray(a)
        a = np.ascontiguousarray(a if a.dtype == np.int16 else a.astype(np.float32))
        y, n = rs.resample(a.reshape((1,) + a.shape), channels=a.shape[1] if a.ndim == 2 else 1)
        out.append(y[0, :int(n[0])].cpu().numpy())
    rs.close()
    return out


def generate(wavs, tokens, loss_coeff, out_dir, names=None, hparams=None, batch=32, spectrogram=None, orig_sr=None):
    """wavs: list of 1-D arrays or `.npy` paths; tokens: list of int arrays; loss_coeff: a number or one per utterance.
    Writes OUT_DIR/<name>.npz (names default to the `.npy` base names, or 000000, 000001, ...; two utterances that would get the same
    name are refused, nothing is written) and returns the paths in input order."""
    import taco_amd
    hp = hparams or taco_amd.hparams
    sp = spectrogram or taco_amd.Spectrogram(hp)
    n = len(wavs)
    if len(tokens) != n:
        raise Exception("%d waveforms but %d token arrays" % (n, len(tokens)))
    coeff = list(loss_coeff) if np.ndim(loss_coeff) else [loss_coeff] * n
    if names is None:
        names = [os.path.basename(w).rsplit(".", 1)[0] if isinstance(w, str) else "%06d" % i for i, w in enumerate(wavs)]
    dup = sorted(set(nm for nm in names if names.count(nm) > 1))
    if dup:
        raise Exception("output names are not unique (pass names=): %s" % ", ".join(dup))
    data = [np.load(w) if isinstance(w, str) else np.asarray(w) for w in wavs]
    if orig_sr is not None:
        data = resample_all(data, orig_sr, hp, sp.device)
    os.makedirs(out_dir, exist_ok=True)
    paths = [os.path.join(out_dir, nm + ".npz") for nm in names]
    order = sorted(range(n), key=lambda i: len(data[i]))
    for s in range(0, n, batch):
        idx = order[s:s + batch]
        for i, r in zip(idx, sp.process([data[i] for i in idx])):
            np.savez(paths[i], linear=r["linear"], mel=r["mel"], tokens=np.asarray(tokens[i]), loss_coeff=coeff[i])
    if spectrogram is None:
        sp.close()
    return paths


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out_dir")
    ap.add_argument("wavs", nargs="+", help=".npy waveform files")
    ap.add_argument("--tokens", nargs="*", default=None, help=".npy token files, one per waveform")
    ap.add_argument("--loss-coeff", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--orig-sr", type=int, default=None, help="sample rate of the inputs; they are resampled to hparams.sample_rate on the device")
    a = ap.parse_args()
    tokens = [np.load(t) for t in a.tokens] if a.tokens else [np.zeros((0,), np.int32)] * len(a.wavs)
    for p in generate(a.wavs, tokens, a.loss_coeff, a.out_dir, batch=a.batch, orig_sr=a.orig_sr):
        print(p)


if __name__ == "__main__":
    main()
