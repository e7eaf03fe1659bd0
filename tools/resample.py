#!/usr/bin/env python
"""Recordings at another sample rate -> `.npy` waveforms at the model's: what the reference's load_audio (audio/__init__.py:12-20:
librosa.core.load(path, sr=hparams.sample_rate)) does after decoding -- the mean over channels and resampy's band-limited sinc
interpolation -- on the GPU (taco_amd.Resampler).  Inputs are `.npy` files ([n] or [n, channels]; float, or int16 taken as 16-bit
PCM) or uncompressed `.wav` files, read with the standard library's `wave` module: 16-bit PCM only, anything else is refused;
decoding compressed audio stays outside.  16-bit interleaved multi-channel samples go to the kernel as they are.

    python tools/resample.py OUT_DIR --orig-sr N [--target-sr M] [--filter kaiser_best] a.npy b.wav ...

Writes OUT_DIR/NAME.npy (float32 at --target-sr, default hparams.sample_rate) and prints the paths.  A `.wav` file whose own rate is
not --orig-sr is refused."""
import argparse
import os
import sys
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def read_wav(path, orig_sr=None):
    """-> int16 [n, channels]"""
    with wave.open(path, "rb") as w:
        if w.getcomptype() != "NONE" or w.getsampwidth() != 2:
            raise Exception("%s: only uncompressed 16-bit PCM is read here (sample width %d bytes, compression %s)" % (path, w.getsampwidth(), w.getcomptype()))
        if orig_sr is not None and w.getframerate() != orig_sr:
            raise Exception("%s is at %d Hz, not --orig-sr %d" % (path, w.getframerate(), orig_sr))
        ch = w.getnchannels()
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16).reshape(-1, ch)


def resample_files(recordings, out_dir, orig_sr, target_sr=None, filter="kaiser_best", names=None, device="cuda:0"):
    """recordings: list of arrays, `.npy` or `.wav` paths.  Returns the paths written, in input order; two recordings that would get the
    same name are refused, nothing is written."""
    import taco_amd
    target_sr = int(target_sr or taco_amd.hparams.sample_rate)
    if names is None:
        names = [os.path.basename(r).rsplit(".", 1)[0] if isinstance(r, str) else "%06d" % i for i, r in enumerate(recordings)]
    dup = sorted(set(nm for nm in names if names.count(nm) > 1))
    if dup:
        raise Exception("output names are not unique (pass names=): %s" % ", ".join(dup))
    data = []
    for r in recordings:
        a = (read_wav(r, orig_sr) if r.lower().endswith(".wav") else np.load(r)) if isinstance(r, str) else np.asarray(r)
        if a.ndim not in (1, 2):
            raise Exception("a recording is [n] or [n, channels], got shape %s" % (a.shape,))
        data.append(np.ascontiguousarray(a if a.dtype == np.int16 else a.astype(np.float32)))
    rs = taco_amd.Resampler(orig_sr, target_sr, filter=filter, device=device)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for a, nm in zip(data, names):
        y, n = rs.resample(a.reshape((1,) + a.shape), channels=a.shape[1] if a.ndim == 2 else 1)
        paths.append(os.path.join(out_dir, nm + ".npy"))
        np.save(paths[-1], y[0, :int(n[0])].cpu().numpy())
    rs.close()
    return paths


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out_dir")
    ap.add_argument("recordings", nargs="+", help=".npy or 16-bit PCM .wav files")
    ap.add_argument("--orig-sr", type=int, required=True)
    ap.add_argument("--target-sr", type=int, default=None)
    ap.add_argument("--filter", default="kaiser_best")
    a = ap.parse_args()
    for p in resample_files(a.recordings, a.out_dir, a.orig_sr, a.target_sr, a.filter):
        print(p)


if __name__ == "__main__":
    main()
