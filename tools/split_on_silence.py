#!/usr/bin/env python
"""Long recordings -> utterance-sized segments: what the reference's audio/silence.py:33-76 (split_on_silence_with_librosa) writes per
recording -- NAME.no_breath and NAME.0000, NAME.0001, ... -- with both splits and remove_breath computed on the GPU
(taco_amd.split_on_silence) instead of librosa on the CPU.  Recordings are `.npy` files of float samples at hparams.sample_rate -- or,
with --orig-sr N, at N Hz (float, or int16 PCM; [n] or [n, channels]): each is then resampled to hparams.sample_rate on the device
first (taco_amd.Resampler, what librosa.core.load does on the CPU); decoding wav / mp3 files stays outside, and so does the pydub method.  The segments are waveforms
tools/generate_data.py takes as they are.

    python tools/split_on_silence.py OUT_DIR a.npy b.npy ... [--top-db 40] [--frame-length 1024] [--hop-length 256] [--skip-idx 0]
                                     [--min-segment-length 3] [--max-segment-length 8] [--pre-silence-length 0] [--post-silence-length 0]
                                     [--orig-sr N]

Writes OUT_DIR/NAME.no_breath.npy and OUT_DIR/NAME.%04d.npy (float32; the number is the segment's position among the intervals of the
second split, as in the reference: segments outside the duration bounds leave gaps in the numbering) and prints the paths."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def split_files(recordings, out_dir, names=None, hparams=None, device=None, **kw):
    """recordings: list of 1-D arrays or `.npy` paths.  Returns, per recording, [no_breath path, segment paths ...]; two recordings that
    would get the same name are refused, nothing is written."""
    import taco_amd
    hp = hparams or taco_amd.hparams
    if names is None:
        names = [os.path.basename(r).rsplit(".", 1)[0] if isinstance(r, str) else "%06d" % i for i, r in enumerate(recordings)]
    dup = sorted(set(nm for nm in names if names.count(nm) > 1))
    if dup:
        raise Exception("output names are not unique (pass names=): %s" % ", ".join(dup))
    dev = device or taco_amd.silence.SilenceDevice(hp)
    os.makedirs(out_dir, exist_ok=True)
    out = []
    for r, nm in zip(recordings, names):
        audio = np.load(r) if isinstance(r, str) else np.asarray(r)
        no_breath, segments = taco_amd.split_on_silence(audio, hp, device=dev, **kw)
        paths = [os.path.join(out_dir, nm + ".no_breath.npy")]
        np.save(paths[0], no_breath)
        for idx, start, end, segment in segments:
            paths.append(os.path.join(out_dir, "%s.%04d.npy" % (nm, idx)))
            np.save(paths[-1], segment)
        out.append(paths)
    if device is None:
        dev.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out_dir")
    ap.add_argument("recordings", nargs="+", help=".npy waveform files")
    ap.add_argument("--top-db", type=float, default=40)
    ap.add_argument("--frame-length", type=int, default=1024)
    ap.add_argument("--hop-length", type=int, default=256)
    ap.add_argument("--skip-idx", type=int, default=0)
    ap.add_argument("--min-segment-length", type=float, default=3)
    ap.add_argument("--max-segment-length", type=float, default=8)
    ap.add_argument("--pre-silence-length", type=float, default=0)
    ap.add_argument("--post-silence-length", type=float, default=0)
    ap.add_argument("--orig-sr", type=int, default=None, help="sample rate of the inputs; they are resampled to hparams.sample_rate on the device")
    a = ap.parse_args()
    kw = dict(top_db=a.top_db, frame_length=a.frame_length, hop_length=a.hop_length, skip_idx=a.skip_idx, min_segment_length=a.min_segment_length,
              max_segment_length=a.max_segment_length, pre_silence_length=a.pre_silence_length, post_silence_length=a.post_silence_length)
    if a.orig_sr is not None:
        kw["orig_sr"] = a.orig_sr
    for paths in split_files(a.recordings, a.out_dir, **kw):
        for p in paths:
            print(p)


if __name__ == "__main__":
    main()
