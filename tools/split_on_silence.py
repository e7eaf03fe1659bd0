#!/usr/bin/env python
"""Long recordings -> utterance-sized segments: what the reference's audio/silence.py:33-76 (split_on_silence_with_librosa) writes per
recording -- NAME.no_breath and NAME.0000, NAME.0001, ... -- with both splits and remove_breath computed on the GPU
(taco_amd.split_on_silence) instead of librosa on the CPU.  Recordings are `.npy` files of float samples at hparams.sample_rate -- or,
with --orig-sr N, at N Hz (float, or int16 PCM; [n] or [n, channels]): each is then resampled to hparams.sample_rate on the device
first (taco_amd.Resampler, what librosa.core.load does on the CPU); decoding wav / mp3 files stays outside.  The segments are waveforms
tools/generate_data.py takes as they are.

--method pydub runs the reference's other method instead, the one its README and scripts/prepare_*.sh use (audio/silence.py:81-117,
taco_amd.silence.split_on_silence_pydub): recordings are then `.npy` files of int16 PCM, [n] or [n, channels] interleaved, at
--sample-rate, and only OUT_DIR/NAME.%04d.npy (int16) are written -- that method has no NAME.no_breath.  Without --method the tool does
what it always did.

    python tools/split_on_silence.py OUT_DIR a.npy b.npy ... [--top-db 40] [--frame-length 1024] [--hop-length 256] [--skip-idx 0]
                                     [--min-segment-length 3] [--max-segment-length 8] [--pre-silence-length 0] [--post-silence-length 0]
                                     [--orig-sr N]
    python tools/split_on_silence.py OUT_DIR a.npy b.npy ... --method pydub --sample-rate 44100 [--skip-idx 0] [--silence-thresh -40]
                                     [--min-silence-len 400] [--silence-chunk-len 100] [--keep-silence 100] [--include-last-range]

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


def split_files_pydub(recordings, out_dir, sample_rate, names=None, device=None, **kw):
    """recordings: list of int16 arrays ([n] or [n, channels]) or `.npy` paths.  Returns, per recording, its segment paths; names as split_files."""
    import taco_amd
    if names is None:
        names = [os.path.basename(r).rsplit(".", 1)[0] if isinstance(r, str) else "%06d" % i for i, r in enumerate(recordings)]
    dup = sorted(set(nm for nm in names if names.count(nm) > 1))
    if dup:
        raise Exception("output names are not unique (pass names=): %s" % ", ".join(dup))
    dev = device or taco_amd.silence.PcmDevice()
    os.makedirs(out_dir, exist_ok=True)
    out = []
    for r, nm in zip(recordings, names):
        audio = np.load(r) if isinstance(r, str) else np.asarray(r)
        paths = []
        for idx, start, end, segment in taco_amd.silence.split_on_silence_pydub(audio, sample_rate, device=dev, **kw):
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
    ap.add_argument("--method", choices=["librosa", "pydub"], default="librosa")
    ap.add_argument("--sample-rate", type=int, default=None, help="pydub: the rate of the int16 inputs (required)")
    ap.add_argument("--silence-thresh", type=float, default=-40, help="pydub: dBFS")
    ap.add_argument("--min-silence-len", type=int, default=400, help="pydub: ms between two utterances")
    ap.add_argument("--silence-chunk-len", type=int, default=100, help="pydub: ms, the window of detect_nonsilent")
    ap.add_argument("--keep-silence", type=int, default=100, help="pydub: ms kept on both sides of an utterance")
    ap.add_argument("--include-last-range", action="store_true", help="pydub: keep the last utterance, which the reference's loop drops")
    a = ap.parse_args()
    if a.method == "pydub":
        if a.sample_rate is None:
            ap.error("--method pydub needs --sample-rate")
        for paths in split_files_pydub(a.recordings, a.out_dir, a.sample_rate, skip_idx=a.skip_idx, silence_thresh=a.silence_thresh,
                                       min_silence_len=a.min_silence_len, silence_chunk_len=a.silence_chunk_len, keep_silence=a.keep_silence,
                                       include_last_range=a.include_last_range):
            for p in paths:
                print(p)
        return
    kw = dict(top_db=a.top_db, frame_length=a.frame_length, hop_length=a.hop_length, skip_idx=a.skip_idx, min_segment_length=a.min_segment_length,
              max_segment_length=a.max_segment_length, pre_silence_length=a.pre_silence_length, post_silence_length=a.post_silence_length)
    if a.orig_sr is not None:
        kw["orig_sr"] = a.orig_sr
    for paths in split_files(a.recordings, a.out_dir, **kw):
        for p in paths:
            print(p)


if __name__ == "__main__":
    main()
