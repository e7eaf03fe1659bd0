#!/usr/bin/env python
"""recognition.json -> alignment.json: every recognised utterance matched to a line of its speaker's script, what the reference's
recognition/alignment.py does, with the scores computed on the GPU (taco_amd.alignment.align_text_batch: taco_text_matches and
taco_text_best_two).  The command line is the reference's:

    python tools/align_text.py --recognition_path datasets/NAME/recognition.json [--alignment_filename alignment.json] [--score_threshold 0.4]
                               [--dictionaries FILE.json]

recognition.json maps audio paths (.../audio/SCRIPT.NNNN.wav) to recognised texts.  The lines of a script are read from
.../assets/SCRIPT.txt, the `assets` directory next to `audio`: at the path the audio path gives, or, where that does not exist from the
current directory, in `assets` beside recognition.json.  alignment.json is written beside recognition.json (sorted keys, indent 4, UTF-8 as
it is); an existing one is renamed to NAME.backup_TIME.json first.  The two summary lines of the reference are printed; its report of the
audio durations, which needs the audio files, is not.  --dictionaries: the Korean normaliser's word lists (korean.load_dictionaries), used only
to count symbols where no part of a script line could be cut out."""
import argparse
import json
import os
import re
import sys
from datetime import datetime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_recognition(path):
    """the JSON mapping; a comma before a closing brace or bracket is tolerated, as the reference's loader tolerates it"""
    with open(path, encoding="utf-8") as f:
        content = f.read()
    return json.loads(re.sub(r",\s*([}\]])", r"\1", content))


def read_scripts(recognition, base_dir):
    from taco_amd.alignment import script_of
    scripts = {}
    for audio_path in recognition:
        path, name = script_of(audio_path)
        if name in scripts:
            continue
        if not os.path.exists(path):
            path = os.path.join(base_dir, "assets", name + ".txt")
        with open(path, encoding="utf-8") as f:
            scripts[name] = f.readlines()
    return scripts


def align_file(recognition_path, alignment_filename="alignment.json", score_threshold=0.4, normalizer=None, device=None):
    """-> (path of the alignment file written, the results)"""
    from taco_amd.alignment import align_text_batch
    recognition = load_recognition(recognition_path)
    base_dir = os.path.dirname(recognition_path)
    results = align_text_batch(recognition, read_scripts(recognition, base_dir), score_threshold, normalizer=normalizer, device=device)
    exact = sum(isinstance(v, str) for v in results.values())
    n = max(len(recognition), 1)
    print(" [*] # found: {:.5f}% ({}/{})".format(len(results) / n, len(results), len(recognition)))
    print(" [*] # exact match: {:.5f}% ({}/{})".format(exact / n, exact, len(recognition)))
    out = os.path.join(base_dir, alignment_filename)
    if os.path.exists(out):
        root, ext = os.path.splitext(out)
        backup = "{}.backup_{}{}".format(root, datetime.now().strftime("%Y-%m-%d_%H-%M-%S"), ext)
        os.rename(out, backup)
        print(" [*] {} has backup: {}".format(out, backup))
    with open(out, "w", encoding="utf-8") as f:
        json.dump(results, f, indent=4, sort_keys=True, ensure_ascii=False)
    return out, results


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--recognition_path", required=True)
    ap.add_argument("--alignment_filename", default="alignment.json")
    ap.add_argument("--score_threshold", default=0.4, type=float)
    ap.add_argument("--dictionaries", default=None, help="JSON of the Korean normaliser's word lists")
    a, _ = ap.parse_known_args(argv)
    normalizer = None
    if a.dictionaries:
        from taco_amd.korean import load_dictionaries
        normalizer = load_dictionaries(a.dictionaries)
    align_file(a.recognition_path, a.alignment_filename, a.score_threshold, normalizer)


if __name__ == "__main__":
    main()
