#!/usr/bin/env python
"""Records what the reference's own allocation script writes, for tests/test_egs_cpu.py -> tests/golden/egs_alloc.npz.

Runs the reference's UNMODIFIED ``local/tf/create_egs.py`` (checkout named by ``XV_REFERENCE_DIR``, default /root/reference) as a
subprocess on a generated toy table and stores the input tables and the bytes of every file it wrote, for three configurations:

  a  --num-repeats=20 --num-jobs=2 --minibatch-size=4 --min/max-frames-per-chunk=20/40 --frames-per-iter=1000 --num-archives=3
  b  the same with --num-repeats=2                  (takes the "Ran out of speakers" branch)
  c  a with --prefix=valid --randomize-chunk-length=false --num-jobs=1 --num-archives=2

The table: 6 speakers with 3-5 base utterances each plus their -reverb / -noise copies, 28-120 frames, so some utterances are
shorter than the longest chunk (the redraw branch) and copies share their offset lists with the clean utterance.

Layout of the npz (data only, no pickles): ``utt2len`` / ``utt2int`` = the two input files as uint8; per configuration X in a, b, c:
``X_args`` (the flags, a unicode array), ``X_names`` (paths relative to the egs dir, a unicode array), ``X_<i>`` (uint8 bytes of
``X_names[i]``), ``X_stdout_retries`` (how often the reference printed "is smaller than segment length").
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = {
    "a": ["--num-repeats=20", "--num-jobs=2", "--minibatch-size=4", "--min-frames-per-chunk=20", "--max-frames-per-chunk=40",
          "--frames-per-iter=1000", "--num-archives=3"],
    "b": ["--num-repeats=2", "--num-jobs=2", "--minibatch-size=4", "--min-frames-per-chunk=20", "--max-frames-per-chunk=40",
          "--frames-per-iter=1000", "--num-archives=3"],
    "c": ["--prefix=valid", "--randomize-chunk-length=false", "--num-repeats=20", "--num-jobs=1", "--minibatch-size=4",
          "--min-frames-per-chunk=20", "--max-frames-per-chunk=40", "--frames-per-iter=1000", "--num-archives=2"],
}


def toy_table(seed=7):
    rng = np.random.default_rng(seed)
    utt2len, utt2int = [], []
    for spk in range(6):
        for j in range(int(rng.integers(3, 6))):
            base = "spk%d_utt%d" % (spk, j)
            for name in (base, base + "-reverb", base + "-noise"):
                utt2len.append((name, int(rng.integers(28, 121))))
                utt2int.append((name, spk))
    return utt2len, utt2int


def main():
    ref = os.environ.get("XV_REFERENCE_DIR", "/root/reference")
    script = os.path.join(ref, "local", "tf", "create_egs.py")
    utt2len, utt2int = toy_table()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        p_len, p_int = os.path.join(tmp, "utt2len"), os.path.join(tmp, "utt2int")
        open(p_len, "w").write("".join("%s %d\n" % e for e in utt2len))
        open(p_int, "w").write("".join("%s %d\n" % e for e in utt2int))
        out["utt2len"] = np.frombuffer(open(p_len, "rb").read(), np.uint8)
        out["utt2int"] = np.frombuffer(open(p_int, "rb").read(), np.uint8)
        for tag, flags in CONFIGS.items():
            egs = os.path.join(tmp, "egs_" + tag)
            os.makedirs(egs)
            res = subprocess.run([sys.executable, script] + flags + ["--utt2len-filename=" + p_len, "--utt2int-filename=" + p_int,
                                                                      "--egs-dir=" + egs], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                 check=True, timeout=120)
            names = sorted(os.path.relpath(os.path.join(d, f), egs) for d, _, fs in os.walk(egs) for f in fs)
            out[tag + "_args"] = np.array(flags)
            out[tag + "_names"] = np.array(names)
            for i, n in enumerate(names):
                out["%s_%d" % (tag, i)] = np.frombuffer(open(os.path.join(egs, n), "rb").read(), np.uint8)
            text = res.stdout.decode()
            out[tag + "_stdout_retries"] = np.array(text.count("is smaller than segment length"))
            counts = open(os.path.join(egs, "temp", ("valid_" if tag == "c" else "") + "archive_minibatch_count")).read().split("\n")
            print("%s: %d files, minibatch counts %s, %d short-utterance redraws, ran out of speakers %d times" % (
                tag, len(names), [c.split()[1] for c in counts if c], int(out[tag + "_stdout_retries"]), text.count("Ran out of speakers")))
    np.savez_compressed(os.path.join(HERE, "egs_alloc.npz"), **out)
    print("wrote", os.path.join(HERE, "egs_alloc.npz"), os.path.getsize(os.path.join(HERE, "egs_alloc.npz")), "bytes")


if __name__ == "__main__":
    main()
