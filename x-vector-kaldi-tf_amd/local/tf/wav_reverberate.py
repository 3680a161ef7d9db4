#!/usr/bin/env python
"""Kaldi's wav-reverberate on the MI355X, for inspection: the same command line, a 16-bit PCM WAV out.

  wav_reverberate.py [--shift-output=true] [--impulse-response=RX] [--additive-signals=RX,RX --snrs=S,S --start-times=T,T]
                     [--volume=V] [--duration=D] [--normalize-output=false] [--input-wave-channel=C] [--rir-channel=C]
                     [--noise-channel=C] <in-rxfilename> <out-wxfilename|->

The semantics are DESIGN.md §8.7's (xvector_amd/augment.py); rxfilenames are paths, ``-`` or ``cmd |`` pipes, and a nested
``wav-reverberate ... - |`` in any of them is evaluated in-process too.  wav.scp entries need no call to this: compute-mfcc-feats
(mfcc_vad.py) evaluates them itself.
"""
from __future__ import print_function

import logging
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))

from xvector_amd import augment, mfcc  # noqa: E402

logging.getLogger("augment").addHandler(logging.StreamHandler())


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__.split("\n\n")[1], file=sys.stderr)
        return 1
    pos = [i for i, a in enumerate(argv) if not a.startswith("--")]
    if len(pos) != 2:
        print("wav_reverberate.py: expected <in-rxfilename> <out-wxfilename>", file=sys.stderr)
        return 1
    out = argv[pos[1]]
    try:
        node = augment.parse_argv(argv[:pos[1]] + ["-"] + argv[pos[1] + 1:])
        waves, _, plan = augment.Augmenter().evaluate([("wav-reverberate", node)])
    except augment.AugmentError as e:
        print("wav_reverberate.py: %s" % e, file=sys.stderr)
        return 1
    data = mfcc.wav_bytes(waves[0], plan.top[0].rate)
    if out == "-":
        sys.stdout.buffer.write(data)
        sys.stdout.buffer.flush()
    else:
        with open(out, "wb") as f:
            f.write(data)
    return 0


if __name__ == "__main__":
    sys.exit(main())
