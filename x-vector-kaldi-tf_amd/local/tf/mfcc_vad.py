#!/usr/bin/env python
"""Stage 1 of run.sh without Kaldi binaries.  Each subcommand is named after the binary it replaces:

  compute-mfcc-feats [--config F] [--name=value ...] [--write-num-frames ark,t:F] scp:wav.scp <wspec>
  compute-vad        [--config F] [--name=value ...] <feats-rspec> <wspec>
  compute-mfcc-vad   [--config F] [--vad-config F] [--name=value ...] [--write-num-frames ark,t:F] scp:wav.scp <feats-wspec>
                     <vad-wspec>       (both in one pass: the VAD reads the features on the device, nothing is re-read)
  wav-to-duration    [--read-entire-file] scp:wav.scp ark,t:utt2dur
  copy-feats         [--compress[=true|false]] <feats-rspec> <wspec>     (FM, DM and CM* tables in; plain or compressed out)
  vad-to-segments    [--max-gap 30] [--min-segment-length 50] [--pad 10] [--max-segment-length 1000] [--frame-shift 10]
                     <vad-rspec> segments      (diarization/vad_to_segments.sh: a Kaldi segments file from VAD decisions, on the
                     host; lengths in frames, --frame-shift in milliseconds; the rule of DESIGN.md §8.18)

Options carry Kaldi's names and defaults (xvector_amd/mfcc.py); a ``--config`` file is read first, the command line
overrides it.  ``--seed`` keys the dither noise with the utterance id.  Outputs are ``ark,scp:A,S`` or
``ark:A``; features are written as ``FM`` records, VAD decisions as ``FV`` records, ``--write-num-frames`` as ``key N`` lines.
``--compress[=true|false]`` (compute-mfcc-feats, compute-mfcc-vad, copy-feats; default false, as in the binaries -- Kaldi's
steps/make_mfcc.sh passes true) writes features as Kaldi CompressedMatrix records instead (``CM``, or ``CM2`` for matrices of up
to 8 rows), encoded on the GPU (xvector_amd/compress.py); a matrix without rows stays an ``FM`` record.
wav.scp entries are paths or ``cmd |`` pipes; 16-bit PCM WAV only.  A pipe that is exactly ``sph2pipe -f wav [-p] [-c 1|2]
x.sph |`` (what the recipe's data-preparation scripts write) is read in-process and, for the feature commands, decoded on the
GPU: no sph2pipe process is started (xvector_amd/sphere.py; mu-law, A-law and 16-bit PCM files of one or two
channels; anything else, and everything under ``XVECTOR_NATIVE_SPH=0``, runs in the shell as before).  A pipe whose last stage is
``wav-reverberate`` (what
Kaldi's reverberate_data_dir.py / augment_data_dir.py write) is evaluated in-process on the GPU (xvector_amd/augment.py,
DESIGN.md §8.7); no wav-reverberate process is started.  ``--allow-downsample`` / ``--allow-upsample`` (compute-mfcc-feats,
compute-mfcc-vad; also through ``--config``) take a wave whose rate differs from ``--sample-frequency`` as it is and resample it
on the GPU (xvector_amd/resample.py); frame counts are those of the resampled wave.  Without them such a wave
is skipped with a warning, and an augmented entry at another rate is skipped either way (the augmenter's output is not
resampled).  The arithmetic runs on the MI355X: no CPU fallback.
"""
from __future__ import print_function

import argparse
import logging
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))

import kaldi_io  # noqa: E402
from xvector_amd import augment, compress, mfcc, sphere  # noqa: E402

logger = logging.getLogger('mfcc_vad')
logger.addHandler(logging.StreamHandler())
logger.setLevel(logging.INFO)
logging.getLogger('mfcc').addHandler(logging.StreamHandler())
logging.getLogger('augment').addHandler(logging.StreamHandler())

WINDOW_SAMPLES = 1 << 26          # samples per launch (128 MiB of int16; coded SPHERE entries add a side buffer of their
                                  # files' bytes, at most 4 per sample: both channels of 16-bit PCM)


def _flags(p, cls):
    for name in cls.names():
        p.add_argument("--" + name.replace("_", "-"), dest="opt_" + name, nargs="?", const="true", default=None)


def _options(cls, config, args):
    o = cls()
    if config:
        o.update(mfcc.read_config(config))
    o.update((n, getattr(args, "opt_" + n)) for n in cls.names() if getattr(args, "opt_" + n, None) is not None)
    return o


class _Out(object):
    """A table wspecifier: ``ark,scp:A,S`` (TableWriter) or ``ark[,b]:A``."""

    def __init__(self, wspec):
        kind, _, path = wspec.partition(":")
        opts = kind.split(",")
        if not path or opts[0] != "ark" or any(o not in ("ark", "scp", "b", "t", "f", "nf", "p", "np") for o in opts):
            raise SystemExit("unsupported wspecifier %r (ark,scp:A,S or ark:A)" % wspec)
        if "scp" in opts:
            ark, _, scp = path.partition(",")
            if not scp:
                raise SystemExit("wspecifier %r: ark,scp needs A,S" % wspec)
            self.fd = kaldi_io.TableWriter(ark, scp)
        else:
            self.fd = open(path, "wb")

    def close(self):
        self.fd.close()


class _NumFrames(object):
    def __init__(self, wspec):
        path = wspec.split(":", 1)[1] if ":" in wspec else wspec
        self.f = open(path, "wt")

    def write(self, key, n):
        self.f.write("%s %d\n" % (key, n))

    def close(self):
        self.f.close()


def _compress_flag(p):
    p.add_argument("--compress", default="false",
                   help="write features as Kaldi CompressedMatrix records (default false, as in the Kaldi binary)")


def _want_compress(args):
    return mfcc._convert("compress", bool, args.compress)


def _write_feats(fd, f, key):
    """One feature matrix: a compress.Packed as a CM / CM2 record, an array (also the empty one of a compressed run) as FM / DM."""
    if isinstance(f, compress.Packed):
        kaldi_io.write_cm_payload(fd, f.payload, f.rows, key=key)
    else:
        kaldi_io.write_mat(fd, f, key=key)


def _wav_scp_path(rspec):
    kind, _, path = rspec.partition(":")
    if kind.split(",")[0] != "scp" or not path:
        raise SystemExit("expected scp:wav.scp, got %r" % rspec)
    return path


def _read_waves(path, opts, state=None):
    """(key, int16 samples) of every usable entry, in order (Kaldi's skip rules applied; a wave to be resampled is a
    ``mfcc.Wave`` carrying its rate).  An entry that is one recognised ``sph2pipe`` command comes as a ``mfcc.CodedWave``: only its
    header is read here, its bytes go to the GPU as they lie in the file (xvector_amd/sphere.py).  An entry whose last pipeline stage
    is wav-reverberate comes as (key, augment.Pending) added to ``state['plan']``: only its length is known here, the GPU makes
    its samples (xvector_amd/augment.py)."""
    for key, rx in mfcc.read_wav_scp(path):
        node = None
        if augment.is_augmented(rx):
            try:
                node = augment.parse_rx(rx)
                if isinstance(node, augment.Reverb):
                    if state is None:
                        raise augment.AugmentError("augmented entry outside a batch")
                    if state.get("plan") is None:
                        state["plan"] = augment.Plan()
                    top = state["augmenter"].plan([(key, node)], state["plan"]).top[-1]
                    p = augment.Pending(top, state["plan"])
                    if _select_pending(key, p, opts):
                        yield key, p
                    continue
            except augment.AugmentError as e:
                raise SystemExit("Failed to read the wave of %s: %s" % (key, e))
        try:
            coded = sphere.recognise(key, rx)
            if coded is None:
                rate, x = mfcc.load_wav(key, rx)
        except mfcc.WavError as e:
            raise SystemExit("Failed to read the wave of %s: %s" % (key, e))
        w = mfcc.select_coded(key, coded, opts) if coded is not None else mfcc.select_channel(key, rate, x, opts)
        if w is not None:
            yield key, w


def _select_pending(key, p, opts):
    """mfcc.select_channel's rules for an augmented entry (one channel, p.M samples at p.rate).  Its samples are made on the
    device at p.rate and are not resampled: another rate is skipped whatever --allow-downsample / --allow-upsample say."""
    if opts.channel not in (-1, 0):
        logger.warning("Invalid channel %d/1 for key %s; skipping", opts.channel, key)
        return False
    if p.rate != opts.sample_frequency:
        logger.warning("Sample frequency %g of key %s differs from --sample-frequency=%g; skipping (no resampling)",
                       p.rate, key, opts.sample_frequency)
        return False
    if p.M < opts.min_duration * p.rate:
        logger.warning("File: %s is too short (%g sec): producing no output.", key, p.M / float(p.rate))
        return False
    return True


def _batches(items, max_samples):
    keys, waves, tot = [], [], 0
    for k, w in items:
        if keys and tot + w.shape[0] > max_samples:
            yield keys, waves
            keys, waves, tot = [], [], 0
        keys.append(k)
        waves.append(w)
        tot += w.shape[0]
    if keys:
        yield keys, waves


def _planned_batches(path, opts, augmenter, max_samples):
    """_batches over _read_waves.  _batches reads the entry that overflows a batch before it yields the batch, so that entry is
    already planned into the current plan: it keeps that plan (augment.Pending.plan), and the entries read after the yield start a
    plan of their own, so no plan (and no decoded RIR or noise) outlives the batches that use it."""
    state = dict(augmenter=augmenter, plan=None)
    for keys, waves in _batches(_read_waves(path, opts, state), max_samples):
        state["plan"] = None
        yield keys, waves


def cmd_mfcc(args, with_vad):
    opts = _options(mfcc.MfccOptions, args.config, args)
    vopts = _options(mfcc.VadOptions, args.vad_config, args) if with_vad else None
    try:
        opts.check(resample=True)
    except (NotImplementedError, ValueError) as e:
        raise SystemExit(str(e))
    path = _wav_scp_path(args.wav_rspecifier)
    feats_out = _Out(args.feats_wspecifier)
    vad_out = _Out(args.vad_wspecifier) if with_vad else None
    nf_out = _NumFrames(args.write_num_frames) if args.write_num_frames else None
    engine = mfcc.Mfcc(opts, vopts, window_samples=WINDOW_SAMPLES)
    augmenter = augment.Augmenter()
    want_cm = _want_compress(args)
    n_done = n_vad_skipped = 0
    for keys, waves in _planned_batches(path, opts, augmenter, WINDOW_SAMPLES):
        if any(isinstance(w, augment.Pending) for w in waves):
            feats, vads, _ = augment.mfcc_compute(engine, augmenter, keys, waves, compress=want_cm)
        else:
            feats, vads, _ = engine.compute(keys, waves, compress=want_cm)
        for i, (k, f) in enumerate(zip(keys, feats)):
            _write_feats(feats_out.fd, f, k)
            if nf_out:
                nf_out.write(k, f.shape[0])
            if with_vad:
                if f.shape[0] == 0:
                    logger.warning("Empty feature matrix for utterance %s", k)
                    n_vad_skipped += 1
                else:
                    kaldi_io.write_vec_flt(vad_out.fd, vads[i], key=k)
            n_done += 1
    feats_out.close()
    if vad_out:
        vad_out.close()
    if nf_out:
        nf_out.close()
    logger.info("Done %d utterances (%d frames)%s", n_done, engine.stats["frames"],
                ", %d without a VAD vector" % n_vad_skipped if with_vad else "")


def _read_feats(rspec):
    kind, _, path = rspec.partition(":")
    kind = kind.split(",")[0]
    if kind == "scp":
        return kaldi_io.read_mat_scp(path)
    if kind == "ark":
        return kaldi_io.read_mat_ark(path)
    raise SystemExit("unsupported rspecifier %r (scp: or ark:)" % rspec)


def cmd_vad(args):
    vopts = _options(mfcc.VadOptions, args.config, args)
    out = _Out(args.vad_wspecifier)
    keys, mats = [], []
    for k, m in _read_feats(args.feats_rspecifier):
        if m.shape[0] == 0:
            logger.warning("Empty feature matrix for utterance %s", k)
            continue
        keys.append(k)
        mats.append(np.asarray(m, np.float32))
    runs = mfcc.compute_vad(mats, vopts)
    for k, v in zip(keys, runs):
        kaldi_io.write_vec_flt(out.fd, v, key=k)
    out.close()
    logger.info("Applied energy based voice activity detection; processed %d utterances", len(keys))


COPY_WINDOW_ROWS = 1 << 20        # rows held (and, compressed, uploaded) per window of copy-feats


def cmd_copy_feats(args):
    """copy-feats: every matrix of the input table to the output, plain (FM / DM as read; CM* decoded to FM) or compressed."""
    want_cm = _want_compress(args)
    out = _Out(args.feats_wspecifier)
    n = 0

    def flush(keys, mats):
        packed = compress.encode_host(mats, keys=keys, window_rows=COPY_WINDOW_ROWS) if want_cm else mats
        for k, m, f in zip(keys, mats, packed):
            _write_feats(out.fd, m if f is None else f, k)

    keys, mats, rows = [], [], 0
    for k, m in _read_feats(args.feats_rspecifier):
        m = np.asarray(m)
        if keys and rows + m.shape[0] > COPY_WINDOW_ROWS:
            flush(keys, mats)
            keys, mats, rows = [], [], 0
        keys.append(k)
        mats.append(m)
        rows += m.shape[0]
        n += 1
    if keys:
        flush(keys, mats)
    out.close()
    logger.info("Copied %d feature matrices.", n)


def _read_vecs(rspec):
    kind, _, path = rspec.partition(":")
    kind = kind.split(",")[0]
    if kind == "scp" and path:
        return kaldi_io.read_vec_flt_scp(path)
    if kind == "ark" and path:
        return kaldi_io.read_vec_flt_ark(path)
    raise SystemExit("unsupported rspecifier %r (scp: or ark:)" % rspec)


def cmd_vad_to_segments(args):
    """One ``<reco>-<first>-<end> <reco> <start s> <end s>`` line per segment of every recording of the VAD table (the key and line
    formats of the sliding mode's subsegments file), written under ``.tmp`` and renamed: what ``extract_embedding.py --segments``
    reads back.  Host only: the NumPy twin of the kernel the ``--segment-by-vad`` route runs."""
    from xvector_amd import segment
    from xvector_amd.extract_stream import subsegment_key, subsegment_line
    opts = segment.SegmentOptions(args.max_gap, args.min_segment_length, args.pad, args.max_segment_length)
    try:
        opts.check()
    except ValueError as e:
        raise SystemExit(str(e))
    if args.frame_shift <= 0:
        raise SystemExit("--frame-shift must be positive")
    n_reco = n_seg = n_none = 0
    with open(args.segments + ".tmp", "wt") as f:
        for reco, v in _read_vecs(args.vad_rspecifier):
            tab = segment.vad_segments_host(v, opts)
            if not len(tab):
                logger.warning("No segment for recording: '%s'", reco)
                n_none += 1
            f.write("".join(subsegment_line(subsegment_key(reco, a, a + n), reco, a, a + n, args.frame_shift) for a, n in tab.tolist()))
            n_reco += 1
            n_seg += len(tab)
    os.rename(args.segments + ".tmp", args.segments)
    logger.info("Wrote %d segments of %d recordings (%d without a segment)", n_seg, n_reco, n_none)


def cmd_wav_to_duration(args):
    """key + samples / rate per entry (Kaldi's wav-to-duration); an augmented entry's length comes from its options and the
    header of its input, without evaluating it."""
    path = _wav_scp_path(args.wav_rspecifier)
    kind, _, out = args.duration_wspecifier.partition(":")
    if kind.split(",")[0] != "ark" or not out:
        raise SystemExit("unsupported wspecifier %r (ark,t:F)" % args.duration_wspecifier)
    aug = augment.Augmenter()
    n = 0
    with open(out, "wt") as f:
        for key, rx in mfcc.read_wav_scp(path):
            try:
                samples, rate = augment.duration_samples(key, rx, aug)
            except (mfcc.WavError, augment.AugmentError) as e:
                raise SystemExit("Failed to read the wave of %s: %s" % (key, e))
            f.write("%s %.7g\n" % (key, np.float32(samples) / np.float32(rate)))
            n += 1
    logger.info("Printed duration for %d audio files.", n)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = p.add_subparsers(dest="cmd")
    m = sub.add_parser("compute-mfcc-feats")
    m.add_argument("--config", default=None)
    m.add_argument("--write-num-frames", default=None)
    _compress_flag(m)
    _flags(m, mfcc.MfccOptions)
    m.add_argument("wav_rspecifier")
    m.add_argument("feats_wspecifier")
    v = sub.add_parser("compute-vad")
    v.add_argument("--config", default=None)
    _flags(v, mfcc.VadOptions)
    v.add_argument("feats_rspecifier")
    v.add_argument("vad_wspecifier")
    b = sub.add_parser("compute-mfcc-vad")
    b.add_argument("--config", default=None)
    b.add_argument("--vad-config", default=None)
    b.add_argument("--write-num-frames", default=None)
    _compress_flag(b)
    _flags(b, mfcc.MfccOptions)
    _flags(b, mfcc.VadOptions)
    b.add_argument("wav_rspecifier")
    b.add_argument("feats_wspecifier")
    b.add_argument("vad_wspecifier")
    c = sub.add_parser("copy-feats")
    _compress_flag(c)
    c.add_argument("feats_rspecifier")
    c.add_argument("feats_wspecifier")
    g = sub.add_parser("vad-to-segments")
    g.add_argument("--max-gap", type=int, default=30, help="pauses of up to this many frames are closed")
    g.add_argument("--min-segment-length", type=int, default=50, help="shorter runs are dropped (frames)")
    g.add_argument("--pad", type=int, default=10, help="frames added on both sides of a kept run (at most half of --max-gap)")
    g.add_argument("--max-segment-length", type=int, default=1000, help="longer runs are split evenly (frames; 0: never)")
    g.add_argument("--frame-shift", type=float, default=10.0, help="milliseconds per frame")
    g.add_argument("vad_rspecifier")
    g.add_argument("segments")
    d = sub.add_parser("wav-to-duration")
    d.add_argument("--read-entire-file", action="store_true", help="accepted for Kaldi compatibility: every file is read whole")
    d.add_argument("wav_rspecifier")
    d.add_argument("duration_wspecifier")
    return p


def parse_args(argv):
    argv = list(argv)
    if argv[:1] == ["wav-to-duration"]:               # Kaldi's --read-entire-file=true|false form
        argv = [a.split("=")[0] if a.startswith("--read-entire-file=") else a for a in argv]
    # Kaldi's bare boolean: "--compress scp:wav.scp ..." must not take the rspecifier for its value
    argv = ["--compress=true" if a == "--compress" else a for a in argv]
    return build_parser().parse_args(argv)


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    try:
        if args.cmd == "compute-mfcc-feats":
            args.vad_config = None
            cmd_mfcc(args, False)
        elif args.cmd == "compute-mfcc-vad":
            cmd_mfcc(args, True)
        elif args.cmd == "compute-vad":
            cmd_vad(args)
        elif args.cmd == "copy-feats":
            cmd_copy_feats(args)
        elif args.cmd == "vad-to-segments":
            cmd_vad_to_segments(args)
        elif args.cmd == "wav-to-duration":
            cmd_wav_to_duration(args)
        else:
            build_parser().print_help()
            return 1
    except ValueError as e:               # unknown / malformed options in a config file
        raise SystemExit(str(e))
    return 0


if __name__ == "__main__":
    sys.exit(main())
