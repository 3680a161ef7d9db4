#!/usr/bin/env python
"""Stages 3-5 of the recipe without Kaldi binaries: from a raw data directory (feats.scp, vad.scp, utt2spk) to the egs directory
train_dnn.py reads (xvector_amd/egs.py).

  prepare   --data DIR --out-dir DIR [--min-len 500] [--min-num-utts 8]
            run.sh stage 3 without writing features: utt2num_frames after silence removal (from vad.scp), utterances with MORE
            than --min-len voiced frames, speakers with AT LEAST --min-num-utts of them -> utt2spk, spk2utt, utt2num_frames
  lists     --utt2spk F --spk2utt F --utt2num-frames F --temp DIR [--num-heldout-utts 200] [--seed 0]
            the held-out lists and label tables of get_egs.sh stage 0 (valid_uttlist, train_subset_uttlist, spk2int, utt2int*,
            utt2num_frames.*), the shuffles from a seeded Python stream
  info      --egs-dir DIR --feat-dim F [--num-repeats 10] [--frames-per-iter 10000000] [--num-diagnostic-archives 1]
            info/{feat_dim,num_frames,num_archives,num_diagnostic_archives} as get_egs.sh derives them from
            temp/utt2num_frames.train; prints the number of training archives
  allocate  create_egs.py's flags and defaults -> temp/ranges.*, temp/archive_minibatch_count, temp/outputs.*, pdf2num
  write     create_tar_files.py's flags + --feats-scp --vad-scp [--cmn-window 300] [--cmn-center yes] [--min-window 100]
            -> egs.<n>.tar + egs.<n>.npy of one job, cut from the RAW features on the MI355X (no CPU fallback)
"""
from __future__ import print_function

import argparse
import logging
import os
import random
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))

from xvector_amd import egs  # noqa: E402

logger = logging.getLogger("make_egs")
logger.addHandler(logging.StreamHandler())
logger.setLevel(logging.INFO)


def _bool(text):
    if text.lower() in ("true", "yes", "1"):
        return True
    if text.lower() in ("false", "no", "0"):
        return False
    raise argparse.ArgumentTypeError("expected true or false, got %r" % text)


def get_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = parser.add_subparsers(dest="command")
    sub.required = True

    p = sub.add_parser("prepare")
    p.add_argument("--data", required=True, help="Raw data directory: feats.scp, vad.scp, utt2spk.")
    p.add_argument("--out-dir", dest="out_dir", required=True)
    p.add_argument("--min-len", dest="min_len", type=int, default=500)
    p.add_argument("--min-num-utts", dest="min_num_utts", type=int, default=8)

    p = sub.add_parser("lists")
    p.add_argument("--utt2spk", required=True)
    p.add_argument("--spk2utt", required=True)
    p.add_argument("--utt2num-frames", dest="utt2num_frames", required=True)
    p.add_argument("--temp", required=True)
    p.add_argument("--num-heldout-utts", dest="num_heldout_utts", type=int, default=200)
    p.add_argument("--seed", type=int, default=0)

    p = sub.add_parser("info")
    p.add_argument("--egs-dir", dest="egs_dir", required=True)
    p.add_argument("--feat-dim", dest="feat_dim", type=int, required=True)
    p.add_argument("--num-repeats", dest="num_repeats", type=int, default=10)
    p.add_argument("--frames-per-iter", dest="frames_per_iter", type=int, default=10000000)
    p.add_argument("--num-diagnostic-archives", dest="num_diagnostic_archives", type=int, default=1)

    p = sub.add_parser("allocate")
    p.add_argument("--prefix", type=str, default="")
    p.add_argument("--num-repeats", dest="num_repeats", type=int, default=10)
    p.add_argument("--min-frames-per-chunk", dest="min_frames_per_chunk", type=int, default=50)
    p.add_argument("--max-frames-per-chunk", dest="max_frames_per_chunk", type=int, default=300)
    p.add_argument("--randomize-chunk-length", dest="randomize_chunk_length", type=str, default="true", choices=["false", "true"])
    p.add_argument("--frames-per-iter", dest="frames_per_iter", type=int, default=1000000)
    p.add_argument("--num-archives", dest="num_archives", type=int, default=-1)
    p.add_argument("--num-jobs", dest="num_jobs", type=int, default=-1)
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--num-pdfs", dest="num_pdfs", type=int, default=-1)
    p.add_argument("--accepted-overlap", dest="accepted_overlap", type=float, default=0.2)
    p.add_argument("--minibatch-size", dest="minibatch_size", type=int, default=128)
    p.add_argument("--utt2len-filename", dest="utt2len_filename", type=str, required=True)
    p.add_argument("--utt2int-filename", dest="utt2int_filename", type=str, required=True)
    p.add_argument("--egs-dir", dest="egs_dir", type=str, required=True)

    p = sub.add_parser("write")
    p.add_argument("--prefix", type=str, default="")
    p.add_argument("--egs-dir", dest="egs_dir", type=str, required=True)
    p.add_argument("--shuffle", type=_bool, default=True)
    p.add_argument("--random-seed", dest="random_seed", type=int, default=0)
    p.add_argument("--feature-dim", dest="feature_dim", type=int, required=True)
    p.add_argument("--minibatch-size", dest="minibatch_size", type=int, required=True)
    p.add_argument("--outputs-file", dest="outputs_file", type=str, required=True)
    p.add_argument("--feats-scp", dest="feats_scp", type=str, required=True, help="RAW features (no CMN, all frames).")
    p.add_argument("--vad-scp", dest="vad_scp", type=str, required=True)
    p.add_argument("--cmn-window", dest="cmn_window", type=int, default=300)
    p.add_argument("--cmn-center", dest="cmn_center", type=str, default="yes", choices=("yes", "no"))
    p.add_argument("--min-window", dest="min_window", type=int, default=100)
    p.add_argument("--frame-budget", dest="frame_budget", type=int, default=4000000,
                   help="Raw frames resident on the device per window of utterances.")
    return parser


def _write_pairs(path, pairs):
    with open(path, "wt") as f:
        for k, v in pairs:
            f.write("%s %s\n" % (k, v))


def prepare(args):
    if os.path.exists(os.path.join(args.data, "segments")):
        raise SystemExit("%s/segments exists: segmented recordings are not supported" % args.data)
    utt2spk = egs.read_pairs(os.path.join(args.data, "utt2spk"))
    voiced = egs.voiced_counts(os.path.join(args.data, "vad.scp"))
    lengths = egs.feat_lengths(os.path.join(args.data, "feats.scp"))
    u2s, s2u, u2n = egs.filter_utterances(utt2spk, voiced, lengths, args.min_len, args.min_num_utts)
    os.makedirs(args.out_dir, exist_ok=True)
    _write_pairs(os.path.join(args.out_dir, "utt2spk"), u2s)
    _write_pairs(os.path.join(args.out_dir, "spk2utt"), [(s, " ".join(u)) for s, u in s2u])
    _write_pairs(os.path.join(args.out_dir, "utt2num_frames"), u2n)
    dims = set(lengths[u][1] for u, _ in u2s)
    if len(dims) > 1:
        raise SystemExit("feats.scp mixes feature dimensions %s" % sorted(dims))
    with open(os.path.join(args.out_dir, "feat_dim"), "wt") as f:
        f.write("%d\n" % (dims.pop() if dims else 0))
    logger.info("prepare: kept %d of %d utterances, %d speakers" % (len(u2s), len(utt2spk), len(s2u)))


def lists(args):
    temp = args.temp
    os.makedirs(temp, exist_ok=True)
    utt2spk = egs.read_pairs(args.utt2spk)
    u2n = egs.read_pairs(args.utt2num_frames)
    rng = random.Random(args.seed)
    utts = [u for u, _ in utt2spk]
    rng.shuffle(utts)
    valid = utts[:args.num_heldout_utts]
    vset = set(valid)
    train = [(u, n) for u, n in u2n if u not in vset]
    tutts = [u for u, _ in train]
    rng.shuffle(tutts)
    subset = tutts[:args.num_heldout_utts]
    sset = set(subset)
    with open(os.path.join(temp, "valid_uttlist"), "wt") as f:
        f.write("".join(u + "\n" for u in valid))
    with open(os.path.join(temp, "train_subset_uttlist"), "wt") as f:
        f.write("".join(u + "\n" for u in subset))
    _write_pairs(os.path.join(temp, "utt2num_frames"), u2n)
    tables = {"train": train, "valid": [(u, n) for u, n in u2n if u in vset], "train_subset": [(u, n) for u, n in train if u in sset]}
    spk2int = dict((s, i) for i, (s, _) in enumerate(egs.read_pairs(args.spk2utt)))
    _write_pairs(os.path.join(temp, "spk2int"), sorted(spk2int.items(), key=lambda e: e[1]))
    utt2int = [(u, spk2int[s]) for u, s in utt2spk]
    _write_pairs(os.path.join(temp, "utt2int"), utt2int)
    for name, table in tables.items():
        _write_pairs(os.path.join(temp, "utt2num_frames." + name), table)
        keep = set(u for u, _ in table)
        _write_pairs(os.path.join(temp, "utt2int." + name), [(u, i) for u, i in utt2int if u in keep])


def info(args):
    num_frames = sum(int(n) for _, n in egs.read_pairs(os.path.join(args.egs_dir, "temp", "utt2num_frames.train")))
    num_archives = (num_frames * args.num_repeats) // args.frames_per_iter + 1
    os.makedirs(os.path.join(args.egs_dir, "info"), exist_ok=True)
    for name, value in (("feat_dim", args.feat_dim), ("num_frames", num_frames), ("num_archives", num_archives),
                        ("num_diagnostic_archives", args.num_diagnostic_archives)):
        with open(os.path.join(args.egs_dir, "info", name), "wt") as f:
            f.write("%d\n" % value)
    print(num_archives)
    return num_archives


def allocate(args):
    for path in (args.utt2int_filename, args.utt2len_filename):
        if not os.path.exists(path):
            raise SystemExit("%s does not exist" % path)
    counts = egs.allocate(egs.read_pairs(args.utt2len_filename), egs.read_pairs(args.utt2int_filename), args.egs_dir, prefix=args.prefix,
                          num_repeats=args.num_repeats, min_frames_per_chunk=args.min_frames_per_chunk,
                          max_frames_per_chunk=args.max_frames_per_chunk, randomize_chunk_length=args.randomize_chunk_length == "true",
                          frames_per_iter=args.frames_per_iter, num_archives=args.num_archives, num_jobs=args.num_jobs, seed=args.seed,
                          num_pdfs=args.num_pdfs, accepted_overlap=args.accepted_overlap, minibatch_size=args.minibatch_size)
    logger.info("allocate: %d archives, %d minibatches" % (len(counts), sum(counts)))


def write(args, gather=None):
    if not args.outputs_file or not os.path.exists(args.outputs_file):
        raise SystemExit("The specified outputs file '%s' not exist." % args.outputs_file)
    w = egs.EgsWriter(args.egs_dir, args.feats_scp, args.vad_scp, args.feature_dim, args.minibatch_size, prefix=args.prefix,
                      shuffle=args.shuffle, random_seed=args.random_seed, gather=gather, cmn_window=args.cmn_window,
                      center=args.cmn_center == "yes", min_window=args.min_window, frame_budget=args.frame_budget, logger=logger)
    w.write_job(args.outputs_file)
    logger.info("write: %d archives, %d raw frames read, %d frames written" % (w.stats["archives"], w.stats["frames_in"],
                                                                              w.stats["frames_out"]))


def main(argv=None):
    args = get_parser().parse_args(argv)
    {"prepare": prepare, "lists": lists, "info": info, "allocate": allocate, "write": write}[args.command](args)


if __name__ == "__main__":
    main()
