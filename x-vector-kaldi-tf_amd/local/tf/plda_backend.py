#!/usr/bin/env python
"""The recipe's back-end (stages 8-10 of run.sh) without Kaldi binaries.  Each subcommand is named after the binary it replaces:

  mean         ivector-mean scp:xvector.scp mean.vec
  compute-lda  ivector-subtract-global-mean scp:xvector.scp ark:- | ivector-compute-lda --total-covariance-factor=f --dim=d
               ark:- utt2spk transform.mat
  compute-plda ivector-compute-plda [--num-em-iters n] ark:spk2utt <vectors> plda; with --lda transform.mat the vectors first
               go through stage 8's chain on the GPU (subtract the set's own mean | transform-vec | ivector-normalize-length)
  score        ivector-plda-scoring [--num-utts=ark:num_utts.ark] plda <enrol> <test> trials scores; with --mean / --lda the
               stage-9 chain (ivector-subtract-global-mean mean.vec | transform-vec | ivector-normalize-length) runs on the GPU
               instead of Kaldi pipes; --scoring cosine scores the cosine of the same chain's vectors instead of the PLDA LLR;
               --cohort <vectors> [--cohort-top-n N] writes AS-norm scores (adaptive symmetric normalisation against the top N
               cohort scores of each side; the cohort goes through the same --mean / --lda chain as the tests)
  adapt-plda   ivector-adapt-plda [--within-covar-scale f] [--between-covar-scale f] [--mean-diff-scale f] plda <vectors>
               plda_adapt (stage 10's model); with --lda transform.mat the unlabelled in-domain vectors first go through stage
               8's chain on the GPU, as in compute-plda, and their fp64 moments are taken there on the f64 MFMA without the
               rows leaving the device
  cluster      [--lda transform.mat] [--threshold t] [--num-clusters n] [--prefix c] plda <vectors> utt2cluster: clustering-based
               adaptation, the step Kaldi has no binary for.  The PLDA scores of the unlabelled in-domain vectors
               against themselves and their average-linkage agglomerative clustering both run on the GPU; with --lda the
               vectors first go through stage 8's chain there, as in adapt-plda.  Writes one ``utt cluster`` line per vector.
               Turn utt2cluster into a spk2utt, fit an in-domain model with compute-plda --lda, mix it with interpolate-plda
  diarize      ivector-plda-scoring-dense | agglomerative-cluster --reco2utt [--reco2num-spk] | diarization/make_rttm.py
               (DESIGN.md §8.15): [--mean mean.vec] [--lda transform.mat] [--threshold t] [--reco2num-spk FILE] [--rttm OUT.rttm]
               [--vbx [--vbx-fa --vbx-fb --vbx-loop-prob --vbx-max-iters --vbx-epsilon --vbx-init-smoothing]]
               [--rttm-channel c] plda <vectors> <segments> <labels-out>.  <segments> is what extract_embedding.py
               --subsegments-file writes (``key reco start end``; any Kaldi segments file).  The vectors are grouped by recording;
               every recording's PLDA score matrix comes from one launch and every recording's average-linkage clustering runs in
               a workgroup of its own, all at once.  Writes ``key label`` lines (labels 1..K per recording) and, with --rttm, the
               speaker turns
  interpolate-plda   [--alpha a] plda_out plda_in plda: (1 - a) plda_out + a plda_in on the models' covariances and means (host)
  compute-eer  compute-eer <file of "score target|nontarget" lines, or ->   (prints the EER in percent)

Vector tables are ``scp:<file>`` or ``ark:<file>`` (options before the colon, e.g. ``ark,s,cs:``, are accepted and ignored).
The fits run on the host in float64 (xvector_amd/backend.py), preparing and scoring on the MI355X: there is no CPU fallback.
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

logger = logging.getLogger('plda_backend')
logger.addHandler(logging.StreamHandler())
logger.setLevel(logging.INFO)


def read_vectors(rspec):
    """{key: float32 vector} of an ``scp:`` / ``ark:`` table (insertion order kept)."""
    kind, _, path = rspec.partition(":")
    if not path:
        raise SystemExit("expected scp:<file> or ark:<file>, got %r" % rspec)
    kind = kind.split(",")[0]
    if kind == "scp":
        it = kaldi_io.read_vec_flt_scp(path)
    elif kind == "ark":
        it = kaldi_io.read_vec_flt_ark(path)
    else:
        raise SystemExit("unsupported table %r (scp: or ark: files only, no pipes)" % rspec)
    return {k: np.asarray(v, dtype=np.float32) for k, v in it}


def read_table(path):
    """Lines ``key value...`` -> {key: [values]}; ``ark:``/``ark,t:`` prefixes are stripped."""
    if ":" in path and path.split(":", 1)[0].split(",")[0] == "ark":
        path = path.split(":", 1)[1]
    out = {}
    with open(path, "rt") as f:
        for line in f:
            parts = line.split()
            if parts:
                out[parts[0]] = parts[1:]
    return out


def _stack(vectors, keys):
    return np.stack([vectors[k] for k in keys]).astype(np.float32)


def _read_lda_checked(args_lda, x, plda, nothing_written):
    """(t, dim): the LDA of --lda (None without one) and the dimension of the vectors x after it.  SystemExit when the LDA does not
    take the vectors or the PLDA not what comes out; nothing_written ends that message ("no model written")."""
    from xvector_amd import backend
    t = backend.read_transform(args_lda) if args_lda else None
    if t is not None and t.shape[1] not in (x.shape[1], x.shape[1] + 1):
        raise SystemExit("%s has %d columns, the vectors have dimension %d" % (args_lda, t.shape[1], x.shape[1]))
    dim = x.shape[1] if t is None else t.shape[0]
    if dim != plda.dim:
        raise SystemExit("the vectors have dimension %d%s, the PLDA %d: %s" %
                         (dim, " after the LDA" if t is not None else "", plda.dim, nothing_written))
    return t, dim


def _stage8_chain(x, t, mean_only=False):
    """stage 8's chain on the device: subtract the set's own mean (taken in float64, cast to float32), transform-vec with the LDA
    t, ivector-normalize-length.  -> (mean, the PLAIN-prepared device rows; None with mean_only, for a caller that hands the mean
    and t to a function that runs the chain itself)."""
    from xvector_amd import backend, hiplib
    mean = x.astype(np.float64).mean(axis=0).astype(np.float32)
    if mean_only:
        return mean, None
    return mean, backend.prepare(x, hiplib.SIDE_PLAIN, mean=mean, transform=t, length_norm=True)[0]


def cmd_mean(args):
    vectors = read_vectors(args.vectors)
    x = _stack(vectors, list(vectors)).astype(np.float64)
    mean = x.mean(axis=0).astype(np.float32)
    kaldi_io.write_vec_flt(args.mean_vec, mean)
    logger.info("Wrote mean of %d vectors of dimension %d" % (x.shape[0], x.shape[1]))


def cmd_compute_lda(args):
    from xvector_amd import backend
    vectors = read_vectors(args.vectors)
    utt2spk = {u: v[0] for u, v in read_table(args.utt2spk).items()}
    keys = [k for k in vectors if k in utt2spk]
    for k in vectors:
        if k not in utt2spk:
            logger.warning("No speaker for utterance %s" % k)
    x = _stack(vectors, keys).astype(np.float64)
    x -= x.mean(axis=0)                                  # ivector-subtract-global-mean without a mean argument
    t = backend.fit_lda(x, [utt2spk[k] for k in keys], args.dim, args.total_covariance_factor)
    backend.write_transform(args.transform, t, binary=args.binary)
    logger.info("Wrote LDA transform of dimension %d x %d" % t.shape)


def cmd_compute_plda(args):
    from xvector_amd import backend
    vectors = read_vectors(args.vectors)
    spk2utt = read_table(args.spk2utt)
    keys = list(vectors)
    x = _stack(vectors, keys)
    if args.lda:
        t = backend.read_transform(args.lda)
        x = _stage8_chain(x, t)[1][:, :t.shape[0]].cpu().numpy()
    pos = {k: i for i, k in enumerate(keys)}
    groups, missing = [], 0
    for spk, utts in spk2utt.items():
        have = [pos[u] for u in utts if u in pos]
        missing += len(utts) - len(have)
        if not have:
            logger.warning("Not producing output for speaker %s since no utterances had iVectors" % spk)
            continue
        groups.append(have)
    if missing:
        logger.warning("%d utterances of spk2utt absent from input" % missing)
    plda = backend.fit_plda(x, groups, num_em_iters=args.num_em_iters)
    backend.write_plda(args.plda, plda, binary=args.binary)


def cmd_adapt_plda(args):
    from xvector_amd import backend, hiplib
    for name in ("within_covar_scale", "between_covar_scale", "mean_diff_scale"):
        v = getattr(args, name)
        if not (np.isfinite(v) and v >= 0.0):
            raise SystemExit("--%s must be in [0, inf), got %r" % (name.replace("_", "-"), v))
    hiplib.require_gpu()                                 # no CPU fallback: fail before reading anything
    plda = backend.read_plda(args.plda_in)
    vectors = read_vectors(args.vectors)
    if not vectors:
        raise SystemExit("no vectors in %s: nothing to adapt to, no model written" % args.vectors)
    x = _stack(vectors, list(vectors))
    t, dim = _read_lda_checked(args.lda, x, plda, "no model written")
    if dim > hiplib.MOMENT_DIM_MAX:
        raise SystemExit("vectors of dimension %d: the moments kernel takes at most %d" % (dim, hiplib.MOMENT_DIM_MAX))
    # with an LDA the rows of stage 8's chain stay on the device
    n, s1, s2 = backend.moment_stats(x if t is None else _stage8_chain(x, t)[1], dim)
    logger.info("Read %d vectors of dimension %d" % (n, dim))
    out = backend.adapt_plda(plda, n, s1, s2, args.within_covar_scale, args.between_covar_scale, args.mean_diff_scale)
    backend.write_plda(args.plda_out, out, binary=args.binary)


def cmd_cluster(args):
    from xvector_amd import backend, hiplib
    if np.isnan(args.threshold):
        raise SystemExit("--threshold must be a number, got %r" % args.threshold)
    if args.num_clusters is not None and args.num_clusters < 1:
        raise SystemExit("--num-clusters must be at least 1, got %d" % args.num_clusters)
    hiplib.require_gpu()                                 # no CPU fallback: fail before reading anything
    plda = backend.read_plda(args.plda)
    vectors = read_vectors(args.vectors)
    if not vectors:
        raise SystemExit("no vectors in %s: nothing to cluster, no utt2cluster written" % args.vectors)
    keys = list(vectors)
    x = _stack(vectors, keys)
    n = len(keys)
    t, dim = _read_lda_checked(args.lda, x, plda, "no utt2cluster written")
    if n > hiplib.AHC_MAX_N:
        raise SystemExit("%d vectors: the clustering kernel takes at most %d" % (n, hiplib.AHC_MAX_N))
    if args.num_clusters is not None and args.num_clusters > n:
        raise SystemExit("--num-clusters %d exceeds the number of vectors %d" % (args.num_clusters, n))
    mean = _stage8_chain(x, t, mean_only=True)[0] if t is not None else None       # cluster_vectors runs the chain
    try:
        labels, _ = backend.cluster_vectors(x, plda, mean=mean, transform=t, threshold=args.threshold, num_clusters=args.num_clusters)
    except ValueError as e:
        raise SystemExit("%s: no utt2cluster written" % e)
    distinct, rank, counts = np.unique(labels, return_inverse=True, return_counts=True)
    width = len(str(n))
    with open(args.utt2cluster, "wt") as f:
        f.write("".join("%s %s%0*d\n" % (k, args.prefix, width, r + 1) for k, r in zip(keys, rank.tolist())))
    logger.info("Clustered %d vectors of dimension %d into %d clusters (%d with a single vector)" %
                (n, dim, len(distinct), int((counts == 1).sum())))


def parse_ms(tok):
    """A time in seconds -> integer milliseconds."""
    return int(round(1000 * float(tok)))


def read_segments(path):
    """A Kaldi segments file -> [(key, reco, start ms, end ms)] in file order.  SystemExit on a malformed line, a repeated key or
    end < start."""
    out, seen = [], set()
    with open(path, "rt") as f:
        for ln, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) < 4:
                raise SystemExit("%s:%d: expected <key> <reco> <start> <end>, got %r" % (path, ln, line.strip()))
            try:
                t0, t1 = parse_ms(parts[2]), parse_ms(parts[3])
            except (ValueError, OverflowError):
                raise SystemExit("%s:%d: bad times %r %r" % (path, ln, parts[2], parts[3]))
            if t1 < t0:
                raise SystemExit("%s:%d: segment %s ends before it starts (%s < %s)" % (path, ln, parts[0], parts[3], parts[2]))
            if parts[0] in seen:
                raise SystemExit("%s:%d: key %s appears twice" % (path, ln, parts[0]))
            seen.add(parts[0])
            out.append((parts[0], parts[1], t0, t1))
    return out


def group_segments(segments, have):
    """Group the segments that have a vector by recording: -> (recos, groups, n_missing).  recos: the recordings in order of first
    appearance; groups[r]: the indices into ``segments`` of recording r's lines, in file order (they need not be contiguous);
    n_missing: lines whose key is not in ``have``, which are skipped."""
    recos, index, groups, missing = [], {}, [], 0
    for i, (key, reco, _, _) in enumerate(segments):
        if key not in have:
            missing += 1
            continue
        if reco not in index:
            index[reco] = len(recos)
            recos.append(reco)
            groups.append([])
        groups[index[reco]].append(i)
    return recos, groups, missing


def number_labels(slots):
    """Cluster slots of one recording's vectors, in the recording's order -> labels 1..K, the clusters numbered by their first
    member (the kernel names a cluster by its first member, so this is the rank rule of ``cluster``, applied per recording)."""
    number = {}
    return [number.setdefault(s, len(number) + 1) for s in np.asarray(slots).tolist()]


def rttm_text(recos, channel=0):
    """The RTTM of recos = [(reco, [(start ms, end ms, key, label)])], the recordings in the given order.  Per recording: sort by
    (start, end, key); where consecutive segments of different labels overlap, both meet at the midpoint (end + start) // 2;
    consecutive segments of one label that touch or overlap merge (the end is the maximum); pieces of no length are dropped."""
    lines = []
    for reco, segs in recos:
        segs = sorted(segs, key=lambda s: (s[0], s[1], s[2]))
        start = [s[0] for s in segs]
        end = [s[1] for s in segs]
        label = [s[3] for s in segs]
        for i in range(len(segs) - 1):
            if label[i] != label[i + 1] and end[i] > start[i + 1]:
                end[i] = start[i + 1] = (end[i] + start[i + 1]) // 2
        pieces = []
        for t0, t1, l in zip(start, end, label):
            if pieces and pieces[-1][2] == l and t0 <= pieces[-1][1]:
                pieces[-1][1] = max(pieces[-1][1], t1)
            else:
                pieces.append([t0, t1, l])
        for t0, t1, l in pieces:
            if t1 > t0:
                lines.append("SPEAKER %s %d %7.3f %7.3f <NA> <NA> %s <NA> <NA>\n" % (reco, channel, t0 / 1000.0, (t1 - t0) / 1000.0, l))
    return "".join(lines)


def _write_renamed(path, text):
    with open(path + ".tmp", "wt") as f:
        f.write(text)
    os.replace(path + ".tmp", path)


def cmd_diarize(args):
    from xvector_amd import backend, hiplib
    if np.isnan(args.threshold):
        raise SystemExit("--threshold must be a number, got %r" % args.threshold)
    if args.rttm_channel < 0:
        raise SystemExit("--rttm-channel must not be negative, got %d" % args.rttm_channel)
    try:
        backend.check_target_energy(args.target_energy)
    except ValueError:
        raise SystemExit("--target-energy must be in (0, 1], got %r" % args.target_energy)
    try:
        vbx = backend.check_vbx_params(args.vbx_fa, args.vbx_fb, args.vbx_loop_prob, args.vbx_init_smoothing, args.vbx_max_iters,
                                       args.vbx_epsilon)
    except ValueError as e:
        raise SystemExit("the --vbx-* options: %s" % e)
    if not args.vbx:
        vbx = None
    segments = read_segments(args.segments)
    num_spk = {}
    if args.reco2num_spk:
        for reco, v in read_table(args.reco2num_spk).items():
            try:
                num_spk[reco] = int(v[0])
            except (IndexError, ValueError):
                raise SystemExit("%s: no speaker count for recording %s" % (args.reco2num_spk, reco))
            if num_spk[reco] < 1:
                raise SystemExit("%s: the speaker count of recording %s must be at least 1, got %d" %
                                 (args.reco2num_spk, reco, num_spk[reco]))
    hiplib.require_gpu()                                 # no CPU fallback: fail before reading the model or the vectors
    plda = backend.read_plda(args.plda)
    vectors = read_vectors(args.vectors)
    if not vectors:
        raise SystemExit("no vectors in %s: nothing to diarize, no labels written" % args.vectors)
    recos, groups, missing = group_segments(segments, vectors)
    listed = set(segments[i][0] for g in groups for i in g)
    for k in vectors:
        if k not in listed:
            raise SystemExit("vector %s has no line in %s: no labels written" % (k, args.segments))
    if missing:
        logger.warning("%d segments of %s have no vector: skipped" % (missing, args.segments))
    keys = [segments[i][0] for g in groups for i in g]
    x = _stack(vectors, keys)
    t, dim = _read_lda_checked(args.lda, x, plda, "no labels written")
    mean = kaldi_io.read_vec_flt(args.mean).astype(np.float32) if args.mean else None
    if mean is not None and mean.shape[0] != x.shape[1]:
        raise SystemExit("%s has dimension %d, the vectors %d: no labels written" % (args.mean, mean.shape[0], x.shape[1]))
    sizes = [len(g) for g in groups]
    counts = None
    if num_spk:
        counts = [num_spk.get(r) for r in recos]
        for r, n, k in zip(recos, sizes, counts):
            if k is not None and k > n:
                logger.warning("recording %s: %d speakers asked for, %d vectors: using %d" % (r, k, n, n))
    pca, vbx_rep = {}, {}
    if vbx is not None:
        # VBx visits a recording's vectors in the RTTM's own order, (start, end, key); the clustering keeps the file order
        order = [sorted(range(len(g)), key=lambda j: (segments[g[j]][2], segments[g[j]][3], segments[g[j]][0])) for g in groups]
        vbx = dict(vbx, time_order=np.concatenate(order), keep=np.asarray([r in num_spk for r in recos]))
    try:
        slots, _ = backend.diarize(x, sizes, plda, mean=mean, transform=t, threshold=args.threshold, num_spk=counts,
                                   target_energy=args.target_energy, pca_report=pca, vbx=vbx, vbx_report=vbx_rep)
    except ValueError as e:
        raise SystemExit("%s: no labels written" % e)
    label_of, by_reco, n_speakers, at = {}, [], 0, 0
    for reco, g in zip(recos, groups):
        labels = number_labels(slots[at:at + len(g)])
        at += len(g)
        n_speakers += max(labels)
        by_reco.append((reco, [(segments[i][2], segments[i][3], segments[i][0], l) for i, l in zip(g, labels)]))
        for i, l in zip(g, labels):
            label_of[i] = l
    _write_renamed(args.labels_out, "".join("%s %d\n" % (segments[i][0], label_of[i]) for i in sorted(label_of)))
    if args.rttm:
        _write_renamed(args.rttm, rttm_text(by_reco, args.rttm_channel))
    logger.info("Diarized %d recordings: %d vectors of dimension %d into %d speakers (%d segments without a vector skipped)" %
                (len(recos), len(keys), dim, n_speakers, missing))
    if pca:
        info = pca["info"]
        logger.info("Per-recording PCA at target energy %g: mean retained dimension %.2f of %d; %d recordings fell back to the "
                    "global model (%d without energy, %d without convergence)" %
                    (args.target_energy, float(pca["dim"].mean()), dim, int((info != 0).sum()), int((info == 1).sum()),
                     int((info == 2).sum())))
    if vbx_rep:
        ran = vbx_rep["ran"]
        many = int((vbx_rep["spk_before"] > hiplib.VBX_MAX_SPK).sum())
        logger.info("VBx resegmentation: %d recordings, mean %.2f iterations, %d speakers before and %d after; %d fell back to the "
                    "clustering (info 2); kept as clustered: %d named in --reco2num-spk, %d with more than %d clusters" %
                    (int(ran.sum()), float(vbx_rep["iters"][ran].mean()) if ran.any() else 0.0, int(vbx_rep["spk_before"][ran].sum()),
                     int(vbx_rep["spk_after"][ran].sum()), int((vbx_rep["info"] == 2).sum()),
                     int(vbx["keep"].sum()), many, hiplib.VBX_MAX_SPK))


def cmd_interpolate_plda(args):
    from xvector_amd import backend
    if not (np.isfinite(args.alpha) and 0.0 <= args.alpha <= 1.0):
        raise SystemExit("--alpha must be in [0, 1], got %r" % args.alpha)
    a, b = backend.read_plda(args.plda_out), backend.read_plda(args.plda_in)
    if a.dim != b.dim:
        raise SystemExit("the models have dimensions %d and %d: no model written" % (a.dim, b.dim))
    backend.write_plda(args.plda, backend.interpolate_plda(a, b, args.alpha), binary=args.binary)
    logger.info("Wrote (1 - %g) %s + %g %s, dimension %d" % (args.alpha, args.plda_out, args.alpha, args.plda_in, a.dim))


def cmd_score(args):
    from xvector_amd import backend, hiplib
    if args.cohort_top_n < 2:
        raise SystemExit("--cohort-top-n must be at least 2 (the std of a single cohort score is 0), got %d" % args.cohort_top_n)
    hiplib.require_gpu()                                 # no CPU fallback: fail before reading anything
    if args.smoothing != 0:
        raise SystemExit("only --smoothing 0 is supported (what run.sh uses)")
    plda = backend.read_plda(args.plda) if args.scoring == "plda" else None
    enrol = read_vectors(args.enrol)
    test = read_vectors(args.test)
    num_utts = None
    if args.num_utts:
        num_utts = {k: int(v[0]) for k, v in read_table(args.num_utts).items()}
    ekeys, tkeys = list(enrol), list(test)
    if num_utts is not None:
        for k in ekeys:
            if k not in num_utts:
                raise SystemExit("Number of utterances not given for speaker %s" % k)
    epos = {k: i for i, k in enumerate(ekeys)}
    tpos = {k: i for i, k in enumerate(tkeys)}
    k1s, k2s, ei, ti = [], [], [], []
    n_train_err = n_test_err = 0
    with open(args.trials, "rt") as f:
        for line in f:
            parts = line.split()
            if len(parts) < 2:
                continue
            a, b = parts[0], parts[1]
            if a not in epos:
                logger.warning("Key %s not present in training iVectors." % a)
                n_train_err += 1
                continue
            if b not in tpos:
                logger.warning("Key %s not present in test iVectors." % b)
                n_test_err += 1
                continue
            k1s.append(a); k2s.append(b); ei.append(epos[a]); ti.append(tpos[b])
    mean = kaldi_io.read_vec_flt(args.mean).astype(np.float32) if args.mean else None
    lda = backend.read_transform(args.lda) if args.lda else None
    counts = None if num_utts is None else np.array([num_utts[k] for k in ekeys], np.int32)
    cohort, top_n = None, args.cohort_top_n
    if args.cohort:
        cvec = read_vectors(args.cohort)
        if not cvec:
            raise SystemExit("the cohort %s is empty" % args.cohort)
        cohort = _stack(cvec, list(cvec))
        if top_n > len(cohort):
            logger.warning("--cohort-top-n %d exceeds the cohort size %d: using %d" % (top_n, len(cohort), len(cohort)))
            top_n = len(cohort)
    scorer = backend.Scorer(_stack(enrol, ekeys), _stack(test, tkeys), plda, counts, mean, lda, args.scoring, cohort=cohort,
                            cohort_top_n=top_n)
    if cohort is None:
        scores = scorer.score_trials(ei, ti)
    else:
        try:
            scores = scorer.score_trials(ei, ti, norm="asnorm")
        except backend.CohortStatsError as e:
            key = (ekeys if e.side == "enrol" else tkeys)[e.row]
            raise SystemExit("AS-norm: the cohort scores of %s %s have standard deviation %g; no scores written" %
                             ("enrolment" if e.side == "enrol" else "test vector", key, e.std))
        logger.info("AS-norm: cohort of %d vectors, top-N %d, cohort statistics took %.3f s" %
                    (len(cohort), top_n, scorer.stats_seconds))
    write_scores(args.scores, k1s, k2s, scores)
    logger.info("Processed %d trials, %d had errors." % (len(k1s) + n_train_err + n_test_err, n_train_err + n_test_err))
    return n_train_err + n_test_err


def write_scores(path, k1s, k2s, scores):
    """``key1 key2 score`` lines, the score as %g (C++ ostream default precision, what ivector-plda-scoring prints)."""
    with open(path, "wt") as f:
        f.write("".join("%s %s %g\n" % (a, b, s) for a, b, s in zip(k1s, k2s, scores.tolist())))


def cmd_compute_eer(args):
    from xvector_amd import backend
    fid = sys.stdin if args.scores == "-" else open(args.scores, "rt")
    tgt, non = [], []
    for line in fid:
        parts = line.split()
        if len(parts) != 2:
            raise SystemExit("Invalid input line (must have two fields): %s" % line.strip())
        if parts[1] == "target":
            tgt.append(float(parts[0]))
        elif parts[1] == "nontarget":
            non.append(float(parts[0]))
        else:
            raise SystemExit("Invalid input line (second field must be 'target' or 'nontarget'): %s" % line.strip())
    e, thr = backend.eer(tgt, non)
    logger.info("Equal error rate is %g%%, at threshold %g" % (100.0 * e, thr))
    print("%g" % (100.0 * e))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd")
    sub.required = True
    p = sub.add_parser("mean", help="ivector-mean")
    p.add_argument("vectors"); p.add_argument("mean_vec")
    p.set_defaults(fn=cmd_mean)
    p = sub.add_parser("compute-lda", help="ivector-compute-lda")
    p.add_argument("--dim", type=int, required=True)
    p.add_argument("--total-covariance-factor", type=float, default=0.0)
    p.add_argument("--binary", type=lambda s: s.lower() in ("true", "1"), default=True)
    p.add_argument("vectors"); p.add_argument("utt2spk"); p.add_argument("transform")
    p.set_defaults(fn=cmd_compute_lda)
    p = sub.add_parser("compute-plda", help="ivector-compute-plda")
    p.add_argument("--num-em-iters", type=int, default=10)
    p.add_argument("--lda", help="transform.mat: apply stage 8's chain to the vectors first (on the GPU)")
    p.add_argument("--binary", type=lambda s: s.lower() in ("true", "1"), default=True)
    p.add_argument("spk2utt"); p.add_argument("vectors"); p.add_argument("plda")
    p.set_defaults(fn=cmd_compute_plda)
    p = sub.add_parser("adapt-plda", help="ivector-adapt-plda")
    p.add_argument("--within-covar-scale", type=float, default=0.3)
    p.add_argument("--between-covar-scale", type=float, default=0.7)
    p.add_argument("--mean-diff-scale", type=float, default=1.0)
    p.add_argument("--lda", help="transform.mat: apply stage 8's chain to the vectors first (on the GPU)")
    p.add_argument("--binary", type=lambda s: s.lower() in ("true", "1"), default=True)
    p.add_argument("plda_in"); p.add_argument("vectors"); p.add_argument("plda_out")
    p.set_defaults(fn=cmd_adapt_plda)
    p = sub.add_parser("cluster", help="cluster unlabelled vectors by PLDA score (average linkage)")
    p.add_argument("--lda", help="transform.mat: apply stage 8's chain to the vectors first (on the GPU)")
    p.add_argument("--threshold", type=float, default=0.0, help="stop when no pair of clusters has an average score this large")
    p.add_argument("--num-clusters", type=int, help="stop at this many clusters at the latest")
    p.add_argument("--prefix", default="c", help="cluster names are <prefix><rank>")
    p.add_argument("plda"); p.add_argument("vectors"); p.add_argument("utt2cluster")
    p.set_defaults(fn=cmd_cluster)
    p = sub.add_parser("diarize", help="per-recording PLDA scoring, average-linkage clustering and RTTM")
    p.add_argument("--mean", help="mean.vec: subtract it first (ivector-subtract-global-mean)")
    p.add_argument("--lda", help="transform.mat: transform-vec + ivector-normalize-length after the mean")
    p.add_argument("--threshold", type=float, default=0.0, help="stop when no pair of clusters has an average score this large")
    p.add_argument("--reco2num-spk", help="lines <reco> <count>: these recordings stop at exactly that many clusters")
    p.add_argument("--target-energy", type=float, default=1.0,
                   help="ivector-plda-scoring-dense --target-energy, in (0, 1]: score every recording in the PCA subspace of its own "
                        "vectors that holds this share of their variance, under the PLDA projected into it (the callhome recipe "
                        "passes 0.1).  The default here is 1.0 -- no PCA, the scores of earlier versions -- where Kaldi's is 0.5")
    p.add_argument("--vbx", action="store_true",
                   help="VBx resegmentation after the clustering (a variational-Bayes HMM over each recording's vectors in time order, "
                        "under the global PLDA, initialised from the clustering; DESIGN.md §8.17).  Recordings named in "
                        "--reco2num-spk and recordings with more than 64 clusters keep their clustering")
    p.add_argument("--vbx-fa", type=float, default=0.3, help="VBx: the scale of the acoustic statistics (> 0)")
    p.add_argument("--vbx-fb", type=float, default=17.0, help="VBx: the scale of the speaker regularisation (> 0)")
    p.add_argument("--vbx-loop-prob", type=float, default=0.99, help="VBx: the probability of staying with the speaker, in [0, 1)")
    p.add_argument("--vbx-max-iters", type=int, default=40, help="VBx: iterations at most, in [1, 100]")
    p.add_argument("--vbx-epsilon", type=float, default=1e-6, help="VBx: stop when the ELBO gains less than this")
    p.add_argument("--vbx-init-smoothing", type=float, default=5.0, help="VBx: the softmax weight of the clustering's label (>= 0)")
    p.add_argument("--rttm", help="write the speaker turns here")
    p.add_argument("--rttm-channel", type=int, default=0)
    p.add_argument("plda"); p.add_argument("vectors"); p.add_argument("segments"); p.add_argument("labels_out")
    p.set_defaults(fn=cmd_diarize)
    p = sub.add_parser("interpolate-plda", help="a PLDA between two")
    p.add_argument("--alpha", type=float, default=0.5, help="weight of plda_in, in [0, 1]")
    p.add_argument("--binary", type=lambda s: s.lower() in ("true", "1"), default=True)
    p.add_argument("plda_out"); p.add_argument("plda_in"); p.add_argument("plda")
    p.set_defaults(fn=cmd_interpolate_plda)
    p = sub.add_parser("score", help="ivector-plda-scoring")
    p.add_argument("--num-utts", help="ark:num_utts.ark (enrolment utterance counts)")
    p.add_argument("--mean", help="mean.vec: subtract it first (ivector-subtract-global-mean)")
    p.add_argument("--lda", help="transform.mat: transform-vec + ivector-normalize-length after the mean")
    p.add_argument("--scoring", choices=("plda", "cosine"), default="plda")
    p.add_argument("--smoothing", type=float, default=0.0)
    p.add_argument("--cohort", help="scp: / ark: cohort vectors: write AS-norm scores (DESIGN.md §8.5)")
    p.add_argument("--cohort-top-n", type=int, default=300, help="cohort scores per side in the AS-norm statistics (>= 2; "
                   "clamped to the cohort size)")
    p.add_argument("plda"); p.add_argument("enrol"); p.add_argument("test"); p.add_argument("trials"); p.add_argument("scores")
    p.set_defaults(fn=cmd_score)
    p = sub.add_parser("compute-eer", help="compute-eer")
    p.add_argument("scores")
    p.set_defaults(fn=cmd_compute_eer)
    args = ap.parse_args(argv)
    return args.fn(args)


if __name__ == "__main__":
    main()
