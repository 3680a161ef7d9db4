"""Test-side NumPy restatement of diarization: per-recording average-linkage clustering through tests/ahc_ref.py,
the rule that numbers a recording's clusters, and the RTTM rule of `plda_backend.py diarize`.

RTTM rule (per recording; times are integer milliseconds, round(1000 * seconds)):
  1. sort the segments by (start, end, key);
  2. for consecutive segments i, i + 1 with different labels and end_i > start_{i+1}: both become (end_i + start_{i+1}) // 2;
  3. consecutive segments of the same label merge when start_{i+1} <= end_i (the end of the merged piece is the maximum);
  4. pieces of zero length are dropped (so is a piece squeezed from both sides until its end lies before its start);
  5. one line ``SPEAKER <reco> <channel> %7.3f %7.3f <NA> <NA> <label> <NA> <NA>`` (start, duration in seconds) per piece."""
import numpy as np

import ahc_ref


def blocks(scores, sizes):
    """The [n, n] blocks of packed scores: group g at the running offset, row stride n rounded up to a multiple of 4."""
    out, at = [], 0
    for n in sizes:
        ld = (n + 3) // 4 * 4
        out.append(np.asarray(scores[at:at + n * ld]).reshape(n, ld)[:, :n])
        at += n * ld
    return out


def cluster_groups(group_scores, thresholds, min_clusters):
    """Per group: (labels, (a, b, score)) of ahc_ref.ahc on that group's [n, n] scores with its own stop rule."""
    return [ahc_ref.ahc(s, threshold=t, min_clusters=m) for s, t, m in zip(group_scores, thresholds, min_clusters)]


def stop_rules(sizes, threshold, num_spk):
    """(thresholds, min_clusters): a recording with a speaker count stops at exactly min(count, n) clusters."""
    thr, minc = [], []
    for g, n in enumerate(sizes):
        k = None if num_spk is None else num_spk[g]
        thr.append(threshold if k is None else -np.inf)
        minc.append(1 if k is None else min(k, n))
    return thr, minc


def number_labels(slots):
    """Labels 1..K of one recording: clusters numbered in the order in which their first member appears."""
    seen, out = {}, []
    for s in np.asarray(slots).tolist():
        if s not in seen:
            seen[s] = len(seen) + 1
        out.append(seen[s])
    return out


def to_ms(tok):
    return int(round(1000 * float(tok)))


def rttm(recos, channel=0):
    """recos: [(reco, [(start ms, end ms, key, label)])] in output order -> the RTTM text."""
    text = ""
    for reco, segs in recos:
        segs = [list(s) for s in sorted(segs, key=lambda s: (s[0], s[1], s[2]))]
        for cur, nxt in zip(segs[:-1], segs[1:]):
            if cur[3] != nxt[3] and cur[1] > nxt[0]:
                mid = (cur[1] + nxt[0]) // 2
                cur[1] = mid
                nxt[0] = mid
        merged = []
        for s in segs:
            if merged and merged[-1][3] == s[3] and s[0] <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], s[1])
            else:
                merged.append(list(s))
        for s in merged:
            if s[1] - s[0] > 0:
                text += "SPEAKER %s %d %7.3f %7.3f <NA> <NA> %s <NA> <NA>\n" % (reco, channel, s[0] / 1000.0, (s[1] - s[0]) / 1000.0, s[3])
    return text


def group_by_reco(segments, have):
    """segments: [(key, reco, start, end)] -> (recos in order of first appearance, {reco: [segment index]}, skipped) over the
    lines whose key is in ``have``."""
    recos, members, skipped = [], {}, 0
    for i, seg in enumerate(segments):
        if seg[0] not in have:
            skipped += 1
        else:
            if seg[1] not in members:
                recos.append(seg[1])
                members[seg[1]] = []
            members[seg[1]].append(i)
    return recos, members, skipped
