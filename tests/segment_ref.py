"""The segmentation rule of DESIGN.md §8.18 as a literal per-frame loop: close, drop, pad, split, one step after the other on
Python lists.  Written from the rule's text, not from ``xvector_amd.segment.vad_segments_host`` or the kernel (both walk the voiced
frames and never form the closed mask).  Also the inputs the CPU and GPU tests share."""
import numpy as np


def segments(v, G, M, P, L):
    """[(first frame, length)] of an utterance with decisions ``v`` (voiced iff != 0; NaN != 0 holds)."""
    T = len(v)
    mask = [bool(x != 0) for x in v]
    # 1. close: maximal unvoiced runs [a, b) with a > 0, b < T, b - a <= G
    closed = list(mask)
    t = 0
    while t < T:
        if mask[t]:
            t += 1
            continue
        a = t
        while t < T and not mask[t]:
            t += 1
        if a > 0 and t < T and t - a <= G:
            for s in range(a, t):
                closed[s] = True
    # 2. drop: maximal voiced runs of the result with b - a >= M
    runs, t = [], 0
    while t < T:
        if not closed[t]:
            t += 1
            continue
        a = t
        while t < T and closed[t]:
            t += 1
        if t - a >= M:
            runs.append((a, t))
    # 3. pad
    runs = [(max(a - P, 0), min(b + P, T)) for a, b in runs]
    # 4. split
    out = []
    for a, b in runs:
        n = b - a
        if L > 0 and n > L:
            k = (n + L - 1) // L
            for i in range(k):
                out.append((a + (i * n) // k, ((i + 1) * n) // k - (i * n) // k))
        else:
            out.append((a, n))
    return out


def capacity(T, G, M, L):
    return (T + G + 1) // (M + G + 1) + (T // L if L else 0)


def check_properties(segs, T, G, M, L):
    """Ordered, disjoint, inside [0, T), every length in [M, L], the count within the capacity."""
    end = 0
    for a, n in segs:
        assert a >= end and n >= M and (L == 0 or n <= L) and a + n <= T, (segs, T, G, M, L)
        end = a + n
    assert len(segs) <= capacity(T, G, M, L), (len(segs), T, G, M, L)


def bursty(rng, T, run_scale, gap_scale, lead=None):
    """T decisions of alternating voiced and unvoiced bursts with geometric lengths around the two scales (values 1.0 / 0.0)."""
    v = np.zeros(T, np.float32)
    t = int(rng.integers(0, gap_scale + 1)) if lead is None else lead
    while t < T:
        n = int(rng.geometric(1.0 / max(run_scale, 1)))
        v[t:t + n] = 1.0
        t += n + int(rng.geometric(1.0 / max(gap_scale, 1)))
    return v


def hand_cases(G, M, P, L):
    """[(name, decisions)] around every threshold of the rule, for the parameters given."""
    one, zero = (lambda n: [1.0] * n), (lambda n: [0.0] * n)
    g1 = max(G, 1)
    cases = [
        ("gap of exactly G", one(M) + zero(G) + one(M)),
        ("gap of G + 1", one(M) + zero(G + 1) + one(M)),
        ("run of M - 1", zero(5) + one(M - 1) + zero(5)),
        ("run of M", zero(5) + one(M) + zero(5)),
        ("two short runs a closed gap makes long enough", zero(3) + one(M // 2) + zero(min(G, 2)) + one(M - M // 2) + zero(3)),
        ("unclosed gap at frame 0", zero(g1) + one(M)),
        ("unclosed gap at T", one(M) + zero(g1)),
        ("unclosed gaps at both ends", zero(g1) + one(M) + zero(g1)),
        ("all voiced", one(3 * M + 1)),
        ("all unvoiced", zero(3 * M + 1)),
        ("T = 0", []),
        ("T = 1 voiced", one(1)),
        ("padding clipped at 0", zero(max(P - 1, 0)) + one(M) + zero(P + 3)),
        ("padding clipped at T", zero(P + 3) + one(M) + zero(max(P - 1, 0))),
        ("padding not clipped", zero(P) + one(M) + zero(P)),
        ("a NaN decision", zero(4) + one(M // 2) + [float("nan")] + one(M - M // 2 - 1) + zero(4)),
        ("negative and tiny decisions are voiced", zero(4) + [-1.0, 1e-30] * ((M + 1) // 2) + zero(4)),
    ]
    if L > 0:
        for n in (L, L + 1, 2 * L, 2 * L + 1):
            cases.append(("whole utterance of n = %d" % n, one(n)))
            if n - 2 * P >= M:
                cases.append(("padded run of n = %d" % n, zero(P + 2) + one(n - 2 * P) + zero(P + 2)))
    return [(name, np.array(v, np.float32)) for name, v in cases]
