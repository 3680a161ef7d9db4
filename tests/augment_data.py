"""Hand-built descriptor tables, inputs and references for the six wav-reverberate kernels (csrc/xv_augment.hip), one kernel at a
time: what tests/test_gpu_augment_elementwise.py feeds hiplib.augment_* and what tests/test_augment_bounds_cpu.py settles
without a GPU.  NumPy and Python integers only; nothing is imported from xvector_amd, and nothing here follows the order in
which xvector_amd/augment.py lays its tables out.  Tile sizes and field positions are restated from include/xvector_hip.h (the
CPU test compares them with the header and with augment.py).

References:
* power, conv on the 2^-15 grid, write: one right answer per element, in Python / int64 integers;
* mix, gains, level: a replay of the one order the ABI fixes (list order, tile order), each operation rounded once in fp64;
* sums of squares whose tree the kernel is free to round differently (FMA contraction of ss += v * v): the exact value as a
  Fraction (exact_sumsq) and a bound k * 2^-53 * exact * 1.01, k the longest chain of roundings one term passes through."""
import fractions

import numpy as np

Fr = fractions.Fraction
LD = np.longdouble
F32 = np.float32

POWER_TILE, CONV_TILE, ELEM_TILE = 16384, 2048, 1024       # samples per workgroup: power; conv; mix and write
CONV_CHUNK = 1024                                          # taps per LDS chunk of the convolution
UTT_FIELDS, REF_FIELDS = 16, 4
UTT_NAMES = ("X_OFF", "N", "Y_OFF", "Y_LEN", "RIR", "EARLY_TILE0", "EARLY_NTILES", "EARLY_LEN", "REF0", "NREF", "SHIFT", "M",
             "OUT_OFF", "MIX_TILE0", "MIX_NTILES", "X_SEG")
(X_OFF, N_, Y_OFF, Y_LEN, RIR, EARLY_TILE0, EARLY_NTILES, EARLY_LEN, REF0, NREF, SHIFT, M_, OUT_OFF, MIX_TILE0, MIX_NTILES,
 X_SEG) = range(UTT_FIELDS)
REF_NAMES = ("NOISE_OFF", "NOISE_LEN", "OFFSET", "NOISE_SEG")
NOISE_OFF, NOISE_LEN, OFFSET, NOISE_SEG = range(REF_FIELDS)

# Longest chain of roundings one term of a per-tile sum of squares passes through, counted from the kernels as written:
# a thread adds its terms in series (ss += v * v: one rounding per add when the product is contracted into an FMA, the square's own
# rounding otherwise -- the "+ 1"), then block_sum halves the workgroup log2(256) = 8 times.
K_MIX = 4 + 8 + 1          # aug_mix_kernel: EPT = 4 samples per thread, 256 threads
K_CONV = 8 + 8 + 1         # aug_conv_kernel: CR = 8 outputs per thread, 256 threads
INT16_SENTINEL = -21846    # 0xAAAA: the canary of an int16 output
GARBAGE = 12345            # what the sample pool holds between the described runs: a read one sample too far changes a sum


def scramble(n, seed):
    """A fixed order of range(n) that is not the ascending one (n >= 2)."""
    p = np.random.default_rng(seed).permutation(n)
    if n >= 2 and np.array_equal(p, np.arange(n)):
        p = p[::-1].copy()
    return p


def exact_sumsq(a):
    """The sum of squares of fp64 values as a Fraction: integer mantissas squared and shifted to the smallest exponent."""
    a = np.asarray(a, np.float64).ravel()
    assert np.isfinite(a).all()
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)                  # exact: |m| < 1 has 53 bits
    nz = mi != 0
    if not nz.any():
        return Fr(0)
    e = e.astype(np.int64) - 53
    emin = int(e[nz].min())
    tot = 0
    for q, s in zip(mi[nz].tolist(), (e[nz] - emin).tolist()):
        tot += (q * q) << (2 * s)
    return Fr(tot) * Fr(2) ** (2 * emin)


def sumsq_ratio(got, exact, k):
    """|got - exact| / (k * 2^-53 * exact * 1.01) with exact a Fraction of non-negative terms; 0 / 0 counts as 0."""
    got = float(got)
    if not np.isfinite(got):
        return float("inf")
    err = abs(Fr(got) - exact)
    bound = Fr(k) * Fr(1, 2 ** 53) * exact * Fr(101, 100)
    if bound == 0:
        return 0.0 if err == 0 else float("inf")
    return float(err / bound)


def ulps32(a, b):
    """Distance in fp32 steps between finite values of one sign (or zero)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def seq_sum(values):
    """The fp64 sum in list order, each add rounded once."""
    s = 0.0
    for v in values:
        s = s + float(v)
    return s


def _signal(rng, n, lim=32767):
    """Non-zero integers in [-lim, lim] (int16)."""
    v = rng.integers(1, lim + 1, size=n) * rng.choice((-1, 1), size=n)
    return v.astype(np.int16)


# ------------------------------------------------------------------------------------------------
# power
# ------------------------------------------------------------------------------------------------
POWER_LENS = (1, 255, 256, 257, 16383, 16384, 16385, 40000)


def power_case(seed=11):
    """-> sig (int16 pool), segments [S, 4], tiles [T, 2] in a scrambled order, want [T] (Python integers), names [S].
    Segments at odd offsets with garbage between; an empty one in the middle; a full tile of -32768; two touching segments
    whose meeting samples are 32767 and -32768."""
    rng = np.random.default_rng(seed)
    data, names = [], []
    for n in POWER_LENS[:4]:
        data.append(_signal(rng, n))
        names.append("len%d" % n)
    data.append(np.zeros(0, np.int16))
    names.append("empty")
    for n in POWER_LENS[4:]:
        data.append(_signal(rng, n))
        names.append("len%d" % n)
    data.append(np.full(POWER_TILE, -32768, np.int16))
    names.append("all_min")
    a, b = np.full(300, 1000, np.int16), np.full(300, -7, np.int16)
    a[-1], b[0] = 32767, -32768
    data += [a, b]
    names += ["touch_a", "touch_b"]
    for d in data:                                         # the first and last sample of every run count
        if len(d):
            d[0] = d[0] if abs(int(d[0])) > 1000 else 32767
            d[-1] = d[-1] if abs(int(d[-1])) > 1000 else -32768
    off, offs = 3, []
    for i, d in enumerate(data):
        offs.append(off)
        off += len(d) + (0 if names[i] == "touch_a" else 5 + 2 * i)
    sig = np.full(off + 9, GARBAGE, np.int16)
    segments, tiles = [], []
    for s, (o, d) in enumerate(zip(offs, data)):
        sig[o:o + len(d)] = d
        t0 = list(range(0, len(d), POWER_TILE))
        segments.append((o, len(d), len(tiles), len(t0)))
        tiles += [(s, i0) for i0 in t0]
    tiles = np.array(tiles, np.int64)[scramble(len(tiles), seed)]
    want = []
    for s, i0 in tiles.tolist():
        d = data[s][i0:i0 + POWER_TILE]
        want.append(sum(int(v) * int(v) for v in d.tolist()))
    return sig, np.array(segments, np.int64), tiles, want, names


# ------------------------------------------------------------------------------------------------
# conv
# ------------------------------------------------------------------------------------------------
CONV_SHAPES = ((1, 1), (5, 3), (2048, 1), (2047, 2), (2049, 1024), (3000, 1025), (2100, 1030), (100, 2500), (700, 4100))
CONV_KINDS = ("full", "small")
SMALL = 16                                                 # |x|, |k| <= 16 in the small-integer data


def conv_small_cap(N, L):
    """|m| of an output m * 2^-15 of the small-integer data: at most min(N, L) products of at most 16 * 16."""
    return SMALL * SMALL * min(N, L)


def conv_tile_taps(N, L, n0):
    """(k_lo, k_hi): the taps that meet a sample of x for some output of the tile at n0 (n - k in [0, N), k in [0, L))."""
    return max(0, n0 - N + 1), min(L - 1, n0 + CONV_TILE - 1)


def _place(parts, start, gap):
    offs, off = [], start
    for i, p in enumerate(parts):
        offs.append(off)
        off += len(p) + gap + 2 * i
    return offs, off


def conv_case(kind, seed=23):
    """One launch: the nine shapes of CONV_SHAPES, each with its own x and taps, and three more jobs -- an early-window form
    (a sub-range of another job's taps on that job's x, y_off = -1), a second job on one x with other taps, and a sub-range of
    taps whose y is written.  -> dict: sig, k (int16 taps pool), taps (fp32 = k / 32768), jobs [J, 5], tiles [T, 2] scrambled,
    y_len (pool size), names [J], x [J], kk [J] (the int16 runs of each job), m [J] (int64: y = m * 2^-15)."""
    assert kind in CONV_KINDS
    rng = np.random.default_rng(seed + CONV_KINDS.index(kind))
    lim = 32767 if kind == "full" else SMALL
    xs = [_signal(rng, N, lim) for N, _ in CONV_SHAPES]
    ks = [_signal(rng, L, lim) for _, L in CONV_SHAPES]
    if kind == "full":                                     # the extremes, where products are largest
        for x, k in zip(xs, ks):
            x[0], k[-1] = -32768, -32768
            x[-1], k[0] = (32767, 32767) if len(x) > 1 and len(k) > 1 else (x[-1], k[0])
    x_offs, sig_len = _place(xs, 11, 3)
    k_offs, k_len = _place(ks, 5, 1)
    sig = np.full(sig_len + 7, GARBAGE, np.int16)
    kpool = np.full(k_len + 3, 16384, np.int16)            # 0.5 between the runs: a tap read too far changes the answer
    for o, x in zip(x_offs, xs):
        sig[o:o + len(x)] = x
    for o, k in zip(k_offs, ks):
        kpool[o:o + len(k)] = k
    spec = [("N%d_L%d" % s, i, k_offs[i], s[1], True) for i, s in enumerate(CONV_SHAPES)]      # name, x of, h_off, L, written
    spec.append(("early_of_2100_1030", 6, k_offs[6] + 37, 600, False))
    spec.append(("x_of_3000_taps_of_2049", 5, k_offs[4], 1024, True))
    spec.append(("subrange_of_700_4100", 8, k_offs[8] + 1000, 2100, True))
    jobs, tiles, names, jx, jk, jm = [], [], [], [], [], []
    y_off = 7
    for j, (name, xi, h_off, L, written) in enumerate(spec):
        x, k = xs[xi], kpool[h_off:h_off + L]
        ylen = len(x) + L - 1
        jobs.append((x_offs[xi], len(x), h_off, L, y_off if written else -1))
        tiles += [(j, n0) for n0 in range(0, ylen, CONV_TILE)]
        names.append(name)
        jx.append(x)
        jk.append(k.copy())
        jm.append(np.convolve(x.astype(np.int64), k.astype(np.int64)))
        if written:
            y_off += ylen + 13 + 2 * j
    tiles = np.array(tiles, np.int64)[scramble(len(tiles), seed)]
    return dict(sig=sig, k=kpool, taps=(kpool.astype(np.float64) / 32768.0).astype(F32), jobs=np.array(jobs, np.int64), tiles=tiles,
                y_len=y_off + 5, names=names, x=jx, kk=jk, m=jm)


def conv_fp32_case(seed=29):
    """(3000, 1025) with taps off the 2^-15 grid: arbitrary fp32 values.  -> sig, taps, jobs, tiles (scrambled), x, h, and the
    long double convolution with sum |h| |x| over each output's window (fp64)."""
    rng = np.random.default_rng(seed)
    N, L = 3000, 1025
    x = _signal(rng, N)
    h = (rng.standard_normal(L) * np.exp(-np.arange(L) / 300.0)).astype(F32)
    h[h == 0] = F32(0.25)
    sig = np.full(N + 40, GARBAGE, np.int16)
    sig[17:17 + N] = x
    taps = np.full(L + 20, 0.5, F32)
    taps[9:9 + L] = h
    ylen = N + L - 1
    tiles = np.array([(0, n0) for n0 in range(0, ylen, CONV_TILE)], np.int64)[scramble(2, seed)]
    ref = np.convolve(x.astype(LD), h.astype(LD))
    mag = np.convolve(np.abs(x.astype(np.float64)), np.abs(h.astype(np.float64)))
    return dict(sig=sig, taps=taps, jobs=np.array([(17, N, 9, L, 3)], np.int64), tiles=tiles, y_len=ylen + 11, x=x, h=h, ref=ref,
                mag=mag, bound=min(N, L) * 2.0 ** -53 * mag)


def conv_fraction(x, h, n):
    """Output n of the full convolution as a Fraction (x integers, h floats)."""
    return sum(Fr(int(x[n - k])) * Fr(float(h[k])) for k in range(max(0, n - len(x) + 1), min(len(h) - 1, n) + 1))


# ------------------------------------------------------------------------------------------------
# gains
# ------------------------------------------------------------------------------------------------
ORDER_TILES = (1e16, 1.0, -1e16, 1.0)                      # in order 1.0; pairwise or sorted anything else
SNRS = (10.0, 5.0, 0.0, 19.0, 13.0, 7.5, -3.25, 0.1)
GAINS_KINDS = ("pinned", "early", "no_early", "no_refs")


def scale_ld(snr, e, pn):
    """fp32 of a long double evaluation of sqrt(10^(-snr / 10) E / Pn); snr an fp32 value."""
    v = np.sqrt(np.power(LD(10), -LD(float(F32(snr))) / LD(10)) * LD(e) / LD(pn))
    return F32(v)


def scale_f64(snr, e, pn):
    return F32(np.sqrt(10.0 ** (-float(F32(snr)) / 10.0) * e / pn))


def gains_case(kinds, seed=31):
    """Utterances of the given kinds.  "pinned": its own segment and its early window hold ORDER_TILES (E = 1 / 4), and its
    references are the four built to be exact (snr 0, E / Pn = 1, 4, 1/4, 2^-20), an empty noise (NOISE_LEN = 0), a silent one
    and an ordinary one.  The others: one to four tiles of non-integer sums, with or without an early window, 0 to 3 references.
    -> dict of the tables, power_sumsq, conv_sumsq, and want: p0, e [U], ref_power [R], scale_ld [R], exact [R] (bool)."""
    rng = np.random.default_rng(seed + len(kinds))
    segs, psum, csum = [], [3.25], [0.125, 77.7]           # (tile sums start past a few entries nobody names)
    utt, refs, snr, exact = [], [], [], []

    def seg(values, ln):
        segs.append((int(rng.integers(0, 1000)), ln, len(psum), len(values)))
        psum.extend(values)
        return len(segs) - 1

    def some_tiles():
        return [float(v) for v in rng.uniform(1e3, 1e9, size=int(rng.integers(1, 5)))]

    for kind in kinds:
        d = np.zeros(UTT_FIELDS, np.int64)
        d[REF0] = len(refs)
        if kind == "pinned":
            d[N_] = 7
            d[X_SEG] = seg(list(ORDER_TILES), 7)
            d[EARLY_TILE0], d[EARLY_NTILES], d[EARLY_LEN] = len(csum), 4, 4
            csum.extend(ORDER_TILES)
            for pn_num, ln in ((1.0, 4), (0.5, 8), (4.0, 4), (2.0 ** 20, 4)):          # Pn = 1/4, 1/16, 1, 2^18
                refs.append((0, ln, 0, seg([pn_num / 2, pn_num / 2], ln)))
                snr.append(0.0)
                exact.append(True)
            refs.append((0, 0, 0, seg(some_tiles(), 0)))                               # empty: Pn = 0 whatever the tiles say
            refs.append((0, 100, 0, seg([0.0, 0.0], 100)))                             # silent
            refs.append((0, 1234, 0, seg(some_tiles(), 1234)))
            snr += [10.0, 5.0, 7.5]
            exact += [True, True, False]
        else:
            n = int(rng.integers(1, 50000))
            d[N_] = n
            d[X_SEG] = seg(some_tiles(), n)
            if kind != "no_early":
                t = some_tiles()
                d[EARLY_TILE0], d[EARLY_NTILES], d[EARLY_LEN] = len(csum), len(t), n + int(rng.integers(0, 500))
                csum.extend(t)
            for _ in range(0 if kind == "no_refs" else int(rng.integers(1, 4))):
                ln = int(rng.integers(1, 50000))
                refs.append((0, ln, 0, seg(some_tiles(), ln)))
                snr.append(SNRS[int(rng.integers(0, len(SNRS)))])
                exact.append(False)
        d[NREF] = len(refs) - d[REF0]
        utt.append(d)
    psum, csum = np.array(psum), np.array(csum)
    seg_sum = [seq_sum(psum[t0:t0 + nt]) for _, _, t0, nt in segs]
    p0, e = [], []
    for d in utt:
        p0.append(seg_sum[d[X_SEG]] / float(d[N_]))
        e.append(seq_sum(csum[d[EARLY_TILE0]:d[EARLY_TILE0] + d[EARLY_NTILES]]) / float(d[EARLY_LEN]) if d[EARLY_NTILES] else p0[-1])
    pn, sc, sc64 = [], [], []
    for u, d in enumerate(utt):
        for r in range(d[REF0], d[REF0] + d[NREF]):
            ln = refs[r][NOISE_LEN]
            p = seg_sum[refs[r][NOISE_SEG]] / float(ln) if ln > 0 else 0.0
            pn.append(p)
            sc.append(scale_ld(snr[r], e[u], p) if p > 0 else F32(0))
            sc64.append(scale_f64(snr[r], e[u], p) if p > 0 else F32(0))
    return dict(utt=np.stack(utt), refs=np.array(refs, np.int64).reshape(-1, REF_FIELDS), snr=np.array(snr, F32),
                segments=np.array(segs, np.int64), power_sumsq=psum, conv_sumsq=csum, kinds=list(kinds),
                want=dict(p0=np.array(p0), e=np.array(e), ref_power=np.array(pn), scale_ld=np.array(sc, F32),
                          scale_f64=np.array(sc64, F32), exact=np.array(exact, bool)))


def kinds_for(all_kinds, n_utts):
    """n_utts = 1: every kind in a launch of its own; else the kinds in rotation."""
    if n_utts == 1:
        return [[k] for k in all_kinds]
    return [[all_kinds[u % len(all_kinds)] for u in range(n_utts)]]


# ------------------------------------------------------------------------------------------------
# mix
# ------------------------------------------------------------------------------------------------
MIX_LENS = (1, 1023, 1024, 1025, 2500)
SCALES = (0.3, -1234.567, 17.25, 1e-3, -0.7071, 30000.334, 0.11)
# The pair whose order is pinned: after the long reference at 30000.334f has taken v to ~2^30 (fp64 steps of 2^-22) both products
# (steps of 2^-25 and 2^-24) are rounded as they are added, so (v + a) + b and (v + b) + a differ where the two roundings do.
BIG_SCALE, PAIR_SCALES = 30000.334, (0.3, -0.7071)


def mix_replay(v, noises, scales, offsets, skip=None, swap=None):
    """v (fp64, one utterance) plus the references in list order: v = v + fp64(scale) * fp64(noise), one rounding per add
    (the product of an fp32 and an int16 is exact).  swap = (i, j): those two references change places in the order."""
    v = np.array(v, np.float64)
    order = list(range(len(noises)))
    if swap:
        i, j = swap
        order[i], order[j] = order[j], order[i]
    n = np.arange(len(v))
    for r in order:
        j = n - offsets[r]
        ok = (j >= 0) & (j < len(noises[r]))
        v[ok] = v[ok] + np.float64(F32(scales[r])) * noises[r][j[ok]].astype(np.float64)
    return v


def mix_case(integers=False, seed=41):
    """Ten utterances with references (Y_LEN of MIX_LENS, RIR 0 and 1) and two without, at odd pool offsets.  Per utterance, in
    this order: a reference at offset 0 ending inside y (in mid-tile for the longer ones), one longer than y, one starting at
    Y_LEN and one past it (they add nothing), one at a negative OFFSET, and two over the same samples whose order changes the
    bits (pair = their positions in the list).  integers = True: |samples| <= 1024, scales +-2: every sum is exact.
    -> dict: sig, y0 (the y pool before: NaN outside RIR utterances), utt, refs, scale [R + 1], tiles scrambled, per utterance
    start (fp64), noises, scales, offsets; pair."""
    rng = np.random.default_rng(seed + int(integers))
    lim = 1024 if integers else 32767
    lens = [(n, r) for r in (0, 1) for n in MIX_LENS] + [(1500, 0), (1500, 1)]
    sig_parts, per = [], []
    for u, (ylen, rir) in enumerate(lens):
        x = _signal(rng, ylen, lim)
        if rir:
            start = _signal(rng, ylen, lim).astype(np.float64) if integers else rng.standard_normal(ylen) * 3000.0 + 1.0 / 3
        else:
            start = x.astype(np.float64)
        if u >= 2 * len(MIX_LENS):
            shapes = []
        else:
            third = max(1, ylen // 3)
            shapes = [(third, 0), (ylen + 100, ylen // 2), (50, ylen), (50, ylen + 77), (ylen // 2 + 9, -5),
                      (third, ylen // 4), (third, ylen // 4)]
        noises = [_signal(rng, ln, lim) for ln, _ in shapes]
        if integers:
            scales = [float(rng.choice((-2.0, 2.0))) for _ in shapes]
        else:
            scales = [SCALES[(u + i) % len(SCALES)] for i in range(len(shapes))]
            if shapes:
                scales[1], scales[-2:] = BIG_SCALE, list(PAIR_SCALES)
        per.append(dict(ylen=ylen, rir=rir, x=x, start=start, noises=noises, scales=scales, offsets=[o for _, o in shapes]))
        sig_parts += [x] + noises
    offs, total = _place(sig_parts, 13, 1)
    sig = np.full(total + 5, GARBAGE, np.int16)
    for o, p in zip(offs, sig_parts):
        sig[o:o + len(p)] = p
    utt, refs, scale, tiles = [], [], [], []
    y_off, si = 9, 0
    for u, p in enumerate(per):
        d = np.zeros(UTT_FIELDS, np.int64)
        d[X_OFF], d[N_], d[Y_OFF], d[Y_LEN], d[RIR] = offs[si], p["ylen"], y_off, p["ylen"], p["rir"]
        si += 1
        d[REF0], d[NREF] = len(refs), len(p["noises"])
        for nz, s, o in zip(p["noises"], p["scales"], p["offsets"]):
            refs.append((offs[si], len(nz), o, 0))
            scale.append(s)
            si += 1
        t = list(range(0, p["ylen"], ELEM_TILE))
        d[MIX_TILE0], d[MIX_NTILES] = len(tiles), len(t)
        tiles += [(u, n0) for n0 in t]
        utt.append(d)
        y_off += p["ylen"] + 3 + 2 * u
    y0 = np.full(y_off + 4, np.nan)
    for d, p in zip(utt, per):
        if p["rir"]:
            y0[d[Y_OFF]:d[Y_OFF] + p["ylen"]] = p["start"]
    tiles = np.array(tiles, np.int64)[scramble(len(tiles), seed)]
    return dict(sig=sig, y0=y0, utt=np.stack(utt), refs=np.array(refs, np.int64), scale=np.array(scale + [99.0], F32), tiles=tiles,
                per=per, pair=(5, 6))


# ------------------------------------------------------------------------------------------------
# level
# ------------------------------------------------------------------------------------------------
LEVEL_KINDS = ("volume", "no_normalize", "silent", "no_tiles", "negative_volume", "ratio1", "ratio4", "ratio_quarter", "ordinary",
               "ordinary_volume_zero")


def level_ld(p0, p1):
    return F32(np.sqrt(LD(p0) / LD(p1)))


def level_case(kinds, seed=53):
    """-> utt, utt_param [U, 2], mix_sumsq, p0 [U] (what utt_out[:, 0] holds going in), want p1 [U], level [U] (fp32), exact [U]."""
    rng = np.random.default_rng(seed + len(kinds))
    msum = [5.5, 1e9]
    utt, param, p0, p1, level, exact = [], [], [], [], [], []
    for kind in kinds:
        d = np.zeros(UTT_FIELDS, np.int64)
        ylen = int(rng.integers(1, 60000))
        t = [float(v) for v in rng.uniform(1e3, 1e9, size=int(rng.integers(1, 6)))]
        vol, norm, q0 = 0.0, 1.0, float(rng.uniform(1.0, 1e6))
        if kind == "volume":                               # the order-sensitive tiles; a volume wins over normalize
            t, ylen, vol = list(ORDER_TILES), 3, 0.1
        elif kind == "no_normalize":
            norm = 0.0
        elif kind == "silent":
            t = [0.0, 0.0, 0.0]
        elif kind == "no_tiles":
            t = []
        elif kind == "negative_volume":
            vol = -1.0
        elif kind.startswith("ratio"):                     # P1 = 24 exactly, P0 = 24 x the ratio
            t, ylen = [1000.5, 2000.25, 71.25], 128
            q0 = 24.0 * {"ratio1": 1.0, "ratio4": 4.0, "ratio_quarter": 0.25}[kind]
        d[Y_LEN], d[MIX_TILE0], d[MIX_NTILES] = ylen, len(msum), len(t)
        msum.extend(t)
        p = seq_sum(t) / float(ylen)
        if vol > 0:
            lv = F32(vol)
        elif norm != 0 and p > 0:
            lv = level_ld(q0, p)
        else:
            lv = F32(1)
        utt.append(d)
        param.append((vol, norm))
        p0.append(q0)
        p1.append(p)
        level.append(lv)
        exact.append(not kind.startswith("ordinary") and kind != "negative_volume")
    return dict(utt=np.stack(utt), param=np.array(param), mix_sumsq=np.array(msum + [123.0]), p0=np.array(p0), kinds=list(kinds),
                want=dict(p1=np.array(p1), level=np.array(level, F32), exact=np.array(exact, bool)))


# ------------------------------------------------------------------------------------------------
# write
# ------------------------------------------------------------------------------------------------
LEVELS = (F32(1.0), F32(0.5), F32(0.1))
# y x level -> (output, clipped) of aug_write_kernel's rule: trunc toward zero in fp64, saturated where the truncated value
# leaves [-32768, 32767]; NaN saturates low and counts
EDGES = ((32767.9, 32767, False), (32768.0, 32767, True), (-32768.5, -32768, False), (-32769.0, -32768, True), (0.5, 0, False),
         (-0.5, 0, False), (1.5, 1, False), (-1.5, -1, False), (float("nan"), -32768, True), (float("inf"), 32767, True),
         (float("-inf"), -32768, True))


def write_ref(y, level):
    """-> (value after truncation and saturation as fp64, clipped flags) of fp64 y times the fp32 level."""
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.asarray(y, np.float64) * np.float64(F32(level)))
        low = ~(t >= -32768.0)
        high = t > 32767.0
    return np.where(low, -32768.0, np.where(high, 32767.0, t)), low | high


def edge_y(target, level):
    """The fp64 y nearest target / level whose product with the level has the outcome EDGES lists for the target (exactly the
    target for the levels 1 and 0.5; for 0.1f the nearest product on the right side of the edge)."""
    if not np.isfinite(target):
        return target
    want = [e for e in EDGES if e[0] == target][0]
    y = np.float64(target) / np.float64(F32(level))
    cand = [y]
    lo = hi = y
    for _ in range(8):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cand += [lo, hi]
    good = []
    for c in cand:
        v, cl = write_ref(np.array([c]), level)
        if v[0] == want[1] and bool(cl[0]) == want[2]:
            good.append((abs(float(c) * float(F32(level)) - target), float(c)))
    return min(good)[1]


def write_case(seed=61):
    """Utterances (N, M, SHIFT, level): trim with a shift, M = N over two tiles, repeat (M = 3 N + 5) over three tiles, N = 1
    (M = 8 = 3 N + 5, nothing saturates), and a second trim.  y: non-integers that stay inside int16 after the level, the EDGES
    placed in every wave (threads 5, 70, 133, 200) and every pass (m = thread + 256 i) of two tiles of the longer utterances.
    -> y pool, utt, utt_out [U + 1, 4] (NaN but the level column), tiles scrambled (utterances interleaved), out_len, and per
    utterance want (fp64 values), nclip."""
    rng = np.random.default_rng(seed)
    shapes = [(2500, 1500, 321, LEVELS[2]), (1300, 1300, 0, LEVELS[1]), (700, 2105, 0, LEVELS[0]), (1, 8, 0, LEVELS[1]),
              (3000, 2049, 17, LEVELS[0])]
    utt, tiles, per = [], [], []
    y_off, out_off = 5, 3
    for u, (N, M, shift, level) in enumerate(shapes):
        ylen = N + shift + 11
        y = rng.uniform(-32000.0, 32000.0, size=ylen) / float(level)
        if N > 1:
            e = 0
            for tile in (0, 1):
                for i in range(4):
                    for thread in (5, 70, 133, 200):
                        m = ELEM_TILE * tile + thread + 256 * i
                        if m < min(N, M):
                            y[shift + m] = edge_y(EDGES[e % len(EDGES)][0], level)
                            e += 1
        else:
            y[shift] = edge_y(0.5, level)
        d = np.zeros(UTT_FIELDS, np.int64)
        d[N_], d[Y_OFF], d[Y_LEN], d[SHIFT], d[M_], d[OUT_OFF] = N, y_off, ylen, shift, M, out_off
        utt.append(d)
        tiles += [(u, m0) for m0 in range(0, M, ELEM_TILE)]
        want, cl = write_ref(y[shift + np.arange(M) % N], level)
        per.append(dict(y=y, level=level, want=want, nclip=int(cl.sum()), N=N, M=M))
        y_off += ylen + 7 + 2 * u
        out_off += M + 9 + 2 * u
    ypool = np.full(y_off + 3, 1e30)                       # between the utterances: anything read from there saturates
    for d, p in zip(utt, per):
        ypool[d[Y_OFF]:d[Y_OFF] + len(p["y"])] = p["y"]
    utt_out = np.full((len(utt) + 1, 4), np.nan)
    utt_out[:len(utt), 3] = [float(p["level"]) for p in per]
    tiles = np.array(tiles, np.int64)[scramble(len(tiles), seed)]
    return dict(y=ypool, utt=np.stack(utt), utt_out=utt_out, tiles=tiles, out_len=out_off + 6, per=per)


# ------------------------------------------------------------------------------------------------
# one utterance alone and in a batch
# ------------------------------------------------------------------------------------------------
def chain_case(alone, seed=71):
    """conv -> mix -> write tables for utterance "target" (N 3000, L 1025, two noises, a trim with a shift, level 0.37f) alone
    at the start of every pool, or as the third of four utterances at other offsets.  -> dict of tables (tiles scrambled) and
    target = its index; the target's own rows are found through its descriptor."""
    rng = np.random.default_rng(seed)
    target = dict(x=_signal(rng, 3000), k=_signal(rng, 1025), noises=[_signal(rng, 900), _signal(rng, 5000)], offsets=[100, 1500],
                  scales=[0.3, -1.7], shift=40, M=2900, level=F32(0.37))
    others = [dict(x=_signal(rng, n), k=_signal(rng, L), noises=[_signal(rng, 400)], offsets=[7], scales=[0.9], shift=0, M=n,
                   level=F32(0.5)) for n, L in ((1200, 300), (2500, 2100), (777, 5))]
    items = [target] if alone else others[:2] + [target] + others[2:]
    sig_parts = []
    for it in items:
        sig_parts += [it["x"]] + it["noises"]
    offs, total = _place(sig_parts, 0 if alone else 19, 0 if alone else 5)
    sig = np.full(total + 3, GARBAGE, np.int16)
    for o, p in zip(offs, sig_parts):
        sig[o:o + len(p)] = p
    kpool = np.concatenate([np.full(0 if alone else 7, 16384, np.int16)] + [it["k"] for it in items])
    utt, refs, scale, jobs, conv_tiles, mix_tiles, write_tiles, levels = [], [], [], [], [], [], [], []
    si, h_off, y_off, out_off = 0, 0 if alone else 7, 0 if alone else 33, 0 if alone else 21
    for u, it in enumerate(items):
        N, L = len(it["x"]), len(it["k"])
        ylen = N + L - 1
        d = np.zeros(UTT_FIELDS, np.int64)
        d[X_OFF], d[N_], d[Y_OFF], d[Y_LEN], d[RIR] = offs[si], N, y_off, ylen, 1
        si += 1
        jobs.append((d[X_OFF], N, h_off, L, y_off))
        conv_tiles += [(u, n0) for n0 in range(0, ylen, CONV_TILE)]
        d[REF0], d[NREF] = len(refs), len(it["noises"])
        for nz, o, s in zip(it["noises"], it["offsets"], it["scales"]):
            refs.append((offs[si], len(nz), o, 0))
            scale.append(s)
            si += 1
        d[SHIFT], d[M_], d[OUT_OFF] = it["shift"], it["M"], out_off
        mix_tiles += [(u, n0) for n0 in range(0, ylen, ELEM_TILE)]
        write_tiles += [(u, m0) for m0 in range(0, it["M"], ELEM_TILE)]
        levels.append(float(it["level"]))
        utt.append(d)
        h_off += L
        y_off += ylen + (0 if alone else 3)
        out_off += it["M"] + (0 if alone else 5)
    utt_out = np.full((len(items), 4), np.nan)
    utt_out[:, 3] = levels

    def sc(t, s):
        t = np.array(t, np.int64)
        return t[scramble(len(t), s)]
    return dict(sig=sig, taps=(kpool.astype(np.float64) / 32768.0).astype(F32), jobs=np.array(jobs, np.int64),
                conv_tiles=sc(conv_tiles, seed + int(alone)), utt=np.stack(utt), refs=np.array(refs, np.int64),
                scale=np.array(scale, F32), mix_tiles=sc(mix_tiles, seed + 2 + int(alone)),
                write_tiles=sc(write_tiles, seed + 4 + int(alone)), utt_out=utt_out, y_len=y_off + 2, out_len=out_off + 2,
                target=0 if alone else 2)
