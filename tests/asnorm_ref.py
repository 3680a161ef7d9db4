"""Test-side float64 reference of adaptive symmetric score normalisation (AS-norm), written from the definition:
top-N cohort statistics by a full sort, the normalised score, and the whole pipeline from raw vectors on top of backend_ref."""
import numpy as np

import backend_ref as ref


def topn_stats(scores, n):
    """scores[R, C] -> (mean[R], population std[R]) of the n largest values of each row, as a multiset, in float64."""
    top = np.sort(np.asarray(scores, dtype=np.float64), axis=1)[:, -n:]
    return top.mean(axis=1), top.std(axis=1, ddof=0)


def asnorm(s, mu_e, sd_e, mu_t, sd_t):
    """s' = 1/2 ((s - mu_e) / sd_e + (s - mu_t) / sd_t)."""
    return 0.5 * ((s - mu_e) / sd_e + (s - mu_t) / sd_t)


def pipeline(enrol, num_utts, test, cohort, mean, transform, plda, scoring, e_idx, t_idx, top_n):
    """Raw and AS-normalised scores of the trials (e_idx[i], t_idx[i]) in float64 from raw vectors.  plda = (m, P, psi) for
    scoring 'plda'; 'cosine' scores the cosine of the chain without the PLDA.  -> (s[M], s_norm[M], Se[Ne, Nc], St[Nt, Nc])."""
    if scoring == "plda":
        psi = plda[2]
        ze = ref.chain(enrol, mean, transform, True, plda, num_utts)
        zt = ref.chain(test, mean, transform, True, plda, None)
        zc = ref.chain(cohort, mean, transform, True, plda, None)
        E, r = ref.side_rows_enrol(ze, num_utts, psi)
        TE, rt = ref.side_rows_enrol(zt, np.ones(len(zt)), psi)          # the test vectors as one-utterance enrolments
        T, C = ref.side_rows_test(zt), ref.side_rows_test(zc)
    else:
        E = ref.side_rows_cosine(ref.chain(enrol, mean, transform, True))
        T = TE = ref.side_rows_cosine(ref.chain(test, mean, transform, True))
        C = ref.side_rows_cosine(ref.chain(cohort, mean, transform, True))
        r, rt = np.zeros(len(E)), np.zeros(len(T))
    s = np.einsum("ik,ik->i", E[e_idx], T[t_idx]) + r[e_idx]
    Se = E @ C.T + r[:, None]
    St = TE @ C.T + rt[:, None]
    mu_e, sd_e = topn_stats(Se, top_n)
    mu_t, sd_t = topn_stats(St, top_n)
    return s, asnorm(s, mu_e[e_idx], sd_e[e_idx], mu_t[t_idx], sd_t[t_idx]), Se, St
