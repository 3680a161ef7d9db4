"""AS-norm without a GPU: the float64 reference against a hand-computed example (with a tie at the top-N threshold), and the
score CLI's refusal of --cohort-top-n below 2 before it touches the device."""
import os
import subprocess
import sys

import numpy as np

import asnorm_ref
from conftest import ROOT, TWIN


def test_topn_stats_hand_computed():
    # row 0: top 3 of {5, 1, 5, 3, 5, 2} are 5, 5, 5 -> mean 5, std 0; top 4 add one 3 -> mean 4.5, std sqrt(0.75)
    # row 1: a tie at the threshold: top 3 of {4, 2, 2, 2, -1, 2} are 4, 2, 2 (two of the four 2s) -> mean 8/3,
    #        std sqrt(((4 - 8/3)^2 + 2 (2 - 8/3)^2) / 3) = sqrt(8/9)
    s = np.array([[5, 1, 5, 3, 5, 2], [4, 2, 2, 2, -1, 2]], np.float32)
    mu, sd = asnorm_ref.topn_stats(s, 3)
    assert np.allclose(mu, [5.0, 8.0 / 3.0], rtol=0, atol=1e-15) and np.allclose(sd, [0.0, np.sqrt(8.0 / 9.0)], rtol=0, atol=1e-15)
    mu, sd = asnorm_ref.topn_stats(s, 4)
    assert np.allclose(mu, [4.5, 2.5]) and np.allclose(sd, [np.sqrt(0.75), np.sqrt(0.75)])
    mu, sd = asnorm_ref.topn_stats(s, 6)
    assert np.allclose(mu, s.mean(axis=1)) and np.allclose(sd, s.astype(np.float64).std(axis=1))
    # s' = ((3 - 1) / 2 + (3 - 5) / 4) / 2 = 0.25
    assert asnorm_ref.asnorm(3.0, 1.0, 2.0, 5.0, 4.0) == 0.25


def test_score_cli_refuses_top_n_below_two(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "x-vector-kaldi-tf_amd"), TWIN] + [env.get("PYTHONPATH", "")])
    env["HIP_VISIBLE_DEVICES"] = "-1"                   # the refusal must come before any device is needed
    p = str(tmp_path)
    for n in ("1", "0"):
        res = subprocess.run([sys.executable, os.path.join(TWIN, "plda_backend.py"), "score", "--cohort", "scp:" + p + "/cohort.scp",
                              "--cohort-top-n", n, p + "/plda", "scp:" + p + "/e.scp", "scp:" + p + "/t.scp", p + "/trials",
                              p + "/scores"], env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode != 0
        assert "--cohort-top-n must be at least 2" in res.stderr, res.stderr
        assert not os.path.exists(p + "/scores")
