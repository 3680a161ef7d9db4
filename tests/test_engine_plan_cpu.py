"""The host side of the f16bf8 route, without a GPU: the probe ladder of engine.select_model against a scripted stand-in for
DeviceModel (which models are built and probed, in which order, what comes back and the whole selection report -- the expected
table was recorded from the three hand-written rungs the ladder's loop replaced), and engine.f16bf8_plan against a transcription of
the per-batch conditionals it replaced."""
import itertools
import math

import numpy as np
import pytest

from xvector_amd import engine, hiplib

# ---- the ladder ----------------------------------------------------------------------------------------------------------------------
SWITCHES = ("fold_shift", "first_mx6", "layer_mx6")
LETTER = dict(fold_shift="F", first_mx6="1", layer_mx6="L")
# what the k-th f16bf8 candidate of a run measures against the bf16x3 twin: M misses the limit, P passes, C passes but left the fp16
# range; every (outcome, k) has a value of its own, so the report shows whose value landed under which key
BASE = dict(M=2.0 ** -14, P=2.0 ** -17, C=2.0 ** -18)
VAL = dict(("%s%d" % (o, k), BASE[o] * (1 + k / 4.0)) for o in BASE for k in range(4))
X_PASS, X_MISS = 2.0 ** -16, 2.0 ** -13                  # the exact rung's vector against the twin's: inside / outside PROBE_LIMIT_BF16X3
VAL.update(XP=X_PASS / math.sqrt(1 + X_PASS * X_PASS), XM=X_MISS / math.sqrt(1 + X_MISS * X_MISS))
assert max(VAL["P3"], VAL["C3"]) < engine.PROBE_LIMIT_F16BF8 < VAL["M0"] and VAL["XP"] < engine.PROBE_LIMIT_BF16X3 < VAL["XM"]


class _Script(object):
    """One run: which forms the checkpoint supports, the outcome of every f16bf8 candidate in build order, the exact rung's."""

    def __init__(self, supported, outcomes, exact):
        self.supported, self.outcomes, self.exact = supported, outcomes, exact
        self.built, self.probes, self.candidates = [], 0, 0


class _Status(object):
    def __init__(self):
        self.value = 0

    def item(self):
        return self.value

    def zero_(self):
        self.value = 0


class FakeModel(object):
    """DeviceModel as select_model sees it; ``weights`` is the _Script."""

    def __init__(self, weights, topo, device="cuda:0", embedding_index=0, precision="bf16x3", fold_shift=None, layer_mx6=None,
                 first_mx6=None):
        self.script, self.topo, self.device, self.embedding_index = weights, topo, device, embedding_index
        self.f16bf8 = precision == "f16bf8"
        self.arithmetic = precision
        for name, asked in (("fold_shift", fold_shift), ("first_mx6", first_mx6), ("layer_mx6", layer_mx6)):
            setattr(self, name, self.f16bf8 and name in weights.supported and asked is not False)
            assert not (asked and not getattr(self, name)), name
        self.feat_dim, self.in_dim, self.gap, self.align = 5, 8, 2, 8
        self.status = _Status()
        self._fallback = None
        self.forms = "".join(LETTER[s] for s in SWITCHES if getattr(self, s)) or "-"
        self.tag = self.forms if self.f16bf8 else precision
        if self.f16bf8:
            self.outcome, self.index = weights.outcomes[weights.candidates], weights.candidates
            weights.candidates += 1
        weights.built.append(self.tag)

    def probe_vectors(self, batch):
        self.script.probes += 1
        if self.f16bf8:
            self.status.value = int(self.outcome == "C")
            return np.array([[VAL["%s%d" % (self.outcome, self.index)], 1.0]])
        if self.arithmetic == "bf16x3":
            return np.array([[0.0, 1.0]])
        return np.array([[X_PASS if self.script.exact == "pass" else X_MISS, 1.0]])

    def fallback(self):
        if self._fallback is None:
            self._fallback = FakeModel(self.script, self.topo, self.device, self.embedding_index, "bf16x3")
        return self._fallback


def observe(monkeypatch, supported, asked, outcomes, exact):
    """(models built in order, probe forwards, the model that came back, selection less its constants) of one scripted run."""
    monkeypatch.setattr(engine, "DeviceModel", FakeModel)
    monkeypatch.delenv("XVECTOR_EXACT_RUNG", raising=False)
    script = _Script(supported, outcomes, exact)
    model = engine.select_model(script, {}, probe=True, **asked)
    sel = dict(model.selection)
    assert sel.pop("requested") == "f16bf8" and sel.pop("probed") is True and sel.pop("probe_frames") == 8 * 256
    assert sel.pop("f16bf8_limit") == engine.PROBE_LIMIT_F16BF8 and sel.pop("selected") == model.arithmetic
    if "bf16x3_vs_fp32" in sel:
        assert sel.pop("bf16x3_limit") == engine.PROBE_LIMIT_BF16X3 and sel.pop("exact_rung") == "fp32tc"
    else:
        assert "bf16x3_limit" not in sel and "exact_rung" not in sel
    if model.f16bf8:
        assert model.fallback().tag == "bf16x3"
    assert script.built.count("bf16x3") == 1                         # one twin, shared: never one per candidate
    return " ".join(script.built), script.probes, model.tag, sel


ALL = frozenset(SWITCHES)
CONFIGS = dict([("default", (ALL, {}))] +
               [("%s=False" % s, (ALL, {s: False})) for s in SWITCHES] +
               [("%s=True" % s, (ALL, {s: True})) for s in SWITCHES] +
               [("no %s" % s, (ALL - {s}, {})) for s in SWITCHES])
# outcomes of the f16bf8 candidates in build order (a run that ends sooner leaves the rest unread) / the exact rung's
PATTERNS = dict([("first passes", ("P", "pass"))] +
                [("passes at rung %d" % k, ("M" * k + "P", "pass")) for k in (1, 2, 3)] +
                [("clamped at rung %d" % k, ("M" * k + "CP", "pass")) for k in (0, 1, 2, 3)] +
                [("all miss -> bf16x3", ("MMMM", "pass")), ("all miss -> exact rung", ("MMMM", "miss"))])

# The selection report in the table's shorthand: ``layer=yes err=P1 folded=M0`` is {"layer_mx6": True, "f16bf8_vs_bf16x3": VAL["P1"],
# "folded_f16bf8_vs_bf16x3": VAL["M0"]} -- M0 the miss of candidate 0 -- and a key that is not named must be absent.
SHORT = dict(layer="layer_mx6", first="first_mx6", fold="fold_shift", err="f16bf8_vs_bf16x3", left="probe_left_fp16_range",
             folded="folded_f16bf8_vs_bf16x3", first_missed="first_mx6_f16bf8_vs_bf16x3", mx6_missed="mx6_f16bf8_vs_bf16x3",
             exact="bf16x3_vs_fp32")


def report(text):
    word = dict(VAL, yes=True, no=False)
    return dict((SHORT[k], word[v]) for k, v in (item.split("=") for item in text.split()))


# Recorded from select_model as it stood with its three hand-written rungs (the reference of this test, not the loop that replaced
# them): config -> pattern -> (models built in order: an f16bf8 candidate by its forms F / 1 / L, "-" for none; probe forwards; the
# model that came back; its selection report)
EXPECTED = {
    'default': {
        'first passes': ('F1L bf16x3', 2, 'F1L', 'layer=yes first=yes err=P0 left=no'),
        'passes at rung 1': ('F1L bf16x3 1L', 3, '1L', 'layer=yes first=yes fold=no err=P1 left=no folded=M0'),
        'passes at rung 2': ('F1L bf16x3 1L L', 4, 'L', 'layer=yes first=no fold=no err=P2 left=no folded=M0 first_missed=M1'),
        'passes at rung 3': ('F1L bf16x3 1L L -', 5, '-', 'layer=no first=no fold=no err=P3 left=no folded=M0 first_missed=M1 mx6_missed=M2'),
        'clamped at rung 0': ('F1L bf16x3 1L', 3, '1L', 'layer=yes first=yes fold=no err=P1 left=no folded=C0'),
        'clamped at rung 1': ('F1L bf16x3 1L L', 4, 'L', 'layer=yes first=no fold=no err=P2 left=no folded=M0 first_missed=C1'),
        'clamped at rung 2': ('F1L bf16x3 1L L -', 5, '-', 'layer=no first=no fold=no err=P3 left=no folded=M0 first_missed=M1 mx6_missed=C2'),
        'clamped at rung 3': ('F1L bf16x3 1L L - fp32tc', 6, 'bf16x3', 'layer=no first=no fold=no err=C3 left=yes folded=M0 first_missed=M1 mx6_missed=M2 exact=XP'),
        'all miss -> bf16x3': ('F1L bf16x3 1L L - fp32tc', 6, 'bf16x3', 'layer=no first=no fold=no err=M3 left=no folded=M0 first_missed=M1 mx6_missed=M2 exact=XP'),
        'all miss -> exact rung': ('F1L bf16x3 1L L - fp32tc', 6, 'fp32tc', 'layer=no first=no fold=no err=M3 left=no folded=M0 first_missed=M1 mx6_missed=M2 exact=XM'),
    },
    'fold_shift=False': {
        'first passes': ('1L bf16x3', 2, '1L', 'layer=yes first=yes err=P0 left=no'),
        'passes at rung 1': ('1L bf16x3 L', 3, 'L', 'layer=yes first=no err=P1 left=no first_missed=M0'),
        'passes at rung 2': ('1L bf16x3 L -', 4, '-', 'layer=no first=no err=P2 left=no first_missed=M0 mx6_missed=M1'),
        'passes at rung 3': ('1L bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 0': ('1L bf16x3 L', 3, 'L', 'layer=yes first=no err=P1 left=no first_missed=C0'),
        'clamped at rung 1': ('1L bf16x3 L -', 4, '-', 'layer=no first=no err=P2 left=no first_missed=M0 mx6_missed=C1'),
        'clamped at rung 2': ('1L bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no err=C2 left=yes first_missed=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 3': ('1L bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XP'),
        'all miss -> bf16x3': ('1L bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XP'),
        'all miss -> exact rung': ('1L bf16x3 L - fp32tc', 5, 'fp32tc', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XM'),
    },
    'first_mx6=False': {
        'first passes': ('FL bf16x3', 2, 'FL', 'layer=yes first=no err=P0 left=no'),
        'passes at rung 1': ('FL bf16x3 L', 3, 'L', 'layer=yes first=no fold=no err=P1 left=no folded=M0'),
        'passes at rung 2': ('FL bf16x3 L -', 4, '-', 'layer=no first=no fold=no err=P2 left=no folded=M0 mx6_missed=M1'),
        'passes at rung 3': ('FL bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 0': ('FL bf16x3 L', 3, 'L', 'layer=yes first=no fold=no err=P1 left=no folded=C0'),
        'clamped at rung 1': ('FL bf16x3 L -', 4, '-', 'layer=no first=no fold=no err=P2 left=no folded=M0 mx6_missed=C1'),
        'clamped at rung 2': ('FL bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=C2 left=yes folded=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 3': ('FL bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XP'),
        'all miss -> bf16x3': ('FL bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XP'),
        'all miss -> exact rung': ('FL bf16x3 L - fp32tc', 5, 'fp32tc', 'layer=no first=no fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XM'),
    },
    'layer_mx6=False': {
        'first passes': ('F1 bf16x3', 2, 'F1', 'layer=no first=yes err=P0 left=no'),
        'passes at rung 1': ('F1 bf16x3 1', 3, '1', 'layer=no first=yes fold=no err=P1 left=no folded=M0'),
        'passes at rung 2': ('F1 bf16x3 1 -', 4, '-', 'layer=no first=no fold=no err=P2 left=no folded=M0 first_missed=M1'),
        'passes at rung 3': ('F1 bf16x3 1 - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XP'),
        'clamped at rung 0': ('F1 bf16x3 1', 3, '1', 'layer=no first=yes fold=no err=P1 left=no folded=C0'),
        'clamped at rung 1': ('F1 bf16x3 1 -', 4, '-', 'layer=no first=no fold=no err=P2 left=no folded=M0 first_missed=C1'),
        'clamped at rung 2': ('F1 bf16x3 1 - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=C2 left=yes folded=M0 first_missed=M1 exact=XP'),
        'clamped at rung 3': ('F1 bf16x3 1 - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XP'),
        'all miss -> bf16x3': ('F1 bf16x3 1 - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XP'),
        'all miss -> exact rung': ('F1 bf16x3 1 - fp32tc', 5, 'fp32tc', 'layer=no first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XM'),
    },
    'fold_shift=True': {
        'first passes': ('F1L bf16x3', 2, 'F1L', 'layer=yes first=yes err=P0 left=no'),
        'passes at rung 1': ('F1L bf16x3 FL', 3, 'FL', 'layer=yes first=no err=P1 left=no first_missed=M0'),
        'passes at rung 2': ('F1L bf16x3 FL F', 4, 'F', 'layer=no first=no err=P2 left=no first_missed=M0 mx6_missed=M1'),
        'passes at rung 3': ('F1L bf16x3 FL F fp32tc', 5, 'bf16x3', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 0': ('F1L bf16x3 FL', 3, 'FL', 'layer=yes first=no err=P1 left=no first_missed=C0'),
        'clamped at rung 1': ('F1L bf16x3 FL F', 4, 'F', 'layer=no first=no err=P2 left=no first_missed=M0 mx6_missed=C1'),
        'clamped at rung 2': ('F1L bf16x3 FL F fp32tc', 5, 'bf16x3', 'layer=no first=no err=C2 left=yes first_missed=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 3': ('F1L bf16x3 FL F fp32tc', 5, 'bf16x3', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XP'),
        'all miss -> bf16x3': ('F1L bf16x3 FL F fp32tc', 5, 'bf16x3', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XP'),
        'all miss -> exact rung': ('F1L bf16x3 FL F fp32tc', 5, 'fp32tc', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XM'),
    },
    'first_mx6=True': {
        'first passes': ('F1L bf16x3', 2, 'F1L', 'layer=yes first=yes err=P0 left=no'),
        'passes at rung 1': ('F1L bf16x3 1L', 3, '1L', 'layer=yes first=yes fold=no err=P1 left=no folded=M0'),
        'passes at rung 2': ('F1L bf16x3 1L 1', 4, '1', 'layer=no first=yes fold=no err=P2 left=no folded=M0 mx6_missed=M1'),
        'passes at rung 3': ('F1L bf16x3 1L 1 fp32tc', 5, 'bf16x3', 'layer=no first=yes fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 0': ('F1L bf16x3 1L', 3, '1L', 'layer=yes first=yes fold=no err=P1 left=no folded=C0'),
        'clamped at rung 1': ('F1L bf16x3 1L 1', 4, '1', 'layer=no first=yes fold=no err=P2 left=no folded=M0 mx6_missed=C1'),
        'clamped at rung 2': ('F1L bf16x3 1L 1 fp32tc', 5, 'bf16x3', 'layer=no first=yes fold=no err=C2 left=yes folded=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 3': ('F1L bf16x3 1L 1 fp32tc', 5, 'bf16x3', 'layer=no first=yes fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XP'),
        'all miss -> bf16x3': ('F1L bf16x3 1L 1 fp32tc', 5, 'bf16x3', 'layer=no first=yes fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XP'),
        'all miss -> exact rung': ('F1L bf16x3 1L 1 fp32tc', 5, 'fp32tc', 'layer=no first=yes fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XM'),
    },
    'layer_mx6=True': {
        'first passes': ('F1L bf16x3', 2, 'F1L', 'layer=yes first=yes err=P0 left=no'),
        'passes at rung 1': ('F1L bf16x3 1L', 3, '1L', 'layer=yes first=yes fold=no err=P1 left=no folded=M0'),
        'passes at rung 2': ('F1L bf16x3 1L L', 4, 'L', 'layer=yes first=no fold=no err=P2 left=no folded=M0 first_missed=M1'),
        'passes at rung 3': ('F1L bf16x3 1L L fp32tc', 5, 'bf16x3', 'layer=yes first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XP'),
        'clamped at rung 0': ('F1L bf16x3 1L', 3, '1L', 'layer=yes first=yes fold=no err=P1 left=no folded=C0'),
        'clamped at rung 1': ('F1L bf16x3 1L L', 4, 'L', 'layer=yes first=no fold=no err=P2 left=no folded=M0 first_missed=C1'),
        'clamped at rung 2': ('F1L bf16x3 1L L fp32tc', 5, 'bf16x3', 'layer=yes first=no fold=no err=C2 left=yes folded=M0 first_missed=M1 exact=XP'),
        'clamped at rung 3': ('F1L bf16x3 1L L fp32tc', 5, 'bf16x3', 'layer=yes first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XP'),
        'all miss -> bf16x3': ('F1L bf16x3 1L L fp32tc', 5, 'bf16x3', 'layer=yes first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XP'),
        'all miss -> exact rung': ('F1L bf16x3 1L L fp32tc', 5, 'fp32tc', 'layer=yes first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XM'),
    },
    'no fold_shift': {
        'first passes': ('1L bf16x3', 2, '1L', 'layer=yes first=yes err=P0 left=no'),
        'passes at rung 1': ('1L bf16x3 L', 3, 'L', 'layer=yes first=no err=P1 left=no first_missed=M0'),
        'passes at rung 2': ('1L bf16x3 L -', 4, '-', 'layer=no first=no err=P2 left=no first_missed=M0 mx6_missed=M1'),
        'passes at rung 3': ('1L bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 0': ('1L bf16x3 L', 3, 'L', 'layer=yes first=no err=P1 left=no first_missed=C0'),
        'clamped at rung 1': ('1L bf16x3 L -', 4, '-', 'layer=no first=no err=P2 left=no first_missed=M0 mx6_missed=C1'),
        'clamped at rung 2': ('1L bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no err=C2 left=yes first_missed=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 3': ('1L bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XP'),
        'all miss -> bf16x3': ('1L bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XP'),
        'all miss -> exact rung': ('1L bf16x3 L - fp32tc', 5, 'fp32tc', 'layer=no first=no err=M2 left=no first_missed=M0 mx6_missed=M1 exact=XM'),
    },
    'no first_mx6': {
        'first passes': ('FL bf16x3', 2, 'FL', 'layer=yes first=no err=P0 left=no'),
        'passes at rung 1': ('FL bf16x3 L', 3, 'L', 'layer=yes first=no fold=no err=P1 left=no folded=M0'),
        'passes at rung 2': ('FL bf16x3 L -', 4, '-', 'layer=no first=no fold=no err=P2 left=no folded=M0 mx6_missed=M1'),
        'passes at rung 3': ('FL bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 0': ('FL bf16x3 L', 3, 'L', 'layer=yes first=no fold=no err=P1 left=no folded=C0'),
        'clamped at rung 1': ('FL bf16x3 L -', 4, '-', 'layer=no first=no fold=no err=P2 left=no folded=M0 mx6_missed=C1'),
        'clamped at rung 2': ('FL bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=C2 left=yes folded=M0 mx6_missed=M1 exact=XP'),
        'clamped at rung 3': ('FL bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XP'),
        'all miss -> bf16x3': ('FL bf16x3 L - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XP'),
        'all miss -> exact rung': ('FL bf16x3 L - fp32tc', 5, 'fp32tc', 'layer=no first=no fold=no err=M2 left=no folded=M0 mx6_missed=M1 exact=XM'),
    },
    'no layer_mx6': {
        'first passes': ('F1 bf16x3', 2, 'F1', 'layer=no first=yes err=P0 left=no'),
        'passes at rung 1': ('F1 bf16x3 1', 3, '1', 'layer=no first=yes fold=no err=P1 left=no folded=M0'),
        'passes at rung 2': ('F1 bf16x3 1 -', 4, '-', 'layer=no first=no fold=no err=P2 left=no folded=M0 first_missed=M1'),
        'passes at rung 3': ('F1 bf16x3 1 - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XP'),
        'clamped at rung 0': ('F1 bf16x3 1', 3, '1', 'layer=no first=yes fold=no err=P1 left=no folded=C0'),
        'clamped at rung 1': ('F1 bf16x3 1 -', 4, '-', 'layer=no first=no fold=no err=P2 left=no folded=M0 first_missed=C1'),
        'clamped at rung 2': ('F1 bf16x3 1 - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=C2 left=yes folded=M0 first_missed=M1 exact=XP'),
        'clamped at rung 3': ('F1 bf16x3 1 - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XP'),
        'all miss -> bf16x3': ('F1 bf16x3 1 - fp32tc', 5, 'bf16x3', 'layer=no first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XP'),
        'all miss -> exact rung': ('F1 bf16x3 1 - fp32tc', 5, 'fp32tc', 'layer=no first=no fold=no err=M2 left=no folded=M0 first_missed=M1 exact=XM'),
    },
}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_ladder_builds_probes_and_reports_as_the_hand_written_rungs_did(monkeypatch, config):
    supported, asked = CONFIGS[config]
    assert list(EXPECTED[config]) == list(PATTERNS)
    for pattern, (outcomes, exact) in PATTERNS.items():
        got = observe(monkeypatch, supported, asked, outcomes, exact)
        want = EXPECTED[config][pattern]
        assert got[:3] == want[:3], (config, pattern)
        assert got[3] == report(want[3]), (config, pattern)                     # every key, and no other


def test_ladder_table_reaches_every_rung_from_both_sides():
    assert list(EXPECTED) == list(CONFIGS) and len(CONFIGS) == 10 and len(PATTERNS) == 10
    cases = [e for c in EXPECTED.values() for e in c.values()]
    assert "F1L bf16x3 1L L - fp32tc" in [e[0] for e in cases]                      # all three rungs miss, in their order
    for key in ("folded", "first_missed", "mx6_missed"):
        # each rung's miss path to both of its ends: the rung's candidate passes, and it misses too
        assert any(key + "=" in e[3] and e[2] not in ("bf16x3", "fp32tc") for e in cases), key
        assert any(key + "=" in e[3] and e[2] in ("bf16x3", "fp32tc") for e in cases), key
    assert EXPECTED["default"]["first passes"][:3] == ("F1L bf16x3", 2, "F1L")      # a model that passes at once: two small forwards


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
S3, S8, S6 = hiplib.FMT_SPLIT, hiplib.FMT_SPLIT8, hiplib.FMT_SPLIT6


def former_plan(n, pair, pair8, takes, first_mx6, layer_mx6):
    """The expressions f16bf8_plan replaced, transcribed: the two selection blocks of DeviceModel.__init__ and the conditionals of
    _frame_level_f16bf8.  (mx6_layers, first_mx6, launches [(layer, pack, format read, format written)]); None where __init__
    asserted the request out."""
    mx6_layers = set()
    if layer_mx6 is None or layer_mx6:
        for i in range(2, n - 2 if pair else n - 1):
            if takes(i) and takes(i - 1):
                mx6_layers.add(i)
    if layer_mx6 and not mx6_layers:
        return None
    first = False
    if (first_mx6 is None or first_mx6) and (n - 2 if pair else n - 1) > 1:
        if takes(1):
            first = True
    if first_mx6 and not first:
        return None
    stop = n - 2 if pair else n - 1
    pair_fmt = S8 if pair8 else S3
    h = pair_fmt if (pair and stop == 1) else S6 if first else S8
    launches = [(0, None, None, h)]
    for i in range(1, stop):
        y = pair_fmt if (pair and i == stop - 1) else S6 if i + 1 in mx6_layers else S8
        mx6 = i in mx6_layers or (i == 1 and first)
        launches.append((i, "wp6" if mx6 else "wp8", h, y))
        h = y
    return mx6_layers, first, launches


def test_plan_is_the_former_expressions_for_every_small_model():
    seen = set()
    cases = 0
    for n, (pair, pair8), first_mx6, layer_mx6 in itertools.product((3, 4, 5, 6), ((False, False), (True, False), (True, True)),
                                                                    (None, False, True), (None, False, True)):
        for pattern in itertools.product((False, True), repeat=n):
            takes = pattern.__getitem__
            want = former_plan(n, pair, pair8, takes, first_mx6, layer_mx6)
            if want is None:
                continue
            cases += 1
            mx6, fmts, packs = engine.f16bf8_plan(n, (S8 if pair8 else S3) if pair else None, takes, first_mx6, layer_mx6)
            stop = n - 2 if pair else n - 1
            assert len(fmts) == len(packs) == stop
            got = [(i, packs[i], fmts[i - 1] if i else None, fmts[i]) for i in range(stop)]
            # the public names as DeviceModel derives them from the one set
            assert (mx6 - {1}, 1 in mx6, got) == want, (n, pair, pair8, pattern, first_mx6, layer_mx6)
            # a producer and its consumer agree: 6-bit rows are read by the e2m3 pack and by nothing else
            assert all((read == S6) == (pack == "wp6") for i, pack, read, wrote in got[1:])
            assert (fmts[-1] == (S8 if pair8 else S3)) if pair else (fmts[-1] == S8)      # what the pair / the pooling launch reads
            seen.add(("e2m3", tuple(sorted(mx6))))
            if stop == 1:
                seen.add("stop == 1")
            if pair and stop - 1 in mx6:
                seen.add("e2m3 in front of the pair kernel")
            if pair and not pair8 and stop - 1 in mx6:
                seen.add("e2m3 writing bf16 split rows")
    # the enumeration holds what it is for
    assert {("e2m3", (1,)), ("e2m3", (2,)), ("e2m3", (1, 2)), ("e2m3", (2, 3)), ("e2m3", ()), "stop == 1", "e2m3 in front of the pair kernel",
            "e2m3 writing bf16 split rows"} <= seen
    assert cases > 2000


def test_plan_of_the_default_topology():
    """Five layers, K = 5 3 3 1 1 at 512 channels, the f16bf8 pair kernel: layers 1 and 2 on e2m3, layer 2 writes split8 for the pair."""
    mx6, fmts, packs = engine.f16bf8_plan(5, S8, lambda i: i in (1, 2))
    assert (mx6, fmts, packs) == ({1, 2}, [S6, S6, S8], [None, "wp6", "wp6"])
    assert engine.f16bf8_plan(5, S8, lambda i: i in (1, 2), first_mx6=False) == ({2}, [S8, S6, S8], [None, "wp8", "wp6"])
    assert engine.f16bf8_plan(5, S8, lambda i: i in (1, 2), layer_mx6=False) == ({1}, [S6, S8, S8], [None, "wp6", "wp8"])
    # layer 2 needs a producer that can write the 6-bit rows: the kernel form layer 1's shape selects, whatever layer 1 itself reads
    assert engine.f16bf8_plan(5, S8, lambda i: i == 2) == (set(), [S8, S8, S8], [None, "wp8", "wp8"])
