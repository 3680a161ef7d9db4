"""bench.py's command line: a plain run measures the headline alone, ``--full`` adds the rest of the line.  CPU only."""
import importlib.util
import os
import sys

from conftest import ROOT


def _parse(monkeypatch, *flags):
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(flags))
    return mod.parse()


def test_full_is_off_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.full is False and a.steps == 7 and a.warmup == 2 and a.gpus == 1 and a.dump_outputs is None


def test_full_keeps_the_sub_record_options(monkeypatch):
    a = _parse(monkeypatch, "--full", "--cpu-budget", "0", "--no-fp32-leg", "--no-extra-legs", "--e2e-utts", "0")
    assert a.full is True and a.cpu_budget == 0 and a.no_fp32_leg and a.no_extra_legs and a.e2e_utts == 0
