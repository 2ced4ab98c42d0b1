"""CPU: bench.py's command line - what a plain run leaves out, what --full brings back, --steps, --dump-outputs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

EXTRAS = ("no_cpu_baseline", "no_profile", "no_inflight", "no_extra")


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_measures_the_headline_only(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert all(getattr(a, k) for k in EXTRAS)


def test_full_run_keeps_the_extras_and_their_switches(monkeypatch):
    a = parse(monkeypatch, "--full")
    assert a.full and not any(getattr(a, k) for k in EXTRAS)
    a = parse(monkeypatch, "--full", "--no-cpu-baseline", "--no-inflight")
    assert a.no_cpu_baseline and a.no_inflight and not a.no_profile and not a.no_extra


def test_steps_below_one_are_refused(monkeypatch):
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--steps", "0")


def test_dump_outputs_writes_the_proof_bytes_exactly(tmp_path):
    proof = bytes(range(256)) * 3 + b"\x00\xff"
    bench.dump_outputs(str(tmp_path / "out"), proof)
    got = np.load(tmp_path / "out" / "proof.npy")
    assert got.dtype == np.float64 and got.shape == (len(proof),)
    assert bytes(got.astype(np.uint8)) == proof
