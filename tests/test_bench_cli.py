"""bench.py's command line and output dump (host only, no GPU)."""

import os
import sys

import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_measures_only_the_headline(monkeypatch):
    """without --full every sub-benchmark is off, whatever its own option says"""
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2", "--knn-q", "1024", "--pcie-steps", "4")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    assert (a.alt_steps, a.pcie_steps, a.knn_q, a.local_kpts, a.latency) == (0, 0, 0, 0, 0)
    assert a.extras is False and a.no_cpu_baseline is True


def test_full_run_keeps_every_sub_benchmark(monkeypatch):
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"
    assert (a.alt_steps, a.pcie_steps, a.knn_q, a.local_kpts, a.latency) == (10, 4, 1024, 2048, 1)
    assert a.extras is True and a.no_cpu_baseline is False
    a = _parse(monkeypatch, "--full", "--no-extras", "--knn-q", "0")
    assert a.extras is False and a.knn_q == 0


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_dtypes_and_size_cap(tmp_path, monkeypatch):
    """float32 stays float32, everything else becomes float64; an array over its share of
    the byte cap is cut to the same sorted sample of leading slices in every call"""
    g = torch.Generator().manual_seed(3)
    arrays = {"descriptors": torch.rand((64, 8), generator=g),
              "knn_scores": torch.rand((256, 10), generator=g, dtype=torch.float64),
              "knn_indices": torch.randint(0, 1000000, (256, 10), generator=g)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    got = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in arrays}
    assert got["descriptors"].dtype == np.float32 and got["knn_scores"].dtype == np.float64
    assert got["knn_indices"].dtype == np.float64
    for n, t in arrays.items():
        assert np.array_equal(got[n], t.numpy())
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 3 * 4096)       # 4096 bytes per array
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    cut = {n: np.load(str(tmp_path / "b" / (n + ".npy"))) for n in arrays}
    assert np.array_equal(cut["descriptors"], got["descriptors"])  # 2048 bytes: whole
    assert cut["knn_scores"].shape == (51, 10)                     # 4096 // 80 rows of 256
    rows = [int(np.flatnonzero((got["knn_scores"] == r).all(1))[0]) for r in cut["knn_scores"]]
    assert rows == sorted(rows) and len(set(rows)) == 51
    assert sum(os.path.getsize(str(tmp_path / "b" / f)) for f in os.listdir(str(tmp_path / "b"))) <= 3 * 4096 + 3 * 128
    for n in arrays:
        assert np.array_equal(cut[n], np.load(str(tmp_path / "c" / (n + ".npy"))))
