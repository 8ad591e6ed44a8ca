"""bench.py's host-side legs on CPU (the driver runs bench.py only on the GPU box): the configs[2]
CPU baseline (cpu_baseline_c3: the oracle over S2 + S3 + gathers + S4/S5 + S5 check + S6 on a
bounded sample) runs on a small fusion world and reports every stage, and genome_subset cuts the
gene loci +- flank out of a world's contigs."""
import types

import numpy as np
import pytest
import torch

import afpkg  # noqa: F401
import bench
from anchored_fusion_amd import io as afio
from anchored_fusion_amd import pipeline
from fusion_world import make_world


def test_cpu_baseline_c3_runs_every_stage(tmp_path):
    paths, _ = make_world(str(tmp_path / "w"), n_fusion=400, n_anchor=300, n_background=800)
    names, reads, lens = afio.read_pairs(paths["fq1"], paths["fq2"])
    subset = [(h.split()[0], s.upper()) for h, s in pipeline.read_fasta(paths["genome"])]
    anchor = afio.anchor_sequence(paths["anchor"])
    args = types.SimpleNamespace(cpu_sample=1000, cpu_seconds=0.5, cpu_threads=2)
    out = bench.cpu_baseline_c3(anchor, torch.from_numpy(reads), args, subset)
    assert out["value"] > 0 and out["cores"] == 2 and out["kind"] == "port"
    assert set(out["stages_s_per_pass"]) == {"s2_s3", "gather", "s4", "s5", "s5_check", "s6"}
    q = out["queries_per_pass"]
    assert q["s4_pairs"] > 0 and q["s5_split_reads"] > 0 and q["s6_queries"] > 0, q


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "1"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 1)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.steps == 12


def test_dump_helpers(tmp_path):
    # the sample is the same rows in every run, sorted, and every row when there are few
    s = bench._dump_sample(1_000_000, 4096)
    assert np.array_equal(s, bench._dump_sample(1_000_000, 4096))
    assert len(np.unique(s)) == 4096 and (np.diff(s) > 0).all() and 0 <= s[0] and s[-1] < 1_000_000
    assert np.array_equal(bench._dump_sample(5, 4096), np.arange(5))
    # slots past a row's live count read 0, scalar and sub-array fields alike
    dt = np.dtype([("a", "<i4"), ("b", "<i8", (3,))])
    rec = np.zeros((2, 4), dt)
    rec["a"], rec["b"] = 7, 2**40 + 1
    out = {}
    bench._dump_fields(rec, "r", np.array([1, 3]), out)
    assert out["r_a"].dtype == np.float64 and out["r_b"].shape == (2, 4, 3)
    assert out["r_a"].tolist() == [[7, 0, 0, 0], [7, 7, 7, 0]]
    assert (out["r_b"][1, :3] == 2**40 + 1).all() and not out["r_b"][1, 3].any() and not out["r_b"][0, 1:].any()
    bench._dump_write(str(tmp_path / "d"), out)
    assert np.array_equal(np.load(tmp_path / "d" / "r_b.npy"), out["r_b"])
    big = {"x": np.zeros(bench.DUMP_BUDGET // 8 + 1)}
    with pytest.raises(RuntimeError):
        bench._dump_write(str(tmp_path / "e"), big)


def test_genome_subset_windows():
    W = types.SimpleNamespace(names=["c1", "c2"], lens=[10_000, 5_000], offsets=[0, 10_512],
                              loci={"anchor": [("c1", 1000, 1200), ("c1", 3000, 3300)],
                                    "p0": [("c2", 4700, 4900)]})
    blob = np.frombuffer(b"A" * 10_000 + b"N" * 512 + b"C" * 5_000, np.uint8)
    W.blob = torch.from_numpy(blob.copy())
    sub = bench.genome_subset(W, flank=500)
    # the anchor's exons on c1 -> one window (500 .. 3800); the partner's on c2 clipped at its end
    assert [n for n, _ in sub] == ["c1:500-3800", "c2:4200-5000"]
    assert sub[0][1] == b"A" * 3300 and sub[1][1] == b"C" * 800
