"""pipeline.run on the C1 world (tests/test_c1_pipeline.py) with its FASTQ pair rewritten as BGZF:
the device reader (gpu_ingest=True) and the host reader must lead to byte-identical tables, and
the log must say which reader ran."""
import gzip
import os

import pytest

import afpkg  # noqa: F401
import bgzf_cases as bc
from anchored_fusion_amd import pipeline
from test_c1_pipeline import PATHS

pytestmark = pytest.mark.gpu


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            if n.endswith(".txt"):
                p = os.path.join(d, n)
                out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_tables_equal_with_and_without_gpu_ingest(tmp_path):
    fq = [bc.write_bgzf(tmp_path / f"c1_{m}.fq.gz", gzip.open(PATHS[f"fq{m}"], "rb").read()) for m in (1, 2)]
    logs = {True: [], False: []}
    for on in (True, False):
        pipeline.run(PATHS["anchor"], fq[0], fq[1], PATHS["genome"], PATHS["gtf"], str(tmp_path / f"out_{on}"),
                     log=logs[on].append, gpu_ingest=on)
    dev, host = _files(tmp_path / "out_True"), _files(tmp_path / "out_False")
    assert sorted(dev) == sorted(host)
    assert any(k.endswith("BCR_fusion_predictions.txt") for k in dev)
    assert any(k.endswith("BCR_fusion_predictions_abridged.txt") for k in dev)
    for k in host:
        assert dev[k] == host[k], k
    assert any("device reader" in ln and "11258 pairs" in ln for ln in logs[True])
    assert not any("device reader" in ln for ln in logs[False])


def test_gpu_ingest_falls_back_on_plain_gzip(tmp_path):
    logs = []
    pipeline.run(PATHS["anchor"], PATHS["fq1"], PATHS["fq2"], PATHS["genome"], PATHS["gtf"], str(tmp_path / "out"),
                 log=logs.append, gpu_ingest=True)
    assert any("declined" in ln and "host reader" in ln for ln in logs)
    assert any(ln.startswith("ingest: 11258 pairs") for ln in logs)
    assert os.path.exists(tmp_path / "out" / "BCR_fusion" / "BCR_fusion_predictions.txt")
