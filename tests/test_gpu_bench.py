"""bench.py as a command on the GPU, at a reduced size (140 k pairs, the 2 % world): a plain run
times --steps steps and prints one result line without the --full legs, and --dump-outputs writes
the last step's outputs as float64 .npy files inside the byte budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu


def test_plain_run_and_dump(tmp_path):
    d = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(bench.ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--pairs", "140000", "--genome-scale", "0.02", "--dump-outputs", str(d)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["metric"] == "paired reads/sec through anchored split-read align"
    assert res["unit"] == "pairs/s" and res["higher_is_better"] is True and res["dtype"] == "int32"
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(140000 / (res["ms_per_step"] * 1e-3), rel=1e-3)
    assert "cpu_baseline" not in res and "issue_roofline" not in res
    files = sorted(os.listdir(d))
    arrs = {f[:-4]: np.load(d / f) for f in files}
    assert all(f.endswith(".npy") for f in files) and all(a.dtype == np.float64 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= bench.DUMP_BUDGET
    nq, n6, _ = (int(v) for v in arrs["counts"])
    c = res["counts_per_step"]
    assert (nq, n6) == (c["queries_s4_s5"], c["s6_queries"]) and nq > 0 and n6 > 0
    assert arrs["q_rows"].shape == arrs["q_nrec"].shape == (nq,)
    assert arrs["s6_src"].shape == arrs["s6_nrows"].shape == (n6,)
    assert int(arrs["q_nrec"].sum()) == c["genome_records"]
    assert int((arrs["s6_nrows"] > 0).sum()) == c["s6_placed"]
    # the sampled S2 records behind the queries: their read rows, a CIGAR wherever the read is mapped
    assert np.array_equal(arrs["s2q_rows"], arrs["q_rows"][arrs["grec_query"].astype(int)])
    mapped = (arrs["s2q_flag"].astype(np.int64) & 4) == 0
    assert mapped.any() and (arrs["s2q_cigar"][mapped, 0] > 0).all()
    assert (arrs["s2q_n_cigar"][mapped] > 0).all()
    # records and PSL rows: every query's live slots hold a record, the rest read 0
    live = np.arange(arrs["grec_flag"].shape[1])[None, :] < arrs["q_nrec"][arrs["grec_query"].astype(int)][:, None]
    assert not arrs["grec_n_cigar"][~live].any() and not arrs["grec_cigar"][~live].any()
    plive = np.arange(arrs["psl_score"].shape[1])[None, :] < arrs["s6_nrows"][arrs["psl_s6_query"].astype(int)][:, None]
    assert (arrs["psl_score"][plive] >= 20).all() and not arrs["psl_score"][~plive].any()
