"""A long-lived context that grows, shrinks and grows again: each object makes a small call, a
larger call that reallocates its device buffers, then the small call again, and every result is
bit-exact against the CPU oracle's for the same inputs.  The sizes are the smallest that regrow a
buffer without a floor (the host-API staging and output arrays, the BLAT order and stage buffers) or
cross a floor (the chunk tables' 16, k_blat's 64 scratch slots)."""
import numpy as np
import pytest

import afpkg  # noqa: F401
import oracle
from cases import ragged, synthetic_pairs
from genome_world import make_genome, sample_pairs, sample_reads
from helpers import assert_records_equal
from oracle_backends import OracleTileReference

pytestmark = pytest.mark.gpu


def test_anchor_align_pairs_regrows(anchor):
    """8 pairs, 200 ragged pairs (the lengths buffer), 8 pairs: staging, the six output arrays and
    the packed CIGAR rows are reallocated by the second call."""
    from anchored_fusion_amd.align import AnchorAligner
    small = synthetic_pairs(anchor, 8, 100, seed=81)[0]
    large, lens = ragged(synthetic_pairs(anchor, 200, 100, seed=82)[0], 83)
    oidx = oracle.OracleIndex(anchor)
    with AnchorAligner(anchor, device=0) as al:
        got = []
        for reads, ln in ((small, None), (large, lens), (small, None)):
            g = al.align_pairs(reads, ln).as_dict()
            r = oidx.align_pairs(reads, ln, threads=8, chunk_bases=int(al.pe.chunk_bases))
            assert_records_equal(g, r, reads)
            got.append(g)
    assert_records_equal(got[2], got[0], small)
    assert int(((got[1]["flag"] & 4) == 0).sum()) > 100 and int(((got[0]["flag"] & 4) == 0).sum()) > 0


def _rec_equal(a, b, n):
    for k in range(n):
        x, y = a[k], b[k]
        for f in ("flag", "rid", "mrid", "pos", "mpos", "score", "n_cigar", "seq_b", "seq_e"):
            if int(x[f]) != int(y[f]):
                return f"record {k} field {f}: {int(x[f])} != {int(y[f])}"
        nc = int(x["n_cigar"])
        if not np.array_equal(x["cigar"][:nc], y["cigar"][:nc]):
            return f"record {k} cigar"
    return None


def _recs_equal(ro, no, rg, ng, what):
    assert np.array_equal(no, ng), what
    for r in range(len(no)):
        msg = _rec_equal(ro[r], rg[r], min(no[r], 8))
        assert msg is None, (what, r, msg)


def test_genome_align_regrows():
    """4 pairs at max_ins 500 in one chunk, 60 pairs at max_ins 4000 in 20 chunks of 3 pairs (past
    the chunk tables' floor of 16; a larger zero-filled histogram), the first call again, then 30
    single-end reads: staging, records, chunk tables and histogram are reallocated by the second call."""
    from anchored_fusion_amd import _lib
    from anchored_fusion_amd.genome import GenomeIndex
    contigs = make_genome()
    small, large = sample_pairs(contigs, 4, seed=91), sample_pairs(contigs, 60, seed=92)
    calls = [(small, dict(max_ins=500)), (large, dict(max_ins=4000, chunk_bases=900)), (small, dict(max_ins=500))]
    assert 2 * 60 * large.shape[1] // 900 >= 20
    og, gg = oracle.OracleGenome(contigs), GenomeIndex(contigs, device=0)
    try:
        for k, (reads, opt) in enumerate(calls):
            lens = np.full(reads.shape[0], reads.shape[1], np.int32)
            ro, no = og.align_pe(reads, lens, pe=oracle.default_pe(**opt), threads=8)
            rg, ng = gg.align_pe(reads, lens, pe=_lib.default_pe(**opt))
            _recs_equal(ro, no, rg, ng, f"align_pe call {k}")
            assert int(((rg[:, 0]["flag"] & 4) == 0).sum()) > len(reads) // 2  # most reads mapped
        reads, lens = sample_reads(contigs, 30, seed=93, chimeric=0.4)
        ro, no = og.align_se(reads, lens, threads=8)
        rg, ng = gg.align_se(reads, lens)
        _recs_equal(ro, no, rg, ng, "align_se")
        assert gg.stats()["cap_overflow"] == 0
    finally:
        gg.close()


def test_tile_search_regrows():
    """3 queries, 70 queries, 3 queries: k_blat's scratch goes from 64 slots to 192, the order and
    stage buffers are reallocated for 70 queries and again (smaller) for 3."""
    from anchored_fusion_amd import blat
    from test_gpu_blat import _queries, _world
    ctgs, rep = _world(13, n_ctg=2, ctg_len=200_000)
    qs = _queries(ctgs, rep, 5, n=70)
    p = blat.params("split_tail")
    g = blat.TileReference(ctgs, p.step_size)
    o = OracleTileReference(ctgs, p.step_size)
    try:
        total = 0
        for batch in (qs[:3], qs, qs[:3]):
            rg, ng = g.search(batch, p)
            ro, no = o.search(batch, p)
            assert np.array_equal(ng, no), (len(batch), np.nonzero(ng != no)[0][:10])
            for i in range(len(batch)):
                for k in range(ng[i]):
                    for f in blat.PSL_DTYPE.names:
                        assert np.array_equal(rg[i, k][f], ro[i, k][f]), (len(batch), i, k, f, rg[i, k][f], ro[i, k][f])
            assert g.caps() == o.caps(), len(batch)
            total += int(ng.sum())
        assert total > 0
    finally:
        g.close()
