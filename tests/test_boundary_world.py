"""The boundary world (tests/boundary_world.py) on the oracle alone: the reference engine
(oracle/bwa_pe.c, FM mode -- bntseq.c's rules restated literally) itself meets every condition
that tests/test_gpu_genome.py's boundary tests put on the GPU's records without going through the
oracle, and the world's reads do reach the rules it is built for."""
import numpy as np
import pytest

import afpkg  # noqa: F401
import boundary_world as bw
import oracle


@pytest.fixture(scope="module", params=["A", "B"])
def ow(request):
    w = bw.world(request.param)
    return w, oracle.OracleGenome(w.contigs)


def test_world_shape(ow):
    w, og = ow
    assert og.l_pac == w.l_pac == bw.L_PAC[w.variant] and w.n_ctg == 54
    assert int(w.off[2]) == bw.BKT and w.l_pac - 4 * bw.BKT == (w.variant == "B")
    # boundaries per bucket: one inside bucket 0 (65,466), 48 in bucket 1 (its first on the bucket's
    # first base), 4 in bucket 2, none from there on
    per = np.bincount(w.off[1:-1] >> 16, minlength=5)
    assert per.tolist() == [1, 48, 4, 0, 0]
    assert not (set(b"".join(s for _, s in w.contigs)) - set(b"ACGT"))
    # the planted stretches: one occurrence bridges a boundary, the copy lies inside one contig
    for (src, dst), flip in ((w.plant_a, False), (w.plant_b, True)):
        a, b = w.pac[src:src + bw.L], w.pac[dst:dst + bw.L]
        assert np.array_equal(bw.rc(a) if flip else a, b)
        assert int(w.intv2rid(src, src + bw.L)) == -1 and int(w.intv2rid(dst, dst + bw.L)) == bw.BIG


def test_builders_are_deterministic():
    for v in "AB":
        a, b = bw.World(v), bw.World(v)
        assert a.contigs == b.contigs
        ra, rb = bw.junction_reads(a), bw.junction_reads(b)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]
        pa, pb = bw.boundary_pairs(a), bw.boundary_pairs(b)
        assert np.array_equal(pa[0], pb[0]) and pa[1] == pb[1]
    assert bw.World("A").contigs != bw.World("B").contigs


def test_oracle_reads_stay_inside_their_contigs(ow):
    """Measured on the committed world (both variants alike): 2,914 reads, 188 of them error-free
    windows of one contig that occur once in T; 4,477 seed occurrences bridge a contig boundary and
    69 bridge l_pac (the floors below are half of that)."""
    w, og = ow
    reads, lens, meta = bw.junction_reads(w)
    assert len(meta) <= 3000 and sum(m["origin"] is not None for m in meta) >= 150
    recs, nrec = og.align_se(reads, lens, id_base=0, threads=8)
    bw.check_se_records(w, lens, meta, recs, nrec)
    n_ctg, n_strand = bw.bridging_counts(w, og, reads, lens)
    assert n_ctg >= 2238 and n_strand >= 34, (n_ctg, n_strand)
    # a read of a planted stretch: its bridging occurrence is dropped, the copy is kept
    for r, m in enumerate(meta):
        if m["kind"] == "planted":
            e = recs[r, 0]
            at = (w.plant_a if m["b"] == w.plant_a[0] else w.plant_b)[1] - int(w.off[bw.BIG])
            assert nrec[r] == 1 and (int(e["rid"]), int(e["pos"]), int(e["cigar"][0])) == (bw.BIG, at, bw.L << 4), m


def test_oracle_pairs_at_contig_ends(ow):
    """Measured: 992 pairs; 352 / 352 end and start pairs and 172 / 172 overhanging pairs proper in
    their contig with rescue on (the overhanging mate soft-clipped at the boundary) and 0 / 524 of
    their damaged mates mapped with it off; 84 / 84 clean spanning pairs on two contigs, none
    proper; 84 / 84 damaged spanning mates unmapped either way."""
    w, og = ow
    pairs, meta = bw.boundary_pairs(w)
    kinds = [m["kind"] for m in meta]
    assert (kinds.count("plain"), kinds.count("end") + kinds.count("start"),
            kinds.count("over_end") + kinds.count("over_start"), kinds.count("span"),
            kinds.count("span_damaged")) == (300, 352, 172, 84, 84)
    lens = np.full(len(pairs), bw.L, np.int32)
    for matesw in (50, 0):
        pe = oracle.default_pe()
        pe.max_matesw = matesw
        recs, nrec = og.align_pe(pairs, lens, pe=pe, pair_base=0, threads=8)
        bw.check_pe_records(w, meta, recs, nrec, matesw > 0)
        plain = [p for p, m in enumerate(meta) if m["kind"] == "plain"]
        assert all(int(recs[2 * p, 0]["flag"]) & 2 for p in plain)  # mem_pestat succeeded
