"""A genome of many short contigs and reads at their ends (TEST INFRASTRUCTURE ONLY).

bwa joins the contigs without separators into pac and searches T = pac ++ revcomp(pac); bntseq.c's
rules keep every result inside one contig of one strand: a seed occurrence that bridges two contigs
(bns_intv2rid -1) or the strand boundary at l_pac (-2) is dropped, extension and mate-rescue windows
are clipped to one contig (bns_fetch_seq), and a record's contig is bns_pos2rid of its position.
The GPU answers bns_pos2rid from a table of one entry per 65,536-base bucket (fmindex.hip
k_ctg_bkt).  This world puts reads where those rules decide the answer:

- random ACGT, no N: the FASTA bytes are the index text, reads are cut from pac / T directly;
- contigs (in this order) of 65,466 and 70 bases (a boundary inside bucket 0, the next exactly on
  the bucket edge 65,536, a contig shorter than a read), of 1, 18, 19, 40, 150, 300 and 2,000
  bases, 40 of 500 bases (40 boundaries in one bucket), one of 70,000, then 1, 149 and 151 bases
  and a last one that brings l_pac to 262,144 (variant "A": the table's last bucket is full) or
  262,145 (variant "B": its last bucket holds one base).  Buckets 0..2 hold boundaries, bucket 3
  (and B's bucket 4) holds none;
- two 150-base stretches that span boundaries are planted again inside the 70,000-base contig
  (one as is, one reverse-complemented): a read of either has one occurrence that bridges (dropped)
  and one that is kept.

`junction_reads` (S5) and `boundary_pairs` (S4) return the reads and, per read / pair, what it is
(`meta`), which `check_se_records` / `check_pe_records` use to test the records of either engine
without reference to the other.
"""
import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
L = 150
BKT = 1 << 16
_HEAD = [65_466, 70, 1, 18, 19, 40, 150, 300, 2_000] + [500] * 40 + [70_000, 1, 149, 151]
L_PAC = {"A": 262_144, "B": 262_145}
BIG = 9 + 40               # the 70,000-base contig
JUNCTION_KS = (0, 1, 2, 18, 19, 20, 75, 130, 131, 132, 148, 149, 150)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return np.frombuffer(np.asarray(s, np.uint8)[::-1].tobytes().translate(_COMP), np.uint8)


def damaged(m):
    """A mismatch every 12 bases (no exact 19-mer is left: only mem_matesw can place the mate)."""
    m = m.copy()
    for k in range(6, len(m), 12):
        m[k] = ord("A") if m[k] != ord("A") else ord("G")
    return m


class World:
    def __init__(self, variant):
        self.variant = variant
        lens = _HEAD + [L_PAC[variant] - sum(_HEAD)]
        rng = np.random.default_rng(1000 + ord(variant))
        pac = ACGT[rng.integers(0, 4, sum(lens))]
        self.lens = np.asarray(lens, np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)  # n_ctg + 1 entries
        self.n_ctg = len(lens)
        self.l_pac = int(self.off[-1])
        big = int(self.off[BIG])
        self.plant_j = int(self.off[9 + 20])  # a junction among the 500-base contigs
        self.plant_a = (self.plant_j - 75, big + 20_000)
        self.plant_b = (65_466 - 60, big + 40_000)
        pac[self.plant_a[1]:self.plant_a[1] + L] = pac[self.plant_a[0]:self.plant_a[0] + L]
        pac[self.plant_b[1]:self.plant_b[1] + L] = rc(pac[self.plant_b[0]:self.plant_b[0] + L])
        self.pac = pac
        self.T = np.concatenate([pac, rc(pac)])
        self.contigs = [(f"c{k}", pac[self.off[k]:self.off[k + 1]].tobytes()) for k in range(self.n_ctg)]

    def rid_of(self, pos_f):
        """bns_pos2rid by plain search: the contig holding forward position pos_f."""
        return np.searchsorted(self.off[1:], pos_f, side="right")

    def depos(self, pos):
        pos = np.asarray(pos, np.int64)
        return np.where(pos >= self.l_pac, 2 * self.l_pac - 1 - pos, pos)

    def intv2rid(self, rb, re):
        """bns_intv2rid: -2 across l_pac, -1 across contigs."""
        rb, re = np.asarray(rb, np.int64), np.asarray(re, np.int64)
        a = self.rid_of(self.depos(rb))
        b = np.where(rb < re, self.rid_of(self.depos(re - 1)), a)
        return np.where((rb < self.l_pac) & (re > self.l_pac), -2, np.where(a == b, a, -1))

    def fetch_clip(self, beg, mid, end):
        """bns_fetch_seq's clip of [beg, end) to the contig (on its strand) holding mid."""
        beg, mid, end = (np.asarray(v, np.int64) for v in (beg, mid, end))
        beg, end = np.minimum(beg, end), np.maximum(beg, end)
        rid = self.rid_of(self.depos(mid))
        fb, fe = self.off[rid], self.off[rid + 1]
        rev = mid >= self.l_pac
        fb, fe = np.where(rev, 2 * self.l_pac - fe, fb), np.where(rev, 2 * self.l_pac - fb, fe)
        return np.maximum(beg, fb), np.minimum(end, fe), rid

    def locus(self, s, n, flip):
        """Where a read cut as T[s, s + n) (reverse-complemented when flip) lies: (forward start,
        on the reverse strand?)."""
        if s >= self.l_pac:
            return 2 * self.l_pac - (s + n), not flip
        return s, bool(flip)


_worlds = {}


def world(variant):
    if variant not in _worlds:
        _worlds[variant] = World(variant)
    return _worlds[variant]


def _subst(rng, s, rate):
    s = s.copy()
    m = rng.random(len(s)) < rate
    s[m] = ACGT[(np.searchsorted(ACGT, s[m]) + rng.integers(1, 4, int(m.sum()))) & 3]
    return s


def junction_reads(w, seed=3):
    """S5 reads around every boundary: (reads uint8 [n, 160] padded with N, lens, meta).  meta[r]:
    kind ("window" / "indel" / "clip" / "planted"), b (the boundary on T), k, flip, clean (no
    error put in), and for a window of one contig that occurs once in T its `origin` (rid, pos,
    reverse strand)."""
    rng = np.random.default_rng(seed)
    Tb = w.T.tobytes()
    N = 2 * w.l_pac
    out, meta = [], []
    bounds = [int(b) for b in w.off[1:-1]] + [w.l_pac]
    for b in bounds:
        for k in JUNCTION_KS:
            s = b - k
            if s < 0 or s + L > N:
                continue
            win = w.T[s:s + L]
            whole = s + L <= w.l_pac and int(w.rid_of(s)) == int(w.rid_of(s + L - 1)) or \
                s >= w.l_pac and int(w.rid_of(N - 1 - s)) == int(w.rid_of(N - s - L))
            once = whole and Tb.count(win.tobytes()) == 1 and Tb.count(rc(win).tobytes()) == 1
            for flip in (0, 1):
                r = rc(win) if flip else win
                origin = None
                if once:
                    f, rev = w.locus(s, L, flip)
                    rid = int(w.rid_of(f))
                    origin = (rid, f - int(w.off[rid]), rev)
                out.append(r)
                meta.append(dict(kind="window", b=b, k=k, flip=flip, clean=True, origin=origin))
                out.append(_subst(rng, r, 0.02))
                meta.append(dict(kind="window", b=b, k=k, flip=flip, clean=False, origin=None))
        # a 1-3-base indel within 10 bases of the boundary, on either side of it in turn
        s = b - 75
        win = w.T[s:s + L]
        n = int(rng.integers(1, 4))
        at = 75 + int(rng.integers(1, 11)) * (1 if rng.random() < 0.5 else -1)
        r = np.concatenate([win[:at], ACGT[rng.integers(0, 4, n)], win[at:]]) if rng.random() < 0.5 else \
            np.concatenate([win[:at], win[at + n:]])
        out.append(r)
        meta.append(dict(kind="indel", b=b, k=75, flip=0, clean=False, origin=None))
    # 30 random bases in front of a contig's first 120: a soft clip against the contig start
    for c in range(w.n_ctg):
        if w.lens[c] >= 120:
            s = int(w.off[c])
            out.append(np.concatenate([ACGT[rng.integers(0, 4, 30)], w.pac[s:s + 120]]))
            meta.append(dict(kind="clip", b=s, k=0, flip=0, clean=False, origin=None))
    # the planted stretches themselves (the second is no window of JUNCTION_KS)
    for src, _ in (w.plant_a, w.plant_b):
        for flip in (0, 1):
            win = w.pac[src:src + L]
            out.append(rc(win) if flip else win)
            meta.append(dict(kind="planted", b=src, k=0, flip=flip, clean=True, origin=None))
    reads = np.full((len(out), 160), ord("N"), np.uint8)
    lens = np.zeros(len(out), np.int32)
    for i, r in enumerate(out):
        reads[i, :len(r)] = r
        lens[i] = len(r)
    return reads, lens, meta


def boundary_pairs(w, seed=4, n_plain=300):
    """S4 pairs, pair-major [2 n, 150], and meta[pair]: kind ("plain" / "end" / "start" / "over_end" /
    "over_start" / "span" / "span_damaged"), contig c (span: the left one), d or x, and `bad`, the
    damaged mate (0 / 1) or None."""
    rng = np.random.default_rng(seed)
    pairs, meta = [], []
    large = [c for c in range(w.n_ctg) if w.lens[c] >= 60_000]
    for i in range(n_plain):  # the chunk's insert-size statistics
        c = large[i % len(large)]
        ins = 320 + int(rng.integers(-30, 31))
        a = int(w.off[c]) + int(rng.integers(500, w.lens[c] - 500 - ins))
        frag = w.pac[a:a + ins]
        pairs.append((frag[:L].copy(), rc(frag[-L:])))
        meta.append(dict(kind="plain", c=c, d=None, bad=None))
    for c in range(w.n_ctg):
        if w.lens[c] < 400:
            continue
        for d in (0, 1, 20, 100):
            e = int(w.off[c + 1]) - d
            frag = w.pac[e - 320:e]
            pairs.append((frag[:L].copy(), damaged(rc(frag[-L:]))))
            meta.append(dict(kind="end", c=c, d=d, bad=1))
            s = int(w.off[c]) + d
            frag = w.pac[s:s + 320]
            pairs.append((damaged(frag[:L]), rc(frag[-L:])))
            meta.append(dict(kind="start", c=c, d=d, bad=0))
        # overhanging pairs: the fragment runs d bases past the contig's end (or starts d bases before
        # its start), so the damaged mate's own locus crosses the boundary while the middle of its
        # rescue window lies inside the contig: the clip must stop the rescue at the boundary
        for d in (20, 40):
            if c + 1 < w.n_ctg:
                e = int(w.off[c + 1]) + d
                frag = w.pac[e - 320:e]
                pairs.append((frag[:L].copy(), damaged(rc(frag[-L:]))))
                meta.append(dict(kind="over_end", c=c, d=d, bad=1))
            if c > 0:
                s = int(w.off[c]) - d
                frag = w.pac[s:s + 320]
                pairs.append((damaged(frag[:L]), rc(frag[-L:])))
                meta.append(dict(kind="over_start", c=c, d=d, bad=0))
    for c in range(w.n_ctg - 1):
        if w.lens[c] < 200 or w.lens[c + 1] < 200:
            continue
        for x in (160, 200):
            s = int(w.off[c + 1]) - x
            frag = w.pac[s:s + 330]
            pairs.append((frag[:L].copy(), rc(frag[-L:])))
            meta.append(dict(kind="span", c=c, d=x, bad=None))
            pairs.append((frag[:L].copy(), damaged(rc(frag[-L:]))))
            meta.append(dict(kind="span_damaged", c=c, d=x, bad=1))
    return np.stack([r for p in pairs for r in p]), meta


# ---- checks of an engine's records that do not go through the other engine ----------------------
def _cigar_spans(rec):
    """(bases of the read the CIGAR covers, bases of the reference)."""
    q = t = 0
    for c in rec["cigar"][:int(rec["n_cigar"])]:
        n, op = int(c) >> 4, int(c) & 15
        if op in (0, 1, 4, 5):  # M I S H
            q += n
        if op in (0, 2):        # M D
            t += n
    return q, t


def _inside(w, rec, read_len, who):
    if int(rec["flag"]) & 4:
        return
    rid, pos = int(rec["rid"]), int(rec["pos"])
    assert 0 <= rid < w.n_ctg and pos >= 0, (who, rid, pos)
    q, t = _cigar_spans(rec)
    assert q == read_len, (who, "CIGAR covers", q, "of", read_len)
    assert pos + t <= int(w.lens[rid]), (who, "ends at", pos + t, "in a contig of", int(w.lens[rid]))


def check_se_records(w, lens, meta, recs, nrec):
    for r, m in enumerate(meta):
        who = (m["kind"], m["b"], m["k"], "flip" if m["flip"] else "as is", "clean" if m["clean"] else "errors")
        assert 1 <= nrec[r] <= recs.shape[1], (who, int(nrec[r]))
        for k in range(int(nrec[r])):
            _inside(w, recs[r, k], int(lens[r]), who)
        if m["origin"] is not None:
            rid, pos, rev = m["origin"]
            e = recs[r, 0]
            assert nrec[r] == 1, (who, "records", int(nrec[r]))
            got = (int(e["flag"]) & 4, int(e["rid"]), int(e["pos"]), bool(int(e["flag"]) & 16), int(e["n_cigar"]),
                   int(e["cigar"][0]))
            assert got == (0, rid, pos, rev, 1, L << 4), (who, got, m["origin"])


def check_pe_records(w, meta, recs, nrec, rescue):
    """rescue: mem_matesw on (max_matesw > 0)."""
    for p, m in enumerate(meta):
        who = (m["kind"], m["c"], m["d"])
        for i in (0, 1):
            assert 1 <= nrec[2 * p + i] <= recs.shape[1], (who, i)
            for k in range(int(nrec[2 * p + i])):
                _inside(w, recs[2 * p + i, k], L, who)
        f = [int(recs[2 * p + i, 0]["flag"]) for i in (0, 1)]
        if m["kind"] in ("end", "start", "over_end", "over_start"):
            if rescue:
                assert not (f[0] | f[1]) & 4 and f[0] & f[1] & 2, (who, "not rescued into a proper pair", f)
                rids = [int(recs[2 * p + i, 0]["rid"]) for i in (0, 1)]
                assert rids == [m["c"], m["c"]], (who, "contigs", rids)
            else:
                assert f[m["bad"]] & 4, (who, "the damaged mate is mapped without rescue", f)
        elif m["kind"] == "span":
            assert not (f[0] | f[1]) & 4, (who, "unmapped", f)
            assert int(recs[2 * p, 0]["rid"]) != int(recs[2 * p + 1, 0]["rid"]), (who, "one contig")
            assert not (f[0] | f[1]) & 2, (who, "proper across a boundary", f)
        elif m["kind"] == "span_damaged":
            assert f[1] & 4, (who, "rescued across a contig boundary", f)
            assert not (f[0] | f[1]) & 2, (who, "proper across a boundary", f)


def bridging_counts(w, og, reads, lens, max_occ=500):
    """Seed occurrences (mem_chain's walk over mem_collect_intv's intervals, those above max_occ
    skipped) that bridge a contig boundary and that bridge l_pac."""
    iv, niv = og.intervals(reads, lens, threads=8)
    sa = og.sa()
    n_ctg = n_strand = 0
    for r in range(len(niv)):
        for sa_k, s, qb, qe in iv[r, :max(int(niv[r]), 0)]:
            if s > max_occ:
                continue
            rb = sa[sa_k:sa_k + s]
            rid = w.intv2rid(rb, rb + (qe - qb))
            n_ctg += int((rid == -1).sum())
            n_strand += int((rid == -2).sum())
    return n_ctg, n_strand
