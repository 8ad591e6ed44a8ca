// bwa_mem_dev.h -- the one device copy of the bwa 0.7.17 mem routines that the anchor kernels
// (s2.hip) and the genome kernels (bwa_genome.hip) both run: klib's kbtree of chains, mem_chain's
// merge test and chain weight, the sort keys of the region lists, and the paired-end arithmetic
// (mem_pestat's helpers, mem_matesw's window and its ksw_align2, mem_pair).  oracle/bwa_pe.c is the
// bit-exact contract.  Each path supplies only what differs: where its scratch lives (a store, LDS
// pointers), how wide its index types are, and how a reference position is clipped (one half of
// the anchor's doubled text, or a contig of the genome).  Header-only, anonymous namespace.
#pragma once
#include "bwa_dev.h"

#pragma clang fp contract(off)

namespace {

// ---- klib kbtree (t = 5) over chain indices keyed by chain pos; lane 0 (oracle kb_*) -------
// A store holds the tree:
//   Idx, Pos         the integer types of node entries (chain and node indices) and of chain keys
//   DEPTH            the traversal's stack (levels of a full tree)
//   nd(i)            node i, a KbNode<Idx>
//   pos(x)           chain x's key
//   root(), set_root(i), alloc()   the root, and the index of a fresh node
//   full()           no room for one more insertion (which adds at most depth + 1 nodes)
constexpr int KB_T = 5, KB_MAXK = 2 * KB_T - 1;
template <class I>
struct KbNode { I n, internal, key[KB_MAXK], ptr[KB_MAXK + 1]; };

template <class Store>
__device__ __forceinline__ int kb_cmp(const Store &b, int x, typename Store::Pos kpos) {
    const typename Store::Pos a = b.pos(x);
    return (kpos < a) - (a < kpos);
}
template <class Store>
__device__ int kb_getp_aux(const Store &b, const KbNode<typename Store::Idx> &x, typename Store::Pos kpos, int *r) {
    int tr, *rr, begin = 0, end = x.n;
    if (x.n == 0) return -1;
    rr = r ? r : &tr;
    while (begin < end) {
        const int mid = (begin + end) >> 1;
        if (kb_cmp(b, x.key[mid], kpos) < 0) begin = mid + 1;
        else end = mid;
    }
    if (begin == x.n) { *rr = 1; return x.n - 1; }
    if ((*rr = -kb_cmp(b, x.key[begin], kpos)) < 0) --begin;
    return begin;
}
template <class Store>
__device__ int kb_new(Store &b, int internal) {
    const int zi = b.alloc();
    KbNode<typename Store::Idx> &z = b.nd(zi);
    z.n = 0; z.internal = (typename Store::Idx)internal;
    return zi;
}
// kb_intervalp: the chain with the largest key <= kpos (-1: none)
template <class Store>
__device__ int kb_lower(const Store &b, typename Store::Pos kpos) {
    int r = 0, lower = -1, xi = b.root();
    while (xi >= 0) {
        const KbNode<typename Store::Idx> &x = b.nd(xi);
        const int i = kb_getp_aux(b, x, kpos, &r);
        if (i >= 0 && r == 0) return x.key[i];
        if (i >= 0) lower = x.key[i];
        if (!x.internal) return lower;
        xi = x.ptr[i + 1];
    }
    return lower;
}
template <class Store>
__device__ void kb_split(Store &b, int xi, int i, int yi) {
    typedef typename Store::Idx I;
    const int zi = kb_new(b, b.nd(yi).internal);
    KbNode<I> &x = b.nd(xi), &y = b.nd(yi), &z = b.nd(zi);
    z.n = KB_T - 1;
    for (int u = 0; u < KB_T - 1; ++u) z.key[u] = y.key[KB_T + u];
    if (y.internal)
        for (int u = 0; u < KB_T; ++u) z.ptr[u] = y.ptr[KB_T + u];
    y.n = KB_T - 1;
    for (int u = x.n; u >= i + 1; --u) x.ptr[u + 1] = x.ptr[u];
    x.ptr[i + 1] = (I)zi;
    for (int u = x.n - 1; u >= i; --u) x.key[u + 1] = x.key[u];
    x.key[i] = y.key[KB_T - 1];
    ++x.n;
}
// kb_putp of chain k (its key is b.pos(k)); false, the tree unchanged, when the store is full
template <class Store>
__device__ bool kb_putp(Store &b, int k) {
    typedef typename Store::Idx I;
    const typename Store::Pos kpos = b.pos(k);
    int xi = b.root();
    if (b.full()) return false;
    if (b.nd(xi).n == KB_MAXK) {
        const int si = kb_new(b, 1);
        b.nd(si).ptr[0] = (I)xi;
        b.set_root(si);
        kb_split(b, si, 0, xi);
        xi = si;
    }
    for (;;) {  // __kb_putp_aux, iteratively
        KbNode<I> &x = b.nd(xi);
        if (!x.internal) {
            const int i = kb_getp_aux(b, x, kpos, nullptr);
            for (int u = x.n - 1; u >= i + 1; --u) x.key[u + 1] = x.key[u];
            x.key[i + 1] = (I)k;
            ++x.n;
            return true;
        }
        int i = kb_getp_aux(b, x, kpos, nullptr) + 1;
        if (b.nd(x.ptr[i]).n == KB_MAXK) {
            kb_split(b, xi, i, x.ptr[i]);
            if (kb_cmp(b, b.nd(xi).key[i], kpos) < 0) ++i;  // klib: cmp(*k, key[i]) > 0, k past the promoted key
        }
        xi = b.nd(xi).ptr[i];
    }
}
// in-order traversal into order[] (iterative): for a node, child[i] then key[i] for i < n, then
// child[n]; returns the key count
template <class Store, class O>
__device__ int kb_traverse(const Store &b, O *order) {
    int stk_node[Store::DEPTH], stk_i[Store::DEPTH], top = 1, n = 0;
    stk_node[0] = b.root(); stk_i[0] = 0;
    while (top > 0) {
        const int xi = stk_node[top - 1];
        const int i = stk_i[top - 1];
        const KbNode<typename Store::Idx> &x = b.nd(xi);
        if (!x.internal) {
            for (int u = 0; u < x.n; ++u) order[n++] = (O)x.key[u];
            --top;
            continue;
        }
        if (i > x.n) { --top; continue; }
        stk_i[top - 1] = i + 1;
        if (i > 0) order[n++] = (O)x.key[i - 1];
        stk_node[top] = x.ptr[i]; stk_i[top] = 0; ++top;
    }
    return n;
}
// test hook (af_debug_kbtree), lane 0: chains 0..n-1, their keys already in the store, inserted in
// turn into an empty tree; lower[i] = kb_lower of chain i's key before its insertion (-1 on the
// empty tree), then the traversal.  Returns the traversal's count, -1 when the store filled up.
template <class Store>
__device__ int kb_debug_fill(Store &b, int n, int32_t *lower, int32_t *order) {
    b.set_root(kb_new(b, 0));
    for (int i = 0; i < n; ++i) {
        lower[i] = i ? kb_lower(b, b.pos(i)) : -1;
        if (!kb_putp(b, i)) return -1;
    }
    return kb_traverse(b, order);
}

// ---- mem_chain ------------------------------------------------------------------------------
// test_and_merge's decision (oracle test_and_merge) for a new seed p against a chain's first and
// last seeds: p lies inside the chain, cannot join it, or is appended to it
enum { MERGE_NO = 0, MERGE_CONTAINED = 1, MERGE_APPEND = 2 };
template <class Seed>
__device__ __forceinline__ int chain_merge_test(const Seed &first, const Seed &last, const Seed &p, int64_t l_pac, int w,
                                                int max_chain_gap) {
    const int64_t qend = (int64_t)last.qbeg + last.len, rend = (int64_t)last.rbeg + last.len;
    if (p.qbeg >= first.qbeg && p.qbeg + p.len <= qend && p.rbeg >= first.rbeg && (int64_t)p.rbeg + p.len <= rend)
        return MERGE_CONTAINED;
    if ((last.rbeg < l_pac || first.rbeg < l_pac) && p.rbeg >= l_pac) return MERGE_NO;  // crosses the strand boundary
    const int64_t x = p.qbeg - last.qbeg, y = (int64_t)p.rbeg - last.rbeg;
    if (y >= 0 && x - y <= w && y - x <= w && x - last.len < max_chain_gap && y - last.len < max_chain_gap) return MERGE_APPEND;
    return MERGE_NO;
}

// mem_chain_weight over a chain's n seeds sd (oracle chain_weight)
template <class Seed>
__device__ int chain_weight(const Seed *sd, int n) {
    int64_t end = 0;
    int w = 0, tmp;
    for (int j = 0; j < n; ++j) {
        const Seed s = sd[j];
        if (s.qbeg >= end) w += s.len;
        else if (s.qbeg + s.len > end) w += (int)(s.qbeg + s.len - end);
        end = end > s.qbeg + s.len ? end : s.qbeg + s.len;
    }
    tmp = w; w = 0; end = 0;
    for (int j = 0; j < n; ++j) {
        const Seed s = sd[j];
        if (s.rbeg >= end) w += s.len;
        else if ((int64_t)s.rbeg + s.len > end) w += (int)((int64_t)s.rbeg + s.len - end);
        end = end > (int64_t)s.rbeg + s.len ? end : (int64_t)s.rbeg + s.len;
    }
    w = w < tmp ? w : tmp;
    return w < 1 << 30 ? w : (1 << 30) - 1;
}

// ---- region lists ---------------------------------------------------------------------------
// two query spans overlap by at least half of the shorter one (cal_sub, mem_mark_primary_se)
__device__ __forceinline__ bool q_overlap_half(int qb0, int qe0, int qb1, int qe1) {
    const int b_max = qb0 > qb1 ? qb0 : qb1;
    const int e_min = qe0 < qe1 ? qe0 : qe1;
    const int min_l = qe0 - qb0 < qe1 - qb1 ? qe0 - qb0 : qe1 - qb1;
    return e_min > b_max && (float)(e_min - b_max) >= (float)min_l * 0.5f;
}

// The region lists are sorted through small keys (each region's index with the fields its
// comparator reads): klib's introsort's swaps depend only on the comparator's answers, so the
// order, ties included, is the one the introsort over the regions themselves gives.
template <int SHIFT>
struct KeyRe {  // re << SHIFT | index (mem_sort_dedup_patch's sort by re)
    __device__ bool operator()(uint64_t a, uint64_t b) const { return (a >> SHIFT) < (b >> SHIFT); }
};
struct Key16 { int64_t x; int32_t y; int32_t z; };
template <int SHIFT>
struct KeyArs {  // x = rb, y = score, z = qb << SHIFT | index: score desc, rb, qb (LtArs)
    __device__ bool operator()(const Key16 &a, const Key16 &b) const {
        return a.y > b.y || (a.y == b.y && (a.x < b.x || (a.x == b.x && (a.z >> SHIFT) < (b.z >> SHIFT))));
    }
};
struct KeyHash {  // x = hash, y = score, z = index: score desc, hash (mem_mark_primary_se)
    __device__ bool operator()(const Key16 &a, const Key16 &b) const {
        return a.y > b.y || (a.y == b.y && (uint64_t)a.x < (uint64_t)b.x);
    }
};

// ---- mem_pestat's inputs --------------------------------------------------------------------
// the bwa chunk of pair pp
__device__ __forceinline__ int chunk_of(const S2Work &w, int64_t pp) {
    if (w.ppc) return (int)(pp / w.ppc);
    int lo = 0, hi = *w.n_chunks;  // cstart[lo] <= pp < cstart[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (w.cstart[mid] <= pp) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t *dist) {
    const int r1 = b1 >= l_pac, r2 = b2 >= l_pac;
    const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
    *dist = p2 > b1 ? p2 - b1 : b1 - p2;
    return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

// cal_sub (oracle cal_sub) over a region list
template <class Reg>
__device__ int cal_sub(const Reg *a, int n, int msl, int asc) {
    const int qb0 = a[0].qb, qe0 = a[0].qe;
    int j;
    for (j = 1; j < n; ++j)
        if (q_overlap_half(a[j].qb, a[j].qe, qb0, qe0)) break;
    return j < n ? a[j].score : msl * asc;
}

// ---- mem_matesw -----------------------------------------------------------------------------
constexpr int PE_TW = 2048;  // rescue windows up to this many bases are staged in LDS

// ksw_align2 with KSW_XSUBO | KSW_XSTART (oracle ksw_align2): score, te, qe and the start (tb, qb).
// rq2: LDS for the query's reversed prefix (the start pass)
__device__ void ksw_align2(const uint8_t *q, int qlen, const uint8_t *target, int tlen, int P, int minsc,
                           const af_params &p, uint8_t *rq2, int &score, int &te, int &qe, int &tb, int &qb, int lane) {
    const SwRes r = ksw_pass_any(q, qlen, target, tlen, -1, P, p, 0x10000, lane);
    score = r.score; te = r.te; qe = r.qe; tb = -1; qb = -1;
    if (r.score < minsc || r.qe < 0) return;
    for (int x = lane; x <= r.qe; x += 64) rq2[x] = q[r.qe - x];
    wave_sync();
    const SwRes rr = ksw_pass_any(rq2, r.qe + 1, target, tlen, r.te, P, p, r.score, lane);
    wave_sync();
    if (r.score == rr.score) { tb = r.te - rr.te; qb = r.qe - rr.qe; }
}

// the strand of direction r's rescue: the mate is searched reverse-complemented
__device__ __forceinline__ bool mate_is_rev(int r) { return (r >> 1) != (r & 1); }

// mem_matesw's window of direction r for a mate region starting at a_rb on reference a_rid (the
// rescued read l_ms long): [rb, re) within the doubled text, then clip(rb, re, rid) -- bwa's
// bns_fetch_seq -- narrows it to one reference and names it in rid.  True when bwa runs its SW.
template <class Clip>
__device__ __forceinline__ bool mate_window(int64_t l_pac, const af_params &p, const S2Pes &pe, int r, int64_t a_rb,
                                            int a_rid, int l_ms, int64_t &rb, int64_t &re, int &rid, Clip clip) {
    const bool is_rev = mate_is_rev(r);
    const bool is_larger = !(r >> 1);
    if (!is_rev) {
        rb = is_larger ? a_rb + pe.low : a_rb - pe.high;
        re = (is_larger ? a_rb + pe.high : a_rb - pe.low) + l_ms;
    } else {
        rb = (is_larger ? a_rb + pe.low : a_rb - pe.high) - l_ms;
        re = is_larger ? a_rb + pe.high : a_rb - pe.low;
    }
    if (rb < 0) rb = 0;
    if (re > l_pac << 1) re = l_pac << 1;
    if (rb < re) clip(rb, re, rid);
    // (rb >= re leaves rid from the previous direction, as bwa does; re - rb < min_seed_len then)
    return a_rid == rid && re - rb >= p.min_seed_len;
}

// that window's ksw_align2 for the rescued read's codes qc (strand of direction r) against the
// text T; rq (the query as searched), tw (the staged window) and rq2 are the wave's LDS
__device__ __forceinline__ void mate_ksw(const uint8_t *T, const af_params &p, const uint8_t *qc, int l_ms, int r,
                                         int64_t rb, int64_t re, uint8_t *rq, uint8_t *tw, uint8_t *rq2, int &sc, int &te,
                                         int &qe, int &tb, int &qb, int lane) {
    const bool is_rev = mate_is_rev(r);
    for (int x = lane; x < l_ms; x += 64) {
        const int c = qc[is_rev ? l_ms - 1 - x : x];
        rq[x] = (uint8_t)(is_rev ? (c < 4 ? 3 - c : 4) : c);
    }
    const bool staged = re - rb <= PE_TW;
    if (staged)
        for (int x = lane; x < (int)(re - rb); x += 64) tw[x] = T[rb + x];
    wave_sync();
    const int P = l_ms * p.a < 250 ? 16 : 8;
    ksw_align2(rq, l_ms, staged ? tw : T + rb, (int)(re - rb), P, p.min_seed_len * p.a, p, rq2, sc, te, qe, tb, qb, lane);
}

// the rescued region's spans from the window's SW result (mem_matesw's epilogue)
template <class Reg>
__device__ __forceinline__ void mate_region_span(Reg &b, int64_t l_pac, bool is_rev, int64_t rb, int l_ms, int te, int qe,
                                                 int tb, int qb) {
    b.qb = is_rev ? l_ms - (qe + 1) : qb;
    b.qe = is_rev ? l_ms - qb : qe + 1;
    b.rb = is_rev ? (l_pac << 1) - (rb + te + 1) : rb + tb;
    b.re = is_rev ? (l_pac << 1) - (rb + tb) : rb + te + 1;
}

// ---- mem_pair -------------------------------------------------------------------------------
struct P64 { uint64_t x, y; };
struct LtP64 {
    __device__ bool operator()(const P64 &a, const P64 &b) const { return a.x < b.x || (a.x == b.x && a.y < b.y); }
};
// mem_pair's key of region i (score, strand) of read r: x the region's strand-folded position, as
// each path orders references
__device__ __forceinline__ P64 mem_pair_key(uint64_t x, int score, int i, bool rev, int r) {
    return P64{x, (uint64_t)(uint32_t)score << 32 | (uint64_t)i << 2 | (uint64_t)rev << 1 | (uint64_t)r};
}
// the pair (entries k < i of the sorted keys, dist apart) as mem_pair ranks it: its score with the
// insert-size penalty, then the hash tie-break on the pair's id
__device__ __forceinline__ P64 mem_pair_score(const P64 &vi, const P64 &vk, int i, int k, int64_t dist, const S2Pes &pe,
                                              const af_params &p, int id) {
    const double ns = ((double)dist - pe.avg) / pe.std;
    int q = (int)((double)((vi.y >> 32) + (vk.y >> 32)) + .721 * log(2. * erfc(fabs(ns) * 0.70710678118654752440)) * p.a + .499);
    if (q < 0) q = 0;
    P64 u;
    u.y = (uint64_t)k << 32 | (uint64_t)i;
    u.x = (uint64_t)q << 32 | (hash_64(u.y ^ (uint64_t)(int64_t)(int32_t)((uint32_t)id << 8)) & 0xffffffffU);
    return u;
}
// the best pair's regions into z[] (by read); returns its score
__device__ __forceinline__ int mem_pair_pick(const P64 *v, const P64 &best, int z[2]) {
    const int i = (int)(best.y >> 32), k = (int)(best.y << 32 >> 32);
    z[v[i].y & 1] = (int)(v[i].y << 32 >> 34);
    z[v[k].y & 1] = (int)(v[k].y << 32 >> 34);
    return (int)(best.x >> 32);
}
// mem_pair (oracle mem_pair) over the nv keys v, lane 0: sorts them, scans bwa's way; the best
// pair's score (0 if none) and z[]
__device__ int mem_pair_scan(P64 *v, int nv, const S2Pes *pes, const af_params &p, int id, int z[2]) {
    ks_introsort(v, nv, LtP64());
    int y[4] = {-1, -1, -1, -1};
    bool have = false;
    P64 best{0, 0};
    for (int i = 0; i < nv; ++i) {
        for (int r = 0; r < 2; ++r) {
            const int dir = r << 1 | (int)(v[i].y >> 1 & 1);
            if (pes[dir].failed) continue;
            const int which = r << 1 | (int)((v[i].y & 1) ^ 1);
            if (y[which] < 0) continue;
            for (int k = y[which]; k >= 0; --k) {
                if ((int)(v[k].y & 3) != which) continue;
                const int64_t dist = (int64_t)v[i].x - (int64_t)v[k].x;
                if (dist > pes[dir].high) break;
                if (dist < pes[dir].low) continue;
                const P64 u = mem_pair_score(v[i], v[k], i, k, dist, pes[dir], p, id);
                if (!have || LtP64()(best, u)) { best = u; have = true; }
            }
        }
        y[v[i].y & 3] = i;
    }
    return have ? mem_pair_pick(v, best, z) : 0;
}

}  // namespace
