// inflate_core.h -- the raw-deflate decoder and CRC32 of the device ingest (ingest_dev.hip), one
// source for the GPU kernel and for the host test hook af_inflate_host.
//
// One BGZF member (a raw deflate stream of at most 64 KiB of output) is decoded by one wave:
//   * lane 0 runs inf_step, a resumable symbol decoder.  It writes literals (and stored bytes)
//     straight into the member's output window and queues each match as a token {at, len, dist};
//     it returns when the token ring is full, when it needs more input staged, when the stream
//     ends, or on an error;
//   * all 64 lanes then apply the queued matches in order (inf_apply_lane), restage input
//     (inf_refill_lane), and at the end compute the CRC32 in 64 chunks (inf_crc_lane) that are
//     combined with a multiply by x^(8 * bytes that follow) mod P.
// The host hook runs the same functions with a loop over 64 virtual lanes where the kernel has a
// barrier between the phases, so the table build, the decoder, the bounds checks, the overlapped
// copy and the CRC combination are the code the GPU runs.
//
// Bounds, by construction ("Device ingest"):
//   * input is read only through inf_refill_bits(): bytes at or past n_in read as zero, and a stream
//     that consumed more bits than the member holds ends with AF_INF_E_TRUNC;
//   * the window has AF_INF_WIN bytes and isize <= AF_INF_WIN is checked before anything runs;
//     a literal needs out_pos < isize and a match out_pos + len <= isize (AF_INF_E_OVER);
//   * a match needs dist <= out_pos (AF_INF_E_FAR), so no copy reads before the window;
//   * a code-length set that over-subscribes the code space, or is incomplete with codes longer
//     than one bit, is refused (AF_INF_E_CODES); an unassigned code is AF_INF_E_SYM.
// Every table and array that is indexed at run time lives in the caller's InfTables (LDS on the
// GPU), so the decoder needs no scratch memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AF_HD __host__ __device__
#else
#define AF_HD
#endif

constexpr int AF_INF_WIN = 65536;    // output window: the BGZF maximum
constexpr int AF_INF_RING = 4096;    // staged input bytes (a ring indexed by position)
constexpr int AF_INF_MARGIN = 1024;  // lane 0 asks for more input below this many staged bytes:
                                     // a dynamic block header is at most 563 bytes, a symbol 6,
                                     // and the bit buffer reads up to 8 bytes ahead
constexpr int AF_INF_TOK = 64;       // match tokens per round
constexpr int AF_INF_LANES = 64;
constexpr int AF_INF_FAST_L = 10;    // bits of the literal/length lookup table
constexpr int AF_INF_FAST_D = 8;     // bits of the distance (and code-length code) lookup table

enum {
    AF_INF_OK = 0,
    AF_INF_E_TRUNC = 1,   // the stream runs past the member's compressed bytes
    AF_INF_E_BTYPE = 2,   // block type 3
    AF_INF_E_STORED = 3,  // stored block: LEN != ~NLEN
    AF_INF_E_CODES = 4,   // over-subscribed or incomplete code lengths, bad counts, bad repeat
    AF_INF_E_SYM = 5,     // an unassigned code, or length symbol 286/287, distance symbol 30/31
    AF_INF_E_OVER = 6,    // output past ISIZE
    AF_INF_E_FAR = 7,     // a distance reaching before the member's output
    AF_INF_E_SHORT = 8,   // the stream ended before ISIZE bytes
    AF_INF_E_CRC = 9,
    AF_INF_E_ISIZE = 10,  // ISIZE above 64 KiB
};

enum { AF_INF_HEADER = 0, AF_INF_STORED = 1, AF_INF_CODED = 2, AF_INF_DONE = 3 };

// what the decoder met (af_inflate_host reports it, so a test can tell that its input reaches
// the case it names)
struct InfStats {
    int32_t stored, fixed, dynamic;  // deflate blocks by type
    int32_t max_code_len;            // the longest literal/length code defined
    int32_t max_dist;                // the largest match distance
    int32_t overlap;                 // matches with distance < length
    int32_t max_match;               // the longest match
};

struct InfTok {
    uint32_t at;         // window position of the first byte written
    uint16_t len, dist;  // 3..258, 1..32768
};

struct InfState {
    uint64_t bitbuf;
    int32_t nbits;
    int32_t pos;    // next input byte to enter bitbuf, a multiple of 4 (counts on past n_in: zeros)
    int32_t n_in;   // the member's compressed bytes
    int32_t fill;   // input bytes staged so far: the ring holds [fill - AF_INF_RING, fill)
    int32_t out_pos, isize;
    int32_t phase, final_blk, stored_left;
    int32_t err;
    int32_t ntok;
    InfStats st;
};

struct InfTables {
    uint16_t fast_l[1 << AF_INF_FAST_L];  // sym << 4 | code length; 0: longer than the table
    uint16_t fast_d[1 << AF_INF_FAST_D];
    uint16_t cnt_l[16], cnt_d[16];        // codes per length
    uint16_t sym_l[288], sym_d[32];       // symbols in canonical order
    uint16_t offs[16], next[16];          // table build work space
    uint8_t lens[320];                    // code lengths of a dynamic block (literal/length ++ distance)
    uint8_t cl[20];                       // lengths of the code-length code
};

AF_HD inline void inf_init(InfState &S, int32_t n_in, int32_t isize) {
    S.bitbuf = 0;
    S.nbits = 0;
    S.pos = 0;
    S.n_in = n_in;
    S.fill = 0;
    S.out_pos = 0;
    S.isize = isize;
    S.phase = AF_INF_HEADER;
    S.final_blk = 0;
    S.stored_left = 0;
    S.err = isize > AF_INF_WIN || isize < 0 ? AF_INF_E_ISIZE : AF_INF_OK;
    S.ntok = 0;
    S.st = InfStats{0, 0, 0, 0, 0, 0, 0};
}

// ---- input staging ------------------------------------------------------------------------
// how far the ring can be filled now: bytes before `pos` are in the bit buffer or consumed
AF_HD inline int32_t inf_fill_target(const InfState &S) {
    const int64_t t = (int64_t)S.pos + AF_INF_RING;
    return (int32_t)(t < S.n_in ? t : S.n_in);
}
// lane `lane` of AF_INF_LANES copies its share of src[fill, target) into the ring
AF_HD inline void inf_refill_lane(const InfState &S, int32_t target, const uint8_t *src, uint8_t *ring, int lane) {
    for (int32_t i = S.fill + lane; i < target; i += AF_INF_LANES) ring[i & (AF_INF_RING - 1)] = src[i];
}

// The bit buffer takes input a 32-bit word at a time (pos stays a multiple of 4, counted from the
// member's first byte, so the ring is read at aligned words): after a refill it holds at least 33
// bits.  The longest read between two refills is 32 bits (a stored block's LEN / NLEN); a
// literal/length code with its extra bits is at most 20, a distance code with its extra bits 28.
struct InfBits {
    uint64_t buf;
    int32_t n, pos;
};
AF_HD inline void inf_refill_bits(InfBits &b, const uint8_t *ring, int32_t n_in) {
    if (b.n > 32) return;
    uint32_t w;
    __builtin_memcpy(&w, __builtin_assume_aligned(ring + (b.pos & (AF_INF_RING - 1)), 4), 4);
    if (b.pos + 4 > n_in) w = b.pos >= n_in ? 0u : w & ((1u << (8 * (n_in - b.pos))) - 1);  // past the member: zero
    b.buf |= (uint64_t)w << b.n;
    b.n += 32;
    b.pos += 4;
}
AF_HD inline uint32_t inf_bits(InfBits &b, int k) {
    const uint32_t v = (uint32_t)(b.buf & ((1ull << k) - 1));
    b.buf >>= k;
    b.n -= k;
    return v;
}

// ---- Huffman tables -----------------------------------------------------------------------
// Canonical code of lens[0, n) (RFC 1951 3.2.2) into a `fbits`-bit lookup table plus the
// counts / sorted symbols that decode the longer codes.  Returns the longest code length, or -1
// when the lengths over-subscribe the code space or leave it incomplete (allowed only when no
// code is longer than one bit, and never when `strict`: the code-length code).
AF_HD inline int inf_build(const uint8_t *lens, int n, uint16_t *fast, int fbits, uint16_t *cnt, uint16_t *sym,
                           uint16_t *offs, uint16_t *next, bool strict) {
    for (int i = 0; i < 16; ++i) cnt[i] = 0;
    for (int i = 0; i < n; ++i) ++cnt[lens[i] & 15];
    cnt[0] = 0;
    int left = 1, maxlen = 0;
    for (int l = 1; l <= 15; ++l) {
        left = (left << 1) - (int)cnt[l];
        if (left < 0) return -1;
        if (cnt[l]) maxlen = l;
    }
    if (left > 0 && (strict || maxlen > 1)) return -1;
    uint32_t code = 0;
    offs[1] = 0;
    next[0] = 0;
    for (int l = 1; l <= 15; ++l) {
        code = (code + cnt[l - 1]) << 1;
        next[l] = (uint16_t)code;
        if (l < 15) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    }
    for (int i = 0; i < (1 << fbits); ++i) fast[i] = 0;
    for (int i = 0; i < n; ++i) {
        const int l = lens[i] & 15;
        if (!l) continue;
        sym[offs[l]++] = (uint16_t)i;
        const uint32_t c = next[l]++;
        if (l > fbits) continue;
        uint32_t rev = 0;  // the stream carries a code's bits most significant first
        for (int k = 0; k < l; ++k) rev |= ((c >> k) & 1u) << (l - 1 - k);
        for (uint32_t j = rev; j < (1u << fbits); j += 1u << l) fast[j] = (uint16_t)(i << 4 | l);
    }
    return maxlen;
}

// the next symbol of the code, or -1 for a bit pattern that no code has
AF_HD inline int inf_decode(InfBits &b, const uint16_t *fast, int fbits, const uint16_t *cnt, const uint16_t *sym) {
    const uint32_t e = fast[b.buf & ((1u << fbits) - 1)];
    if (e) {
        b.buf >>= e & 15;
        b.n -= e & 15;
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)((b.buf >> (l - 1)) & 1);
        const int count = cnt[l];
        if (code - count < first) {
            b.buf >>= l;
            b.n -= l;
            return sym[index + (code - first)];
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return -1;
}

AF_HD inline bool inf_fixed_tables(InfTables &T) {
    for (int i = 0; i < 288; ++i) T.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    for (int i = 0; i < 32; ++i) T.lens[288 + i] = 5;
    return inf_build(T.lens, 288, T.fast_l, AF_INF_FAST_L, T.cnt_l, T.sym_l, T.offs, T.next, false) >= 0 &&
           inf_build(T.lens + 288, 32, T.fast_d, AF_INF_FAST_D, T.cnt_d, T.sym_d, T.offs, T.next, false) >= 0;
}

// the header of a dynamic block (RFC 1951 3.2.7); 0 or an AF_INF_E_* code
AF_HD inline int inf_dynamic_tables(InfBits &b, const uint8_t *ring, int32_t n_in, InfTables &T, InfStats &st) {
    constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    inf_refill_bits(b, ring, n_in);
    const int hlit = (int)inf_bits(b, 5) + 257, hdist = (int)inf_bits(b, 5) + 1, hclen = (int)inf_bits(b, 4) + 4;
    if (hlit > 286 || hdist > 30) return AF_INF_E_CODES;
    for (int i = 0; i < 19; ++i) T.cl[i] = 0;
    for (int i = 0; i < hclen; ++i) {
        inf_refill_bits(b, ring, n_in);
        T.cl[order[i]] = (uint8_t)inf_bits(b, 3);
    }
    // the code-length code borrows the distance tables until the distance code is built
    if (inf_build(T.cl, 19, T.fast_d, 7, T.cnt_d, T.sym_d, T.offs, T.next, true) < 0) return AF_INF_E_CODES;
    const int total = hlit + hdist;
    for (int i = 0; i < total;) {
        inf_refill_bits(b, ring, n_in);
        const int s = inf_decode(b, T.fast_d, 7, T.cnt_d, T.sym_d);
        if (s < 0) return AF_INF_E_SYM;
        if (s < 16) {
            T.lens[i++] = (uint8_t)s;
            continue;
        }
        int prev = 0, rep;
        if (s == 16) {
            if (i == 0) return AF_INF_E_CODES;
            prev = T.lens[i - 1];
            rep = 3 + (int)inf_bits(b, 2);
        } else if (s == 17) {
            rep = 3 + (int)inf_bits(b, 3);
        } else {
            rep = 11 + (int)inf_bits(b, 7);
        }
        if (i + rep > total) return AF_INF_E_CODES;
        for (int k = 0; k < rep; ++k) T.lens[i++] = (uint8_t)prev;
    }
    if (T.lens[256] == 0) return AF_INF_E_CODES;  // no end-of-block code
    const int ml = inf_build(T.lens, hlit, T.fast_l, AF_INF_FAST_L, T.cnt_l, T.sym_l, T.offs, T.next, false);
    if (ml < 0) return AF_INF_E_CODES;
    if (inf_build(T.lens + hlit, hdist, T.fast_d, AF_INF_FAST_D, T.cnt_d, T.sym_d, T.offs, T.next, false) < 0)
        return AF_INF_E_CODES;
    if (ml > st.max_code_len) st.max_code_len = ml;
    return 0;
}

// ---- the decoder (lane 0) -----------------------------------------------------------------
// Decodes until AF_INF_TOK matches are queued (S.ntok of them in tok), more input must be staged
// (S.fill < S.n_in and fewer than AF_INF_MARGIN staged bytes left), the stream is done
// (S.phase == AF_INF_DONE) or an error is met (S.err).  Literals and stored bytes go to win.
AF_HD inline void inf_step(InfState &S, InfTables &T, const uint8_t *ring, uint8_t *win, InfTok *tok) {
    InfBits b{S.bitbuf, S.nbits, S.pos};
    InfStats st = S.st;
    int32_t out = S.out_pos, final_blk = S.final_blk, stored_left = S.stored_left;
    const int32_t isize = S.isize, n_in = S.n_in, fill = S.fill;
    // past `lim` the decoder stops to have input staged, or, with all of it staged, to see whether
    // it has run off the member's end (it reads zeros there, so it cannot run far)
    const int32_t lim = fill < n_in ? fill - AF_INF_MARGIN : n_in + 64;
    int ntok = 0, err = S.err, phase = S.phase;
    while (!err && phase != AF_INF_DONE && ntok < AF_INF_TOK) {
        if (b.pos > lim) {
            if (fill < n_in) break;  // stage more input first
            if ((int64_t)b.pos * 8 - b.n > (int64_t)n_in * 8) {
                err = AF_INF_E_TRUNC;
                break;
            }
        }
        inf_refill_bits(b, ring, n_in);
        if (phase == AF_INF_CODED) {
            int s = inf_decode(b, T.fast_l, AF_INF_FAST_L, T.cnt_l, T.sym_l);
            if (s < 0) {
                err = AF_INF_E_SYM;
            } else if (s < 256) {
                if (out >= isize) err = AF_INF_E_OVER;
                else win[out++] = (uint8_t)s;
            } else if (s == 256) {
                phase = final_blk ? AF_INF_DONE : AF_INF_HEADER;
            } else {
                s -= 257;
                if (s >= 29) {
                    err = AF_INF_E_SYM;
                    break;
                }
                // lengths 3..258: 8 codes without extra bits, then four per extra bit, then 258
                const int le = s < 8 || s == 28 ? 0 : (s >> 2) - 1;
                const int len = s == 28 ? 258 : s < 8 ? 3 + s : 3 + ((4 + (s & 3)) << le) + (int)inf_bits(b, le);
                inf_refill_bits(b, ring, n_in);
                const int d = inf_decode(b, T.fast_d, AF_INF_FAST_D, T.cnt_d, T.sym_d);
                if (d < 0 || d >= 30) {
                    err = AF_INF_E_SYM;
                    break;
                }
                // distances 1..32768: 4 codes without extra bits, then two per extra bit
                const int de = d < 4 ? 0 : (d >> 1) - 1;
                const int dist = d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << de) + (int)inf_bits(b, de);
                if (dist > out) {
                    err = AF_INF_E_FAR;
                    break;
                }
                if (out + len > isize) {
                    err = AF_INF_E_OVER;
                    break;
                }
                tok[ntok++] = InfTok{(uint32_t)out, (uint16_t)len, (uint16_t)dist};
                out += len;
                if (dist > st.max_dist) st.max_dist = dist;
                if (len > st.max_match) st.max_match = len;
                if (dist < len) ++st.overlap;
            }
        } else if (phase == AF_INF_HEADER) {
            final_blk = (int32_t)inf_bits(b, 1);
            const uint32_t type = inf_bits(b, 2);
            if (type == 0) {
                inf_bits(b, b.n & 7);  // to the byte boundary
                inf_refill_bits(b, ring, n_in);
                const uint32_t len = inf_bits(b, 16), nlen = inf_bits(b, 16);
                if ((len ^ 0xffffu) != nlen) err = AF_INF_E_STORED;
                stored_left = (int32_t)len;
                ++st.stored;
                phase = AF_INF_STORED;
            } else if (type == 1) {
                if (!inf_fixed_tables(T)) err = AF_INF_E_CODES;
                ++st.fixed;
                phase = AF_INF_CODED;
            } else if (type == 2) {
                err = inf_dynamic_tables(b, ring, n_in, T, st);
                ++st.dynamic;
                phase = AF_INF_CODED;
            } else {
                err = AF_INF_E_BTYPE;
            }
        } else {  // AF_INF_STORED
            if (stored_left == 0) {
                phase = final_blk ? AF_INF_DONE : AF_INF_HEADER;
            } else if (out >= isize) {
                err = AF_INF_E_OVER;
            } else {
                win[out++] = (uint8_t)inf_bits(b, 8);
                --stored_left;
            }
        }
    }
    if (!err && (int64_t)b.pos * 8 - b.n > (int64_t)n_in * 8) err = AF_INF_E_TRUNC;
    if (!err && phase == AF_INF_DONE && out != isize) err = AF_INF_E_SHORT;
    S.bitbuf = b.buf;
    S.nbits = b.n;
    S.pos = b.pos;
    S.out_pos = out;
    S.phase = phase;
    S.final_blk = final_blk;
    S.stored_left = stored_left;
    S.err = err;
    S.ntok = ntok;
    S.st = st;
}

// lane `lane`'s share of one match.  Every byte is read from [at - dist, at), which is complete
// before the match starts, so the lanes need no order among themselves even when dist < len
// (distance 1, length 258: every lane reads the one byte before the match).
AF_HD inline void inf_apply_lane(uint8_t *win, const InfTok &t, int lane) {
    const uint32_t src = t.at - t.dist;
    if (t.dist >= t.len) {
        for (uint32_t i = lane; i < t.len; i += AF_INF_LANES) win[t.at + i] = win[src + i];
    } else {
        for (uint32_t i = lane; i < t.len; i += AF_INF_LANES) win[t.at + i] = win[src + i % t.dist];
    }
}

// ---- CRC32 (the gzip polynomial, reflected: bit 31 is x^0) -----------------------------------
constexpr uint32_t AF_CRC_POLY = 0xEDB88320u;
AF_HD inline uint32_t crc_tab_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i & 1) ? AF_CRC_POLY ^ (i >> 1) : i >> 1;
    return i;
}
// a * b mod P
AF_HD inline uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if ((a >> (31 - i)) & 1) p ^= b;
        b = (b & 1) ? AF_CRC_POLY ^ (b >> 1) : b >> 1;  // b * x
    }
    return p;
}
// x^(8 n) mod P
AF_HD inline uint32_t crc_xpow8(uint32_t n) {
    uint32_t r = 0x80000000u, sq = 0x00800000u;  // 1, x^8
    for (; n; n >>= 1) {
        if (n & 1) r = crc_mul(r, sq);
        sq = crc_mul(sq, sq);
    }
    return r;
}
// Lane `lane`'s term of the CRC register after win[0, n): the register is linear in (start value,
// bytes), and running it over z further zero-valued terms multiplies it by x^(8 z), so the whole
// register is the XOR over the lanes of (chunk register) * x^(8 * bytes after the chunk).  Lane 0
// starts from the all-ones preset.  The CRC is ~(XOR of the 64 terms).
AF_HD inline uint32_t inf_crc_lane(const uint32_t *tab, const uint8_t *win, int32_t n, int lane) {
    const int32_t chunk = (n + AF_INF_LANES - 1) / AF_INF_LANES;
    int32_t lo = lane * chunk, hi;
    if (lo > n) lo = n;
    hi = lo + chunk > n ? n : lo + chunk;
    uint32_t c = lane == 0 ? 0xffffffffu : 0u;
    for (int32_t i = lo; i < hi; ++i) c = tab[(c ^ win[i]) & 0xff] ^ (c >> 8);
    return c ? crc_mul(crc_xpow8((uint32_t)(n - hi)), c) : 0u;
}
