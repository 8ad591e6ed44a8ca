// ingest_dev.hip -- paired FASTQ ingest on the GPU (af_fastq_dev_*, af_bgzf_inflate_device): the
// device counterpart of ingest.cpp.  Compressed BGZF bytes go to the device; inflate, the CRC32
// check, line and record parsing, name trimming, the mate-name check and row packing run there,
// and the reads land in the pair-major layout of include/afgpu.h without a host copy.
//
//   k_bgzf_inflate   one BGZF member per wave (inflate_core.h): decode into an LDS window, CRC32,
//                    then one coalesced copy of the member's ISIZE bytes to the text window
//   k_nl_count / k_scan_i64 / k_nl_scatter   line ends of the text window and their ordinals
//   k_records        one thread per 4-line record: the strict FASTQ checks, sequence and name spans
//   k_names          names, NUL-terminated, into an arena at scanned offsets
//   k_name_cmp       mate names of the two files compared
//   k_pack           rows of `stride` bytes, 'N'-padded, and lens
//
// Only strict 4-line FASTQ is parsed here.  Anything else (multi-line records, FASTA records,
// blank lines, a quality line of another length) makes the call return AF_E_UNSUPPORTED and the
// caller reads the files with the host reader; so does input that is gzip but not BGZF.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/afgpu.h"
#include "af_internal.h"
#include "dev_buf.h"
#include "inflate_core.h"

namespace {

// one BGZF member of a buffer of compressed bytes
struct BgzfMember {
    int64_t in_off;   // first byte of the deflate stream
    int64_t out_off;  // where its output goes
    int32_t n_in;     // deflate bytes (the trailer's 8 bytes excluded)
    int32_t isize;    // trailer ISIZE
    uint32_t crc;     // trailer CRC32
    int32_t pad;
};

// The member whose header starts at h (n bytes follow): its size, with m's in_off relative to h;
// 0 when h holds only part of it, -1 when it is not a BGZF member.
long bgzf_member_at(const uint8_t *h, size_t n, BgzfMember &m) {
    if (n < 12) return n && h[0] != 31 ? -1 : 0;
    if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return -1;
    const size_t xlen = h[10] | (h[11] << 8);
    if (n < 12 + xlen) return 0;
    long bsize = -1;
    for (size_t o = 12; o + 4 <= 12 + xlen;) {
        const size_t slen = h[o + 2] | (h[o + 3] << 8);
        if (h[o] == 66 && h[o + 1] == 67 && slen == 2 && o + 6 <= 12 + xlen) {
            bsize = (long)(h[o + 4] | (h[o + 5] << 8)) + 1;
            break;
        }
        o += 4 + slen;
    }
    if (bsize < (long)(12 + xlen + 8)) return -1;
    if (n < (size_t)bsize) return 0;
    const uint8_t *t = h + bsize - 8;
    m.in_off = (int64_t)(12 + xlen);
    m.n_in = (int32_t)(bsize - 12 - (long)xlen - 8);
    m.crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    const uint32_t isz = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    m.isize = isz > (uint32_t)AF_INF_WIN ? AF_INF_WIN + 1 : (int32_t)isz;  // anything larger is refused alike
    m.pad = 0;
    return bsize;
}

// ---- inflate ------------------------------------------------------------------------------
struct InfLds {
    uint8_t win[AF_INF_WIN];
    alignas(4) uint8_t ring[AF_INF_RING];  // read a word at a time
    InfTables T;
    InfTok tok[AF_INF_TOK];
    InfState S;
    uint32_t crc_tab[256];
    uint32_t part[AF_INF_LANES];
};

// One wave per workgroup, members handed out round-robin.  status[i] = 0 or the AF_INF_E_* code of
// member i; a member with an error writes nothing to out.
__global__ __launch_bounds__(AF_INF_LANES) void k_bgzf_inflate(const uint8_t *__restrict__ comp,
                                                               const BgzfMember *__restrict__ mem, int32_t n_mem,
                                                               uint8_t *__restrict__ out, int32_t *__restrict__ status) {
    __shared__ InfLds L;
    const int lane = threadIdx.x;
    for (int i = lane; i < 256; i += AF_INF_LANES) L.crc_tab[i] = crc_tab_entry((uint32_t)i);
    for (int32_t mi = blockIdx.x; mi < n_mem; mi += gridDim.x) {
        const BgzfMember m = mem[mi];
        __syncthreads();  // the member before this one is finished by every lane
        if (lane == 0) inf_init(L.S, m.n_in, m.isize);
        __syncthreads();
        const uint8_t *src = comp + m.in_off;
        for (;;) {
            if (L.S.err || L.S.phase == AF_INF_DONE) break;  // the same words for every lane
            const int32_t target = inf_fill_target(L.S);
            inf_refill_lane(L.S, target, src, L.ring, lane);
            __syncthreads();
            if (lane == 0) {
                L.S.fill = target;
                inf_step(L.S, L.T, L.ring, L.win, L.tok);
            }
            __syncthreads();
            const int ntok = L.S.ntok;
            for (int t = 0; t < ntok; ++t) {  // in order: a match may read what the one before wrote
                inf_apply_lane(L.win, L.tok[t], lane);
                __syncthreads();
            }
        }
        int err = L.S.err;
        if (!err) {
            L.part[lane] = inf_crc_lane(L.crc_tab, L.win, m.isize, lane);
            __syncthreads();
            uint32_t c = 0;
            for (int i = 0; i < AF_INF_LANES; ++i) c ^= L.part[i];
            if (~c != m.crc) err = AF_INF_E_CRC;
        }
        if (lane == 0) status[mi] = err;
        if (err) continue;
        // window -> text: bytes up to the first 4-byte boundary of the destination, then words
        uint8_t *dst = out + m.out_off;
        const int32_t n = m.isize;
        int32_t head = (int32_t)((4 - ((uintptr_t)dst & 3)) & 3);
        if (head > n) head = n;
        if (lane < head) dst[lane] = L.win[lane];
        const int32_t nw = (n - head) >> 2;
        uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
        for (int32_t w = lane; w < nw; w += AF_INF_LANES) {
            const uint8_t *s = L.win + head + 4 * w;
            dw[w] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
        }
        const int32_t done = head + 4 * nw;
        if (lane < n - done) dst[done + lane] = L.win[done + lane];
    }
}

// the same member on the host: the kernel's phases, a loop over the lanes where it has a barrier.
// The window, the ring and the tokens are allocations of their own (exactly the kernel's sizes), so
// a host sanitizer sees an access outside any of them.
struct InfHost {
    std::vector<uint8_t> win = std::vector<uint8_t>(AF_INF_WIN);
    std::vector<uint8_t> ring = std::vector<uint8_t>(AF_INF_RING);
    std::vector<InfTok> tok = std::vector<InfTok>(AF_INF_TOK);
    InfTables T;
    InfState S;
    uint32_t crc_tab[256];
};
int inflate_member_host(InfHost &L, const uint8_t *src, const BgzfMember &m) {
    uint8_t *win = L.win.data(), *ring = L.ring.data();
    for (uint32_t i = 0; i < 256; ++i) L.crc_tab[i] = crc_tab_entry(i);
    inf_init(L.S, m.n_in, m.isize);
    while (!L.S.err && L.S.phase != AF_INF_DONE) {
        const int32_t target = inf_fill_target(L.S);
        for (int lane = 0; lane < AF_INF_LANES; ++lane) inf_refill_lane(L.S, target, src, ring, lane);
        L.S.fill = target;
        inf_step(L.S, L.T, ring, win, L.tok.data());
        for (int t = 0; t < L.S.ntok; ++t)
            for (int lane = 0; lane < AF_INF_LANES; ++lane) inf_apply_lane(win, L.tok[t], lane);
    }
    if (L.S.err) return L.S.err;
    uint32_t c = 0;
    for (int lane = 0; lane < AF_INF_LANES; ++lane) c ^= inf_crc_lane(L.crc_tab, win, m.isize, lane);
    return ~c != m.crc ? AF_INF_E_CRC : 0;
}

// ---- lines --------------------------------------------------------------------------------
constexpr int AF_NL_THREADS = 256;
constexpr int AF_NL_PER = 16;  // bytes per thread
constexpr int AF_NL_TILE = AF_NL_THREADS * AF_NL_PER;

// exclusive scan of one value per thread of a 256-thread block; *total = the block's sum
__device__ int64_t block_scan_256(int64_t v, int64_t *sh, int64_t *total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < AF_NL_THREADS; d <<= 1) {
        const int64_t add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const int64_t incl = sh[t];
    *total = sh[AF_NL_THREADS - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(AF_NL_THREADS) void k_nl_count(const uint8_t *__restrict__ t, int64_t n,
                                                            int64_t *__restrict__ tile_cnt) {
    __shared__ int64_t sh[AF_NL_THREADS];
    const int64_t lo = (int64_t)blockIdx.x * AF_NL_TILE + (int64_t)threadIdx.x * AF_NL_PER;
    int c = 0;
    for (int k = 0; k < AF_NL_PER; ++k)
        if (lo + k < n && t[lo + k] == '\n') ++c;
    int64_t total;
    block_scan_256(c, sh, &total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// a[0, n) -> its exclusive prefix sums, a[n] = the total (one block)
__global__ __launch_bounds__(1024) void k_scan_i64(int64_t *a, int64_t n) {
    __shared__ int64_t sh[1024];
    __shared__ int64_t carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t v = base + t < n ? a[base + t] : 0;
        sh[t] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int64_t add = t >= d ? sh[t - d] : 0;
            __syncthreads();
            sh[t] += add;
            __syncthreads();
        }
        const int64_t c0 = carry;
        if (base + t < n) a[base + t] = c0 + sh[t] - v;
        __syncthreads();
        if (t == 0) carry = c0 + sh[1023];
        __syncthreads();
    }
    if (t == 0) a[n] = carry;
}

// line_end[k] = the position of the k-th '\n'
__global__ __launch_bounds__(AF_NL_THREADS) void k_nl_scatter(const uint8_t *__restrict__ t, int64_t n,
                                                              const int64_t *__restrict__ tile_off,
                                                              int64_t *__restrict__ line_end, int64_t n_lines) {
    __shared__ int64_t sh[AF_NL_THREADS];
    const int64_t lo = (int64_t)blockIdx.x * AF_NL_TILE + (int64_t)threadIdx.x * AF_NL_PER;
    int c = 0;
    for (int k = 0; k < AF_NL_PER; ++k)
        if (lo + k < n && t[lo + k] == '\n') ++c;
    int64_t total;
    int64_t ord = tile_off[blockIdx.x] + block_scan_256(c, sh, &total);
    for (int k = 0; k < AF_NL_PER; ++k)
        if (lo + k < n && t[lo + k] == '\n') {
            if (ord < n_lines) line_end[ord] = lo + k;
            ++ord;
        }
}

// ---- records ------------------------------------------------------------------------------
struct RecOut {
    int64_t *seq_start, *name_start;
    int32_t *seq_len, *name_len;
    int64_t *name_tile;  // per 256 records: their name bytes with the NULs
};
// res words: [0], [1] first record of file 0 / 1 that is not a strict 4-line record, [2] first
// pair with unequal names, [3] the longest read
enum { AF_RES_BAD0 = 0, AF_RES_MISMATCH = 2, AF_RES_MAXLEN = 3, AF_RES_N = 4 };

// Record r is lines 4r .. 4r + 3 of the window.  The rules are those under which the host
// reader (ingest.cpp `parse`) reads the same four lines as one record: a non-empty '@' header, a
// sequence line that does not look like a '+' or '>' line, a '+' line, a quality line exactly as
// long as the sequence; '\r' before the line end dropped.
__global__ __launch_bounds__(AF_NL_THREADS) void k_records(const uint8_t *__restrict__ t,
                                                           const int64_t *__restrict__ line_end, int64_t n_rec,
                                                           int which, RecOut o, unsigned long long *res) {
    __shared__ int64_t sh[AF_NL_THREADS];
    const int64_t r = (int64_t)blockIdx.x * AF_NL_THREADS + threadIdx.x;
    int64_t nb = 0;
    if (r < n_rec) {
        int64_t s[4], e[4];
        for (int k = 0; k < 4; ++k) {
            const int64_t li = 4 * r + k;
            s[k] = li ? line_end[li - 1] + 1 : 0;
            e[k] = line_end[li];
            if (e[k] > s[k] && t[e[k] - 1] == '\r') --e[k];
        }
        const int64_t slen = e[1] - s[1];
        bool bad = e[0] == s[0] || t[s[0]] != '@';
        bad = bad || (slen > 0 && (t[s[1]] == '+' || t[s[1]] == '>'));
        bad = bad || e[2] == s[2] || t[s[2]] != '+';
        bad = bad || e[3] - s[3] != slen || slen > 0x7fffffff;
        if (bad) {
            atomicMin(&res[AF_RES_BAD0 + which], (unsigned long long)r);
        } else {
            int64_t x = s[0] + 1;
            while (x < e[0] && t[x] != ' ' && t[x] != '\t') ++x;
            int64_t nl = x - s[0] - 1;
            if (nl > 2 && t[x - 2] == '/' && t[x - 1] >= '0' && t[x - 1] <= '9') nl -= 2;  // bwa's trim_readno
            if (nl > 0x7ffffff0) nl = 0x7ffffff0;
            o.seq_start[r] = s[1];
            o.seq_len[r] = (int32_t)slen;
            o.name_start[r] = s[0] + 1;
            o.name_len[r] = (int32_t)nl;
            nb = nl + 1;
            atomicMax(&res[AF_RES_MAXLEN], (unsigned long long)slen);
        }
    }
    int64_t total;
    block_scan_256(nb, sh, &total);
    if (threadIdx.x == 0) o.name_tile[blockIdx.x] = total;
}

__global__ __launch_bounds__(AF_NL_THREADS) void k_names(const uint8_t *__restrict__ t, RecOut o, int64_t n_rec,
                                                         char *__restrict__ arena, int64_t *__restrict__ name_off) {
    __shared__ int64_t sh[AF_NL_THREADS];
    const int64_t r = (int64_t)blockIdx.x * AF_NL_THREADS + threadIdx.x;
    const int64_t nl = r < n_rec ? o.name_len[r] : 0;
    int64_t total;
    const int64_t at = o.name_tile[blockIdx.x] + block_scan_256(r < n_rec ? nl + 1 : 0, sh, &total);
    if (r >= n_rec) return;
    const uint8_t *s = t + o.name_start[r];
    for (int64_t i = 0; i < nl; ++i) arena[at + i] = (char)s[i];
    arena[at + nl] = '\0';
    name_off[r] = at;
}

__global__ void k_name_cmp(const uint8_t *__restrict__ t1, RecOut a, const uint8_t *__restrict__ t2, RecOut b,
                           int64_t n, unsigned long long *res) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int32_t nl = a.name_len[r];
    bool same = nl == b.name_len[r];
    const uint8_t *x = t1 + a.name_start[r], *y = t2 + b.name_start[r];
    // the host reader compares C strings: a NUL inside a name ends it there
    for (int32_t i = 0; same && i < nl; ++i) {
        same = x[i] == y[i];
        if (!x[i]) break;
    }
    if (!same) atomicMin(&res[AF_RES_MISMATCH], (unsigned long long)r);
}

// record k of file `which` -> row 2k + which: 64 lanes per row
__global__ __launch_bounds__(256) void k_pack(const uint8_t *__restrict__ t, RecOut o, int64_t n_rec, int which,
                                              int32_t stride, uint8_t *__restrict__ reads, int32_t *__restrict__ lens) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_rec) return;
    const int32_t len = o.seq_len[r];
    const uint8_t *s = t + o.seq_start[r];
    const int64_t row = 2 * r + which;
    if (reads) {
        uint8_t *d = reads + row * (int64_t)stride;
        for (int32_t i = lane; i < stride; i += 64) d[i] = i < len ? s[i] : (uint8_t)'N';
    }
    if (lens && lane == 0) lens[row] = len;
}

// ---- host side ----------------------------------------------------------------------------
const char *inf_err_text(int e) {
    return e == AF_INF_E_ISIZE ? "corrupt BGZF block (ISIZE above the 64 KiB BGZF maximum)"
                               : "corrupt BGZF block (inflate or CRC32)";
}

int inflate_grid(int n_mem) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 64;
    return std::max(1, std::min(n_mem, 2 * cus));  // the LDS window leaves room for two waves per CU
}

struct PinnedBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t alloc(size_t n) {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), n, hipHostMallocDefault);
        if (e == hipSuccess) cap = n;
        else p = nullptr;
        return e;
    }
};

// one input file and its device window of inflated text
struct DevFile {
    std::string path;
    FILE *fp = nullptr;
    bool bgzf = false;
    bool file_end = false;  // fread met the end of the file
    bool eof = false;       // every byte of the file is in the window
    PinnedBuf stage;        // compressed bytes read but not yet inflated start at 0
    size_t stage_n = 0;
    std::vector<BgzfMember> mem;
    DevBuf<uint8_t> d_comp;
    DevBuf<BgzfMember> d_mem;
    DevBuf<int32_t> d_status;
    std::vector<int32_t> status;
    DevBuf<uint8_t> text_buf[2];  // the window is text[beg, end), text = text_buf[cur]
    int cur = 0;
    int64_t beg = 0, end = 0;
    // lines and records of the window (valid while beg / end stand)
    bool lines_valid = false;
    int64_t n_lines = 0;
    bool open_last = false;  // the last line has no '\n' (the file ends there)
    DevBuf<int64_t> tile, line_end, name_tile;
    DevBuf<int64_t> seq_start, name_start;
    DevBuf<int32_t> seq_len, name_len;
    int64_t adv = 0;  // bytes of the records handed out by the last af_fastq_dev_next
    ~DevFile() {
        if (fp) fclose(fp);
    }
    uint8_t *text() const { return text_buf[cur].get(); }
    RecOut rec() const { return RecOut{seq_start, name_start, seq_len, name_len, name_tile}; }
};

}  // namespace

struct af_fastq_dev {
    af_ctx *ctx = nullptr;
    int device = 0;
    int64_t batch_bytes = 0;
    DevFile f[2];
    DevBuf<unsigned long long> d_res;
    DevBuf<char> d_names;
    DevBuf<int64_t> d_name_off;
    int64_t n_cur = 0, names_bytes = 0, pairs_done = 0;
    int32_t max_len = 0;
    double times[AF_FASTQ_DEV_TIMES] = {0, 0, 0, 0, 0};  // af_fastq_dev_times
    std::string err;
};

namespace {

constexpr int64_t AF_DEV_BATCH_DEFAULT = 32ll << 20;

// adds the time since its construction to one of the handle's phase totals; every phase it
// brackets ends in a blocking copy or a stream synchronisation, so host time is the phase's time
struct PhaseTimer {
    double &acc;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit PhaseTimer(double &a) : acc(a) {}
    ~PhaseTimer() { acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

int dfail(af_fastq_dev *h, int code, const std::string &msg) {
    h->err = msg;
    return code;
}
#define DHIP(h, expr)                                                                                   \
    do {                                                                                                \
        const hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return dfail(h, AF_E_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
    } while (0)

// room for `add` more bytes after the window's end; the unconsumed tail moves to the front of the
// other buffer when this one is full
int text_room(af_fastq_dev *h, DevFile &F, int64_t add) {
    if (F.end + add <= F.text_buf[F.cur].size()) return AF_OK;
    const int64_t tail = F.end - F.beg;
    DevBuf<uint8_t> &alt = F.text_buf[F.cur ^ 1];
    DHIP(h, alt.grow(tail + add, (tail + add) + (tail + add) / 4 + 4096));
    if (tail) DHIP(h, hipMemcpy(alt.get(), F.text() + F.beg, (size_t)tail, hipMemcpyDeviceToDevice));
    F.cur ^= 1;
    F.beg = 0;
    F.end = tail;
    F.lines_valid = false;
    return AF_OK;
}

// the next batch of file F into its window: about batch_bytes compressed bytes of whole members
int load_batch(af_fastq_dev *h, DevFile &F) {
    if (!F.file_end) {
        PhaseTimer pt(h->times[0]);
        const size_t want = F.stage.cap - F.stage_n;
        const size_t got = fread(F.stage.p + F.stage_n, 1, want, F.fp);
        if (got < want) {
            if (ferror(F.fp)) return dfail(h, AF_E_INVALID, F.path + ": read error");
            F.file_end = true;
        }
        F.stage_n += got;
    }
    F.lines_valid = false;
    if (!F.bgzf) {  // plain text: the bytes are the window's
        const size_t n = std::min<size_t>(F.stage_n, (size_t)h->batch_bytes);
        if (const int rc = text_room(h, F, (int64_t)n)) return rc;
        {
            PhaseTimer pt(h->times[1]);
            if (n) DHIP(h, hipMemcpy(F.text() + F.end, F.stage.p, n, hipMemcpyHostToDevice));
        }
        F.end += (int64_t)n;
        memmove(F.stage.p, F.stage.p + n, F.stage_n - n);
        F.stage_n -= n;
        F.eof = F.file_end && F.stage_n == 0;
        return AF_OK;
    }
    F.mem.clear();
    size_t off = 0;
    int64_t out = 0;
    while (off < F.stage_n && (int64_t)off < h->batch_bytes) {
        BgzfMember m;
        const long bs = bgzf_member_at(F.stage.p + off, F.stage_n - off, m);
        if (bs < 0) return dfail(h, AF_E_INVALID, F.path + ": gzip member without a BGZF size (mixed input?)");
        if (bs == 0) {
            if (F.file_end) return dfail(h, AF_E_INVALID, F.path + ": truncated BGZF block");
            break;
        }
        m.in_off += (int64_t)off;
        m.out_off = out;
        out += m.isize <= AF_INF_WIN ? m.isize : 0;
        F.mem.push_back(m);
        off += (size_t)bs;
    }
    const int n_mem = (int)F.mem.size();
    if (n_mem) {
        if (const int rc = text_room(h, F, out)) return rc;
        DHIP(h, F.d_comp.grow((int64_t)off, (int64_t)F.stage.cap));
        DHIP(h, F.d_mem.grow(n_mem, n_mem + n_mem / 2));
        DHIP(h, F.d_status.grow(n_mem, n_mem + n_mem / 2));
        {
            PhaseTimer pt(h->times[1]);
            DHIP(h, hipMemcpy(F.d_comp.get(), F.stage.p, off, hipMemcpyHostToDevice));
            DHIP(h, hipMemcpy(F.d_mem.get(), F.mem.data(), sizeof(BgzfMember) * (size_t)n_mem, hipMemcpyHostToDevice));
        }
        PhaseTimer pt(h->times[2]);
        k_bgzf_inflate<<<inflate_grid(n_mem), AF_INF_LANES, 0, 0>>>(F.d_comp, F.d_mem, n_mem, F.text() + F.end,
                                                                    F.d_status);
        DHIP(h, hipGetLastError());
        F.status.resize((size_t)n_mem);
        DHIP(h, hipMemcpy(F.status.data(), F.d_status.get(), sizeof(int32_t) * (size_t)n_mem, hipMemcpyDeviceToHost));
        for (int i = 0; i < n_mem; ++i)
            if (F.status[i]) return dfail(h, AF_E_INVALID, F.path + ": " + inf_err_text(F.status[i]));
        F.end += out;
    }
    memmove(F.stage.p, F.stage.p + off, F.stage_n - off);
    F.stage_n -= off;
    F.eof = F.file_end && F.stage_n == 0;
    return AF_OK;
}

// line ends of F's window
int scan_lines(af_fastq_dev *h, DevFile &F) {
    PhaseTimer pt(h->times[3]);
    const int64_t n = F.end - F.beg;
    F.n_lines = 0;
    F.open_last = false;
    F.lines_valid = true;
    if (n == 0) return AF_OK;
    const uint8_t *t = F.text() + F.beg;
    const int64_t tiles = (n + AF_NL_TILE - 1) / AF_NL_TILE;
    DHIP(h, F.tile.grow(tiles + 1, tiles + tiles / 4 + 1));
    k_nl_count<<<(unsigned)tiles, AF_NL_THREADS, 0, 0>>>(t, n, F.tile);
    k_scan_i64<<<1, 1024, 0, 0>>>(F.tile, tiles);
    DHIP(h, hipGetLastError());
    int64_t total = 0;
    uint8_t last = 0;
    DHIP(h, hipMemcpy(&total, F.tile.get() + tiles, sizeof total, hipMemcpyDeviceToHost));
    DHIP(h, hipMemcpy(&last, t + n - 1, 1, hipMemcpyDeviceToHost));
    F.open_last = F.eof && last != '\n';
    F.n_lines = total + (F.open_last ? 1 : 0);
    DHIP(h, F.line_end.grow(F.n_lines + 1, F.n_lines + F.n_lines / 4 + 1));
    k_nl_scatter<<<(unsigned)tiles, AF_NL_THREADS, 0, 0>>>(t, n, F.tile, F.line_end, total);
    DHIP(h, hipGetLastError());
    if (F.open_last) DHIP(h, hipMemcpy(F.line_end.get() + total, &n, sizeof n, hipMemcpyHostToDevice));
    return AF_OK;
}

std::string fetch_name(const DevFile &F, int64_t r) {
    int64_t s = 0;
    int32_t l = 0;
    if (hipMemcpy(&s, F.name_start.get() + r, sizeof s, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&l, F.name_len.get() + r, sizeof l, hipMemcpyDeviceToHost) != hipSuccess)
        return "?";
    std::string nm((size_t)l, '\0');
    if (l && hipMemcpy(&nm[0], F.text() + F.beg + s, (size_t)l, hipMemcpyDeviceToHost) != hipSuccess) return "?";
    return std::string(nm.c_str());
}

int dev_open(af_ctx *ctx, const char *fq1, const char *fq2, int64_t batch_bytes, af_fastq_dev **out) {
    if (!out) return AF_E_INVALID;
    *out = nullptr;
    if (!fq1 || !fq2 || batch_bytes < 0) return AF_E_INVALID;
    af_fastq_dev *h = new (std::nothrow) af_fastq_dev;
    if (!h) return AF_E_NOMEM;
    *out = h;  // the handle carries the message; the caller closes it
    h->ctx = ctx;
    h->batch_bytes = batch_bytes ? batch_bytes : AF_DEV_BATCH_DEFAULT;
    const char *paths[2] = {fq1, fq2};
    for (int m = 0; m < 2; ++m) {
        DevFile &F = h->f[m];
        F.path = paths[m];
        F.fp = fopen(paths[m], "rb");
        if (!F.fp) return dfail(h, AF_E_INVALID, "cannot open " + F.path);
        uint8_t hd[2] = {0, 0};
        const size_t n = fread(hd, 1, 2, F.fp);
        if (n == 2 && hd[0] == 31 && hd[1] == 139) {
            uint8_t hh[512];
            rewind(F.fp);
            const size_t k = fread(hh, 1, sizeof hh, F.fp);
            BgzfMember mm;
            // a header that parses but whose member runs past these 512 bytes answers 0
            if (bgzf_member_at(hh, k, mm) < 0)
                return dfail(h, AF_E_UNSUPPORTED, F.path + ": gzip input that is not BGZF (read it with the host reader)");
            F.bgzf = true;
        }
        rewind(F.fp);
    }
    if (!ctx) return dfail(h, AF_E_INVALID, "null context");
    h->device = af_ctx_device_id(ctx);
    DHIP(h, hipSetDevice(h->device));
    for (int m = 0; m < 2; ++m)
        DHIP(h, h->f[m].stage.alloc((size_t)h->batch_bytes + 2 * AF_INF_WIN));
    DHIP(h, h->d_res.alloc(AF_RES_N));
    return AF_OK;
}

int dev_next(af_fastq_dev *h, int64_t max_pairs, int64_t *n_pairs, int32_t *max_len, int64_t *names_bytes) {
    if (!h || !n_pairs || max_pairs < 0) return AF_E_INVALID;
    *n_pairs = 0;
    DHIP(h, hipSetDevice(h->device));
    for (DevFile &F : h->f)
        if (F.adv) {  // the records of the call before are consumed
            F.beg += F.adv;
            F.adv = 0;
            F.lines_valid = false;
        }
    h->n_cur = 0;
    for (;;) {
        bool loaded = false;
        for (DevFile &F : h->f) {
            if (!F.lines_valid)
                if (const int rc = scan_lines(h, F)) return rc;
            if (F.n_lines / 4 < max_pairs && !F.eof) {
                if (const int rc = load_batch(h, F)) return rc;
                loaded = true;
            }
        }
        if (!loaded) break;
    }
    int64_t n[2];
    for (int m = 0; m < 2; ++m) {
        const DevFile &F = h->f[m];
        if (F.eof && F.n_lines % 4 != 0)
            return dfail(h, AF_E_UNSUPPORTED, F.path + ": not 4-line FASTQ records to the end (read it with the host reader)");
        n[m] = std::min(max_pairs, F.n_lines / 4);
    }
    PhaseTimer pt(h->times[3]);
    const unsigned long long none = ~0ull;
    unsigned long long res[AF_RES_N] = {none, none, none, 0};
    DHIP(h, hipMemcpy(h->d_res.get(), res, sizeof res, hipMemcpyHostToDevice));
    for (int m = 0; m < 2; ++m) {
        DevFile &F = h->f[m];
        if (!n[m]) continue;
        const int64_t tiles = (n[m] + AF_NL_THREADS - 1) / AF_NL_THREADS;
        DHIP(h, F.seq_start.grow(n[m], n[m] + n[m] / 4));
        DHIP(h, F.name_start.grow(n[m], n[m] + n[m] / 4));
        DHIP(h, F.seq_len.grow(n[m], n[m] + n[m] / 4));
        DHIP(h, F.name_len.grow(n[m], n[m] + n[m] / 4));
        DHIP(h, F.name_tile.grow(tiles + 1, tiles + tiles / 4 + 1));
        k_records<<<(unsigned)tiles, AF_NL_THREADS, 0, 0>>>(F.text() + F.beg, F.line_end, n[m], m, F.rec(), h->d_res);
        DHIP(h, hipGetLastError());
    }
    DHIP(h, hipMemcpy(res, h->d_res.get(), sizeof res, hipMemcpyDeviceToHost));
    for (int m = 0; m < 2; ++m)
        if (res[AF_RES_BAD0 + m] != none)
            return dfail(h, AF_E_UNSUPPORTED,
                         h->f[m].path + ": record " + std::to_string(h->pairs_done + (int64_t)res[AF_RES_BAD0 + m] + 1) +
                             " is not a 4-line FASTQ record (read it with the host reader)");
    if (n[0] != n[1])
        return dfail(h, AF_E_INVALID,
                     "paired FASTQs differ in length: " + std::to_string(h->pairs_done + n[0]) + " vs " +
                         std::to_string(h->pairs_done + n[1]) + " records");
    const int64_t np = n[0];
    if (np == 0) return AF_OK;
    const unsigned g = (unsigned)((np + 255) / 256);
    k_name_cmp<<<g, 256, 0, 0>>>(h->f[0].text() + h->f[0].beg, h->f[0].rec(), h->f[1].text() + h->f[1].beg,
                                 h->f[1].rec(), np, h->d_res);
    k_scan_i64<<<1, 1024, 0, 0>>>(h->f[0].name_tile, (np + AF_NL_THREADS - 1) / AF_NL_THREADS);
    DHIP(h, hipGetLastError());
    DHIP(h, hipMemcpy(res, h->d_res.get(), sizeof res, hipMemcpyDeviceToHost));
    if (res[AF_RES_MISMATCH] != none) {
        const int64_t r = (int64_t)res[AF_RES_MISMATCH];
        return dfail(h, AF_E_INVALID,
                     "paired reads have different names: \"" + fetch_name(h->f[0], r) + "\", \"" + fetch_name(h->f[1], r) +
                         "\"");
    }
    DHIP(h, hipMemcpy(&h->names_bytes, h->f[0].name_tile.get() + (np + AF_NL_THREADS - 1) / AF_NL_THREADS,
                      sizeof(int64_t), hipMemcpyDeviceToHost));
    for (DevFile &F : h->f) {
        const int64_t last = 4 * np - 1;
        if (last == F.n_lines - 1 && F.open_last) {
            F.adv = F.end - F.beg;
        } else {
            DHIP(h, hipMemcpy(&F.adv, F.line_end.get() + last, sizeof(int64_t), hipMemcpyDeviceToHost));
            F.adv += 1;
        }
    }
    h->n_cur = np;
    h->max_len = (int32_t)res[AF_RES_MAXLEN];
    h->pairs_done += np;
    *n_pairs = np;
    if (max_len) *max_len = h->max_len;
    if (names_bytes) *names_bytes = h->names_bytes;
    return AF_OK;
}

int dev_export(af_fastq_dev *h, int32_t stride, uint8_t *d_reads, int32_t *d_lens, char *names, int64_t names_cap,
               int64_t *name_off, void *stream) {
    if (!h || stride < 0) return AF_E_INVALID;
    const int64_t np = h->n_cur;
    if (np == 0) return AF_OK;
    if (h->max_len > stride) return dfail(h, AF_E_CAPACITY, "read longer than stride " + std::to_string(stride));
    if (names && h->names_bytes > names_cap) return dfail(h, AF_E_CAPACITY, "names arena too small");
    DHIP(h, hipSetDevice(h->device));
    PhaseTimer pt(h->times[4]);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d_reads || d_lens)
        for (int m = 0; m < 2; ++m) {
            const DevFile &F = h->f[m];
            k_pack<<<(unsigned)((np + 3) / 4), 256, 0, s>>>(F.text() + F.beg, F.rec(), np, m, stride, d_reads, d_lens);
        }
    if (names || name_off) {
        const DevFile &F = h->f[0];
        DHIP(h, h->d_names.grow(h->names_bytes, h->names_bytes + h->names_bytes / 4));
        DHIP(h, h->d_name_off.grow(np, np + np / 4));
        k_names<<<(unsigned)((np + AF_NL_THREADS - 1) / AF_NL_THREADS), AF_NL_THREADS, 0, s>>>(
            F.text() + F.beg, F.rec(), np, h->d_names, h->d_name_off);
        DHIP(h, hipGetLastError());
        if (names)
            DHIP(h, hipMemcpyAsync(names, h->d_names.get(), (size_t)h->names_bytes, hipMemcpyDeviceToHost, s));
        if (name_off)
            DHIP(h, hipMemcpyAsync(name_off, h->d_name_off.get(), sizeof(int64_t) * (size_t)np, hipMemcpyDeviceToHost, s));
    }
    DHIP(h, hipGetLastError());
    DHIP(h, hipStreamSynchronize(s));  // the names are on the host, and the window may move on
    return AF_OK;
}

template <class F>
int dev_guard(af_fastq_dev *h, F &&body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        if (h) h->err = "out of host memory";
        return AF_E_NOMEM;
    } catch (const std::exception &ex) {
        if (h) h->err = ex.what();
        return AF_E_INVALID;
    }
}

}  // namespace

extern "C" {

int af_fastq_dev_open(af_ctx *ctx, const char *fq1, const char *fq2, int64_t batch_bytes, af_fastq_dev **out) {
    try {
        return dev_open(ctx, fq1, fq2, batch_bytes, out);
    } catch (const std::bad_alloc &) {
        return AF_E_NOMEM;
    } catch (const std::exception &) {
        return AF_E_INVALID;
    }
}

int af_fastq_dev_next(af_fastq_dev *h, int64_t max_pairs, int64_t *n_pairs, int32_t *max_len, int64_t *names_bytes) {
    return dev_guard(h, [&] { return dev_next(h, max_pairs, n_pairs, max_len, names_bytes); });
}

int af_fastq_dev_export(af_fastq_dev *h, int32_t stride, uint8_t *d_reads, int32_t *d_lens, char *names,
                        int64_t names_cap, int64_t *name_off, void *stream) {
    return dev_guard(h, [&] { return dev_export(h, stride, d_reads, d_lens, names, names_cap, name_off, stream); });
}

const char *af_fastq_dev_error(const af_fastq_dev *h) { return h ? h->err.c_str() : "null af_fastq_dev handle"; }

int af_fastq_dev_times(const af_fastq_dev *h, double *out) {
    if (!h || !out) return AF_E_INVALID;
    memcpy(out, h->times, sizeof h->times);
    return AF_OK;
}

void af_fastq_dev_close(af_fastq_dev *h) {
    if (h && h->ctx) (void)hipSetDevice(h->device);
    delete h;
}

int af_bgzf_inflate_device(af_ctx *ctx, const uint8_t *file_bytes, int64_t n, uint8_t *out, int64_t out_cap,
                           int64_t *n_out, int32_t *bad_member) {
    if (!ctx) return AF_E_INVALID;
    auto fail = [&](int code, const char *msg) {
        af_ctx_set_error(ctx, msg);
        return code;
    };
    try {
        if (!file_bytes || n < 0 || !n_out || (!out && out_cap)) return fail(AF_E_INVALID, "null argument");
        *n_out = 0;
        if (bad_member) *bad_member = -1;
        std::vector<BgzfMember> mem;
        int64_t off = 0, total = 0;
        while (off < n) {
            BgzfMember m;
            const long bs = bgzf_member_at(file_bytes + off, (size_t)(n - off), m);
            if (bs <= 0) return fail(AF_E_UNSUPPORTED, "not a BGZF file (or a truncated block)");
            m.in_off += off;
            m.out_off = total;
            total += m.isize <= AF_INF_WIN ? m.isize : 0;
            mem.push_back(m);
            off += bs;
        }
        if (mem.empty()) return AF_OK;
        if (hipSetDevice(af_ctx_device_id(ctx)) != hipSuccess) return fail(AF_E_HIP, "hipSetDevice failed");
        const int n_mem = (int)mem.size();
        DevBuf<uint8_t> d_comp, d_out;
        DevBuf<BgzfMember> d_mem;
        DevBuf<int32_t> d_status;
        std::vector<int32_t> status((size_t)n_mem);
        if (d_comp.alloc(n) != hipSuccess || d_out.alloc(std::max<int64_t>(total, 1)) != hipSuccess ||
            d_mem.alloc(n_mem) != hipSuccess || d_status.alloc(n_mem) != hipSuccess)
            return fail(AF_E_HIP, "device allocation failed");
        if (hipMemcpy(d_comp.get(), file_bytes, (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_mem.get(), mem.data(), sizeof(BgzfMember) * (size_t)n_mem, hipMemcpyHostToDevice) != hipSuccess)
            return fail(AF_E_HIP, "copy to the device failed");
        k_bgzf_inflate<<<inflate_grid(n_mem), AF_INF_LANES, 0, 0>>>(d_comp, d_mem, n_mem, d_out, d_status);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpy(status.data(), d_status.get(), sizeof(int32_t) * (size_t)n_mem, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(AF_E_HIP, "k_bgzf_inflate failed");
        for (int i = 0; i < n_mem; ++i)
            if (status[i]) {
                if (bad_member) *bad_member = i;
                return fail(AF_E_INVALID, inf_err_text(status[i]));
            }
        if (total > out_cap) return fail(AF_E_CAPACITY, "output buffer too small");
        if (total && hipMemcpy(out, d_out.get(), (size_t)total, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(AF_E_HIP, "copy from the device failed");
        *n_out = total;
        return AF_OK;
    } catch (const std::bad_alloc &) {
        return fail(AF_E_NOMEM, "out of host memory");
    } catch (const std::exception &ex) {
        return fail(AF_E_INVALID, ex.what());
    }
}

// Test hook: one BGZF member (header, deflate stream, trailer) inflated on the host by the code the
// kernel runs.  stats (8 int32, may be NULL): stored / fixed / dynamic blocks, the longest
// literal/length code, the largest distance, matches with distance < length, the longest match,
// the decoder's AF_INF_E_* code.  On an error nothing is written to out.  Not a product path.
int af_inflate_host(const uint8_t *member, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int32_t *stats) {
    if (!member || n < 0 || !n_out) return AF_E_INVALID;
    *n_out = 0;
    if (stats) memset(stats, 0, 8 * sizeof(int32_t));
    InfHost *L = new (std::nothrow) InfHost;
    if (!L) return AF_E_NOMEM;
    BgzfMember m;
    const long bs = bgzf_member_at(member, (size_t)n, m);
    if (bs <= 0 || bs != n) {
        delete L;
        return AF_E_UNSUPPORTED;
    }
    const int err = inflate_member_host(*L, member + m.in_off, m);
    if (stats) {
        const InfStats &st = L->S.st;
        const int32_t v[8] = {st.stored, st.fixed, st.dynamic, st.max_code_len, st.max_dist, st.overlap, st.max_match, err};
        memcpy(stats, v, sizeof v);
    }
    int rc = AF_OK;
    if (err) rc = AF_E_INVALID;
    else if (m.isize > cap || (!out && m.isize)) rc = AF_E_CAPACITY;
    else {
        if (m.isize) memcpy(out, L->win.data(), (size_t)m.isize);
        *n_out = m.isize;
    }
    delete L;
    return rc;
}

}  // extern "C"
