"""BGZF members for the inflate tests (host hook and GPU kernel): each valid case names the
decoder path it is there for and carries a check of the hook's statistics, so a case cannot pass
without reaching that path; the corrupt cases are one good member damaged in one way each.

The contract for every valid member is ``zlib.decompress(payload, -15)``."""
import random
import struct
import zlib

# stats words of af_inflate_host
STORED, FIXED, DYNAMIC, MAX_CODE_LEN, MAX_DIST, OVERLAP, MAX_MATCH, ERR = range(8)


def member(payload, raw=None, isize=None, crc=None):
    """One BGZF member around a raw deflate stream (the trailer from `raw` unless given)."""
    if raw is None:
        raw = zlib.decompress(payload, -15)
    bsize = 18 + len(payload) + 8
    assert bsize <= 65536, bsize
    head = struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return head + payload + struct.pack("<II", zlib.crc32(raw) if crc is None else crc,
                                        len(raw) if isize is None else isize)


def payload_of(m):
    return m[18:-8]


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(raw) + c.flush()


def fastq_text(n_bytes, seed, read_len=100):
    rng = random.Random(seed)
    out, i = [], 0
    while sum(map(len, out)) < n_bytes:
        seq = "".join(rng.choice("ACGT") for _ in range(read_len))
        qual = "".join(rng.choice("FFFFFF:,#") for _ in range(read_len))
        out.append(f"@run{seed}.{i} {i}/1\n{seq}\n+\n{qual}\n")
        i += 1
    return "".join(out).encode()[:n_bytes]


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):  # k bits, least significant first
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):  # a Huffman code: most significant bit first
        for i in range(k - 1, -1, -1):
            self.put((c >> i) & 1, 1)

    def done(self):
        if self.n:
            self.out.append(self.acc & 0xff)
        return bytes(self.out)


def _fixed_lit(b, v):
    if v < 144:
        b.code(0x30 + v, 8)
    elif v < 256:
        b.code(0x190 + v - 144, 9)
    elif v < 280:
        b.code(v - 256, 7)
    else:
        b.code(0xC0 + v - 280, 8)


def far_match_payload(raw_head):
    """A fixed-Huffman block: the 32,768 literals of raw_head, then one match of length 258 at
    distance 32,768 (zlib's own encoder never looks further back than 32,506)."""
    assert len(raw_head) == 32768
    b = _Bits()
    b.put(1, 1)
    b.put(1, 2)
    for v in raw_head:
        _fixed_lit(b, v)
    _fixed_lit(b, 285)  # length 258, no extra bits
    b.code(29, 5)       # distances 24577..32768: 13 extra bits
    b.put(32768 - 24577, 13)
    _fixed_lit(b, 256)
    return b.done()


def fibonacci_text(seed=3):
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    data = bytearray()
    for i, f in enumerate(fib):
        data += bytes([65 + i]) * f
    rng = random.Random(seed)
    rng.shuffle(data)
    return bytes(data)


def _first_block(p):
    return p[0] & 1, (p[0] >> 1) & 3  # BFINAL, BTYPE


def valid_cases():
    """[(name, member bytes, expected output, check(stats))]"""
    rng = random.Random(11)
    cases = []

    def add(name, payload, raw, check):
        assert zlib.decompress(payload, -15) == raw, name
        cases.append((name, member(payload, raw), raw, check))

    raw = bytes(rng.randrange(256) for _ in range(3000))
    add("stored", deflate(raw, 0), raw, lambda s: s[STORED] >= 1 and s[FIXED] == 0 and s[DYNAMIC] == 0)
    add("eof", b"\x03\x00", b"", lambda s: s[FIXED] == 1 and s[STORED] == 0 and s[DYNAMIC] == 0)
    raw = fastq_text(5000, 1)
    p = deflate(raw, 6, zlib.Z_FIXED)
    assert _first_block(p)[1] == 1
    add("fixed", p, raw, lambda s: s[FIXED] >= 1 and s[DYNAMIC] == 0 and s[MAX_MATCH] >= 3)
    raw = fastq_text(40000, 2)
    add("dynamic6", deflate(raw, 6), raw, lambda s: s[DYNAMIC] >= 1 and s[MAX_CODE_LEN] >= 9)
    add("dynamic9", deflate(raw, 9), raw, lambda s: s[DYNAMIC] >= 1 and s[MAX_CODE_LEN] >= 9)
    raw = fastq_text(60000, 3)
    p = deflate(raw, 6, mem_level=1)
    assert _first_block(p) == (0, 2)
    add("many_blocks", p, raw, lambda s: s[DYNAMIC] >= 4)
    a, b2 = fastq_text(9001, 4), fastq_text(7003, 5)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    p = c.compress(a) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(b2) + c.flush()
    add("sync_flush", p, a + b2, lambda s: s[STORED] >= 1 and s[FIXED] + s[DYNAMIC] >= 2)
    raw = b"A" * 60000
    add("run_60000", deflate(raw), raw, lambda s: s[MAX_DIST] == 1 and s[MAX_MATCH] == 258 and s[OVERLAP] >= 200)
    raw = b"@r1\n" + b"A" * 150 + b"\n+\n" + b"I" * 150 + b"\n"
    add("poly_a_record", deflate(raw), raw, lambda s: s[OVERLAP] >= 2 and s[MAX_MATCH] >= 100)
    head = bytes(rng.randrange(256) for _ in range(32768))
    add("distance_32768", far_match_payload(head), head + head[:258],
        lambda s: s[MAX_DIST] == 32768 and s[MAX_MATCH] == 258 and s[FIXED] == 1)
    raw = fastq_text(65280, 6)
    add("bytes_65280", deflate(raw), raw, lambda s: s[DYNAMIC] >= 1)
    raw = fastq_text(65536, 7)
    add("bytes_65536", deflate(raw), raw, lambda s: s[DYNAMIC] >= 1)
    raw = fibonacci_text()
    add("code_len_15", deflate(raw, 6, zlib.Z_HUFFMAN_ONLY, 9), raw, lambda s: s[MAX_CODE_LEN] == 15)
    return cases


def reference_accepts(m):
    """The host reader's rule for one member: zlib inflates it to exactly ISIZE bytes with the
    trailer's CRC32."""
    crc, isize = struct.unpack("<II", m[-8:])
    if isize > 65536:
        return False
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload_of(m), isize + 1)
    except zlib.error:
        return False
    return d.eof and len(out) == isize and zlib.crc32(out) == crc


def corrupt_cases():
    """[(name, member bytes)]: every one must be refused."""
    raw = fastq_text(20000, 8)
    p = deflate(raw)
    good = member(p, raw)
    assert reference_accepts(good)
    cases = []
    rng = random.Random(5)
    for k in range(50):
        bit = rng.randrange(8 * (len(p) - 1))
        q = bytearray(p)
        q[bit >> 3] ^= 1 << (bit & 7)
        cases.append((f"bit_flip_{k}_at_{bit}", member(bytes(q), raw)))
    cases.append(("isize_small", member(p, raw, isize=len(raw) - 1000)))
    cases.append(("isize_above_64k", member(p, raw, isize=65537)))
    cases.append(("isize_huge", member(p, raw, isize=0x80000010)))
    cases.append(("bad_crc", member(p, raw, crc=zlib.crc32(raw) ^ 0x10)))
    cases.append(("truncated", member(p[:len(p) // 2], raw)))
    for name, m in cases:
        assert not reference_accepts(m), name
    return good, raw, cases


EOF_MEMBER = member(b"\x03\x00", b"")


def bgzf_bytes(data, member_size=65280, level=6):
    """`data` as a BGZF file image: members of member_size input bytes, then the EOF member."""
    out = [member(deflate(data[i:i + member_size], level), data[i:i + member_size])
           for i in range(0, len(data), member_size)]
    return b"".join(out) + EOF_MEMBER


def write_bgzf(path, data, member_size=65280, level=6):
    with open(path, "wb") as fh:
        fh.write(bgzf_bytes(data, member_size, level))
    return str(path)
