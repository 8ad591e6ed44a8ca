"""The device inflate's decoder proven against zlib on the CPU: af_inflate_host runs the kernel's
own source (csrc/inflate_core.h) compiled for the host.  Every case checks the decoder's
statistics too, so it cannot pass without reaching the path it names."""
import ctypes

import numpy as np
import pytest

import bgzf_cases as bc

VALID = bc.valid_cases()
GOOD, GOOD_RAW, CORRUPT = bc.corrupt_cases()


def inflate_host(m, cap=70000, fill=0xAA):
    from anchored_fusion_amd import _lib
    L = _lib.lib()
    src = np.frombuffer(m, dtype=np.uint8)
    out = np.full(cap, fill, dtype=np.uint8)
    stats = np.zeros(8, dtype=np.int32)
    n_out = ctypes.c_int64(-1)
    rc = L.af_inflate_host(src.ctypes.data, len(m), out.ctypes.data, cap, ctypes.byref(n_out), stats.ctypes.data)
    return rc, int(n_out.value), out, [int(v) for v in stats]


@pytest.mark.parametrize("name,m,raw,check", VALID, ids=[c[0] for c in VALID])
def test_valid_member_equals_zlib(name, m, raw, check):
    rc, n_out, out, stats = inflate_host(m)
    assert rc == 0, (name, stats)
    assert n_out == len(raw)
    assert out[:n_out].tobytes() == raw
    assert (out[n_out:] == 0xAA).all()
    assert stats[bc.ERR] == 0
    assert check(stats), (name, stats)


def test_cases_cover_every_block_type_and_limit():
    seen = np.zeros(8, dtype=np.int64)
    for _, m, _, _ in VALID:
        seen = np.maximum(seen, inflate_host(m)[3])
    assert seen[bc.STORED] and seen[bc.FIXED] and seen[bc.DYNAMIC]
    assert seen[bc.MAX_CODE_LEN] == 15 and seen[bc.MAX_DIST] == 32768 and seen[bc.MAX_MATCH] == 258


@pytest.mark.parametrize("name,m", CORRUPT, ids=[c[0] for c in CORRUPT])
def test_corrupt_member_is_refused(name, m):
    rc, n_out, out, stats = inflate_host(m)
    assert rc != 0, (name, stats)
    assert stats[bc.ERR] != 0
    assert n_out == 0
    assert (out == 0xAA).all()  # nothing written, so nothing past the ISIZE bound either


def test_good_member_of_the_corrupt_set_passes():
    rc, n_out, out, _ = inflate_host(GOOD)
    assert rc == 0 and out[:n_out].tobytes() == GOOD_RAW


def test_output_capacity_is_respected():
    from anchored_fusion_amd import _lib
    rc, n_out, out, _ = inflate_host(GOOD, cap=len(GOOD_RAW) - 1)
    assert rc == _lib.AF_E_CAPACITY and n_out == 0 and (out == 0xAA).all()


def test_not_a_member():
    from anchored_fusion_amd import _lib
    assert inflate_host(b"@r1\nACGT\n+\nFFFF\n")[0] == _lib.AF_E_UNSUPPORTED
    assert inflate_host(GOOD + GOOD)[0] == _lib.AF_E_UNSUPPORTED  # exactly one member
