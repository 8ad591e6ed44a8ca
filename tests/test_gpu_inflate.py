"""k_bgzf_inflate against zlib: the members of tests/bgzf_cases.py (each proven to reach its
decoder path by tests/test_inflate_host.py) as multi-member files through af_bgzf_inflate_device,
and the corrupt members, which must be named by index and leave no output.  A corrupt member goes
to the GPU only after the host build of the same decoder has refused it."""
import ctypes

import numpy as np
import pytest

import bgzf_cases as bc
from test_inflate_host import inflate_host

pytestmark = pytest.mark.gpu

VALID = bc.valid_cases()
GOOD, GOOD_RAW, CORRUPT = bc.corrupt_cases()


@pytest.fixture(scope="module")
def ctx():
    from anchored_fusion_amd import _lib
    L = _lib.lib()
    c = ctypes.c_void_p()
    _lib.check(None, L.af_ctx_create(0, ctypes.byref(c)), "af_ctx_create")
    yield c
    L.af_ctx_destroy(c)


def inflate_device(ctx, data, cap):
    from anchored_fusion_amd import _lib
    L = _lib.lib()
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.full(max(cap, 1), 0xAA, dtype=np.uint8)
    n_out, bad = ctypes.c_int64(-1), ctypes.c_int32(-2)
    rc = L.af_bgzf_inflate_device(ctx, src.ctypes.data, len(data), out.ctypes.data, cap, ctypes.byref(n_out),
                                  ctypes.byref(bad))
    return rc, int(n_out.value), out, int(bad.value)


def test_every_case_as_one_file(ctx):
    data = b"".join(m for _, m, _, _ in VALID) + bc.EOF_MEMBER
    want = b"".join(raw for _, _, raw, _ in VALID)
    rc, n_out, out, bad = inflate_device(ctx, data, len(want) + 64)
    assert rc == 0 and bad == -1
    assert n_out == len(want)
    got = out[:n_out].tobytes()
    pos = 0
    for name, _, raw, _ in VALID:  # name the member that differs
        assert got[pos:pos + len(raw)] == raw, name
        pos += len(raw)
    assert (out[n_out:] == 0xAA).all()


def test_more_members_than_workgroups(ctx):
    """The members are dealt round-robin to a grid of two waves per CU: with more members than
    that, every wave decodes several, one after the other, in the same LDS window."""
    reps = 48
    data = b"".join(m for _, m, _, _ in VALID) * reps
    want = b"".join(raw for _, _, raw, _ in VALID) * reps
    assert len(VALID) * reps > 600
    rc, n_out, out, bad = inflate_device(ctx, data, len(want))
    assert rc == 0 and bad == -1 and n_out == len(want)
    assert out.tobytes() == want


@pytest.mark.parametrize("name,m", CORRUPT, ids=[c[0] for c in CORRUPT])
def test_corrupt_member_is_named(ctx, name, m):
    from anchored_fusion_amd import _lib
    assert inflate_host(m)[0] != 0, "the host build of the decoder must refuse it first"
    rc, n_out, out, bad = inflate_device(ctx, GOOD + m + GOOD + bc.EOF_MEMBER, 3 * len(GOOD_RAW))
    assert rc == _lib.AF_E_INVALID
    assert bad == 1
    assert n_out == 0 and (out == 0xAA).all()
    assert "BGZF" in _lib.lib().af_last_error(ctx).decode()


def test_not_bgzf_and_capacity(ctx):
    from anchored_fusion_amd import _lib
    assert inflate_device(ctx, b"@r\nACGT\n+\nFFFF\n", 100)[0] == _lib.AF_E_UNSUPPORTED
    assert inflate_device(ctx, GOOD[:-5], 100000)[0] == _lib.AF_E_UNSUPPORTED  # a truncated block
    assert inflate_device(ctx, GOOD, len(GOOD_RAW) - 1)[0] == _lib.AF_E_CAPACITY
