"""CPU checks of the device-ingest boundary: the symbols and their signatures, and the one call
that needs no GPU (a failed open)."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "afgpu.h")

SIGNATURES = {
    "af_fastq_dev_open": "int af_fastq_dev_open(af_ctx *ctx, const char *fq1, const char *fq2, int64_t batch_bytes, "
                         "af_fastq_dev **out);",
    "af_fastq_dev_next": "int af_fastq_dev_next(af_fastq_dev *f, int64_t max_pairs, int64_t *n_pairs, int32_t *max_len, "
                         "int64_t *names_bytes);",
    "af_fastq_dev_export": "int af_fastq_dev_export(af_fastq_dev *f, int32_t stride, uint8_t *d_reads, int32_t *d_lens, "
                           "char *names, int64_t names_cap, int64_t *name_off, void *stream);",
    "af_fastq_dev_error": "const char *af_fastq_dev_error(const af_fastq_dev *f);",
    "af_fastq_dev_close": "void af_fastq_dev_close(af_fastq_dev *f);",
    "af_bgzf_inflate_device": "int af_bgzf_inflate_device(af_ctx *ctx, const uint8_t *file_bytes, int64_t n, uint8_t *out, "
                              "int64_t out_cap, int64_t *n_out, int32_t *bad_member);",
    "af_inflate_host": "int af_inflate_host(const uint8_t *member, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, "
                       "int32_t *stats);",
}


def _flat(s):
    return re.sub(r"\s+", " ", s)


def test_header_declares_the_signatures():
    txt = _flat(open(HEADER).read())
    for name, sig in SIGNATURES.items():
        assert _flat(sig) in txt, name


def test_library_exports_and_binding_lists_them():
    from anchored_fusion_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in SIGNATURES:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert len(getattr(_lib.lib(), name).argtypes) == SIGNATURES[name].count(",") + 1


def test_open_of_a_missing_file(tmp_path):
    from anchored_fusion_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    missing = os.fsencode(str(tmp_path / "nope_1.fq.gz"))
    rc = L.af_fastq_dev_open(None, missing, missing, 0, ctypes.byref(h))
    try:
        assert rc == _lib.AF_E_INVALID
        assert h.value
        assert "cannot open" in L.af_fastq_dev_error(h).decode()
    finally:
        L.af_fastq_dev_close(h)


def test_io_has_the_device_reader():
    from anchored_fusion_amd import io as afio
    assert callable(afio.read_pairs_device)
    assert issubclass(afio.NotBGZF, ValueError)
