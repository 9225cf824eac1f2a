"""GSE on the device, the parts that need no GPU: dvbs2gpu_crc32_mpeg_shift (the x^(8n) mod P step with which the kernels combine
the CRC-32 of fragments computed apart) against the bitwise CRC of tests/orc_bbts.py, and the new symbols and record sizes."""
import ctypes as C

import numpy as np
import pytest

import orc_bbts as B


@pytest.fixture(scope='module')
def lib(pkg):
    return pkg.load_library()


def crc0(data):
    return B.crc32_mpeg(data, 0)


def test_shift_combines_the_crc_of_two_parts(lib):
    rng = np.random.default_rng(40)
    for _ in range(200):
        n = int(rng.integers(0, 5000))
        cut = int(rng.integers(0, n + 1))
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        a, b = d[:cut], d[cut:]
        assert B.crc32_mpeg(d) == lib.dvbs2gpu_crc32_mpeg_shift(B.crc32_mpeg(a), len(b)) ^ crc0(b)
        assert crc0(d) == lib.dvbs2gpu_crc32_mpeg_shift(crc0(a), len(b)) ^ crc0(b)


@pytest.mark.parametrize('n', [0, 1, 4, 65535, 65536, 200000])
def test_shift_is_n_zero_bytes(lib, n):
    for start in (0xffffffff, 0, 1, 0x80000000, 0x04c11db7, 0xdeadbeef):
        if n <= 70000:      # the bitwise reference over 200000 bytes is checked once, below, through additivity
            assert lib.dvbs2gpu_crc32_mpeg_shift(start, n) == B.crc32_mpeg(bytes(n), start)
    # the register's initial value goes through the same step: crc(d) = shift(0xffffffff, len d) ^ crc0(d)
    d = np.random.default_rng(n).integers(0, 256, min(n, 70000), dtype=np.uint8).tobytes()
    assert B.crc32_mpeg(d) == lib.dvbs2gpu_crc32_mpeg_shift(0xffffffff, len(d)) ^ crc0(d)
    # shifts add up, also past the 2^17-byte table
    assert lib.dvbs2gpu_crc32_mpeg_shift(lib.dvbs2gpu_crc32_mpeg_shift(0x12345678, n), 777) == lib.dvbs2gpu_crc32_mpeg_shift(0x12345678, n + 777)


def test_symbols_and_record_sizes(pkg, lib):
    for name in ('dvbs2gpu_bbts_set_gse_path', 'dvbs2gpu_bbts_get_gse_stats', 'dvbs2gpu_bbts_get_pdu_table', 'dvbs2gpu_bbts_get_pdu_table_device',
                 'dvbs2gpu_crc32_mpeg_shift'):
        assert name in pkg.PROTOTYPES and getattr(lib, name)
    assert C.sizeof(pkg.GseStats) == 96 and C.sizeof(pkg.GsePdu) == 16
    assert [k for k, _ in pkg.GseStats._fields_][-3:] == ['host_fallback_calls', 'fallback_records', 'fallback_capacity']
    for m in ('set_gse_path', 'gse_stats', 'pdu_table'):
        assert callable(getattr(pkg.BbTsParserBank, m))
    # without a handle the calls answer with an error, they do not crash
    assert lib.dvbs2gpu_bbts_set_gse_path(None, 0) < 0 and lib.dvbs2gpu_bbts_get_gse_stats(None, 0, None) < 0
