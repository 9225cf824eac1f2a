"""The FEC encoder's rules through the library's host-only entry point (dvbs2gpu_fec_encode_plan_dump, csrc/fec_encode_rules.h), no GPU:
the BCH generator polynomial of every code against the one the oracle's encoder implies (bch_patterns.generator; that encoder is pinned to the reference's by
test_oracle_bch_all_codes.py), the cut of a frame into chunks, and the argument errors of the entry point."""
import ctypes as C

import numpy as np
import pytest

import bch_patterns as bp
import orc


@pytest.mark.parametrize('rate,short', orc.ALL_CODES, ids=['%s-%s' % (orc.RATE_NAMES[r].replace('/', '_'), 'short' if s else 'normal') for r, s in orc.ALL_CODES])
def test_generator_polynomial_equals_the_oracle_encoders(pkg, rate, short):
    p = orc.fec_params(rate, short)
    plan = pkg.fec_encode_plan(rate, bool(short))
    gen = plan['generator']
    assert gen.dtype == np.uint8 and set(np.unique(gen)) <= {0, 1}
    assert len(gen) - 1 == p['m'] * p['t'] == plan['parity_bits'] == p['K'] - p['kbch'] and gen[-1] == 1 and gen[0] == 1
    g = sum(int(c) << k for k, c in enumerate(gen))
    assert g == bp.generator(rate, short)


@pytest.mark.parametrize('rate,short', orc.ALL_CODES)
def test_plan_counts(pkg, rate, short):
    p = orc.fec_params(rate, short)
    plan = pkg.fec_encode_plan(rate, bool(short))
    kb, L, n = p['kbch'] // 8, plan['chunk_bytes'], plan['bch_chunks']
    assert n == 64 and L == -(-kb // n)
    assert plan['seams'] == [8 * (kb - k * L) for k in range(n - 1, 0, -1) if kb - k * L > 0] and len(plan['seams']) >= 32
    assert all(0 < s < p['kbch'] and s % 8 == 0 for s in plan['seams'])
    assert plan['layers'] * 360 == p['N'] - p['K']
    assert 360 * plan['links'] + 2 * (p['N'] - p['K']) - 1 == pkg.fec_info(rate, bool(short))['ldpc_edges']
    assert plan['bch_frames_per_workgroup'] >= 1 and plan['ldpc_frames_per_workgroup'] >= 1 and plan['max_workgroups'] >= 1 and plan['ber_chunk_frames'] >= 1


def test_plan_dump_argument_errors(pkg):
    lib = pkg.load_library()
    cnt = (C.c_int32 * 80)()
    for rate, short in ((-1, 0), (11, 0), (10, 1), (99, 1)):
        assert lib.dvbs2gpu_fec_encode_plan_dump(rate, short, None, cnt) == -1
        assert b'no such code' in lib.dvbs2gpu_last_error()
        with pytest.raises(pkg.Dvbs2GpuError):
            pkg.fec_encode_plan(rate, bool(short))
    assert lib.dvbs2gpu_fec_encode_plan_dump(6, 0, None, None) == -1 and b'null pointer' in lib.dvbs2gpu_last_error()
    for name in ('dvbs2gpu_bb_scramble_batch', 'dvbs2gpu_bch_encode_batch', 'dvbs2gpu_ldpc_encode_batch', 'dvbs2gpu_fec_encode_batch', 'dvbs2gpu_fec_channel_ber_batch'):
        assert hasattr(lib, name) and name in pkg.PROTOTYPES
    # without a context the calls answer with the argument error, they do not crash
    assert lib.dvbs2gpu_fec_encode_batch(None, 6, 0, None, 1, None, None, 0, None) == -1 and b'no context' in lib.dvbs2gpu_last_error()
    assert lib.dvbs2gpu_fec_channel_ber_batch(None, 6, 0, None, None, None, 1, None, None, None) == -1
