"""GPU tests of the DVB-S outer decoder (dvbs_rs_kernel, dvbs_ts_finish_kernel) on the constructed error patterns of tests/rs_patterns.py, through
DvbsTailBank: every tap and every TS byte against the CPU oracle (oracle/dvbs_tail.cpp, pinned against the reference in
tests/test_oracle_rs_patterns.py) run in the same order, and against what follows from the code alone."""
import functools

import numpy as np
import pytest

import orc_dvbs_tail as ot
import rs_patterns as rp
from orc_dvbs_tail import OracleRsStage, OracleTail

pytestmark = pytest.mark.gpu

FRAME_BITS = 1632 * 8


def stage_capacity(max_bits):
    """packets one rs_stage call takes on a bank created with max_bits (include/dvbs2gpu.h, dvbs2gpu_dvbs_tail_rs_stage)"""
    return 8 * (max_bits // FRAME_BITS + 3)


def max_bits_for(npackets):
    assert npackets % 8 == 0
    return max(FRAME_BITS, (npackets // 8 - 3) * FRAME_BITS)


@functools.lru_cache(maxsize=None)
def fillers():
    """clean codewords (first byte 0x47) for padding and for the quiet parts of a sequence"""
    rng = np.random.default_rng(4711)
    f = np.stack([rp.codeword(rng) for _ in range(32)])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def sequence():
    """all patterns in order, padded to a multiple of 8 with clean packets, and the oracle's run over it: (packets, ts, status, ret, messages)"""
    pats = rp.patterns()
    pk = np.stack([q.packet for q in pats])
    pk = np.concatenate([pk, fillers()[:-len(pk) % 8]])
    out = (pk,) + OracleRsStage().run(pk)
    for a in out:
        a.setflags(write=False)
    return out


def named(name):
    return next(n for n, q in enumerate(rp.patterns()) if q.name == name)


def failing(k):
    """the k-th pattern the oracle gives up on"""
    return rp.patterns()[int(np.flatnonzero(rp.oracle_outcomes().status == 0)[k])].packet


def stage(bank):
    return bank.tap(1).reshape(-1, 204), bank.tap(2), bank.tap(3)


def assert_equals_oracle(packets, got_ts, taps, exp):
    corrected, status, nerr = taps
    ts, est, eret, emsg = exp
    assert np.array_equal(status, est), np.flatnonzero(status != est).tolist()
    assert np.array_equal(nerr, eret), np.flatnonzero(nerr != eret).tolist()
    ok = est.astype(bool)
    assert np.array_equal(corrected[ok, :188], emsg[ok])
    assert np.array_equal(corrected[~ok], packets[~ok])                  # a packet the decoder gives up on stays as it was received
    assert np.array_equal(got_ts, ts), np.flatnonzero((got_ts != ts).any(axis=1)).tolist()


@pytest.fixture(scope='module')
def one_call(engine, pkg):
    pk = sequence()[0]
    bank = pkg.DvbsTailBank(engine, 1, max_bits=max_bits_for(len(pk)))
    assert stage_capacity(bank.max_bits) == len(pk)
    ts = bank.rs_stage(pk)
    out = (ts,) + stage(bank)
    bank.close()
    return out


def test_all_patterns_one_call(one_call):
    pk, *exp = sequence()
    pats = rp.patterns()
    n = len(pats)
    ts, corrected, status, nerr = one_call
    assert ts.shape == (len(pk), 188) and corrected.shape == pk.shape and status.size == nerr.size == len(pk)
    assert_equals_oracle(pk, ts, (corrected, status, nerr), exp)
    rp.check_independent(status[:n], corrected[:n], nerr[:n])
    assert 0 in status[:n] and 1 in status[:n]
    assert sum(q.expect is not None and q.expect.padding > 0 and status[k] == 1 for k, q in enumerate(pats)) >= 1
    assert (ts[:, 0] == 0x47).all()
    # the first packet started the dispersal generator: what comes out is not the plain message
    assert pats[0].name == 'clean/b8' and not np.array_equal(ts[1, 1:], corrected[1, 1:188])


def test_three_calls_equal_one_call_and_reset(engine, pkg, one_call):
    pk, ets, est, eret, emsg = sequence()
    cuts = (0, 96, 256, len(pk))
    assert est[255] == 0 and est[256] == 0                                # the second cut lies inside a run of failed packets
    bank = pkg.DvbsTailBank(engine, 1, max_bits=max_bits_for(len(pk)))
    got = [[], [], [], []]
    for a, b in zip(cuts, cuts[1:]):
        got[0].append(bank.rs_stage(pk[a:b]))
        for k, t in enumerate(stage(bank)):
            got[k + 1].append(t)
    for g, want in zip(got, one_call):
        assert np.array_equal(np.concatenate(g), want)
    # after reset() the first failed packet hands out zeros again, and the dispersal generator is idle
    bank.reset()
    again = np.concatenate([pk[256:257], fillers()[:7]])
    ts = bank.rs_stage(again)
    assert ts[0, 0] == 0x47 and not ts[0, 1:].any()
    assert bank.tap(2)[0] == 0 and bank.tap(3)[0] == np.count_nonzero(again[0, :188])
    assert_equals_oracle(again, ts, stage(bank), OracleRsStage().run(again))
    bank.close()


def test_stale_output_sequences(engine, pkg):
    f = fillers()
    pats = rp.patterns()
    prbs = ot.prbs_bytes(187)

    def run(*calls):
        bank, orc_stage = pkg.DvbsTailBank(engine, 1, max_bits=FRAME_BITS), OracleRsStage()
        out = []
        for pk in calls:
            ts = bank.rs_stage(pk)
            taps = stage(bank)
            assert_equals_oracle(pk, ts, taps, orc_stage.run(pk))
            out.append((ts,) + taps)
        bank.close()
        return out

    # a failure as packet 0 of a fresh bank: zeros come out, and the error count is the packet's non-zero message bytes
    pk = np.concatenate([failing(0)[None], f[:7]])
    (ts, _, status, nerr), = run(pk)
    assert status[0] == 0 and not ts[0, 1:].any() and nerr[0] == np.count_nonzero(pk[0, :188])

    # a decoded packet that starts 0xB8, then two failures: the same message three times, the generator reset each time
    b8 = pats[named('clean/b8')].packet
    pk = np.concatenate([b8[None], failing(1)[None], failing(2)[None], f[:5]])
    (ts, _, status, _), = run(pk)
    assert list(status[:4]) == [1, 0, 0, 1]
    assert np.array_equal(ts[0, 1:], b8[1:188] ^ prbs) and np.array_equal(ts[1], ts[0]) and np.array_equal(ts[2], ts[0])
    assert np.array_equal(ts[3, 1:], f[0, 1:188] ^ ot.prbs_bytes(188 + 187)[188:])          # one PRBS byte skipped over the sync byte

    # a failure as the last packet of one call and as the first of the next
    c1 = np.concatenate([f[:7], failing(3)[None]])
    c2 = np.concatenate([failing(4)[None], f[7:14]])
    (ts1, _, s1, _), (ts2, _, s2, n2) = run(c1, c2)
    assert s1[7] == 0 and s2[0] == 0
    assert np.array_equal(ts1[7], ts1[6]) and np.array_equal(ts2[0], ts1[6])                # (dispersal idle: the message itself comes out)
    assert n2[0] == np.count_nonzero(c2[0, :188] != f[6, :188])

    # a failure directly behind a miscorrected packet: the WRONG message is repeated
    q = pats[named('miscorrect/9+8-inside')]
    pk = np.concatenate([q.packet[None], failing(5)[None], f[:6]])
    (ts, corrected, status, nerr), = run(pk)
    assert list(status[:2]) == [1, 0] and nerr[0] == q.expect.rs_err == 6
    assert np.array_equal(corrected[0], q.expect.corrected) and not np.array_equal(q.expect.corrected[:188], q.sent[:188])
    assert np.array_equal(ts[1, 1:], q.expect.corrected[1:188]) and np.array_equal(ts[0], ts[1])


def test_dispersal_1407_packets_without_reset(engine, pkg):
    """one 0xB8 packet, then 1407 packets without one: the PRBS table wraps at byte 32 767 (after 175 packets) and the byte position at 32 767 * 8
    (packet 1394); in one call, and cut into calls of 352 packets with the state carried between them"""
    rng = np.random.default_rng(99)
    n = 1408
    pk = rng.integers(0, 256, (n, 204), dtype=np.uint8)
    pk[:, 0] = 0x47
    pk[0, 0] = 0xB8
    assert 187 + 188 * (n - 1) > 32767 * 8 + 188
    want = OracleRsStage().run(pk, skip_rs=True)[0]
    # the oracle's bit-serial generator against the period of the byte sequence: 32 767 bytes, of which every sync byte skips one
    idx = 188 * np.arange(n)[:, None] + np.arange(187)[None, :]
    assert idx[175].max() >= 32767 and np.array_equal(want[:, 1:] ^ pk[:, 1:188], ot.prbs_bytes(32767)[idx % 32767])
    big = pkg.DvbsTailBank(engine, 1, max_bits=max_bits_for(n))
    assert stage_capacity(big.max_bits) == n
    got = big.rs_stage(pk, skip_rs=True)
    big.close()
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8].tolist()
    small = pkg.DvbsTailBank(engine, 1, max_bits=41 * FRAME_BITS)
    cap = stage_capacity(small.max_bits)
    assert cap == 352 and n % cap == 0
    got = np.concatenate([small.rs_stage(pk[a:a + cap], skip_rs=True) for a in range(0, n, cap)])
    small.close()
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8].tolist()


def _stream(order, seed):
    """the error patterns of patterns()[order] on codewords that carry the sync bytes of a DVB-S stream (0xB8 on every 8th packet), between 16
    clean packets in front (the de-interleaver's history) and 16 behind (its delay of 11 packets), as the bits of the interleaved stream"""
    rng = np.random.default_rng(seed)
    pats = rp.patterns()
    assert len(order) % 8 == 0
    coded = []
    for p in range(16 + len(order) + 16):
        cw = rp.codeword(rng, 0xB8 if p % 8 == 0 else 0x47)
        if 16 <= p < 16 + len(order):
            q = pats[order[p - 16]]
            cw = cw ^ q.packet ^ q.sent
        coded.append(cw)
    return ot.dvbs_coded_to_bits(np.stack(coded))


def test_three_streams_of_different_length_in_one_batch(engine, pkg):
    import torch
    n = len(rp.patterns())
    order0 = list(range(n)) + [0] * (-n % 8)
    order2 = list(range(n - 1, n - 121, -1))                             # the other way round: failures first, and in other places
    bits = [_stream(order0, 1), None, _stream(order2, 3)]
    bits[1] = bits[2][FRAME_BITS:FRAME_BITS + 5000].copy()               # too short for a frame
    assert bits[0].size == 38 * FRAME_BITS and bits[2].size == 19 * FRAME_BITS
    bank = pkg.DvbsTailBank(engine, 3, max_bits=bits[0].size)
    tin = [torch.from_numpy(b).cuda() for b in bits]
    tout = [torch.zeros(188 * 8 * 40, dtype=torch.uint8, device='cuda') for _ in bits]
    nb = bank.process_batch(tin, tout)
    frames, failed = [], []
    for s in range(3):
        o = OracleTail()
        e, nf = o.process(bits[s])
        assert nb[s] == e.size, (s, nb[s], e.size)
        assert np.array_equal(tout[s][:nb[s]].cpu().numpy(), e), s
        st = bank.stats(s)
        assert st['frames'] == nf, (s, st)
        if nf:
            assert st['rs_errors'] == o.last_rs, (s, st, o.last_rs)
        assert np.array_equal(bank.tap(2, s), np.asarray(o.call_status, np.uint8)), s
        assert np.array_equal(bank.tap(3, s), np.asarray(o.call_rs, np.int32)), s
        frames.append(nf)
        failed.append(np.flatnonzero(np.asarray(o.call_status) == 0).tolist())
    # the deframer may lose a frame where a pattern hits several sync bytes; nearly all of them are found
    assert frames[1] == 0 and nb[1] == 0 and frames[0] >= 34 and 15 <= frames[2] <= 19 and frames[2] <= frames[0] // 2 + 1
    assert len(failed[0]) >= 12 and len(failed[2]) >= 12 and failed[0] != failed[2]
    bank.close()


def test_high_degree_locators(engine, pkg):
    """eight packets that the reference decodes with a locator of degree 9 (tests/golden/rs_high_degree.json): 9 roots, 9 Forney lanes, up to nine
    changed message bytes; the recorded outcomes of the reference, and the oracle's run in the same order"""
    cases = rp.high_degree()
    pk = np.stack([c.packet for c in cases])
    assert pk.shape == (8, 204)
    bank = pkg.DvbsTailBank(engine, 1, max_bits=FRAME_BITS)
    ts = bank.rs_stage(pk)
    corrected, status, nerr = stage(bank)
    bank.close()
    assert status.tolist() == [1] * 8
    assert nerr.tolist() == [c.ret for c in cases] and max(nerr) > 8
    assert np.array_equal(corrected[:, :188], np.stack([c.message for c in cases]))
    assert_equals_oracle(pk, ts, (corrected, status, nerr), OracleRsStage().run(pk))
