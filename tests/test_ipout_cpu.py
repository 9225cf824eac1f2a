"""IP output bank without a GPU: the model of tests/ipout_ref.py against an independent reader -- every datagram stream it writes goes
through the IP-TS bank's model (tests/ipts_ref.py) and must come back as the selected packets, with no complaint -- and then the
library's host bank (IpOutBank.host, csrc/ipout_rules.h) through the C ABI against the model in bytes, rows, counters and needed sizes,
on the constructed cases, each in one call per segment and cut into calls of 1 and 7 packets, at the capacity limit, across set_flow
and reset, and with wrong arguments."""
import ctypes as C

import numpy as np
import pytest

import ipout_cases as K
import ipout_ref as R
import ipts_ref as T

CASES = K.cases()
IDS = [c[0] for c in CASES]


def drive(case, cut, bank=None):
    """the case through the model, and through stream 0 of `bank` beside it, compared call by call -> the model's datagrams per slot,
    joined over the calls, and per slot one (bytes, table) per call"""
    m = R.Stream()
    K.set_flows(m, case)
    if bank is not None:
        K.set_flows(bank, case, 0)
    joined, per_call = [b''] * R.SLOTS, [[] for _ in range(R.SLOTS)]
    for rate, ts, flush in K.calls(case, cut):
        if rate is not None:
            m.set_rate(rate)
            if bank is not None:
                bank.set_rate(0, rate)
        sizes = m.sizes(ts, flush)
        want = m.process(ts, flush)
        assert sizes == [len(w) for w in want]
        if bank is not None:
            got = bank.work(ts, 0, flush=flush)
            for slot in range(R.SLOTS):
                assert got[slot].tobytes() == want[slot], slot
                assert bank.row_table(0, slot) == m.table[slot], slot
                assert bank.needed(0, slot) == len(want[slot]), slot
                assert bank.stats(0, slot) == m.stats(slot), slot
            assert bank.stats(0) == m.stats()
        for slot in range(R.SLOTS):
            joined[slot] += want[slot]
            per_call[slot].append((want[slot], [dict(r) for r in m.table[slot]]))
    return m, joined, per_call


def test_layout(pkg):
    assert pkg.IpOutBank.layout() == R.LAYOUT
    assert C.sizeof(pkg.IpoutRow) == R.LAYOUT['row_bytes'] and C.sizeof(pkg.IpoutFlow) == R.LAYOUT['flow_bytes']
    assert pkg.IpoutRow.offset.offset % 4 == 0 and pkg.IpoutRow.bytes.offset % 4 == 0


@pytest.mark.parametrize('case', CASES, ids=IDS)
@pytest.mark.parametrize('cut', [None, 1, 7])
def test_the_ipts_model_reads_back_what_the_model_writes(case, cut):
    m, joined, per_call = drive(case, cut)
    for slot, f in case[1].items():
        reader = T.Stream()
        reader.set_flow(0, f['family'], f['dst'], f['dst_port'])
        back = b''
        for data, table in per_call[slot]:
            out = reader.process(np.frombuffer(data, np.uint8), [(r['offset'], r['bytes']) for r in table])
            want = (T.RTP if f['mode'] == R.RTP_MODE else T.RAW) | T.TS_ROW
            assert [r['flags'] for r in reader.table] == [want] * len(table)
            assert [(r['packets'], r['rtp_seq'], r['rtp_timestamp']) for r in reader.table] == [(r['packets'], r['rtp_seq'], r['rtp_timestamp']) for r in table]
            assert all(r['rtp_ssrc'] == (f['ssrc'] if f['mode'] == R.RTP_MODE else 0) and r['dst_port'] == f['dst_port'] for r in reader.table)
            back += out[0].tobytes()
        st = reader.stats(0)
        assert st['bad_checksum'] == st['lost'] == st['late'] == st['no_checksum'] == 0 and reader.stats()['bad_ip'] == 0
        sel = K.selected(case, slot)
        assert back == sel[:len(back)] and len(sel) - len(back) == 188 * m.stats(slot)['held']
        assert m.stats(slot)['ts_packets'] * 188 == len(back) and m.stats(slot)['passed'] * 188 == len(sel)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_without_flush_inside_the_cutting_does_not_show(case):
    whole = drive(case, None)[1]
    assert drive(case, 1)[1] == whole and drive(case, 7)[1] == whole


def test_the_cases_hit_what_they_are_for():
    by = {c[0]: c for c in CASES}
    m, _, per_call = drive(by['zero_checksum'], None)
    assert m.computed[0] == [0] and m.table[0][0]['udp_checksum'] == 0xFFFF and per_call[0][0][0][26:28] == b'\xff\xff'
    _, _, per_call = drive(by['wraps_and_rate_change'], None)
    rows = [r for _, t in per_call[2] for r in t]
    assert [r['rtp_seq'] for r in rows[:4]] == [65533, 65534, 65535, 0]
    stamps = [r['rtp_timestamp'] for r in rows]
    assert stamps[0] == 2 ** 32 - 20 and any(a > b for a, b in zip(stamps, stamps[1:])) and stamps[-1] == stamps[-2]      # (rate 0: the clock stands)
    _, _, per_call = drive(by['four_slots'], None)
    assert all(len(per_call[s][0][0]) for s in range(4))
    flags = {r['flags'] for c in CASES for s in c[1] for _, t in drive(c, 1)[2][s] for r in t}
    assert flags >= {0, R.RTP, R.SHORT | R.CARRIED, R.RTP | R.CARRIED, R.RTP | R.SHORT | R.CARRIED}


@pytest.mark.parametrize('case', CASES, ids=IDS)
@pytest.mark.parametrize('cut', [None, 1, 7])
def test_host_bank_equals_model(pkg, case, cut):
    drive(case, cut, pkg.IpOutBank.host(1, 64))


def test_capacity_refusal_advances_nothing_and_can_be_repeated(pkg):
    case = next(c for c in CASES if c[0] == 'four_slots')
    hb, m = pkg.IpOutBank.host(1, 64), R.Stream()
    K.set_flows(hb, case, 0), K.set_flows(m, case)
    hb.set_rate(0, K.RATE), m.set_rate(K.RATE)
    first, second = case[2][0][1], case[2][1][1]
    want = m.process(first)
    assert hb.work(first, 0)[2].tobytes() == want[2]
    before = hb.stats(0)
    need = m.sizes(second, True)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        hb.work(second, 0, cap=max(need) - 1, flush=True)
    assert e.value.code == -5 and e.value.needed == need and [hb.needed(0, k) for k in range(4)] == need
    assert hb.stats(0) == before and all(hb.row_table(0, k) == [] for k in range(4))
    want = m.process(second, True)
    got = hb.work(second, 0, cap=max(need), flush=True)
    assert [g.tobytes() for g in got] == want and hb.stats(0) == m.stats() and [hb.row_table(0, k) for k in range(4)] == m.table


def test_set_flow_and_reset(pkg):
    hb, m = pkg.IpOutBank.host(2, 64), R.Stream()
    f = K.flow(4, R.RTP_MODE, 3, port=5400)
    ts = K.packets([0x70] * 5, seed=1)
    for b in (hb, m):
        at = (1,) if b is hb else ()
        b.set_flow(*at, 0, **f)
        b.set_rate(*at, K.RATE)
    call = lambda flush=False: (hb.work(ts, 1, flush=flush)[0].tobytes(), hb.row_table(1, 0), hb.stats(1)) == (m.process(ts, flush)[0], m.table[0], m.stats())
    assert call() and hb.stats(1)['held'] == 2 and hb.stats(0) == dict.fromkeys(R.STAT_KEYS, 0)
    # set_flow drops what the slot holds and starts its sequence and counters again; the clock runs on
    hb.set_flow(1, 0, **f), m.set_flow(0, **f)
    assert hb.stats(1, 0) == dict.fromkeys(R.STAT_KEYS, 0) and call()
    assert m.table[0][0]['rtp_seq'] == f['seq_base'] and m.table[0][0]['rtp_timestamp'] > f['timestamp_base'] and not m.table[0][0]['flags'] & R.CARRIED
    # reset: state and counters go, flow and rate stay
    hb.reset(), m.reset()
    assert hb.stats(1) == dict.fromkeys(R.STAT_KEYS, 0) and call(True)
    assert m.table[0][0]['rtp_timestamp'] == f['timestamp_base'] and m.table[0][-1]['flags'] == R.RTP | R.SHORT
    # an emptied slot takes nothing
    hb.set_flow(1, 0, family=0), m.set_flow(0, family=0)
    assert call(True) and hb.work(ts, 1)[0].size == 0


def test_argument_errors(pkg):
    hb = pkg.IpOutBank.host(1, 8)
    good = K.flow()
    bad = lambda **kw: pytest.raises(pkg.Dvbs2GpuError, hb.set_flow, 0, 0, **dict(good, **kw))
    for kw in (dict(family=5, src=bytes(16), dst=bytes(16)), dict(packets_per_datagram=0), dict(packets_per_datagram=8), dict(pid_mode=1, pids=(0x2000,)),
               dict(dscp=64), dict(mode=2), dict(pid_mode=3)):
        assert bad(**kw).value.code == -1, kw
    assert hb.stats(0) == dict.fromkeys(R.STAT_KEYS, 0) and hb.work(K.packets([1]), 0)[0].size == 0         # the slot stayed empty
    with pytest.raises(pkg.Dvbs2GpuError):
        hb.set_flow(0, 4, **good)
    with pytest.raises(pkg.Dvbs2GpuError):
        hb.set_flow(1, 0, **good)
    with pytest.raises(pkg.Dvbs2GpuError):
        hb.set_rate(0, 1 << 48)
    hb.set_flow(0, 1, **good)
    lib, h = hb.lib, hb.h
    ts = K.packets([1] * 9)
    out = [np.zeros(4096, np.uint8) for _ in range(4)]
    ptrs = lambda skip=(): (C.c_void_p * 4)(*[None if k in skip else o.ctypes.data for k, o in enumerate(out)])
    nb = (C.c_int * 4)()
    work = lambda n, p: lib.dvbs2gpu_ipout_work(h, 0, C.c_void_p(ts.ctypes.data), n, p, 4096, nb, 0)
    assert work(187, ptrs()) == -1                                      # not whole packets
    assert work(9 * 188, ptrs()) == -1                                  # above max_packets
    assert work(188, ptrs(skip=(1,))) == -1                             # a set slot without a buffer
    assert work(188, ptrs(skip=(0, 2, 3))) == 0                         # empty slots need none
    assert lib.dvbs2gpu_ipout_process_batch(h, None, None, None, 0, None, None, 0, None) == -1
    h2 = C.c_void_p()
    assert lib.dvbs2gpu_ipout_create_host(1, 8193, C.byref(h2)) == -1 and lib.dvbs2gpu_ipout_create_host(0, 8, C.byref(h2)) == -1
