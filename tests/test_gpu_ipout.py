"""GPU tests of the IP output bank (csrc/ipout.hip): the kernels against the library's host bank and the model of tests/ipout_ref.py in
bytes, rows, needed sizes, counters and state through the next call, at the packet counts, datagram sizes, stream shapes and alignments
where the ballot rounds, the ranks across waves, the eight lanes per packet, the copy's and the sum's lead-in and tail, and the held
packets between calls can go wrong; and chained on the device behind the TS monitor's filter and in front of the IP-TS bank, which must
read back what went in."""
import numpy as np
import pytest

import ipout_cases as K
import ipout_ref as R
import ipts_ref as T
import tsmon_ref as TM

pytestmark = pytest.mark.gpu
PIDS = [0x100, 0x101, 0x102, 0x1FFF, 0x33]
FOUR = {0: K.flow(4, R.RTP_MODE, 7, port=5600), 1: K.flow(6, R.RAW, 1, port=5601, pid_mode=1, pids=(0x100, 0x33)),
        2: K.flow(6, R.RTP_MODE, 3, port=5602, pid_mode=2, pids=(0x101,), drop_null=True), 3: K.flow(4, R.RAW, 2, port=5603, drop_null=True)}


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def _dev(a, shift=0):
    """a on the device, `shift` bytes behind a 16-byte boundary"""
    import torch
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.zeros(a.size + 32, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    if a.size:
        buf[shift:shift + a.size] = torch.from_numpy(a.copy()).cuda()
    return buf[shift:shift + a.size]


def mux(seed, n, bad=()):
    rng = np.random.default_rng(seed)
    return K.packets([PIDS[i] for i in rng.integers(0, len(PIDS), n)], seed=seed, bad=bad)


class Rig:
    """a device bank, a host bank and one model per stream, fed the same calls.  flows[i]: {slot: keyword arguments of set_flow}"""

    def __init__(self, pkg, eng, flows, max_packets=2048, cap=1 << 18, rate=K.RATE):
        import torch
        self.pkg, self.eng, self.n = pkg, eng, len(flows)
        self.dv, self.hb = pkg.IpOutBank(eng, self.n, max_packets), pkg.IpOutBank.host(self.n, max_packets)
        self.models = [R.Stream() for _ in flows]
        self.flows, self.cap = flows, cap
        self.outs = [[torch.zeros(cap + 32, dtype=torch.uint8, device='cuda') for _ in range(4)] for _ in flows]
        for i, per in enumerate(flows):
            for slot, f in per.items():
                self.dv.set_flow(i, slot, **f), self.hb.set_flow(i, slot, **f), self.models[i].set_flow(slot, **f)
            self.set_rate(i, rate)

    def set_rate(self, i, rate):
        self.dv.set_rate(i, rate), self.hb.set_rate(i, rate), self.models[i].set_rate(rate)

    def call(self, per_stream, flush=False, shift=0, out_shift=0, cap=None):
        cap = self.cap if cap is None else cap
        ins = [None if ts is None else _dev(ts, shift) for ts in per_stream]
        # an empty slot has no buffer
        outs = [[o[out_shift:out_shift + cap] if k in self.flows[i] else None for k, o in enumerate(per)] for i, per in enumerate(self.outs)]
        k0 = self.eng.get_state('kernel_launches')
        nb = self.dv.process(ins, outs, flush=flush)
        assert self.eng.get_state('kernel_launches') - k0 == 2       # whatever the bank size
        res = []
        for i, ts in enumerate(per_stream):
            ts = np.zeros(0, np.uint8) if ts is None else ts
            want = self.models[i].process(ts, flush)
            host = self.hb.work(ts, i, flush=flush)
            for k in range(4):
                assert nb[i][k] == len(want[k]), (i, k, nb[i][k], len(want[k]))
                got = self.dv.row_table(i, k)
                for j, (a, b) in enumerate(zip(got, self.models[i].table[k])):
                    assert a == b, (i, k, j, a, b)
                assert got == self.models[i].table[k] == self.hb.row_table(i, k), (i, k)
                if k in self.flows[i]:
                    assert outs[i][k][:nb[i][k]].cpu().numpy().tobytes() == want[k], (i, k)
                assert host[k].tobytes() == want[k], (i, k)
                assert self.dv.needed(i, k) == len(want[k]) == self.hb.needed(i, k), (i, k)
                assert self.dv.stats(i, k) == self.models[i].stats(k) == self.hb.stats(i, k), (i, k)
            assert self.dv.stats(i) == self.models[i].stats() == self.hb.stats(i), i
            res.append(want)
        return res


def test_packet_counts_at_lane_wave_and_workgroup_edges(pkg, eng):
    """0, 1, 63, 64, 65, 256, 257 and 1030 packets through one bank with four different flows, so every call starts from what the one
    before left held: fewer packets than lanes, a wave edge, a round edge, more packets than threads; a bad sync byte now and then"""
    rig = Rig(pkg, eng, [FOUR])
    for c, n in enumerate([0, 1, 63, 64, 65, 256, 257, 1030, 1, 0]):
        rig.call([mux(40 + c, n, bad=(n // 2,) if n > 60 else ())], flush=c == 6, shift=c % 4, out_shift=(c + 1) % 4)
    st = rig.models[0].stats()
    assert min(st[k] for k in R.STAT_KEYS) > 0, st
    rig.call([None], flush=True)
    assert rig.models[0].stats()['held'] == 0 and rig.models[0].stats()['short_datagrams'] > 1


@pytest.mark.parametrize('P', [1, 2, 7])
def test_calls_of_one_packet(pkg, eng, P):
    """3 P calls of exactly one packet: every datagram but the first P - 1 is built from held packets and one new one, and what a call
    appends to the held packets must not disturb them"""
    rig = Rig(pkg, eng, [{1: K.flow(4 if P & 1 else 6, R.RTP_MODE, P, port=5700 + P)}], 8, 4096)
    ts = K.packets([0x90 + i for i in range(3 * P)], seed=P).reshape(-1, 188)
    made = b''
    for c, p in enumerate(ts):
        made += rig.call([p.reshape(-1)], shift=c % 4, out_shift=(3 * c) % 4)[0][1]
    assert rig.models[0].stats(1)['datagrams'] == 3 and rig.models[0].stats(1)['held'] == 0
    whole = R.Stream()
    whole.set_flow(1, **rig.flows[0][1]), whole.set_rate(K.RATE)
    assert whole.process(ts.reshape(-1))[1] == made


def test_all_sixteen_source_alignments_of_one_datagram(pkg, eng):
    rig = Rig(pkg, eng, [{0: K.flow(4, R.RTP_MODE, 7, port=5800), 2: K.flow(6, R.RAW, 7, port=5801)}], 16, 4096)
    for s in range(16):
        rig.call([mux(60 + s, 7)], shift=s, out_shift=(5 * s + 3) % 16)
    # and through held packets: 3, then 4 that complete the datagram
    for s in range(16):
        rig.call([mux(80 + s, 3 if s % 2 == 0 else 4)], shift=s, out_shift=(7 * s) % 16)
    assert rig.models[0].stats(0)['datagrams'] == 24 and rig.models[0].stats(2)['held'] == 0


def test_three_streams_with_different_flows(pkg, eng):
    """stream 0 with the four flows, stream 1 with none, stream 2 with a flow in slot 3 alone; now and then an empty input; the same
    stream alone in a bank of one gives the same"""
    flows = [FOUR, {}, {3: FOUR[0]}]
    rig, one = Rig(pkg, eng, flows, 256), Rig(pkg, eng, [FOUR], 256)
    for c in range(5):
        per = [mux(100 + 3 * c + i, 90 - 20 * i + c) for i in range(3)]
        if c in (1, 3):
            per[c % 3] = None
        res = rig.call(per, flush=c == 3, shift=c % 4, out_shift=3 - c % 4)
        assert one.call([per[0]], flush=c == 3, shift=(c + 2) % 4) == [res[0]]
    assert rig.models[1].stats() == dict(dict.fromkeys(R.STAT_KEYS, 0), packets=rig.models[1].stats()['packets'])
    assert rig.models[2].stats(3)['datagrams'] > 20 and rig.models[2].stats(0)['passed'] == 0
    assert [one.dv.stats(0, k) for k in range(4)] == [rig.dv.stats(0, k) for k in range(4)]


def test_constructed_cases_and_the_zero_checksum(pkg, eng):
    """the wraps of seq and timestamp with a rate change, the four-slot case and the datagram whose checksum comes out 0, on the device"""
    for case in K.cases():
        if case[0] not in ('zero_checksum', 'wraps_and_rate_change', 'four_slots', 'P5_family6_mode0'):
            continue
        rig = Rig(pkg, eng, [case[1]], 64, 1 << 14, rate=0)
        for c, (rate, ts, flush) in enumerate(K.calls(case)):
            if rate is not None:
                rig.set_rate(0, rate)
            rig.call([ts], flush=flush, shift=c % 4)
        if case[0] == 'zero_checksum':
            assert rig.models[0].computed[0] == [0] and rig.dv.row_table(0, 0)[0]['udp_checksum'] == 0xFFFF


def test_capacity_one_byte_short_then_exact(pkg, eng):
    rig = Rig(pkg, eng, [FOUR, {0: FOUR[3]}], 256)
    rig.call([mux(200, 50), mux(201, 9)])
    per = [mux(202, 120), mux(203, 30)]
    need = [rig.models[i].sizes(per[i], True) for i in range(2)]
    most = max(max(n) for n in need)
    before = [rig.dv.stats(i) for i in range(2)]
    outs = [[o[:most - 1] if k in rig.flows[i] else None for k, o in enumerate(p)] for i, p in enumerate(rig.outs)]
    k0 = eng.get_state('kernel_launches')
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        rig.dv.process([_dev(p) for p in per], outs, flush=True)
    assert eng.get_state('kernel_launches') - k0 == 1                 # the commit kernel did not run
    assert e.value.code == -5 and e.value.needed == need
    assert [rig.dv.stats(i) for i in range(2)] == before and [rig.dv.needed(i, k) for i in range(2) for k in range(4)] == sum(need, [])
    assert all(rig.dv.row_table(i, k) == [] for i in range(2) for k in range(4))
    rig.call(per, flush=True, cap=most)                                # the exact size works, from the state that the refusal left alone
    rig.call([mux(204, 33), mux(205, 33)], out_shift=1)                # and the state behind it is right


def test_work_with_host_buffers_on_a_device_bank(pkg, eng):
    rig = Rig(pkg, eng, [{0: FOUR[0]}, FOUR], 256)
    rig.call([mux(300, 10), mux(301, 10)])                             # both streams hold packets now
    m = rig.models[1]
    for c, flush in enumerate((False, True, False)):
        ts = mux(310 + c, 40 + c)
        want = m.process(ts, flush)
        k0 = eng.get_state('kernel_launches')
        got = rig.dv.work(ts, 1, flush=flush)
        assert eng.get_state('kernel_launches') - k0 == 2
        assert [g.tobytes() for g in got] == want and [rig.dv.row_table(1, k) for k in range(4)] == m.table and rig.dv.stats(1) == m.stats()
        assert rig.dv.row_table(0, 0) == [] and rig.dv.stats(0) == rig.models[0].stats()      # stream 0 saw nothing, and kept what it holds
    assert rig.models[0].stats()['held'] == 3
    need = m.sizes(ts, True)
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        rig.dv.work(ts, 1, cap=max(need) - 1, flush=True)
    assert e.value.code == -5 and e.value.needed == need
    want = m.process(ts, True)
    assert [g.tobytes() for g in rig.dv.work(ts, 1, cap=max(need), flush=True)] == want and rig.dv.stats(1) == m.stats()
    rig.hb.work(mux(310, 40), 1), rig.hb.work(mux(311, 41), 1, flush=True), rig.hb.work(mux(312, 42), 1), rig.hb.work(ts, 1, flush=True)
    rig.call([mux(320, 11), mux(321, 12)], flush=True)                 # the batch call goes on from there


def test_chained_on_the_device_monitor_ipout_ipts_monitor(pkg, eng):
    """TsMonitorBank (filter, output) -> IpOutBank -> IpTsBank.view_from_ipout -> TsMonitorBank, all in HBM, against the models in
    sequence: the IP-TS bank reads every datagram as RTP | TS with nothing lost and no bad checksum, and the TS that comes out is the TS
    that went in"""
    import torch
    rng = np.random.default_rng(23)
    ts, _ = TM.make_mux(rng, 600, [0x100, 0x101, 0x102, 0x103])
    ts = np.ascontiguousarray(ts, np.uint8).reshape(-1)
    keep = dict(mode=1, pids=(0x100, 0x102, 0x1FFF), drop_bad_sync=True)
    mon1, mon2, direct = (pkg.TsMonitorBank(eng, 1, 1024) for _ in range(3))
    mon1.set_filter(0, **keep)
    filt_dev = torch.zeros(ts.size + 16, dtype=torch.uint8, device='cuda')[1:]
    nfilt = mon1.process([_dev(ts)], [filt_dev])[0]
    f = K.flow(4, R.RTP_MODE, 7, port=5900, seq_base=65530, drop_null=True)
    out = pkg.IpOutBank(eng, 1, 1024)
    out.set_flow(0, 2, **f), out.set_rate(0, K.RATE)
    ip_dev = torch.zeros(nfilt // 188 * 240 + 64, dtype=torch.uint8, device='cuda')[5:]
    nip = out.process([filt_dev], [[None, None, ip_dev]], nbytes=[nfilt], flush=True)[0][2]
    view, src = pkg.IpTsBank.view_from_ipout(out, ip_dev, 0, 2)
    assert src is ip_dev and view.kind == pkg.IpTsBank.KIND_RAW_IP and view.n == out.stats(0, 2)['datagrams'] > 10
    back = pkg.IpTsBank(eng, 1, 512)
    back.set_flow(0, 1, 4, f['dst'], f['dst_port'])
    ts_dev = torch.zeros(nfilt + 8, dtype=torch.uint8, device='cuda')[3:]
    nts = back.process([view], [[None, ts_dev]])[0][1]
    mon2.process([ts_dev], None, nbytes=[nts])
    # the models in sequence
    m1 = TM.Monitor()
    m1.set_filter(**keep)
    filt = m1.process(ts)
    assert nfilt == filt.size and np.array_equal(filt_dev[:nfilt].cpu().numpy(), filt)
    m2 = R.Stream()
    m2.set_flow(2, **f), m2.set_rate(K.RATE)
    ip_want = m2.process(filt, True)[2]
    assert nip == len(ip_want) and ip_dev[:nip].cpu().numpy().tobytes() == ip_want and out.row_table(0, 2) == m2.table[2] and out.stats(0) == m2.stats()
    m3 = T.Stream()
    m3.set_flow(1, 4, f['dst'], f['dst_port'])
    ts_want = m3.process(np.frombuffer(ip_want, np.uint8), [(r['offset'], r['bytes']) for r in m2.table[2]])[1]
    assert back.row_table(0) == m3.table and {r['flags'] for r in m3.table} == {T.RTP | T.TS_ROW}
    st = back.stats(0)
    assert st == m3.stats() and st['lost'] == 0 and st['bad_checksum'] == 0 and st['late'] == 0 and st['ts'] == view.n
    sent = filt.reshape(-1, 188)
    sent = sent[(sent[:, 1] & 31).astype(int) * 256 + sent[:, 2] != 0x1FFF].reshape(-1)           # the flow drops the null packets that the filter let pass
    assert 0 < sent.size < filt.size and nts == ts_want.size == sent.size and np.array_equal(ts_dev[:nts].cpu().numpy(), sent)
    direct.process([_dev(sent)], None)
    m4 = TM.Monitor()
    m4.process(sent)
    assert mon2.stats(0) == direct.stats(0) == m4.stats() and mon2.pid_table(0) == direct.pid_table(0) == m4.table
