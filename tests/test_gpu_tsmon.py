"""GPU tests of the TS monitor bank (csrc/tsmon.hip): the kernels against the library's host bank and the model of tests/tsmon_ref.py,
byte for byte and counter for counter, at the packet counts, PID shapes and call boundaries where the sort, the walk and the prefix
sums can go wrong."""
import numpy as np
import pytest

import orc_bbts as B
import tsmon_ref as T

pytestmark = pytest.mark.gpu

PIDS = [0, 0x11, 0x100, 0x101, 0x1FFE]


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def _damaged(seed, n, pids=PIDS, **kw):
    rng = np.random.default_rng(seed)
    ts, info = T.make_mux(rng, n, pids, **kw)
    for inject in T.INJECTORS:
        ts, info, _ = inject(rng, ts, info)
    return ts


def _dev(ts, shift=0):
    import torch
    buf = torch.zeros(ts.size + 8, dtype=torch.uint8, device='cuda')
    buf[shift:shift + ts.size] = torch.from_numpy(np.ascontiguousarray(ts).reshape(-1)).cuda()
    return buf[shift:]


class Rig:
    """a device bank, a host bank and one model per stream, fed the same calls"""

    def __init__(self, pkg, eng, nstreams, max_packets, filters=None):
        import torch
        self.n, self.mp = nstreams, max_packets
        self.dv, self.hb = pkg.TsMonitorBank(eng, nstreams, max_packets), pkg.TsMonitorBank.host(nstreams, max_packets)
        self.models = [T.Monitor() for _ in range(nstreams)]
        self.outs = [torch.zeros(max_packets * 188 + 8, dtype=torch.uint8, device='cuda') for _ in range(nstreams)]
        for i, f in enumerate(filters or []):
            self.set_filter(i, **f)

    def set_filter(self, i, **f):
        self.dv.set_filter(i, **f), self.hb.set_filter(i, **f), self.models[i].set_filter(**f)

    def call(self, per_stream, filtered=True, shift=0):
        """per_stream[i]: the packets of stream i ([k, 188], k may be 0)"""
        ins = [_dev(ts, shift) for ts in per_stream]
        nbytes = [ts.size for ts in per_stream]
        outs = [o[(4 - shift) % 4:] for o in self.outs]            # with an unaligned input an aligned output, and the other way round
        nb = self.dv.process(ins, outs if filtered else None, nbytes=nbytes)
        for i, ts in enumerate(per_stream):
            want = self.models[i].process(ts)
            host = self.hb.work(ts, stream=i, filtered=filtered)
            if filtered:
                assert nb[i] == want.size, (i, nb[i], want.size)
                assert np.array_equal(outs[i][:nb[i]].cpu().numpy(), want), i
                assert np.array_equal(host, want), i
            assert self.dv.pid_table(i) == self.models[i].table == self.hb.pid_table(i), i
            assert self.dv.stats(i) == self.models[i].stats() == self.hb.stats(i), i


def test_packet_counts_at_wave_and_workgroup_edges(pkg, eng):
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, 600]
    ts = _damaged(1, sum(sizes) + 10)[:sum(sizes)]
    rig = Rig(pkg, eng, 1, 600, [dict(mode=2, pids=[0x100], drop_null=True)])
    stats_only = Rig(pkg, eng, 1, 600, [dict(mode=1, pids=[0x11, 0x101])])
    a = 0
    for k, s in enumerate(sizes):
        rig.call([ts[a:a + s]], shift=k % 2)
        stats_only.call([ts[a:a + s]], filtered=False)
        a += s
    st = rig.models[0].stats()
    assert st['cc_errors'] > 0 and st['duplicates'] > 0 and st['discontinuities'] == 1 and 0 < st['passed_packets'] < st['packets']
    assert stats_only.models[0].stats()['passed_packets'] > 0


def test_pid_shapes(pkg, eng):
    rng = np.random.default_rng(5)
    one = np.array([T.packet(0x44, c & 15, rng=rng) for c in [0, 1, 2, 2, 3, 5] + list(range(6, 500))])     # the longest chain: one PID
    own = list(rng.permutation(np.arange(3, 0x1FFE))[:317]) + [0, 0x1FFE, 0x1FFF]
    each = np.array([T.packet(int(p), 3, rng=rng) for p in rng.permutation(own)])                            # 320 PIDs, one packet each
    mixed = _damaged(6, 400, pids=[0, 0x1FFE, 0x30])
    rig = Rig(pkg, eng, 3, 512, [dict(), dict(mode=1, pids=[0, 0x1FFE, 0x1FFF]), dict(mode=2, pids=[0x1FFE])])
    rig.call([one[:250], each, mixed[:200]])
    assert len(rig.models[1].table) == 320 and rig.models[1].stats()['pids_seen'] == 319
    rig.call([one[250:], each[::-1], mixed[200:]])                                                           # the same CC again: 319 duplicates
    assert rig.models[1].stats()['duplicates'] == 319 and rig.models[0].stats()['cc_errors'] == 1 and rig.models[0].stats()['duplicates'] == 1
    assert {0, 0x1FFE, 0x1FFF} <= {r[0] for r in rig.models[2].table}


def _edge_streams():
    """(first call, second call, third call) per stream: state that must cross a call boundary"""
    pid, out = 0x50, []

    def pk(cc, afc=1, di=0, p=pid):
        return T.packet(p, cc, afc=afc, di=di)
    for run in (2, 3, 4, 5):                                       # equal-CC runs of payload packets, cut after their 1st, 2nd, 3rd packet
        for cut in (1, 2, 3):
            seq = [pk(7)] + [pk(8)] * run + [pk(9), pk(9)]
            out.append((seq[:1 + cut], seq[1 + cut:], []))
    out.append(([pk(1), pk(2), pk(5, p=0x51)], [pk(6, p=0x51), pk(3)], []))          # a PID first seen in the last packet of a call
    out.append(([pk(1), pk(2)], [pk(9, afc=3, di=1), pk(10)], [pk(4, afc=2, di=1), pk(4, afc=2), pk(5)]))   # DI on the first packet of a call
    out.append(([pk(1)], [pk(1, afc=2), pk(2)], [pk(2, afc=2)]))                     # adaptation only, between payload packets, across calls
    out.append(([pk(1), pk(1, afc=2)], [pk(2), pk(2), pk(2, afc=2)], [pk(2), pk(4, afc=2)]))
    out.append(([pk(3), pk(3)], [pk(3)], [pk(3), pk(3)]))          # duplicate, error, duplicate, error
    return [tuple(np.array(c, np.uint8).reshape(-1, 188) for c in s) for s in out]


def test_state_crosses_call_boundaries(pkg, eng):
    streams = _edge_streams()
    rig = Rig(pkg, eng, len(streams), 8)
    for c in range(3):
        rig.call([s[c] for s in streams])
    got = [(m.stats()['duplicates'], m.stats()['cc_errors']) for m in rig.models]
    assert got[:12] == [(2, 0)] * 3 + [(2, 1)] * 3 + [(3, 1)] * 3 + [(3, 2)] * 3, got     # 8 once or run/2 times, 9 once; the rest are errors
    assert got[12:] == [(0, 0), (0, 0), (0, 0), (2, 1), (2, 2)], got
    assert rig.models[13].stats()['discontinuities'] == 2


FILTERS = [dict(mode=1, pids=[0x100]), dict(mode=2, pids=[0x100]), dict(mode=1, pids=list(range(0x0f0, 0x117)) + [0x1FFF]),
           dict(mode=2, pids=list(range(0x101, 0x128)) + [0]), dict(drop_null=True), dict(drop_tei=True), dict(drop_bad_sync=True)]


def test_filters_and_capacity(pkg, eng):
    import torch
    ts = _damaged(9, 300)                                          # its TEI packet and its bad sync byte come in the second call
    rig = Rig(pkg, eng, 1, 300)
    for f in FILTERS:
        assert len(f.get('pids', [0])) in (1, 40)
        rig.dv.reset(), rig.hb.reset()
        rig.models[0] = T.Monitor()
        rig.set_filter(0, **f)
        rig.call([ts[:120]])
        probe = T.Monitor()
        probe.set_filter(**f)
        need = probe.process(ts[120:]).size
        assert 0 < need < ts[120:].size                           # every filter drops something here
        before, table = rig.dv.stats(), rig.dv.pid_table()
        src = _dev(ts[120:])
        short = torch.zeros(need - 188, dtype=torch.uint8, device='cuda')
        with pytest.raises(pkg.Dvbs2GpuError) as e:
            rig.dv.process([src], [short], nbytes=[ts[120:].size])
        assert e.value.code == -5 and e.value.needed == [need]
        assert rig.dv.stats() == before and rig.dv.pid_table() == [] and table != []
        exact = torch.zeros(need, dtype=torch.uint8, device='cuda')
        assert rig.dv.process([src], [exact], nbytes=[ts[120:].size]) == [need]
        want = rig.models[0].process(ts[120:])
        assert np.array_equal(exact.cpu().numpy(), want)           # input order, nothing else
        assert rig.dv.stats() == rig.models[0].stats() and rig.dv.pid_table() == rig.models[0].table
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        rig.dv.process([src], [src], nbytes=[188])                 # the output is the input
    assert e.value.code == -1


# as the sources of the commit before the banks shared their count checks spell them, behind each bank's prefix
COUNT_ERRORS = ('a byte count is a whole number of 188-byte packets', 'packet count exceeds max_packets')


def test_count_error_texts_of_both_banks(pkg, eng):
    """187 bytes and max_packets + 1 packets, through the batch call and through the host-buffer call of a device bank"""
    import torch
    mp = 8
    buf = torch.zeros((mp + 1) * 188, dtype=torch.uint8, device='cuda')
    host = np.zeros((mp + 1) * 188, np.uint8)
    for bank, prefix in ((pkg.TsMonitorBank(eng, 2, mp), 'TS monitor: '), (pkg.PsiBank(eng, 2, mp, 16), 'PSI bank: ')):
        for nbytes, text in zip((187, (mp + 1) * 188), COUNT_ERRORS):
            with pytest.raises(pkg.Dvbs2GpuError) as e:
                bank.process([buf, buf], nbytes=[188, nbytes])
            assert e.value.code == -1 and str(e.value) == 'dvbs2gpu %s (-1): %s%s' % (pkg.ERR_NAMES[-1], prefix, text)
            with pytest.raises(pkg.Dvbs2GpuError) as e:
                bank.work(host[:nbytes], stream=1)
            assert e.value.code == -1 and str(e.value) == 'dvbs2gpu %s (-1): %s%s' % (pkg.ERR_NAMES[-1], prefix, text)
        assert bank.stats(0)['packets'] == bank.stats(1)['packets'] == 0       # nothing was taken


def test_70_streams_and_launch_count(pkg, eng):
    rng = np.random.default_rng(70)
    n, mp = 70, 128
    muxes = [_damaged(200 + i, 40 + 3 * i, pids=[0, 0x20 + i, 0x1000 + i, 0x1FFE]) for i in range(n)]
    filters = [dict(mode=i % 3, pids=[0x20 + i, 0x1FFF][:1 + i % 2], drop_null=i % 5 == 0, drop_tei=i % 7 == 0, drop_bad_sync=i % 4 == 0) for i in range(n)]
    rig = Rig(pkg, eng, n, mp, filters)
    sizes = [[0 if (i + c) % 9 == 0 else int(rng.integers(1, min(mp, len(muxes[i]) // 2) + 1)) for i in range(n)] for c in range(2)]
    k0 = eng.get_state('kernel_launches')
    rig.call([muxes[i][:sizes[0][i]] for i in range(n)])
    many = eng.get_state('kernel_launches') - k0
    rig.call([muxes[i][sizes[0][i]:sizes[0][i] + sizes[1][i]] for i in range(n)])
    single = Rig(pkg, eng, 1, mp, filters[3:4])
    k0 = eng.get_state('kernel_launches')
    single.call([muxes[3][:sizes[0][3]]])
    assert eng.get_state('kernel_launches') - k0 == many == 2
    k0 = eng.get_state('kernel_launches')
    rig.call([muxes[i][:5] for i in range(n)], filtered=False)
    assert eng.get_state('kernel_launches') - k0 == 1


def test_chained_behind_the_packetiser_in_hbm(pkg, eng):
    """the output buffer of a BbTsParserBank call is the monitor's input: no host copy in between"""
    import torch
    rng = np.random.default_rng(9)
    mux, info = T.make_mux(rng, 160, PIDS)
    for inject in (T.drop_packet, T.repeat_twice, T.flip_tei, T.discontinuity):
        mux, info, _ = inject(rng, mux, info)
    kbch, nfr = 14232, 16
    frames = B.bbframes_from_ts(mux, kbch, nfr)
    bank = pkg.BbTsParserBank(eng, 1, kbch, nfr)
    ts_dev = torch.zeros(nfr * kbch // 8 + 376, dtype=torch.uint8, device='cuda')
    nb = bank.process_batch([torch.from_numpy(frames.reshape(-1)).cuda()], [ts_dev])[0]
    assert nb % 188 == 0 and nb // 188 >= nfr * (kbch // 8 - 10) // 188 - 1
    mon = pkg.TsMonitorBank(eng, 1, 256)
    mon.set_filter(0, mode=1, pids=[0x100, 0x11])
    out = torch.zeros(256 * 188, dtype=torch.uint8, device='cuda')
    got = mon.process([ts_dev], [out], nbytes=[nb])[0]
    m = T.Monitor()
    m.set_filter(mode=1, pids=[0x100, 0x11])
    want = m.process(mux[:nb // 188])
    assert mon.pid_table() == m.table and mon.stats() == m.stats() and m.stats()['cc_errors'] > 0
    assert got == want.size and np.array_equal(out[:got].cpu().numpy(), want)
    p, rows = mon.pid_table_device()
    assert rows == len(m.table) and p
