"""GPU test of the three instantiations of the datagram-bank core (csrc/dgram_bank.h) side by side: a T2-MI, an MPE and a ULE bank on
one engine and the same HBM buffers, each against its model and its host bank (the Rigs of test_gpu_t2mi.py, test_gpu_mpe.py and
test_gpu_ule.py)."""
import numpy as np
import pytest

import t2mi_ref as T
import test_gpu_mpe as TM
import test_gpu_t2mi as TT
import test_gpu_ule as TU

pytestmark = pytest.mark.gpu
TP, MP, UP = 0x0310, 0x0311, 0x0312


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def t2mi_feed(rng, cc, mids, last):
    """-> (the TS packets of a T2-MI PID, how many of them lie before the 8202-byte packet, the continuity counter and the
    packet_count behind the first TS packet).  The first TS packet holds two whole packets.  Behind it: a packet whose count skips
    one, BBFRAMEs of 10 to 700 bytes with a CRC-damaged packet between two good ones, an 8202-byte packet that starts in mid TS packet
    and so lies in 46 of them, and more BBFRAMEs.  mids, last: BBFRAME sizes that place that start."""
    z, count = T.Packetiser(TP, cc), int(rng.integers(256))
    data = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))
    bb = lambda n: T.bb_packet(count, (3, 5)[count & 1], data(n), frame_idx=count)

    def some(sizes):
        nonlocal count
        out = []
        for n in sizes:
            count = (count + 1) & 255
            out.append(bb(n))
        return out

    first = z.lay(some([10, 60]))
    cc1, count1 = z.cc, count
    count = (count + 1) & 255                                        # the skipped packet_count
    pre = some([700, mids[0], 300, 10, mids[1], 25, last])
    bad = bytearray(pre[2])
    bad[20] ^= 0x10
    pre[2] = bytes(bad)
    count = (count + 1) & 255
    big = T.t2mi_packet(0x10, count, data(8192), payload_bits=65535)
    tail = some([10, 700, 300, 33, 250])
    before = z.lay(pre, flush=False)
    assert len(first) == 1 and len(z.data) > 77 and len(big) == 8202  # the 8202 bytes start late enough in a TS packet to end in the 46th
    rest = np.concatenate([z.lay([big], flush=False), z.lay(tail)])
    return np.concatenate([first, before, rest]), 1 + len(before), cc1, count1


def multiplex(rng, t, t_before_big, mpe_cc, ule_cc):
    """130 packets: the first T2-MI TS packet alone, then 64 and 65 packets in which the three PIDs mix, 20 of the 46 TS packets of the
    8202-byte packet among the 64"""
    t1 = t_before_big - 1 + 20                                       # T2-MI TS packets of the second call
    t2 = len(t) - 1 - t1
    assert 0 < t1 < 60 and 26 < t2 < 60
    m1, m2 = (64 - t1) // 2, (65 - t2) // 2
    u1, u2 = 64 - t1 - m1, 65 - t2 - m2
    m, u = TM.feed(rng, MP, m1 + m2, [28, 100, 700], cc=mpe_cc), TU.feed(rng, UP, u1 + u2, [28, 100, 700], cc=ule_cc)
    out, at = [t[0]], [1, 0, 0]
    for counts in ((t1, m1, u1), (t2, m2, u2)):
        order = np.concatenate([np.full(c, k) for k, c in enumerate(counts)])
        rng.shuffle(order)
        for k in order:
            out.append((t, m, u)[k][at[k]])
            at[k] += 1
    assert at == [len(t), len(m), len(u)] and len(out) == 130
    return np.array(out, np.uint8).reshape(-1, 188)


def test_a_t2mi_an_mpe_and_a_ule_bank_side_by_side(pkg, eng):
    """the three banks are three instantiations of one core in one process and share no state: on one engine a T2miBank, an MpeBank
    and a UleBank take the same two streams, each carrying a T2-MI, an MPE and a ULE PID interleaved, in calls of 1, 64 and 65 packets,
    turn and turn about.  Every call of every bank equals its model and its host bank in bytes, rows, needed sizes and counters and
    costs two launches (Rig.call in the three modules); the T2-MI bank's frame sizes are its delivered rows' bbframe_bytes in order.
    The T2-MI feed (t2mi_feed) has several packets complete per call, the packet whose count skips one first in the second call, with
    the valid packet before it in the first, a CRC-damaged packet between two good ones, and an 8202-byte packet in 46 TS packets
    across the second and third call.  The call of 64 packets first goes to a trio of banks with max_rows = 2 that took the first call
    too: it fails for capacity in all three and advances nothing -- the T2-MI bank then takes the packet with the next packet_count
    without a COUNT_ERROR -- and is repeated on the banks with room."""
    rng = np.random.default_rng(22)
    feeds = [t2mi_feed(rng, 5 * i, *sizes) for i, sizes in enumerate((((150, 450), 80), ((640, 77), 120)))]
    ts = [multiplex(rng, f[0], f[1], i, 3 + i) for i, f in enumerate(feeds)]
    for f in feeds:
        whole = T.Slot(TP)
        whole.process(f[0])
        assert [r['last_packet'] - r['first_packet'] + 1 for r in whole.table if r['length'] == 8202] == [46]
    wt = [[(0, TP, -1)], [(1, TP, -1), (2, TP, 5), (3, MP, -1)]]
    wm = [[(0, MP, None, None)], [(1, MP, None, None), (2, UP, None, None)]]
    wu = [[(0, UP, None, None, True)], [(3, UP, None, None, True), (1, TP, None, None, True)]]
    t2, mpe, ule = TT.Rig(pkg, eng, 2, 65, 64, watches=wt), TM.Rig(pkg, eng, 2, 65, 64, watches=wm), TU.Rig(pkg, eng, 2, 65, 64, watches=wu)
    rigs = (t2, mpe, ule)
    tight = [pkg.T2miBank(eng, 2, 65, 2), pkg.MpeBank(eng, 2, 65, 2), pkg.UleBank(eng, 2, 65, 2)]
    for bank, watches in zip(tight, (wt, wm, wu)):
        for i in range(2):
            for w in watches[i]:
                bank.set_watch(i, *w)
    calls = [[t[a:b] for t in ts] for a, b in ((0, 1), (1, 65), (65, 130))]
    dev = lambda call: ([TT._dev(t) for t in call], None, [t.size for t in call])

    def t2_call(call, shift):
        t2.call(call, shift=shift)
        for i in range(2):
            for k in range(4):
                sizes = t2.models[i].frame_bytes(k)
                assert t2.dv.frame_bytes(i, k) == [r['bbframe_bytes'] for r in t2.dv.row_table(i, k) if r['offset'] >= 0] == sizes, (i, k)
                assert t2.dv.needed(i, k) == t2.hb.needed(i, k) == (sum(sizes), len(t2.models[i].table(k))), (i, k)

    t2_call(calls[0], 0), mpe.call(calls[0], shift=1), ule.call(calls[0], shift=2)
    assert [len(t2.models[i].table(k)) for i, k in ((0, 0), (1, 1))] == [2, 2]
    undelivered = lambda st: {n: v for n, v in st.items() if n not in ('datagrams_delivered', 'bbframes_delivered', 'bytes_delivered')}   # (they take rows only)
    failed, was = [], []
    for bank, rig in zip(tight, rigs):
        ins, outs, nbytes = dev(calls[0])
        bank.process(ins, outs, nbytes=nbytes)
        was.append([[bank.stats(i, k) for k in range(4)] for i in range(2)])
        assert all(undelivered(was[-1][i][k]) == undelivered(rig.dv.stats(i, k)) and was[-1][i][k]['bytes_delivered'] == 0 for i in range(2) for k in range(4))
    for bank, before in zip(tight, was):
        ins, outs, nbytes = dev(calls[1])
        with pytest.raises(pkg.Dvbs2GpuError) as e:
            bank.process(ins, outs, nbytes=nbytes)
        assert e.value.code == -5 and all(bank.stats(i, k) == before[i][k] and bank.row_table(i, k) == [] for i in range(2) for k in range(4))
        failed.append(e.value)
    assert all(tight[0].frame_bytes(i, k) == [] for i in range(2) for k in range(4))
    t2_call(calls[1], 3), mpe.call(calls[1], shift=2), ule.call(calls[1], shift=1)         # the repeat, with room
    for e, bank, rig in zip(failed, tight, rigs):
        rows = [[rig.dv.needed(i, k)[1] for k in range(4)] for i in range(2)]
        assert e.rows == rows and max(max(r) for r in rows) > 2 and e.needed == [[-1 if n > 2 else 0 for n in r] for r in rows]
        assert [[bank.needed(i, k) for k in range(4)] for i in range(2)] == [[(b, n) for b, n in zip(e.needed[i], rows[i])] for i in range(2)]
    for i, k in ((0, 0), (1, 1)):                                    # the second call as the feed was built
        flags = [r['flags'] for r in t2.models[i].table(k)]
        assert flags[0] & T.COUNT_ERROR and flags[2] == T.CRC_ERROR and not (flags[1] | flags[3]) & T.CRC_ERROR and len(flags) == 7
        assert len(t2.models[i].slot[k].buf) > 184                   # the 8202-byte packet is open
    # the tight T2-MI bank still carries the first call's packet_count: the next one is in order
    for i, (_, _, cc1, count1) in enumerate(feeds):
        nxt = T.Packetiser(TP, cc1).lay([T.bb_packet(count1 + 1, 3, bytes(10))])
        ins, outs, nbytes = dev([nxt if j == i else TT.NONE for j in range(2)])
        tight[0].process(ins, outs, nbytes=nbytes)
        k = (0, 1)[i]
        assert [r['flags'] for r in tight[0].row_table(i, k)] == [T.BBFRAME] and tight[0].stats(i, k)['count_errors'] == 0
    t2_call(calls[2], 1), mpe.call(calls[2], shift=3), ule.call(calls[2], deliver=False)
    assert all(bank.stats(i, k) == before[i][k] for bank, before in zip(tight[1:], was[1:]) for i in range(2) for k in range(4))   # untouched by the others' calls
    for i, k in ((0, 0), (1, 1)):
        rows = t2.models[i].table(k)
        assert (rows[0]['length'], rows[0]['first_packet'], rows[0]['packet_type']) == (8202, -1, 0x10) and len(rows) == 6
    st = t2.models[1].stats(1)
    assert st['t2mi_packets'] == 15 and st['crc_errors'] == 1 and st['count_errors'] == 2 and st['bbframes'] == st['bbframes_delivered'] == 13
    assert 0 < t2.models[1].stats(2)['bbframes_delivered'] < 13 and t2.models[1].stats(3)['bbframes'] == 0 and t2.models[1].stats(3)['packets'] > 0
    assert mpe.models[1].stats(1)['datagrams_delivered'] > 3 and mpe.models[1].stats(2)['datagrams'] == 0
    assert ule.models[1].stats(3)['datagrams'] > 3 and ule.models[1].stats(1)['datagrams'] == 0
