"""The three instantiations of the datagram-bank core (csrc/dgram_bank.h, csrc/dgram_rules.h) without a GPU: a T2-MI, an MPE and a ULE
host bank side by side over one multiplex, each against its model (tests/t2mi_ref.py, mpe_ref.py, ule_ref.py); and the error texts of
the T2-MI bank, which the core now puts together, as the literals they were when the bank had its own copy of every function."""
import ctypes as C

import numpy as np
import pytest

import mpe_ref as RM
import psi_ref as S
import t2mi_ref as T
import ule_ref as RU
from test_gpu_mpe import feed as mpe_feed
from test_gpu_t2mi import feed as t2mi_feed
from test_gpu_ule import feed as ule_feed

TP, MP, UP = 0x0310, 0x0311, 0x0312


class Side:
    """a host bank of one stream and its model, fed the same calls; watches: the arguments of set_watch per slot"""

    def __init__(self, bank, new_model, watches):
        self.hb, self.new_model, self.watches = bank, new_model, dict(watches)
        self.m = new_model()
        for slot, w in self.watches.items():
            self.set_watch(slot, *w)

    def set_watch(self, slot, *w):
        self.watches[slot] = w
        self.hb.set_watch(0, slot, *w), self.m.set_watch(slot, *w)

    def reset(self):
        """the bank's state and counters start afresh, its watches stay"""
        self.hb.reset()
        self.m = self.new_model()
        for slot, w in self.watches.items():
            self.m.set_watch(slot, *w)

    def call(self, ts, deliver=True):
        want = self.m.process(ts, deliver)
        for slot in range(4):
            got = self.hb.work(ts, slot=slot, deliver=deliver)
            assert (got is None) == (want[slot] is None) and (got is None or np.array_equal(got, want[slot])), slot
            assert self.hb.row_table(0, slot) == self.m.table(slot), slot
            assert self.hb.needed(0, slot) == (want[slot].size if deliver else 0, len(self.m.table(slot))), slot
            assert self.hb.stats(0, slot) == self.m.stats(slot), slot
            if hasattr(self.m, 'frame_bytes'):
                assert self.hb.frame_bytes(0, slot) == self.m.frame_bytes(slot), slot
        assert self.hb.stats(0) == self.m.stats()

    def check_tables(self):
        """what the getters hold is still what the bank's own last call left"""
        assert all(self.hb.stats(0, slot) == self.m.stats(slot) for slot in range(4))


def test_three_host_banks_side_by_side_with_a_reset_and_a_rewatch(pkg):
    """one multiplex of a T2-MI, an MPE and a ULE PID in calls of uneven sizes, each call through the three banks in an order that
    turns; in mid-stream the MPE bank is reset and a slot of the T2-MI bank is watched again (both with a unit open), later a slot of
    the ULE bank.  Every bank equals its model after every call, so neither event reaches another bank; a bank that has been reset or
    re-watched drops the unit it had open and, T2-MI, forgets the last packet_count."""
    rng = np.random.default_rng(5)
    ts = S.interleave(rng, [t2mi_feed(rng, TP, 400, [10, 40, 150, 700, 2500]), mpe_feed(rng, MP, 300, [28, 100, 700, 1400]),
                            ule_feed(rng, UP, 300, [28, 100, 700, 1400])])
    sides = [Side(pkg.T2miBank.host(1, 256, 512), T.T2mi, {0: (TP, -1), 2: (TP, 3), 3: (MP, -1)}),
             Side(pkg.MpeBank.host(1, 256, 512), RM.Mpe, {0: (MP, None, None), 1: (UP, None, None)}),
             Side(pkg.UleBank.host(1, 256, 512), RU.Ule, {0: (UP, None, None, True), 3: (TP, None, None, True)})]
    t2, mpe, ule = sides
    cuts = [0, 1, 64, 129, 130, 333, 500, 501, 700, 956, 1000]
    open_at_event = []
    for n, (a, b) in enumerate(zip(cuts, cuts[1:])):
        for k in range(3):
            sides[(n + k) % 3].call(ts[a:b], deliver=(n + k) % 5 != 4)
            for other in sides:
                other.check_tables()
        if n == 3:
            open_at_event += [len(mpe.m.slot[0].buf), len(t2.m.slot[0].buf), t2.m.slot[0].has_count]
            mpe.reset()
            t2.set_watch(0, TP, -1)
        if n == 6:
            open_at_event.append(len(ule.m.slot[0].buf))
            ule.set_watch(0, UP, None, None, True)
    assert all(open_at_event), open_at_event
    st = [s.m.stats(0) for s in sides]
    assert st[0]['t2mi_packets'] > 100 and st[0]['bbframes_delivered'] > 20 and st[1]['datagrams_delivered'] > 20 and st[2]['datagrams_delivered'] > 20
    assert t2.m.stats(2)['t2mi_packets'] > st[0]['t2mi_packets'] and 0 < t2.m.stats(2)['bbframes_delivered'] < t2.m.stats(2)['bbframes']
    assert t2.m.stats(3)['packets'] > 0 and t2.m.stats(3)['bbframes'] == 0 and mpe.m.stats(1)['datagrams'] == 0 and ule.m.stats(3)['datagrams'] == 0


def _text(pkg):
    return pkg.load_library().dvbs2gpu_last_error().decode()


def test_the_t2mi_banks_error_texts(pkg):
    """the texts of the T2-MI bank, letter for letter what they were before the bank became an instance of the datagram-bank core"""
    lib = pkg.load_library()
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        pkg.T2miBank.host(1, 4097, 16)
    assert e.value.code == -1 and str(e.value).endswith(': T2-MI bank: max_packets is at most 4096 per stream and call')
    bank = pkg.T2miBank.host(1, 8, 2)
    for pid, plp in ((0x1FFF, -1), (-2, 0), (0x100, 256), (0x100, -2)):
        with pytest.raises(pkg.Dvbs2GpuError) as e:
            bank.set_watch(0, 0, pid, plp)
        assert str(e.value).endswith(": T2-MI bank: a slot's PID is 0..0x1FFE (-1 empties the slot), its PLP 0..255 or -1 for every PLP"), (pid, plp)
    bank.set_watch(0, 0, TP, -1)
    for packets, kw in ((2, dict(cap=39)), (3, dict(deliver=False))):          # 40 bytes do not fit cap; three rows do not fit max_rows
        ts = T.Packetiser(TP).lay([T.bb_packet(k, 0, bytes(20)) for k in range(packets)])
        assert len(ts) == 1
        with pytest.raises(pkg.Dvbs2GpuError) as e:
            bank.work(ts, **kw)
        assert e.value.code == -5 and (e.value.needed, e.value.rows) == ((40, 2) if packets == 2 else (-1, 3))
        assert str(e.value).endswith(': T2-MI bank: the BBFRAMEs do not fit cap, or the rows max_rows (dvbs2gpu_t2mi_get_needed holds the sizes)')
    buf = np.ascontiguousarray(ts, np.uint8).reshape(-1)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.dvbs2gpu_t2mi_work(bank.h, 0, 0, p, buf.size, p, buf.size) == -1 and _text(pkg) == 'T2-MI bank: the output buffer is the input'
    assert lib.dvbs2gpu_t2mi_work(bank.h, 0, 0, p, 187, None, 0) == -1
    assert _text(pkg) == 'T2-MI bank: a byte count is a whole number of 188-byte packets'
    pin, cnt, nb = (C.c_void_p * 1)(buf.ctypes.data), (C.c_int * 1)(buf.size), (C.c_int * 4)()
    assert lib.dvbs2gpu_t2mi_process_batch(bank.h, pin, cnt, None, 0, nb, None, None) == -1
    assert _text(pkg) == 'T2-MI bank: a host bank takes host buffers (dvbs2gpu_t2mi_work)'
    assert bank.stats(0)['packets'] == 0                             # none of these calls advanced anything
