"""The four watched-PID banks share their host half (csrc/watch_bank.h).  Without a GPU: the PCR, PES, ES and audio host banks live in
one process and are called in interleaved order on one multiplex, each against its model (tests/pcr_ref.py, pes_ref.py, es_ref.py,
aud_ref.py); what one bank is told must not reach the other three.  And the ES and the audio host bank, whose streams share one
packet walk (csrc/es_rules.h), agree on everything that walk decides when they watch the same PIDs."""
import numpy as np
import pytest

import pcr_cases as KC
import pes_cases as KP
import watch_cases as W

NAMES = ('pcr', 'pes', 'es', 'aud')


@pytest.fixture(scope='module')
def mux():
    """the edge cases of the first two banks one after the other (their own PIDs are not watched here: packets that are not looked at)
    and 400 packets in which every bank has two active slots"""
    ts = np.concatenate([KC.whole_stream(), KP.whole_stream(), W.interleaved(np.random.default_rng(5), 400)])
    ts.setflags(write=False)
    return ts


def _banks(pkg, max_rows):
    banks = {'pcr': pkg.PcrBank.host(1, 4096, max_rows), 'pes': pkg.PesBank.host(1, 4096, max_rows), 'es': pkg.EsBank.host(1, 4096, max_rows),
             'aud': pkg.AudBank.host(1, 4096, max_rows)}
    for name in NAMES:
        W.watch(name, banks[name], 0)
    return banks, {name: W.model(name, max_rows) for name in NAMES}


def test_four_host_banks_side_by_side(pkg, mux):
    banks, models = _banks(pkg, 16)
    assert len(mux) <= 4096
    half = len(mux) // 2
    # whole, the banks in turn; then after reset() cut in two, the second halves in another order than the first
    for pieces in ([(NAMES, mux)], [(('es', 'aud', 'pcr', 'pes'), mux[:half]), (('pes', 'es', 'pcr', 'aud'), mux[half:])]):
        for order, ts in pieces:
            for name in order:
                assert banks[name].work(ts) == models[name].process(ts), name
            for name in NAMES:                               # after all four have run: no bank's call wrote to another's
                W.SAME[name](banks[name], models[name])
        for name in NAMES:
            st = banks[name].stats()
            assert all(banks[name].stats(0, s)['packets' if name != 'pcr' else 'pcr_packets'] > 0 for s in W.SLOTS[name]), name
            assert banks[name].stream_stats()['rows_dropped'] > 0, name
            banks[name].reset(), models[name].reset()
            assert banks[name].stats() == {k: 0 for k in st} and banks[name].stream_stats()['packets'] == 0, name
            W.SAME[name](banks[name], models[name])
            for other in NAMES:
                if other != name:
                    W.SAME[other](banks[other], models[other])


def test_rewatching_a_slot_of_one_bank_leaves_the_other_banks_alone(pkg, mux):
    banks, models = _banks(pkg, 4096)
    for name in NAMES:
        banks[name].work(mux), models[name].process(mux)
    for name in NAMES:
        before = {other: W.snapshot(banks[other]) for other in NAMES}
        slot = W.SLOTS[name][0]
        pid = banks[name]._watched[0][slot]
        again = pid if isinstance(pid, tuple) else (pid,)
        banks[name].set_watch(0, slot, *again), models[name].set_watch(slot, *again)
        assert set(banks[name].stats(0, slot).values()) == {0} and before[name][0][slot + 1] != banks[name].stats(0, slot)
        assert banks[name].stats(0, W.SLOTS[name][1]) == before[name][0][W.SLOTS[name][1] + 1]
        for other in NAMES:
            if other != name:
                assert W.snapshot(banks[other]) == before[other], (name, other)
            W.SAME[other](banks[other], models[other])
    # and the next call goes on from there in all four
    for name in NAMES:
        assert banks[name].work(mux[:200]) == models[name].process(mux[:200])
        W.SAME[name](banks[name], models[name])


@pytest.mark.parametrize('per_call', [None, 37, 64])
@pytest.mark.parametrize('feed', ['aud', 'es'])
def test_es_and_audio_host_banks_agree_on_what_the_shared_walk_decides(pkg, feed, per_call):
    ts, pids = W.stream_feeds()[feed]
    es, aud = pkg.EsBank.host(1, 4096, 1 << 16), pkg.AudBank.host(1, 4096, 1 << 16)
    W.watch_same_pids(es, aud, pids, 0)
    step, pes_rows = per_call or len(ts), 0
    for a in range(0, len(ts), step):
        es.work(ts[a:a + step]), aud.work(ts[a:a + step])
        pes_rows += W.same_stream_front(es, aud)
    assert es.stream_stats()['rows_dropped'] == 0 and aud.stream_stats()['rows_dropped'] == 0
    # no empty comparison: every common counter counts something, and the PES rows are those of the models
    assert all(es.stats()[k] > 0 for k in W.COMMON_COUNTERS), es.stats()
    assert pes_rows == es.stats()['pes_starts'] == {'aud': 300, 'es': 368}[feed]
