"""TS monitor without a GPU: the model of tests/tsmon_ref.py on clean and damaged multiplexes (it is the yardstick of the GPU tests),
the library's host bank against the model for every cut of a stream into calls, and the argument checks of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import tsmon_ref as T

PIDS = [0, 0x11, 0x100, 0x101, 0x1FFE]
FILTERS = [dict(), dict(mode=1, pids=[0x100]), dict(mode=1, pids=[0, 0x1FFE, 0x1FFF]), dict(mode=2, pids=[0x100, 0x11]),
           dict(drop_null=True), dict(drop_tei=True), dict(drop_bad_sync=True), dict(mode=2, pids=[0x101], drop_null=True, drop_tei=True, drop_bad_sync=True)]


def _stats_of(ts):
    m = T.Monitor()
    m.process(ts)
    return m.stats()


@pytest.mark.parametrize('seed', range(4))
def test_clean_mux_costs_nothing(seed):
    rng = np.random.default_rng(seed)
    ts, info = T.make_mux(rng, 600, PIDS)
    st = _stats_of(ts)
    assert (st['cc_errors'], st['tei_packets'], st['sync_byte_errors'], st['discontinuities']) == (0, 0, 0, 0)
    assert st['duplicates'] == info['duplicates'] > 0
    assert st['packets'] == st['passed_packets'] == 600 and st['null_packets'] == int((info['kind'] == T.N).sum()) > 0
    assert st['pids_seen'] == len(set(info['pid']) - {T.NULL_PID})
    assert int((info['kind'] == T.A).sum()) > 0


@pytest.mark.parametrize('inject', T.INJECTORS, ids=lambda f: f.__name__)
@pytest.mark.parametrize('seed', range(3))
def test_each_fault_costs_what_its_injector_says(inject, seed):
    rng = np.random.default_rng(100 + seed)
    ts, info = T.make_mux(rng, 400, PIDS)
    clean = _stats_of(ts)
    bad, _, cost = inject(rng, ts, info)
    got = _stats_of(bad)
    for k in T.STAT_KEYS:
        if k != 'passed_packets':
            assert got[k] - clean[k] == cost.get(k, 0), (k, cost)


def _damaged(seed, n=300):
    rng = np.random.default_rng(seed)
    ts, info = T.make_mux(rng, n, PIDS)
    for inject in T.INJECTORS:
        ts, info, _ = inject(rng, ts, info)
    return ts


@pytest.mark.parametrize('split', [1, 2, 7, 0])
@pytest.mark.parametrize('flt', range(len(FILTERS)))
def test_host_bank_equals_model_for_every_split(pkg, flt, split):
    ts = _damaged(flt)
    n = len(ts)
    hb, m = pkg.TsMonitorBank.host(2, 512), T.Monitor()
    hb.set_filter(1, **FILTERS[flt])
    m.set_filter(**FILTERS[flt])
    step = split or n
    cuts = list(range(0, n, step)) + [n]
    for i, a in enumerate(cuts[:-1]):
        if i == 2:                                                 # a call without packets changes nothing but the table
            assert hb.work(ts[:0], stream=1).size == 0 and hb.pid_table(1) == [] and hb.stats(1) == m.stats()
        want, got = m.process(ts[a:cuts[i + 1]]), hb.work(ts[a:cuts[i + 1]], stream=1)
        assert np.array_equal(got, want), a
        assert hb.pid_table(1) == m.table, a
        assert hb.stats(1) == m.stats(), a
    assert hb.stats(0) == T.Monitor().stats()                      # the bank's other stream saw nothing
    if flt == 0:
        assert m.stats()['cc_errors'] > 0 and m.stats()['duplicates'] > 0
    hb.reset()
    assert hb.stats(1) == T.Monitor().stats() and hb.pid_table(1) == []
    m2 = T.Monitor()
    m2.set_filter(**FILTERS[flt])                                  # reset keeps the filter
    assert np.array_equal(hb.work(ts, stream=1), m2.process(ts)) and hb.stats(1) == m2.stats()


def test_statistics_only_call_and_capacity(pkg):
    ts = _damaged(3)
    hb, m = pkg.TsMonitorBank.host(1, 512), T.Monitor()
    assert hb.work(ts[:100], filtered=False) is None
    m.process(ts[:100])
    assert hb.stats() == m.stats() and hb.pid_table() == m.table
    before = hb.stats()
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        hb.work(ts[100:], cap=(len(ts) - 100) * 188 - 188)
    assert e.value.code == -5
    assert hb.stats() == before and hb.pid_table() == []
    want = m.process(ts[100:])
    assert np.array_equal(hb.work(ts[100:], cap=(len(ts) - 100) * 188), want) and hb.stats() == m.stats() and hb.pid_table() == m.table


def test_argument_checks(pkg):
    lib = pkg.load_library()
    ARG = -1
    h = C.c_void_p()
    assert lib.dvbs2gpu_tsmon_create(None, 1, 16, C.byref(h)) == ARG
    assert lib.dvbs2gpu_tsmon_create_host(0, 16, C.byref(h)) == ARG
    assert lib.dvbs2gpu_tsmon_create_host(1, -1, C.byref(h)) == ARG
    assert lib.dvbs2gpu_tsmon_create_host(1, 8193, C.byref(h)) == ARG
    assert lib.dvbs2gpu_tsmon_create_host(1, 16, None) == ARG
    assert lib.dvbs2gpu_tsmon_reset(None) == ARG
    lib.dvbs2gpu_tsmon_destroy(None)
    assert lib.dvbs2gpu_tsmon_create_host(2, 16, C.byref(h)) == 0
    f = pkg.TsMonFilter(1, 0, 0, 0)
    ok, bad = (C.c_uint16 * 2)(0, 0x1FFF), (C.c_uint16 * 2)(5, 0x2000)
    assert lib.dvbs2gpu_tsmon_set_filter(None, 0, C.byref(f), ok, 2) == ARG
    assert lib.dvbs2gpu_tsmon_set_filter(h, 2, C.byref(f), ok, 2) == ARG
    assert lib.dvbs2gpu_tsmon_set_filter(h, 0, None, ok, 2) == ARG
    assert lib.dvbs2gpu_tsmon_set_filter(h, 0, C.byref(f), ok, -1) == ARG
    assert lib.dvbs2gpu_tsmon_set_filter(h, 0, C.byref(f), bad, 2) == ARG
    assert lib.dvbs2gpu_tsmon_set_filter(h, 0, C.byref(pkg.TsMonFilter(3, 0, 0, 0)), ok, 2) == ARG
    assert lib.dvbs2gpu_tsmon_set_filter(h, 0, C.byref(f), ok, 2) == 0
    buf, out = np.zeros(17 * 188, np.uint8), np.zeros(17 * 188, np.uint8)
    pb, po = C.c_void_p(buf.ctypes.data), C.c_void_p(out.ctypes.data)
    assert lib.dvbs2gpu_tsmon_work(None, 0, pb, 188, po, 188) == ARG
    assert lib.dvbs2gpu_tsmon_work(h, -1, pb, 188, po, 188) == ARG
    assert lib.dvbs2gpu_tsmon_work(h, 0, pb, 187, po, 188) == ARG          # not a whole number of packets
    assert lib.dvbs2gpu_tsmon_work(h, 0, pb, -188, po, 188) == ARG
    assert lib.dvbs2gpu_tsmon_work(h, 0, pb, 188, po, -1) == ARG
    assert lib.dvbs2gpu_tsmon_work(h, 0, pb, 17 * 188, po, 17 * 188) == ARG    # more than max_packets
    assert lib.dvbs2gpu_tsmon_work(h, 0, pb, 188, pb, 188) == ARG          # the output is the input
    assert lib.dvbs2gpu_tsmon_work(h, 0, None, 188, po, 188) == ARG
    one = C.c_int(188)
    pp = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    assert lib.dvbs2gpu_tsmon_process_batch(None, pp, C.byref(one), None, 0, None, None) == ARG
    assert lib.dvbs2gpu_tsmon_process_batch(h, pp, (C.c_int * 2)(0, 0), None, 0, None, None) == ARG   # a host bank has no device buffers
    st, n = pkg.TsMonStats(), C.c_int()
    assert lib.dvbs2gpu_tsmon_get_stats(h, 0, None) == ARG and lib.dvbs2gpu_tsmon_get_stats(h, 2, C.byref(st)) == ARG
    assert lib.dvbs2gpu_tsmon_get_pid_table(h, 0, None, 1, C.byref(n)) == ARG
    assert lib.dvbs2gpu_tsmon_get_pid_table(h, 0, None, -1, C.byref(n)) == ARG
    assert lib.dvbs2gpu_tsmon_get_pid_table(h, 0, None, 0, None) == ARG
    p = C.c_void_p()
    assert lib.dvbs2gpu_tsmon_get_pid_table_device(h, 0, C.byref(p), C.byref(n)) == ARG      # device banks only
    assert lib.dvbs2gpu_tsmon_get_stats(h, 0, C.byref(st)) == 0 and st.packets == 0          # nothing above was taken
    lib.dvbs2gpu_tsmon_destroy(h)


def test_device_bank_without_a_device_fails_loudly(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present: the no-device path cannot be shown')
    with pytest.raises(pkg.Dvbs2GpuError) as e:
        pkg.TsMonitorBank(pkg.Engine(0), 1, 64)
    assert 'no CPU fallback' in str(e.value) or 'no HIP device' in str(e.value)
