"""ES bank without a GPU: the library's host bank (EsBank.host, csrc/es_rules.h) against the model of tests/es_ref.py in rows, counters
and state (through the next call), on constructed streams of the three codecs whose rows are written out as numbers, and on the
random faulty multiplex, whole and cut.  Also the condition on the multiplex that the GPU tests use."""
import ctypes as C

import numpy as np
import pytest

import es_cases as K
import es_ref as E
import pes_ref as P

NO = E.NO_TS
HEADER = P.HEADER


class Pair:
    """a host bank and the model, fed the same calls"""

    def __init__(self, pkg, watches, max_packets=4096, max_rows=4096):
        self.hb, self.m = pkg.EsBank.host(1, max_packets, max_rows), E.Es(max_rows)
        for slot, pid, codec in watches:
            self.hb.set_watch(0, slot, pid, codec), self.m.set_watch(slot, pid, codec)

    def call(self, ts):
        assert self.hb.work(ts) == self.m.process(ts)
        K.same(self.hb, self.m)
        return self.m.table

    def cut(self, ts, edges):
        rows, a = [], 0
        for b in list(edges) + [len(ts)]:
            rows += [dict(r, packet=r['packet'] + a) for r in self.call(ts[a:b])]
            a = b
        return rows


def brief(rows):
    return [(r['unit'], r['code'], r['detail'], r['flags'], r['packet'], r['head'], r['es_offset']) for r in rows]


def test_an_mpeg2_sequence_with_every_row_written_out(pkg):
    es = (K.SC + b'\xB3' + b'\x11' * 8 + K.SC + b'\xB8' + b'\x22' * 4 + K.SC + b'\x00' + b'\x01\x4F\x33\x33' + K.SC + b'\x01' + b'\x44' * 190 +
          K.SC + b'\x02' + b'\x44' * 20 + K.SC + b'\x00' + b'\x01\x97\x33\x33' + K.SC + b'\x00' + b'\x01\xDF\x33\x33' + K.SC + b'\x00' + b'\x01\xE7\x33\x33' +
          K.SC + b'\xB2' + b'\x66' * 4 + K.SC + b'\xB7' + b'\x55' * 4)
    ts = K.Line(0x150).pes(es).take()                       # a header of 14 bytes: 170 ES bytes in the first packet, 116 in the second
    pair = Pair(pkg, [(3, 0x150, E.MPEG2)])
    rows = pair.call(ts)
    assert (rows[0]['pts'], rows[0]['dts'], rows[0]['pid'], rows[0]['slot']) == (93600, NO, 0x150, 3) and all(r['pts'] == NO for r in rows[1:])
    assert brief(rows) == [
        (E.PES, 0xE0, HEADER, 0, 0, 0, 0),
        (E.SEQUENCE, 0xB3, 0, 0, 0, 0x11111111, 0),
        (E.GOP, 0xB8, 0, 0, 0, 0x22222222, 12),
        (E.PICTURE, 0x00, E.PIC_I, E.KEY, 0, 0x014F3333, 20),
        (E.PICTURE, 0x00, E.PIC_P, 0, 1, 0x01973333, 246),
        (E.PICTURE, 0x00, E.PIC_B, 0, 1, 0x01DF3333, 254),
        (E.PICTURE, 0x00, 0, 0, 1, 0x01E73333, 262),        # picture_coding_type 4
        (E.END, 0xB7, 0, 0, 1, 0x55555555, 278)]
    st = pair.m.stats(3)
    assert (st['codes'], st['slices'], st['other_codes'], st['pictures'], st['pictures_i'], st['pictures_p'], st['pictures_b'], st['key_pictures']) == (10, 2, 1, 4, 1, 1, 1, 1)
    assert (st['es_bytes'], st['payload_bytes'], st['pes_starts'], st['packets'], st['resets'], st['bytes_unsynced']) == (286, 300, 1, 2, 0, 0)
    assert brief(Pair(pkg, [(3, 0x150, E.MPEG2)]).cut(ts, [1])) == brief(rows)


def test_an_h264_access_unit_sequence_with_every_row_written_out(pkg):
    sl = lambda nal, first, n=30: K.SC + bytes([nal, first]) + b'\x77' * n
    es = (b'\x00' + K.SC + b'\x09\xF0' + b'\x00' + K.SC + b'\x67' + b'\x64' * 6 + K.SC + b'\x68' + b'\xEE' * 4 + K.SC + b'\x06' + b'\x05' * 5 +
          sl(0x65, K.H264_I) + sl(0x65, K.H264_LATER) + K.SC + b'\x09\xF0' + sl(0x41, K.H264_P) + K.SC + b'\x09\xF0' + sl(0x01, K.H264_B) +
          sl(0x41, K.H264_SP) + sl(0x41, 0x80 | 0x40) + sl(0x41, 0x80 | 0x04) + K.SC + b'\xE5' + b'\x99' * 4 + K.SC + b'\x0B' + b'\x99' * 4)
    ts = K.Line(0x151).pes(es, dts=91800).take()
    pair = Pair(pkg, [(0, 0x151, E.H264)])
    rows = pair.call(ts)
    assert (rows[0]['pts'], rows[0]['dts']) == (93600, 91800)
    AUD = lambda off, pk=0: (E.AUD, 0x09, 0, 0, pk, 0xF0000000 | int.from_bytes(es[off + 5:off + 8], 'big'), off)
    assert brief(rows) == [
        (E.PES, 0xE0, HEADER, 0, 0, 0, 0),
        AUD(1),
        (E.SEQUENCE, 0x67, 0, 0, 0, 0x64646464, 7),
        (E.PARAM, 0x68, 0, 0, 0, 0xEEEEEEEE, 17),
        (E.PICTURE, 0x65, E.PIC_I, E.KEY, 0, 0x88777777, 34),
        AUD(104),
        (E.PICTURE, 0x41, E.PIC_P, 0, 0, 0x98777777, 109),
        AUD(144),
        (E.PICTURE, 0x01, E.PIC_B, 0, 0, 0x9C777777, 149),  # (a header of 19 bytes: the first packet holds ES bytes 0..164)
        (E.PICTURE, 0x41, 0, 0, 1, 0x90777777, 184),        # slice_type 3, SP
        (E.PICTURE, 0x41, E.PIC_P, 0, 1, 0xC0777777, 219),  # slice_type 0
        (E.PICTURE, 0x41, 0, 0, 1, 0x84777777, 254),        # four leading zeros
        (E.END, 0x0B, 0, 0, 1, 0x99999999, 297)]
    st = pair.m.stats()
    assert (st['codes'], st['slices'], st['other_codes'], st['bad_codes'], st['auds'], st['params'], st['sequences'], st['ends']) == (15, 1, 1, 1, 3, 1, 1, 1)
    assert brief(Pair(pkg, [(0, 0x151, E.H264)]).cut(ts, [1])) == brief(rows)


def test_an_h265_access_unit_sequence_with_every_row_written_out(pkg):
    nal = lambda t, rest, tid=1: K.SC + bytes([t << 1, tid]) + rest
    es = (nal(35, b'\x50\x11\x11') + nal(32, b'\x0C' * 4) + nal(33, b'\x0D' * 4) + nal(34, b'\x0E' * 4) + nal(39, b'\x0F' * 4) + nal(19, b'\xA0' + b'\x12' * 9) +
          nal(19, b'\x20' + b'\x12' * 9) + nal(1, b'\x90' + b'\x12' * 9) + nal(9, b'\x90' * 3) + nal(10, b'\x90' * 3) + nal(21, b'\x80' * 3) + nal(22, b'\x80' * 3) +
          nal(1, b'\x90' * 3, tid=0) + nal(37, b'\x13' * 3))
    ts = K.Line(0x152).pes(es).take()
    pair = Pair(pkg, [(15, 0x152, E.H265)])
    rows = pair.call(ts)
    assert brief(rows) == [
        (E.PES, 0xE0, HEADER, 0, 0, 0, 0),
        (E.AUD, 0x46, 0, 0, 0, 0x01501111, 0),
        (E.PARAM, 0x40, 0, 0, 0, 0x010C0C0C, 8),
        (E.SEQUENCE, 0x42, 0, 0, 0, 0x010D0D0D, 17),
        (E.PARAM, 0x44, 0, 0, 0, 0x010E0E0E, 26),
        (E.PICTURE, 0x26, E.PIC_I, E.KEY, 0, 0x01A01212, 44),
        (E.PICTURE, 0x02, 0, 0, 0, 0x01901212, 74),
        (E.PICTURE, 0x12, 0, 0, 0, 0x01909090, 89),         # type 9, the last of the trailing and leading pictures
        (E.PICTURE, 0x2A, E.PIC_I, E.KEY, 0, 0x01808080, 105),
        (E.END, 0x4A, 0, 0, 0, 0x01131313, 129)]
    st = pair.m.stats()
    assert (st['codes'], st['slices'], st['other_codes'], st['bad_codes'], st['params'], st['key_pictures'], st['pictures_i'], st['pictures_p']) == (14, 1, 3, 1, 2, 2, 2, 0)


def test_starts_valid_empty_split_and_bad(pkg):
    """a header that ends with its packet (an empty segment), one that runs beyond it (SPLIT_HEADER: unsynced until the next start),
    and a bad start code: what is synced, what is scanned and what the next rows carry"""
    ln = K.Line(0x150)
    code = K.SC + b'\xB8' + b'\x22' * 4
    ln.put(K.head(93600), pusi=1).put(code)                                         # an empty segment, then a code of its own packet
    ln.put(K.head(97200, stuffing=6)[:16], pusi=1).put(b'\xFF' * 4 + code)          # 9 + 11 > 16: split; the code is not scanned
    ln.put(K.head(100800, start=b'\x00\x01\x01') + code, pusi=1).put(code)          # BAD_START
    ln.put(K.head(104400) + code[:5], pusi=1).put(code[5:] + code)                  # valid again; a code across the two packets
    pair = Pair(pkg, [(0, 0x150, E.MPEG2)])
    rows = pair.call(ln.take())
    U, SP, RS = E.UNSYNCED, E.SPLIT_HEADER, E.RESYNC
    assert brief(rows) == [
        (E.PES, 0xE0, HEADER, 0, 0, 0, 0), (E.GOP, 0xB8, 0, 0, 1, 0x22222222, 0),
        (E.PES, 0xE0, HEADER, U | SP, 2, 0, 8),
        (E.PES, 0xE0, P.BAD_START, U | RS, 4, 0, 8),
        (E.PES, 0xE0, HEADER, RS, 6, 0, 8), (E.GOP, 0xB8, 0, 0, 7, 0x22222222, 8), (E.GOP, 0xB8, 0, 0, 7, 0x22222222, 16)]
    st = pair.m.stats()
    assert (st['pes_starts'], st['pes_invalid'], st['split_headers'], st['resets'], st['bytes_unsynced'], st['es_bytes']) == (4, 2, 1, 2, 20, 24)


def test_faults_between_the_bytes_of_a_window(pkg):
    """a duplicate does nothing; a lost packet, a DI and a scrambled packet lose the code and mark the next row"""
    code = K.SC + b'\xB8' + b'\x22' * 4
    rows = {}
    for name in ('plain', 'duplicate', 'lost', 'di', 'scrambled'):
        ln = K.Line(0x150).pes(b'\x33' * 10 + code[:4], sizes=[28])
        if name == 'duplicate':
            ln.again()
        if name == 'lost':
            ln.lose()
        if name == 'di':
            ln.no_payload(di=1)
        if name == 'scrambled':
            ln.put(b'\x5A' * 184, tsc=1)
        ln.put(code[4:] + b'\x33' * 3 + code)
        rows[name] = brief(Pair(pkg, [(0, 0x150, E.MPEG2)]).call(ln.take()))
    first = (E.PES, 0xE0, HEADER, 0, 0, 0, 0)
    assert rows['plain'] == [first, (E.GOP, 0xB8, 0, 0, 1, 0x22222222, 10), (E.GOP, 0xB8, 0, 0, 1, 0x22222222, 21)]
    assert rows['duplicate'] == [first, (E.GOP, 0xB8, 0, 0, 2, 0x22222222, 10), (E.GOP, 0xB8, 0, 0, 2, 0x22222222, 21)]
    assert rows['lost'] == [first, (E.GOP, 0xB8, 0, E.RESYNC, 1, 0x22222222, 21)]
    assert rows['di'] == rows['scrambled'] == [first, (E.GOP, 0xB8, 0, E.RESYNC, 2, 0x22222222, 21)]


def test_the_random_multiplex_whole_and_cut(pkg):
    rng = np.random.default_rng(3)
    watches = [(2, 0x150, E.MPEG2), (0, 0x151, E.H264), (7, 0x152, E.H265)]
    mux = K.random_mux(rng, 1500, [(p, c) for _, p, c in watches])
    whole = Pair(pkg, watches)
    want = whole.cut(mux, [])
    assert len(want) > 300
    for edges in ([700], [1, 2, 3, 500, 501], list(range(97, 1500, 97))):
        pair = Pair(pkg, watches)
        assert pair.cut(mux, edges) == want and pair.m.stats() == whole.m.stats(), edges
    small = Pair(pkg, watches, max_rows=50)                                 # a table of 50 rows: the counters do not change
    assert small.cut(mux, [])[:50] == want[:50] and small.m.stats() == whole.m.stats() and small.hb.stream_stats()['rows_dropped'] == len(want) - 50
    whole.hb.reset(), whole.m.reset()                                       # reset: the watches stay
    assert whole.cut(mux, []) == want


CODEC_KEYS = {
    E.MPEG2: ('pictures_i', 'pictures_p', 'pictures_b', 'key_pictures', 'sequences', 'gops', 'ends', 'slices', 'other_codes'),
    E.H264: ('pictures_i', 'pictures_p', 'pictures_b', 'key_pictures', 'sequences', 'params', 'auds', 'ends', 'slices', 'other_codes', 'bad_codes'),
    E.H265: ('pictures_i', 'key_pictures', 'sequences', 'params', 'auds', 'ends', 'slices', 'other_codes', 'bad_codes')}
COMMON_KEYS = ('packets', 'payload_bytes', 'es_bytes', 'bytes_unsynced', 'duplicates', 'cc_errors', 'scrambled_packets', 'malformed_packets', 'resets', 'pes_starts',
               'pes_invalid', 'split_headers', 'codes', 'pictures')
CODEC_UNITS = {E.MPEG2: (E.PES, E.PICTURE, E.SEQUENCE, E.GOP, E.END), E.H264: (E.PES, E.PICTURE, E.SEQUENCE, E.PARAM, E.AUD, E.END),
               E.H265: (E.PES, E.PICTURE, E.SEQUENCE, E.PARAM, E.AUD, E.END)}


def test_the_multiplex_of_the_gpu_tests_yields_ten_of_everything_per_codec():
    """a condition on the input of tests/test_gpu_es.py: at least 10 of every counter and of every unit that the codec has (MPEG-2 has
    neither parameter sets, AUDs nor bad codes; H.264 no GOP headers; the H.265 head gives no P or B), and of RESYNC rows"""
    m = E.Es()
    for slot, (codec, pid) in enumerate(K.PIDS.items()):
        m.set_watch(slot, pid, codec)
    m.process(K.gpu_mux())
    for slot, codec in enumerate(K.PIDS):
        st = m.stats(slot)
        low = [k for k in COMMON_KEYS + CODEC_KEYS[codec] if st[k] < 10]
        assert not low, (codec, low, st)
        rows = [r for r in m.table if r['slot'] == slot]
        for unit in CODEC_UNITS[codec]:
            assert sum(r['unit'] == unit for r in rows) >= 10, (codec, unit)
        for flag in (E.RESYNC, E.UNSYNCED, E.SPLIT_HEADER, E.KEY):
            assert sum(bool(r['flags'] & flag) for r in rows) >= 10, (codec, flag)


def test_argument_errors(pkg):
    lib, ARG = pkg.load_library(), -1
    h = C.c_void_p()
    assert lib.dvbs2gpu_es_create(None, 1, 16, 16, C.byref(h)) == ARG
    assert lib.dvbs2gpu_es_create_host(1, 4097, 16, C.byref(h)) == ARG and b'4096' in lib.dvbs2gpu_last_error()
    b = pkg.EsBank.host(2, 16, 16)
    b.set_watch(0, 0, 0x100, E.H264)
    b.set_watch(1, 0, 0x100, E.H264)                                        # the same PID on another stream
    for args in ((0, 1, 0x100, E.H264), (0, 1, 0x101, 0), (0, 1, 0x101, 4), (0, 1, 0x1FFF, 1), (0, 16, 5, 1), (2, 0, 5, 1)):
        with pytest.raises(pkg.Dvbs2GpuError):
            b.set_watch(*args)
    b.set_watch(0, 0, -1)                                                   # cleared: the PID is free again
    b.set_watch(0, 1, 0x100, E.MPEG2)
    with pytest.raises(pkg.Dvbs2GpuError):
        b.work(np.zeros(187, np.uint8))
    with pytest.raises(pkg.Dvbs2GpuError):
        b.work(np.zeros(17 * 188, np.uint8))
    with pytest.raises(pkg.Dvbs2GpuError):
        b.stats(0, 16)
    assert lib.dvbs2gpu_es_process_batch(b.h, None, None, None, None) == ARG
