"""Audio bank without a GPU: the library's host bank (AudBank.host, csrc/aud_rules.h) against the model of tests/aud_ref.py in rows,
counters and state (through the next call): one constructed stream per codec whose rows are written out as numbers, every header
field value of the three codecs, every invalid one, and the random faulty multiplex, whole and cut.  Also the condition on the
multiplex that the other tests rely on."""
import ctypes as C

import numpy as np
import pytest

import aud_cases as K
import aud_ref as A
import pes_ref as P

NO = A.NO_TS
HEADER = P.HEADER
# frame bytes of AC-3 at 44.1 kHz by frmsizecod, written out: the second statement of floor(320 br / 147) + (frmsizecod & 1) words
AC3_441_WORDS = [69, 70, 87, 88, 104, 105, 121, 122, 139, 140, 174, 175, 208, 209, 243, 244, 278, 279, 348, 349, 417, 418, 487, 488, 557, 558, 696, 697, 835, 836,
                 975, 976, 1114, 1115, 1253, 1254, 1393, 1394]


class Pair:
    """a host bank and the model, fed the same calls"""

    def __init__(self, pkg, watches, max_packets=4096, max_rows=4096):
        self.hb, self.m = pkg.AudBank.host(1, max_packets, max_rows), A.Aud(max_rows)
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
    return [(r['unit'], r['code'], r['detail'], r['flags'], r['packet'], r['head'], r['es_offset'], r['frame_bytes'], r['sample_rate'], r['samples'], r['kbps']) for r in rows]


def one(pkg, codec, hdr):
    """the 8 bytes `hdr` (padded with 55) behind a PES start: the FRAME or LOSS row of the host bank, which is the model's"""
    pair = Pair(pkg, [(0, 0x160, codec)])
    rows = pair.call(K.Line(0x160).pes((hdr + b'\x55' * 8)[:8] + b'\x55' * 20).take())
    assert len(rows) >= 2 and rows[1]['flags'] == A.ACQUIRED and rows[1]['es_offset'] == 0 and rows[1]['head'] == int.from_bytes((hdr + b'\x55' * 4)[:4], 'big')
    if rows[1]['unit'] == A.LOSS or rows[1]['frame_bytes'] > 20:            # (a frame that ends inside the 28 bytes is followed by a LOSS in the filler)
        assert len(rows) == 2 and pair.m.stats()['sync_losses'] == (rows[1]['unit'] == A.LOSS) and pair.m.stats()['frames'] == (rows[1]['unit'] == A.FRAME)
    return rows[1]


def test_an_mpa_stream_with_every_row_written_out(pkg):
    rng = np.random.default_rng(1)
    f192 = K.mpa_frame(rng, bri=10, sri=1, mode=1)                  # MPEG-1 layer II, 192 kbit/s at 48 kHz, joint stereo: 576 bytes
    f128 = K.mpa_frame(rng, bri=8, sri=0, pad=1, mode=3)            # 128 kbit/s at 44.1 kHz, padded, mono: 418 bytes
    assert (len(f192), len(f128)) == (576, 418)
    ts = K.Line(0x160).pes(f192 + f192).pes(f128 + b'\xFF\xFD\xA4\x00' + b'\x00' * 30).take()      # the last header's 8th byte arrives, its frame does not
    pair = Pair(pkg, [(3, 0x160, A.MPA)])
    rows = pair.call(ts)
    assert (rows[0]['pts'], rows[0]['dts'], rows[0]['pid'], rows[0]['slot'], rows[0]['code']) == (93600, NO, 0x160, 3, 0xC0) and all(r['pts'] == NO for r in rows[1:3])
    assert brief(rows) == [
        (A.PES, 0xC0, HEADER, 0, 0, 0, 0, 0, 0, 0, 0),
        (A.FRAME, 14, 1, A.ACQUIRED, 0, 0xFFFDA440, 0, 576, 48000, 1152, 192),
        (A.FRAME, 14, 1, 0, 3, 0xFFFDA440, 576, 576, 48000, 1152, 192),    # (a header of 14 bytes: 170 ES bytes in the first packet, then 184 each)
        (A.PES, 0xC0, HEADER, 0, 7, 0, 1152, 0, 0, 0, 0),
        (A.FRAME, 14, 3, A.CHANGE, 7, 0xFFFD82C0, 1152, 418, 44100, 1152, 128),
        (A.FRAME, 14, 0, A.CHANGE, 9, 0xFFFDA400, 1570, 576, 48000, 1152, 192)]
    st = pair.m.stats(3)
    assert (st['frames'], st['frame_bytes_total'], st['samples_total'], st['acquisitions'], st['sync_losses'], st['param_changes'], st['unaligned_starts'],
            st['bytes_unlocked'], st['es_bytes'], st['pes_starts']) == (4, 2146, 4608, 1, 0, 2, 0, 0, 1604, 2)
    assert brief(Pair(pkg, [(3, 0x160, A.MPA)]).cut(ts, [1, 4, 8])) == brief(rows)


def test_an_adts_stream_with_every_row_written_out(pkg):
    rng = np.random.default_rng(2)
    a = K.adts_frame(rng, 200, sfi=3, chan=2)                       # AAC-LC, 48 kHz, stereo: 200 bytes in 1024 samples, 75 kbit/s
    b = K.adts_frame(rng, 9, sfi=4, chan=1, absent=0, blocks=1, profile=0, ident=1)
    bad = bytes([a[0], a[1] | 0x02]) + a[2:]                        # layer bits set
    ts = K.Line(0x161).pes(a + b + a).pes(bad + a).pes(a).take()
    pair = Pair(pkg, [(0, 0x161, A.ADTS)])
    rows = pair.call(ts)
    ha, hb = int.from_bytes(a[:4], 'big'), int.from_bytes(b[:4], 'big')
    assert brief(rows) == [
        (A.PES, 0xC0, HEADER, 0, 0, 0, 0, 0, 0, 0, 0),
        (A.FRAME, 1, 2, A.ACQUIRED, 0, ha, 0, 200, 48000, 1024, 75),
        (A.FRAME, 4, 1, A.CHANGE, 1, hb, 200, 9, 44100, 2048, 1),
        (A.FRAME, 1, 2, A.CHANGE, 1, ha, 209, 200, 48000, 1024, 75),
        (A.PES, 0xC0, HEADER, 0, 3, 0, 409, 0, 0, 0, 0),
        (A.LOSS, 0, 0, 0, 3, ha | 0x20000, 409, 0, 0, 0, 0),
        (A.PES, 0xC0, HEADER, 0, 6, 0, 809, 0, 0, 0, 0),
        (A.FRAME, 1, 2, A.ACQUIRED, 6, ha, 809, 200, 48000, 1024, 75)]
    st = pair.m.stats()
    assert (st['frames'], st['sync_losses'], st['acquisitions'], st['param_changes'], st['bytes_unlocked'], st['es_bytes']) == (4, 1, 2, 2, 392, 1009)
    assert brief(Pair(pkg, [(0, 0x161, A.ADTS)]).cut(ts, [1, 2, 3, 4])) == brief(rows)


def test_an_ac3_stream_with_every_row_written_out(pkg):
    rng = np.random.default_rng(3)
    a = K.ac3_frame(rng, fscod=0, frmsizecod=20, bsid=8, acmod=2)   # 192 kbit/s at 48 kHz: 768 bytes
    e = K.eac3_frame(rng, frmsiz=383, fscod=0, c2=3, acmod=7, lfeon=1)      # E-AC-3, 768 bytes in 1536 samples
    ts = K.Line(0x162).pes(a[:500]).pes(a[500:] + e).pes(e[:8]).take()     # the first frame straddles a PES start: unaligned
    pair = Pair(pkg, [(15, 0x162, A.AC3)])
    rows = pair.call(ts)
    assert brief(rows) == [
        (A.PES, 0xC0, HEADER, 0, 0, 0, 0, 0, 0, 0, 0),
        (A.FRAME, 8, 2, A.ACQUIRED, 0, 0x0B77ABCD, 0, 768, 48000, 1536, 192),
        (A.PES, 0xC0, HEADER, 0, 3, 0, 500, 0, 0, 0, 0),
        (A.FRAME, 16, 15, A.CHANGE, 4, 0x0B77017F, 768, 768, 48000, 1536, 192),
        (A.PES, 0xC0, HEADER, 0, 9, 0, 1536, 0, 0, 0, 0),
        (A.FRAME, 16, 15, 0, 9, 0x0B77017F, 1536, 768, 48000, 1536, 192)]
    st = pair.m.stats()
    assert (st['frames'], st['acquisitions'], st['unaligned_starts'], st['param_changes']) == (3, 1, 1, 1)
    assert brief(Pair(pkg, [(15, 0x162, A.AC3)]).cut(ts, [1, 4, 5, 9])) == brief(rows)


def test_every_mpa_version_layer_bitrate_and_rate(pkg):
    seen = set()
    for ver in range(4):
        for layer in range(4):
            for bri in range(16):
                for sri in range(4):
                    r = one(pkg, A.MPA, K.mpa_header(ver, layer, bri, sri, pad=(bri + sri) & 1))
                    bad = ver == 1 or layer == 0 or bri in (0, 15) or sri == 3
                    assert (r['unit'] == A.LOSS) == bad, (ver, layer, bri, sri)
                    if not bad:
                        key = ('V1L%d' % (4 - layer)) if ver == 3 else 'V2L1' if layer == 3 else 'V2L23'
                        fs = [44100, 48000, 32000][sri] // {3: 1, 2: 2, 0: 4}[ver]
                        assert (r['kbps'], r['sample_rate'], r['code']) == (A.MPA_KBPS[key][bri - 1], fs, ver << 2 | layer)
                        assert r['samples'] == (384 if layer == 3 else 1152 if layer == 2 or ver == 3 else 576)
                        seen.add((r['kbps'], fs, r['frame_bytes']))
    assert len(seen) > 300
    assert one(pkg, A.MPA, b'\xFF\xFB\x90\x00')['frame_bytes'] == 417 and one(pkg, A.MPA, b'\xFF\xFB\x92\x00')['frame_bytes'] == 418      # the familiar 128 kbit/s at 44.1 kHz
    assert one(pkg, A.MPA, b'\xFF\xDB\x90\x00')['unit'] == A.LOSS                   # 10 sync bits


def test_every_adts_sampling_index_and_length_bound(pkg):
    for sfi in range(16):
        r = one(pkg, A.ADTS, K.adts_header(100, sfi=sfi, blocks=sfi & 3))
        assert (r['unit'] == A.LOSS) == (sfi > 12)
        if sfi <= 12:
            assert (r['sample_rate'], r['samples'], r['frame_bytes']) == (A.ADTS_RATES[sfi], 1024 * ((sfi & 3) + 1), 100)
    for length, absent, ok in ((6, 1, False), (7, 1, True), (8, 0, False), (9, 0, True), (8191, 1, True), (0, 1, False)):
        assert (one(pkg, A.ADTS, K.adts_header(length, absent=absent))['unit'] == A.FRAME) == ok, (length, absent)
    for layer in (1, 2, 3):
        assert one(pkg, A.ADTS, K.adts_header(100, layer=layer))['unit'] == A.LOSS
    assert one(pkg, A.ADTS, b'\xFF\xE1' + K.adts_header(100)[2:])['unit'] == A.LOSS  # 11 sync bits
    assert one(pkg, A.ADTS, K.adts_header(100, chan=7))['detail'] == 7


def test_every_ac3_rate_and_frame_size_code_and_every_eac3_block_code(pkg):
    for fscod in range(4):
        for fsc in range(64):
            r = one(pkg, A.AC3, K.ac3_header(fscod, fsc))
            assert (r['unit'] == A.LOSS) == (fscod == 3 or fsc > 37), (fscod, fsc)
            if r['unit'] == A.FRAME:
                br = A.AC3_KBPS[fsc >> 1]
                words = {0: 2 * br, 1: AC3_441_WORDS[fsc], 2: 3 * br}[fscod]
                assert (r['frame_bytes'], r['kbps'], r['samples'], r['sample_rate']) == (2 * words, br, 1536, [48000, 44100, 32000][fscod])
    for bsid in range(32):
        assert (one(pkg, A.AC3, K.ac3_header(bsid=bsid) if bsid <= 10 else K.eac3_header(bsid=bsid))['unit'] == A.FRAME) == (bsid <= 16), bsid
    for fscod in range(4):
        for c2 in range(4):
            r = one(pkg, A.AC3, K.eac3_header(frmsiz=200, fscod=fscod, c2=c2))
            assert (r['unit'] == A.LOSS) == (fscod == 3 and c2 == 3)
            if r['unit'] == A.FRAME:
                fs, blocks = ([24000, 22050, 16000][c2], 6) if fscod == 3 else ([48000, 44100, 32000][fscod], [1, 2, 3, 6][c2])
                assert (r['frame_bytes'], r['sample_rate'], r['samples']) == (402, fs, 256 * blocks)
    assert [one(pkg, A.AC3, K.eac3_header(frmsiz=f))['unit'] for f in (0, 1, 2, 3, 2047)] == [A.LOSS, A.LOSS, A.LOSS, A.FRAME, A.FRAME]
    assert one(pkg, A.AC3, b'\x0B\x76' + K.ac3_header()[2:])['unit'] == A.LOSS and one(pkg, A.AC3, b'\x77\x0B' + K.ac3_header()[2:])['unit'] == A.LOSS


def test_the_random_multiplex_whole_and_cut(pkg):
    mux = K.mux()
    whole = Pair(pkg, K.WATCHES)
    want = whole.cut(mux, [])
    for edges in (range(1, len(mux)), range(37, len(mux), 37), [700], [1, 2, 3, 500, 501]):
        pair = Pair(pkg, K.WATCHES)
        assert pair.cut(mux, edges) == want and pair.m.stats() == whole.m.stats(), edges
    small = Pair(pkg, K.WATCHES, max_rows=50)                               # a table of 50 rows: the counters do not change
    assert small.cut(mux, [])[:50] == want[:50] and small.m.stats() == whole.m.stats() and small.hb.stream_stats()['rows_dropped'] == len(want) - 50
    whole.hb.reset(), whole.m.reset()                                       # reset: the watches stay
    assert whole.cut(mux, []) == want


def test_the_multiplex_yields_every_counter_and_row_kind():
    """a condition on the input of the multiplex tests, here and on the GPU, that the model alone shows: every counter above 0, more
    than 200 FRAME rows, at least 3 LOSS rows, 3 acquisitions and an unaligned start, and every flag"""
    m = K.model()
    m.process(K.mux())
    st = m.stats()
    assert not [k for k in A.STAT_KEYS if st[k] <= 0], st
    assert sum(r['unit'] == A.FRAME for r in m.table) > 200 and sum(r['unit'] == A.LOSS for r in m.table) >= 3
    assert st['acquisitions'] >= 3 and st['unaligned_starts'] >= 1
    for slot, _, _ in K.WATCHES:
        s = m.stats(slot)
        assert s['frames'] > 20 and s['acquisitions'] >= 3 and s['sync_losses'] >= 1 and s['resets'] >= 3, (slot, s)
    for flag in (A.ACQUIRED, A.RESYNC, A.UNSYNCED, A.SPLIT_HEADER, A.CHANGE):
        assert sum(bool(r['flags'] & flag) for r in m.table) >= 3, flag
    assert m.stats(5)['unaligned_starts'] > 10 and all(m.stats(s)['unaligned_starts'] == 0 for s in (0, 3, 11))


def test_argument_errors(pkg):
    lib, ARG = pkg.load_library(), -1
    h = C.c_void_p()
    assert lib.dvbs2gpu_aud_create(None, 1, 16, 16, C.byref(h)) == ARG
    assert lib.dvbs2gpu_aud_create_host(1, 4097, 16, C.byref(h)) == ARG and b'4096' in lib.dvbs2gpu_last_error()
    b = pkg.AudBank.host(2, 16, 16)
    b.set_watch(0, 0, 0x100, A.ADTS)
    b.set_watch(1, 0, 0x100, A.ADTS)                                        # the same PID on another stream
    for args in ((0, 1, 0x100, A.ADTS), (0, 1, 0x101, 0), (0, 1, 0x101, 4), (0, 1, 0x1FFF, 1), (0, 16, 5, 1), (2, 0, 5, 1)):
        with pytest.raises(pkg.Dvbs2GpuError):
            b.set_watch(*args)
    b.set_watch(0, 0, -1)                                                   # cleared: the PID is free again
    b.set_watch(0, 1, 0x100, A.MPA)
    with pytest.raises(pkg.Dvbs2GpuError):
        b.work(np.zeros(187, np.uint8))
    with pytest.raises(pkg.Dvbs2GpuError):
        b.work(np.zeros(17 * 188, np.uint8))
    with pytest.raises(pkg.Dvbs2GpuError):
        b.stats(0, 16)
    assert lib.dvbs2gpu_aud_process_batch(b.h, None, None, None, None) == ARG
