"""Builders for the tests of the audio bank (include/dvbs2gpu.h, audio bank): frames of the three codecs with chosen parameters whose
payload is filler full of false sync words (runs of FF, and the words 0B 77 and FF Fx), their PES packets -- aligned, a whole number of
frames each, or unaligned, cut anywhere -- laid into TS packets of any payload length (the packet builders are those of
tests/es_cases.py), and a random faulty multiplex."""
import numpy as np

import aud_ref as A
import es_cases as E
import pes_ref as P

PIDS = {A.MPA: 0x160, A.ADTS: 0x161, A.AC3: 0x162}
pkt, head = E.pkt, E.head


def filler(rng, n):
    """n bytes in which a free-running sync search would find a header every few bytes"""
    out = bytearray()
    while len(out) < n:
        r = int(rng.integers(0, 5))
        out += (b'\xFF' * int(rng.integers(1, 9)), b'\x0B\x77', bytes([0xFF, 0xF0 | int(rng.integers(0, 16))]), b'\xFF\xFB\x90\x00',
                bytes(rng.integers(0, 256, int(rng.integers(1, 6)), dtype=np.uint8)))[r]
    return bytes(out[:n])


def _fill(hdr, codec, rng, body=None):
    got = A.parse(codec, (hdr + b'\x00' * 8)[:8])
    assert got is not None, hdr.hex()
    n = got['frame_bytes'] - len(hdr)
    return hdr + (filler(rng, n) if body is None else (body * n)[:n])


def mpa_header(ver=3, layer=2, bri=9, sri=1, pad=0, mode=0, prot=1):
    """ver / layer: the header's bits (3 MPEG-1, 2 MPEG-2, 0 MPEG-2.5; 3 I, 2 II, 1 III)"""
    return (0x7FF << 21 | ver << 19 | layer << 17 | prot << 16 | bri << 12 | sri << 10 | pad << 9 | mode << 6).to_bytes(4, 'big')


def adts_header(length, sfi=3, chan=2, profile=1, blocks=0, absent=1, ident=0, layer=0):
    v = 0xFFF << 44 | ident << 43 | layer << 41 | absent << 40 | profile << 38 | sfi << 34 | chan << 30 | length << 13 | 0x7FF << 2 | blocks
    return v.to_bytes(7, 'big')


def ac3_header(fscod=0, frmsizecod=20, bsid=8, acmod=2, bsmod=0):
    return b'\x0B\x77\xAB\xCD' + bytes([fscod << 6 | frmsizecod, bsid << 3 | bsmod, acmod << 5 | 0x1F])


def eac3_header(frmsiz=383, fscod=0, c2=3, acmod=2, lfeon=0, bsid=16, strmtyp=0, substreamid=0):
    return b'\x0B\x77' + bytes([strmtyp << 6 | substreamid << 3 | frmsiz >> 8, frmsiz & 255, fscod << 6 | c2 << 4 | acmod << 1 | lfeon, bsid << 3 | 4])


def mpa_frame(rng, body=None, **kw):
    return _fill(mpa_header(**kw), A.MPA, rng, body)


def adts_frame(rng, length, body=None, **kw):
    return _fill(adts_header(length, **kw), A.ADTS, rng, body)


def ac3_frame(rng, body=None, **kw):
    return _fill(ac3_header(**kw), A.AC3, rng, body)


def eac3_frame(rng, body=None, **kw):
    return _fill(eac3_header(**kw), A.AC3, rng, body)


def random_frames(rng, codec, nbytes, bad=0.0):
    """frames of at least nbytes: the parameters change now and then (a CHANGE), and a share `bad` of the headers is broken (a LOSS)"""
    out, n = [], 0
    bri, length, fsc = 9, 300, 20
    while n < nbytes:
        if rng.random() < 0.05:
            bri, length, fsc = int(rng.integers(1, 15)), int(rng.integers(7, 700)), int(rng.integers(0, 38))
        if codec == A.MPA:
            f = mpa_frame(rng, ver=3, layer=2, bri=bri, sri=1, pad=int(rng.integers(0, 2)), mode=bri % 4)
        elif codec == A.ADTS:
            f = adts_frame(rng, length + int(rng.integers(0, 40)), sfi=3 + bri % 3, chan=2)
        elif rng.random() < 0.5:
            f = ac3_frame(rng, fscod=bri % 3, frmsizecod=fsc, acmod=2)
        else:
            f = eac3_frame(rng, frmsiz=100 + 8 * fsc, fscod=0, c2=3)
        if rng.random() < bad:
            f = bytes([f[0] ^ 0x40]) + f[1:]
        out.append(f)
        n += len(f)
    return out


class Line(E.Line):
    """the TS packets of one audio PID (stream_id C0)"""

    def pes(self, es, sizes=None, **kw):
        return super().pes(es, sizes, stream_id=0xC0, **kw)


def random_mux(rng, n, watches, other=0x300, faults=True, unaligned=()):
    """n packets: on every (pid, codec) of `watches` PES packets of random frames -- one to four whole frames each, or, on the PIDs of
    `unaligned`, cut anywhere and now and then at a frame's end, so that a later start can acquire -- in TS packets of mostly 184 and sometimes few bytes, interleaved at random with packets of PID `other`
    and null packets; with faults a share of the frame headers is broken, a share of the packets is dropped, repeated, scrambled,
    given a DI or an adaptation field that leaves no payload, and a share of the PES headers is bad, split over two packets or
    scrambled -> [n, 188]"""
    state = {}
    for pid, codec in watches:
        frames = random_frames(rng, codec, n * 200 // len(watches), bad=0.02 if faults else 0.0)
        state[pid] = dict(cc=int(rng.integers(0, 16)), frames=frames, es=b''.join(frames), ends=np.cumsum([len(f) for f in frames]), at=0, left=b'',
                          pts=int(rng.integers(0, 1 << 33)))
    pids = [p for p, _ in watches]
    out = []
    while len(out) < n:
        r = rng.random()
        if r < 0.08:
            out.append(P.null_packets(1)[0])
            continue
        if r < 0.16:
            out.append(P.ts_packet(other, len(out), b'', fill=int(rng.integers(0, 256))))
            continue
        pid = pids[int(rng.integers(0, len(pids)))]
        s = state[pid]
        kw, pusi = {}, 0
        if not s['left']:
            if pid in unaligned:
                end = s['at'] + int(rng.integers(1, 1500))
                if rng.random() < 0.4:                                              # now and then up to a frame's end: the next start can acquire
                    end = int(s['ends'][np.searchsorted(s['ends'], min(end, len(s['es'])))])
                es = s['es'][s['at']:end]
                s['at'] = end if end < len(s['es']) else 0
            else:
                k = int(rng.integers(1, 5))
                es = b''.join(s['frames'][s['at']:s['at'] + k])
                s['at'] = s['at'] + k if s['at'] + k < len(s['frames']) else 0
            s['pts'] += 3600
            hk = dict(pts=s['pts'], dts=None, stuffing=int(rng.integers(0, 4)), stream_id=0xC0)
            f = rng.random() if faults else 1.0
            if f < 0.04:
                hk.update(start=b'\x00\x01\x01')
            elif f < 0.08:
                hk.update(pts_markers=(1, 0, 1))
            elif f < 0.12:
                kw.update(tsc=2)
            s['left'], pusi = head(**hk) + es, 1
            take = 184
            if faults and 0.12 <= f < 0.2:
                take = int(rng.choice([5, 8, 13, 14, 15]))                          # the header is short of its packet: SHORT, or HEADER and split
            elif rng.random() < 0.1:
                take = len(head(**hk)) + int(rng.integers(0, 9))                    # the header ends with the packet, or a few bytes of a frame header follow
        else:
            take = int(rng.choice([1, 2, 3, 7, 8, 40])) if rng.random() < 0.1 else 184
        take = min(take, len(s['left']))
        pk = pkt(pid, s['cc'], s['left'][:take], pusi, **kw)
        s['left'] = s['left'][take:]
        s['cc'] = (s['cc'] + 1) & 15
        if faults:
            f = rng.random()
            if f < 0.02:
                continue                                                # lost
            if f < 0.05:
                out.append(pk)                                          # repeated (and perhaps once more below)
                if rng.random() < 0.3:
                    out.append(pk)
            elif f < 0.07:
                pk = pk.copy()
                pk[3] |= 0x80                                           # scrambled
            elif f < 0.085:
                pk = P.ts_packet(pid, s['cc'] - 1, b'', af_len=183, afc=3)  # an adaptation field that leaves no payload
            elif f < 0.10:
                pk = P.ts_packet(pid, s['cc'] - 1, b'', afc=2, di=int(rng.random() < 0.5))
                s['cc'] = (s['cc'] - 1) & 15                            # no payload: the counter does not advance
            elif f < 0.11:
                pk = pk.copy()
                if pk[3] & 0x20 and pk[4] > 0:
                    pk[5] |= 0x80                                       # an announced discontinuity on a packet that goes on
        out.append(pk)
    return np.array(out[:n])


MUX_SEED, MUX_PACKETS = 31, 2600
WATCHES = [(3, PIDS[A.MPA], A.MPA), (0, PIDS[A.ADTS], A.ADTS), (11, PIDS[A.AC3], A.AC3), (5, 0x163, A.MPA)]
_mux = []


def mux():
    """the faulty multiplex of the tests on the three PIDS and an unaligned MPA PID 0x163; built once, not to be written to
    (tests/test_aud_cpu.py checks what it yields)"""
    if not _mux:
        m = random_mux(np.random.default_rng(MUX_SEED), MUX_PACKETS, [(p, c) for _, p, c in WATCHES], unaligned=(0x163,))
        m.setflags(write=False)
        _mux.append(m)
    return _mux[0]


def model(max_rows=1 << 30, watches=WATCHES):
    m = A.Aud(max_rows)
    for slot, pid, codec in watches:
        m.set_watch(slot, pid, codec)
    return m


def same(bank, model, stream=0):
    """a bank (device or host) and the model agree on everything the last call of `stream` left"""
    got, want = bank.rows(stream), model.table
    assert len(got) == len(want), (stream, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (stream, i, g, w)
    for slot in range(-1, 16):
        assert bank.stats(stream, slot) == model.stats(slot), (stream, slot, bank.stats(stream, slot), model.stats(slot))
    assert bank.stream_stats(stream) == model.stream_stats(), stream
