"""Builders for the tests of the ES bank (include/dvbs2gpu.h, ES bank): elementary streams of the three codecs written unit by unit
(sequence / GOP / picture headers and slices of MPEG-2; AUD, SPS, PPS, SEI, IDR and non-IDR slices of H.264; AUD, VPS, SPS, PPS, SEI,
IRAP and trailing slices of H.265), their PES packets laid into TS packets of any payload length, and a random faulty multiplex.
Filler bytes are never 0, so the only start codes of a stream are the ones written here."""
import numpy as np

import es_ref as E
import pes_ref as P

PIDS = {E.MPEG2: 0x150, E.H264: 0x151, E.H265: 0x152}
SC = b'\x00\x00\x01'
# the first head byte of an H.264 slice with first_mb_in_slice = 0 and slice_type I (7), P (5), B (6), SP (3), and one of a later slice
H264_I, H264_P, H264_B, H264_SP, H264_LATER = 0x88, 0x98, 0x9C, 0x90, 0x23


def body(rng, n):
    return bytes(rng.integers(1, 256, n, dtype=np.uint8))


def mpeg2_picture(rng, kind, tref=0, slices=3, seq=False, gop=False, end=False, size=(40, 300)):
    """kind 1 I, 2 P, 3 B (others: as written) -> the bytes of one coded picture with what precedes it"""
    out = b''
    if seq:
        out += SC + b'\xB3' + body(rng, 8) + SC + b'\xB5' + body(rng, 6)          # sequence header, sequence extension
    if gop:
        out += SC + b'\xB8' + body(rng, 4)
    out += SC + b'\x00' + bytes([tref >> 2 & 255, (tref & 3) << 6 | kind << 3 | 7]) + body(rng, 2)
    out += SC + b'\xB5' + body(rng, 5)                                            # picture coding extension
    for s in range(slices):
        out += SC + bytes([1 + s]) + body(rng, int(rng.integers(*size)))
    if end:
        out += SC + b'\xB7'
    return out


def h264_picture(rng, first, idr=False, slices=2, aud=True, sps=False, sei=False, end=False, bad=False, long_code=False, size=(40, 300)):
    """first: the first head byte of the picture's first slice (H264_I ...)"""
    out = b''
    if aud:
        out += (b'\x00' if long_code else b'') + SC + b'\x09' + b'\xF0'
    if sps:
        out += b'\x00' + SC + b'\x67' + body(rng, 12) + b'\x00' + SC + b'\x68' + body(rng, 4)
    if sei:
        out += SC + b'\x06' + body(rng, 9)
    if bad:
        out += SC + b'\xE5' + body(rng, 5)                                        # forbidden_zero_bit set
    nal = 0x65 if idr else 0x41
    for s in range(slices):
        out += SC + bytes([nal, first if s == 0 else H264_LATER]) + body(rng, int(rng.integers(*size)))
    if end:
        out += SC + b'\x0A'
    return out


def h265_picture(rng, nal_type, slices=2, aud=True, sps=False, sei=False, end=False, bad=False, size=(40, 300)):
    """nal_type: 19 IDR_W_RADL, 21 CRA, 1 TRAIL_R, 0 TRAIL_N ..."""
    hdr = lambda t, tid=1: bytes([t << 1, tid])
    out = b''
    if aud:
        out += SC + hdr(35) + b'\x50'
    if sps:
        out += SC + hdr(32) + body(rng, 10) + SC + hdr(33) + body(rng, 14) + SC + hdr(34) + body(rng, 4)
    if sei:
        out += SC + hdr(39) + body(rng, 7)
    if bad:
        out += SC + hdr(1, 0) + body(rng, 5)                                      # nuh_temporal_id_plus1 = 0
    for s in range(slices):
        out += SC + hdr(nal_type) + bytes([0x80 | 0x15 if s == 0 else 0x15]) + body(rng, int(rng.integers(*size)))
    if end:
        out += SC + hdr(36) + b'\x01'
    return out


def random_es(rng, codec, nbytes):
    """an elementary stream of at least nbytes: GOPs of 6 pictures, every unit of the codec among them"""
    out, n = [], 0
    while sum(map(len, out)) < nbytes:
        g, first = n % 6, n % 6 == 0
        r = rng.random()
        if codec == E.MPEG2:
            kind = 1 if first else (2 if g % 3 == 0 else 3) if r > 0.05 else 4    # now and then a D picture: detail 0
            out.append(mpeg2_picture(rng, kind, n & 1023, int(rng.integers(1, 5)), seq=first, gop=first, end=first and r < 0.5))
        elif codec == E.H264:
            kind = H264_I if first else (H264_P if g % 3 == 0 else H264_B) if r > 0.05 else H264_SP
            out.append(h264_picture(rng, kind, idr=first and n % 12 == 0, slices=int(rng.integers(1, 4)), sps=first, sei=r < 0.3, end=first and r < 0.5,
                                    bad=r > 0.9, long_code=r < 0.5))
        else:
            out.append(h265_picture(rng, (19 if n % 12 == 0 else 21) if first else int(rng.integers(0, 10)), slices=int(rng.integers(1, 4)), sps=first,
                                    sei=r < 0.3, end=first and r < 0.5, bad=r > 0.9))
        n += 1
    return b''.join(out)


def pkt(pid, cc, payload, pusi=0, **kw):
    """one TS packet whose payload is exactly `payload` (1..184 bytes): the adaptation field takes the rest"""
    assert 1 <= len(payload) <= 184
    return P.ts_packet(pid, cc, payload, af_len=None if len(payload) == 184 else 183 - len(payload), pusi=pusi, **kw)


def head(pts=None, dts=None, stream_id=0xE0, stuffing=0, **kw):
    """a PES header with `stuffing` bytes more of PES_header_data_length"""
    h = P.pes_head(stream_id, pts, dts, 0, **kw)
    return h[:8] + bytes([h[8] + stuffing]) + h[9:] + b'\xFF' * stuffing if stuffing else h


class Line:
    """the TS packets of one PID: PES packets of an elementary stream, the counter going on by itself"""

    def __init__(self, pid, cc=5, pts=90000):
        self.pid, self.cc, self.pts, self.out = pid, cc, pts, []

    def put(self, payload, pusi=0, **kw):
        self.out.append(pkt(self.pid, self.cc, payload, pusi, **kw))
        self.cc += 1
        return self

    def pes(self, es, sizes=None, **kw):
        """one PES packet with the ES bytes `es`; sizes: the payload lengths of its TS packets (the last takes the rest, each at most
        184; default: 184 each and the rest in the last, behind an adaptation field)"""
        self.pts += 3600
        data, first = head(self.pts, **kw) + es, True
        sizes = list(sizes or [])
        while data:
            n = min(sizes.pop(0) if sizes else 184, 184, len(data))
            self.put(data[:n], pusi=int(first))
            data, first = data[n:], False
        return self

    def again(self):
        self.out.append(self.out[-1])
        return self

    def lose(self):
        self.cc += 1
        return self

    def no_payload(self, di=0):
        self.out.append(P.ts_packet(self.pid, self.cc - 1, b'', afc=2, di=di))
        return self

    def take(self):
        out, self.out = np.array(self.out).reshape(-1, 188), []
        return out


def random_mux(rng, n, watches, other=0x300, faults=True):
    """n packets: on every (pid, codec) of `watches` PES packets of a random elementary stream, cut into TS packets of mostly 184 and
    sometimes few bytes, interleaved at random with packets of PID `other` and null packets; with faults a share of the packets is
    dropped, repeated, scrambled, given a DI or an adaptation field that leaves no payload, and a share of the PES headers is bad,
    split over two packets or scrambled -> [n, 188]"""
    state = {}
    for pid, codec in watches:
        state[pid] = dict(cc=int(rng.integers(0, 16)), es=random_es(rng, codec, n * 200 // len(watches)), at=0, left=b'', pts=int(rng.integers(0, 1 << 33)))
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
            size = int(rng.integers(1, 1500))
            es = s['es'][s['at']:s['at'] + size]
            s['at'] += size
            if s['at'] >= len(s['es']):
                s['at'] = 0
            s['pts'] += 3600
            hk = dict(pts=s['pts'], dts=s['pts'] - 1800 if rng.random() < 0.3 else None, stuffing=int(rng.integers(0, 4)))
            f = rng.random() if faults else 1.0
            if f < 0.04:
                hk.update(start=b'\x00\x01\x01')
            elif f < 0.08:
                hk.update(pts_markers=(1, 0, 1))
            elif f < 0.12:
                kw.update(tsc=2)
            s['left'], pusi = head(**hk) + es, 1
            take = 184
            if faults and 0.12 <= f < 0.26:
                take = int(rng.choice([5, 8, 14, 14, 15, 19, 20]))                  # the header is short of its packet: SHORT, or HEADER and split
            elif rng.random() < 0.1:
                take = len(head(**hk)) + int(rng.integers(0, 3))        # the header ends with the packet, or nearly
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


GPU_MUX_SEED, GPU_MUX_PACKETS = 21, 9300
_gpu_mux = []


def gpu_mux():
    """the faulty multiplex of the GPU tests on the three PIDS, long enough for every packet count there; built once, not to be written to
    (tests/test_es_cpu.py checks that it holds at least 10 of everything)"""
    if not _gpu_mux:
        mux = random_mux(np.random.default_rng(GPU_MUX_SEED), GPU_MUX_PACKETS, [(pid, codec) for codec, pid in PIDS.items()])
        mux.setflags(write=False)
        _gpu_mux.append(mux)
    return _gpu_mux[0]


def same(bank, model, stream=0):
    """a bank (device or host) and the model agree on everything the last call of `stream` left"""
    got, want = bank.rows(stream), model.table
    assert len(got) == len(want), (stream, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (stream, i, g, w)
    for slot in range(-1, 16):
        assert bank.stats(stream, slot) == model.stats(slot), (stream, slot)
    assert bank.stream_stats(stream) == model.stream_stats(), stream
