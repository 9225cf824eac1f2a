"""GSE decapsulation on the GPU (csrc/bbts_gse.hip): every case runs the same calls through a bank on the device path, a bank forced to
the host parser (dvbs2gpu_bbts_set_gse_path(1)) and one oracle per stream (oracle/bbframe_ts.cpp), and compares output bytes per call,
get_stats, gse_stats and the PDU table.  host_fallback_calls must be 0 wherever a case does not set out to trigger a fallback."""
import zlib

import numpy as np
import pytest

import orc_bbts as B
from test_gpu_bbts import _same_state

pytestmark = pytest.mark.gpu

PKT_CAP = 256                       # GSE_PKT_CAP of csrc/bbts_common.h: packet records per frame
FALLBACK_KEYS = ('host_fallback_calls', 'fallback_records', 'fallback_capacity')
_REV = bytes(int('{:08b}'.format(i)[::-1], 2) for i in range(256))


@pytest.fixture(scope='module')
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def crc32_mpeg(data):
    """CRC-32/MPEG through zlib's reflected CRC-32 (bit order reversed on the way in and out); checked against orc_bbts below"""
    v = zlib.crc32(bytes(data).translate(_REV)) ^ 0xffffffff
    return int('{:032b}'.format(v)[::-1], 2)


def test_fast_crc_is_the_oracle_helpers_crc():
    d = np.random.default_rng(1).integers(0, 256, 333, dtype=np.uint8).tobytes()
    assert crc32_mpeg(d) == B.crc32_mpeg(d) and crc32_mpeg(b'') == 0xffffffff


def fragments(proto, pdu, cuts, frag_id, label=None, corrupt_crc=False):
    """orc_bbts.gse_fragments with the fast CRC"""
    lt = 0 if label is not None else 2
    lab = bytes(label) if label is not None else b''
    total = 2 + len(lab) + len(pdu)
    head = bytes([total >> 8, total & 0xff, proto >> 8, proto & 0xff]) + lab
    crc = crc32_mpeg(head + bytes(pdu)) ^ (0x1000 if corrupt_crc else 0)
    tail = bytes(pdu) + crc.to_bytes(4, 'big')
    pieces = [tail[a:b] for a, b in zip([0] + list(cuts), list(cuts) + [len(tail)])]
    out = []
    for i, pc in enumerate(pieces):
        body = bytes([frag_id]) + (head if i == 0 else b'') + pc
        h = (0x80 | (lt << 4)) if i == 0 else (0x70 if i == len(pieces) - 1 else 0x30)
        out.append(bytes([h | (len(body) >> 8), len(body) & 0xff]) + body)
    return out


def gre(proto, pdu):
    return b'\0\0' + (bytes([proto >> 8, proto & 0xff]) if proto in (0x0800, 0x86DD) else b'') + bytes(pdu)


def pack_frames(packets, kbch):
    """GSE packets in order into data fields; a packet that does not fit any more starts the next frame (zero padding ends a frame).
    An empty frame goes first: a parser that is not synchronised starts SYNCD/8 + 1 bytes into its first frame."""
    room = kbch // 8 - 10
    frames, cur = [B.gse_bbframe([], kbch)], []
    for p in packets:
        if sum(map(len, cur)) + len(p) > room:
            frames.append(B.gse_bbframe(cur, kbch))
            cur = []
        cur.append(p)
    frames.append(B.gse_bbframe(cur, kbch))
    return np.stack(frames)


def transmitter(rng, nbytes, max_pdu=1500):
    """A well-formed GSE packet sequence of about nbytes and what must come out: [(proto, pdu, reassembled, label)].
    Up to three fragmented PDUs are open at once (the three slots, first fit, are modelled here); now and then a fourth is started
    (no slot: ignored with all its fragments), a frag id is restarted while open (the first PDU is lost), or a CRC-32 is corrupted
    (dropped at its END)."""
    pk, want, size = [], [], 0
    slots = [None, None, None]                 # [frag id, remaining packets, survivor or None]
    ghosts = {}                                # ids of ignored fourth PDUs -> remaining packets
    protos = (0x0800, 0x86DD, 0x88B5)

    def pdu_of(n):
        proto = protos[int(rng.integers(0, 3))]
        lab = bytes(rng.integers(0, 256, 6, dtype=np.uint8)) if rng.random() < 0.5 else None
        return proto, rng.integers(0, 256, n, dtype=np.uint8).tobytes(), lab

    while size < nbytes or any(slots):
        r = rng.random()
        draining = size >= nbytes
        busy = [i for i in range(3) if slots[i]]
        new = None
        if not draining and r < 0.45:
            proto, pdu, lab = pdu_of(int(rng.integers(40, max_pdu + 1)))
            new = B.gse_complete(proto, pdu, label=lab)
            want.append((proto, pdu, False, lab is not None))
        elif not draining and r < 0.65:
            sizes = rng.integers(40, min(max_pdu, 1400), int(rng.integers(2, 6)))
            proto, pdu, lab = pdu_of(int(sizes.sum()) - 4)
            cuts = [int(x) for x in np.cumsum(sizes)[:-1]]
            bad = rng.random() < 0.1
            if len(busy) == 3 and rng.random() < 0.5:
                fid = next(i for i in range(200, 256) if i not in ghosts)
                fr = fragments(proto, pdu, cuts, fid, lab)
                ghosts[fid] = fr[1:]
                new = fr[0]
            else:
                # a restart takes the slot that holds the id only if no free slot comes before it (first fit)
                restartable = [i for i in busy if all(slots[j] for j in range(i))]
                if restartable and (len(busy) == 3 or rng.random() < 0.15):
                    i = restartable[int(rng.integers(0, len(restartable)))]
                    fid = slots[i][0]
                else:
                    i = next(j for j in range(3) if not slots[j])
                    fid = next(int(x) for x in rng.permutation(64) if all(not sl or sl[0] != int(x) for sl in slots))
                fr = fragments(proto, pdu, cuts, fid, lab, corrupt_crc=bad)
                slots[i] = [fid, fr[1:], None if bad else (proto, pdu, True, lab is not None)]
                new = fr[0]
        elif ghosts and r < 0.72:
            fid = next(iter(ghosts))
            new = ghosts[fid].pop(0)
            if not ghosts[fid]:
                del ghosts[fid]
        elif busy:
            i = busy[int(rng.integers(0, len(busy)))]
            new = slots[i][1].pop(0)
            if not slots[i][1]:
                if slots[i][2] is not None:
                    want.append(slots[i][2])
                slots[i] = None
        if new:
            pk.append(new)
            size += len(new)
    return pk, want


def chain_walk_counts(frames, kbch):
    """packets per frame by the parser's own chain rule (next = at + 2 + field), for frames that are walked from byte 10"""
    fb = kbch // 8
    flat = np.ascontiguousarray(frames).reshape(-1)
    out = []
    for f in range(len(flat) // fb):
        h = flat[f * fb:f * fb + 10]
        if B.crc8(h) != 0 or h[0] >> 6 != 1:
            continue
        at, end, n = f * fb + 10, f * fb + 10 + ((int(h[4]) << 8 | int(h[5])) // 8), 0
        while at < end and at + 2 <= flat.size:
            h1 = int(flat[at])
            if not h1 & 0xc0 and not h1 & 0x30:
                break
            first, last = h1 & 0x80, h1 & 0x40
            fixed = 2 if first and last else 5 if first else 1
            label = 6 if first and not h1 & 0x30 else 0
            nxt = at + 2 + fixed + label + ((((h1 & 15) << 8 | int(flat[at + 1])) - fixed - label) & 0xffff)
            if nxt > flat.size:
                break
            n, at = n + 1, nxt
        out.append(n)
    return out


class Trio:
    """device-path bank, forced host-path bank, oracles; run() compares them call by call"""

    def __init__(self, pkg, eng, kbch, nstreams, max_frames=8, oracle_streams=None):
        self.pkg, self.kbch, self.n = pkg, kbch, nstreams
        self.dev = pkg.BbTsParserBank(eng, nstreams, kbch, max_frames)
        self.host = pkg.BbTsParserBank(eng, nstreams, kbch, max_frames)
        self.host.set_gse_path(1)
        self.osel = list(range(nstreams)) if oracle_streams is None else list(oracle_streams)
        self.orcs = {s: B.OracleBbTs(kbch) for s in self.osel}
        self.outs = [[] for _ in range(nstreams)]
        self.tables = [[] for _ in range(nstreams)]

    def set_frame_size(self, kbch):
        for x in (self.dev, self.host, *self.orcs.values()):
            x.set_frame_size(kbch)
        self.kbch = kbch

    def run(self, frames, cap=None, tin=None):
        import torch
        fb = self.kbch // 8
        # the bound of include/dvbs2gpu.h that keeps fallback (b) away: input + 376 + what three open reassemblies can hold
        cap = cap if cap is not None else max(f.size for f in frames) + 376 + 3 * 65536
        if tin is None:
            tin = [torch.from_numpy(np.ascontiguousarray(f).reshape(-1)).cuda() if f.size else torch.zeros(0, dtype=torch.uint8, device='cuda') for f in frames]
        od = torch.zeros((self.n, cap), dtype=torch.uint8, device='cuda')
        oh = torch.zeros((self.n, cap), dtype=torch.uint8, device='cuda')
        nd = self.dev.process_batch(tin, list(od))
        nh = self.host.process_batch(tin, list(oh))
        assert nd == nh
        od, oh = od.cpu().numpy(), oh.cpu().numpy()
        keep = np.arange(cap)[None, :] < np.array(nd)[:, None]
        assert np.array_equal(od * keep, oh * keep)
        for s in self.osel:
            want = self.orcs[s].work(frames[s].reshape(-1, fb), cap=cap)
            assert want is not None and nd[s] == want.size, (s, nd[s], None if want is None else want.size)
            assert np.array_equal(od[s, :nd[s]], want), s
            _same_state(self.dev, s, self.orcs[s])
            _same_state(self.host, s, self.orcs[s])
            a, b = self.dev.gse_stats(s), self.host.gse_stats(s)
            assert {k: v for k, v in a.items() if k not in FALLBACK_KEYS} == {k: v for k, v in b.items() if k not in FALLBACK_KEYS}, s
            ta, tb = self.dev.pdu_table(s), self.host.pdu_table(s)
            assert ta == tb, s
            self.outs[s].append(od[s, :nd[s]].copy())
            self.tables[s].append(ta)
        return nd

    def fallbacks(self, s):
        st = self.dev.gse_stats(s)
        assert st['host_fallback_calls'] == st['fallback_records'] + st['fallback_capacity']
        assert all(self.host.gse_stats(s)[k] == 0 for k in FALLBACK_KEYS)
        return st['fallback_records'], st['fallback_capacity']

    def no_fallbacks(self):
        for s in self.osel:
            assert self.fallbacks(s) == (0, 0), s


def check_rows(out, rows, want):
    """the rows of one call against the expected PDUs: GRE header, protocol type, flags, bytes; returns how many were used"""
    at = 0
    for (off, n, proto, flags), (wp, pdu, reasm, lab) in zip(rows, want):
        assert off == at and proto == wp and flags == (1 if reasm else 0) | (2 if lab else 0)
        assert bytes(out[off:off + n]) == gre(wp, pdu)
        at += n
    assert at == len(out)
    return len(rows)


def split_calls(rng, frames, lo, hi):
    calls, at = [], 0
    while at < len(frames):
        k = int(rng.integers(lo, hi + 1))
        calls.append(frames[at:at + k])
        at += k
    return calls


@pytest.mark.parametrize('kbch', [14232, 58192])
def test_well_formed_bank(pkg, eng, kbch):
    S, fb = 64, kbch // 8
    rng = np.random.default_rng(kbch)
    streams = []
    for s in range(S):
        pk, want = transmitter(np.random.default_rng(1000 * kbch + s), 20 * (fb - 10))
        streams.append((pack_frames(pk, kbch), want))
    assert max(max(chain_walk_counts(f, kbch)) for f, _ in streams) < PKT_CAP
    concat = []
    for cut in range(2):
        t = Trio(pkg, eng, kbch, S)
        per = [split_calls(rng, f, 0, 8)[:5] for f, _ in streams]
        for s, (f, _) in enumerate(streams):       # six calls: the sixth takes what is left, up to 8 frames at a time afterwards
            done = sum(len(c) for c in per[s])
            per[s].append(f[done:done + 8])
            per[s] += [f[a:a + 8] for a in range(done + 8, len(f), 8)]
        empty = np.zeros((0, fb), np.uint8)
        for c in range(max(len(p) for p in per)):
            t.run([p[c] if c < len(p) else empty for p in per])
        t.no_fallbacks()
        for s, (f, want) in enumerate(streams):
            used = 0
            for out, rows in zip(t.outs[s], t.tables[s]):
                used += check_rows(out, rows, want[used:])
            assert used == len(want), (s, used, len(want))        # exactly the PDUs that survive, in order
            st = t.dev.gse_stats(s)
            assert st['complete_pdus'] + st['reassembled_pdus'] == len(want) and st['frames'] == len(f)
            assert st['bytes_delivered'] == sum(len(gre(p, d)) for p, d, _, _ in want)
        concat.append([np.concatenate(o) for o in t.outs])
    assert all(np.array_equal(a, b) for a, b in zip(*concat))      # the cut into calls does not show in the output


def test_mixed_ts_and_gse_frames_in_one_call(pkg, eng):
    kbch = 14232
    fb, rng = kbch // 8, np.random.default_rng(50)
    D = fb - 10
    tsp = B.ts_packets(6 * D // 188 + 2, rng)
    ts = B.bbframes_from_ts(tsp, kbch, 6)
    pk, want = transmitter(rng, 4.3 * D)
    g = pack_frames(pk, kbch)
    assert 5 <= len(g) <= 20
    t = Trio(pkg, eng, kbch, 2, max_frames=16)
    a = np.stack([ts[0], g[0], ts[1], ts[2], g[1], g[2]])
    b = np.stack([g[3], ts[3], ts[4], g[4], ts[5]])
    t.run([a, a[:3]])
    t.run([b, np.stack([g[1], ts[5]])])
    t.run([g[5:], ts[:0]])
    t.no_fallbacks()
    out = np.concatenate(t.outs[0])
    # frame order: what no row covers is the TS, intact and in order; what the rows cover is the PDUs
    mask = np.ones(out.size, bool)
    base, got = 0, []
    for o, rows in zip(t.outs[0], t.tables[0]):
        for off, n, proto, flags in rows:
            mask[base + off:base + off + n] = False
            got.append(bytes(o[off:off + n]))
        base += o.size
    n_ts = (6 * D - 1) // 188
    assert np.array_equal(out[mask].reshape(-1, 188), tsp[:n_ts])
    assert got == [gre(p, d) for p, d, _, _ in want]
    first_gse_row = t.tables[0][0][0][0]
    assert first_gse_row > 0 and first_gse_row % 188 == 0           # TS of frame 0 first


@pytest.mark.parametrize('kbch', [3072, 14232, 48408])
@pytest.mark.parametrize('seed', [21, 22, 23])
def test_fuzz(pkg, eng, kbch, seed):
    rng = np.random.default_rng(seed * 100000 + kbch)
    S = 8
    calls = [[B.fuzz_frames(rng, kbch, int(rng.integers(0, 7)), ts_gs_choices=(1, 1, 1, 3, 0), p_bad=0.15) for _ in range(S)] for _ in range(20)]
    most = max([max(chain_walk_counts(f, kbch), default=0) for c in calls for f in c if len(f)], default=0)
    assert 0 < most < PKT_CAP            # random length fields: a few packets per frame, far from the record capacity
    t = Trio(pkg, eng, kbch, S)
    for c in calls:
        t.run(c)
    t.no_fallbacks()
    assert sum(t.dev.gse_stats(s)['packets'] for s in range(S)) > 0


def test_resync_and_header_skips(pkg, eng):
    kbch = 14232
    fb, rng = kbch // 8, np.random.default_rng(60)
    pk, want = transmitter(rng, 8 * (fb - 10), max_pdu=600)
    g = pack_frames(pk, kbch)
    assert len(g) >= 8
    bad = g[2].copy(); bad[9] ^= 0x5a                               # BBHEADER CRC-8: the frame is lost, the next one resynchronises
    nxt = g[3].copy(); nxt[:10] = B.bbheader(1, (fb - 10) * 8, syncd_bits=24 * 8)     # ... SYNCD/8 + 1 bytes in, for DFL/8 bytes
    issy = g[4].copy(); issy[:10] = B.bbheader(1, (fb - 10) * 8, 0, issyi=1)
    npd = g[5].copy(); npd[:10] = B.bbheader(1, (fb - 10) * 8, 0, npd=1)
    long_ = g[6].copy()                                             # a complete packet announcing more bytes than the call has left
    long_[10:14] = [0xC0 | 0x20 | 0x0f, 0xff, 0x08, 0x00]
    t = Trio(pkg, eng, kbch, 1)
    t.run([np.stack([g[0], g[1], bad, nxt, g[4]])])
    t.run([np.stack([issy, npd, g[5]])])
    t.run([np.stack([g[6], long_])])                                # runs past the end of the call's input: that frame's parse ends
    t.run([np.stack([long_, g[7], g[0], g[1]])])                    # the same packet with enough frames behind it is a packet
    t.no_fallbacks()
    assert t.dev.gse_stats(0)['frames'] == 11 and t.tables[0][-1][0] == (0, 4097, 0x0800, 0)


def test_fallback_a_more_packets_than_records(pkg, eng):
    kbch = 14232
    rng = np.random.default_rng(70)
    small = [B.gse_complete(0x0800, rng.integers(0, 256, 1, dtype=np.uint8)) for _ in range(PKT_CAP + 1)]     # 5 bytes each
    exact = small[:PKT_CAP]
    pk, want = transmitter(rng, 4 * (kbch // 8 - 10), max_pdu=500)
    g = pack_frames(pk, kbch)[:8]
    assert len(g) >= 3
    t = Trio(pkg, eng, kbch, 2)
    t.run([np.stack([g[0], B.gse_bbframe(exact, kbch)]), g[:1]])    # exactly the capacity: still on the device
    assert t.fallbacks(0) == (0, 0)
    t.run([np.stack([g[1], B.gse_bbframe(small, kbch)]), g[1:2]])
    assert t.fallbacks(0) == (1, 0) and t.fallbacks(1) == (0, 0)
    assert len(t.tables[0][1]) >= PKT_CAP + 1
    t.run([g[2:], g[2:]])                                           # and back on the device, from the state the host parser left
    assert t.fallbacks(0) == (1, 0) and t.fallbacks(1) == (0, 0)


def test_fallback_b_capacity_and_64k_overflow(pkg, eng):
    kbch = 58192
    fb, rng = kbch // 8, np.random.default_rng(80)
    pdu = rng.integers(0, 256, 60 * 1024, dtype=np.uint8).tobytes()
    cuts = list(range(4000, len(pdu), 4000))
    fr = fragments(0x0800, pdu, cuts, 7)
    g = pack_frames(fr, kbch)
    t = Trio(pkg, eng, kbch, 1, max_frames=16)
    t.run([g[:-1]], cap=16 * fb + 376)
    assert t.fallbacks(0) == (0, 0)
    t.run([g[-1:]], cap=fb + 376)                                    # the documented minimum: the 60 KiB PDU does not fit, it is dropped
    assert t.fallbacks(0) == (0, 1) and t.outs[0][-1].size == 0
    assert t.dev.gse_stats(0)['dropped_no_fit'] == 1
    # the same with room: delivered, on the device
    t2 = Trio(pkg, eng, kbch, 1, max_frames=16)
    t2.run([g[:-1]], cap=16 * fb + 376)
    t2.run([g[-1:]], cap=fb + 376 + 3 * 65536)
    t2.no_fallbacks()
    assert bytes(t2.outs[0][-1]) == gre(0x0800, pdu) and t2.tables[0][-1] == [(0, len(pdu) + 4, 0x0800, 1)]
    # 64 KiB overflow frees the slot: 17 fragments of 4000 bytes under one START; what follows the overflow is ignored, a new START is taken
    over = [fr[0]] + [fr[1]] * 17 + [fr[-1]] + fragments(0x86DD, pdu[:3000], [1000], 7)
    go = pack_frames(over, kbch)
    t3 = Trio(pkg, eng, kbch, 1, max_frames=16)
    t3.run([go[:16]], cap=16 * fb + 376)
    t3.run([go[16:]], cap=16 * fb + 376)
    t3.no_fallbacks()
    st = t3.dev.gse_stats(0)
    assert st['dropped_overflow'] == 1 and st['reassembled_pdus'] == 1 and bytes(t3.outs[0][-1]) == gre(0x86DD, pdu[:3000])


def test_set_frame_size_keeps_open_reassemblies(pkg, eng):
    rng = np.random.default_rng(90)
    pdu = rng.integers(0, 256, 2500, dtype=np.uint8).tobytes()
    fr = fragments(0x0800, pdu, [700, 1500], 3, label=bytes(6))
    t = Trio(pkg, eng, 14232, 1)
    t.run([np.stack([B.gse_bbframe([b'\0'] + fr[:1], 14232)])])
    t.set_frame_size(58192)
    t.run([np.stack([B.gse_bbframe([b'\0'] + fr[1:2], 58192)])])
    t.set_frame_size(14232)          # every change forgets the synchronisation: each of these frames is walked from its second byte
    t.run([np.stack([B.gse_bbframe([b'\0'] + fr[2:], 14232)])])
    t.no_fallbacks()
    assert bytes(t.outs[0][-1]) == gre(0x0800, pdu) and t.tables[0][-1] == [(0, 2504, 0x0800, 3)]


def test_path_can_change_between_calls(pkg, eng):
    """state moves with the path: host parser first, then the device, then the host parser again"""
    kbch = 14232
    rng = np.random.default_rng(95)
    pk, want = transmitter(rng, 12 * (kbch // 8 - 10))
    g = pack_frames(pk, kbch)
    import torch
    bank, o = pkg.BbTsParserBank(eng, 1, kbch, 8), B.OracleBbTs(kbch)
    for k, a in enumerate(range(0, len(g), 3)):
        bank.set_gse_path(1 if k % 2 == 0 else 0)
        fr = g[a:a + 3]
        out = torch.zeros(fr.size + 376, dtype=torch.uint8, device='cuda')
        nb = bank.process_batch([torch.from_numpy(fr.reshape(-1)).cuda()], [out])
        assert np.array_equal(out[:nb[0]].cpu().numpy(), o.work(fr))
        _same_state(bank, 0, o)
    assert bank.gse_stats(0)['host_fallback_calls'] == 0


def test_4096_streams_one_call(pkg, eng):
    import torch
    kbch, S, P = 58192, 4096, 64
    fb = kbch // 8
    pats = []
    for p in range(P):
        pk, _ = transmitter(np.random.default_rng(7000 + p), 9 * (fb - 10))
        pats.append(pack_frames(pk, kbch)[:8])
    assert all(len(p) == 8 for p in pats)
    tens = [torch.from_numpy(p.reshape(-1)).cuda() for p in pats]
    frames = [pats[s % P] for s in range(S)]
    t = Trio(pkg, eng, kbch, S, oracle_streams=range(0, S, 65))       # 64 streams, every pattern once
    nd = t.run(frames, tin=[tens[s % P] for s in range(S)], cap=8 * fb + 376)       # nothing is open before the call: the input bounds the output
    assert min(nd) > 0
    t.no_fallbacks()
    for s in (1, 2047, 4095):
        assert t.dev.gse_stats(s)['host_fallback_calls'] == 0 and t.dev.pdu_table(s) == t.host.pdu_table(s)
