"""Constructed cases of the PES bank (include/dvbs2gpu.h, PES bank), shared by the CPU tests, the GPU tests and the sanitizer run: each
is a short stream on PID `PID` in which one rule decides, with what the rule must give written out as numbers.  The cases run one
after the other on a bank that watches PID in slot 0 at rate TPP_Q24; each opens with a plain video start S0 (HEADER with a PTS,
declared 0), so what a case's first row closes belongs to the case before and the literal rows are those behind the first."""
import numpy as np

import pes_ref as P

PID, OTHER = 0x1E1, 0x1E2
TPP = 90000                     # 27 MHz ticks per packet: a packet lasts 300 ticks of 90 kHz, 0.7 s are 210 packets
TPP_Q24 = TPP << 24
LATE = 210
STEP = 3600                     # 90 kHz ticks between the PTS of two starts unless a case says otherwise
H, SH, BAD, PL, MAL, SCR = P.HEADER, P.SHORT, P.BAD_START, P.PLAIN, P.MALFORMED, P.SCRAMBLED
C, GAP, MIS, UNC, UNB = P.CLOSED, P.CLOSED_GAP, P.CLOSED_MISMATCH, P.CLOSED_UNCHECKED, P.UNBOUNDED_NONVIDEO
CU, CG, CM = C | UNC, C | GAP, C | MIS


class Line:
    """the packets of one PID as a multiplexer would write them: the counter and the PTS go on by themselves"""

    def __init__(self, pid=PID, cc=3, pts=(1 << 33) - 40 * STEP):
        self.pid, self.cc, self.pts, self.out = pid, cc, pts, []

    def start(self, pts=True, step=STEP, **kw):
        """a start; pts True: the line's next PTS, None: none, a number: that PTS (the line goes on from it)"""
        if pts is True:
            self.pts += step
        elif pts is not None:
            self.pts = pts
        self.out.append(P.pes_packet(self.pid, self.cc, pts=None if pts is None else self.pts, **kw))
        self.cc += 1
        return self

    def body(self, n=1, **kw):
        for _ in range(n):
            self.out.append(P.body_packet(self.pid, self.cc, **kw))
            self.cc += 1
        return self

    def again(self):
        self.out.append(self.out[-1])                                   # a duplicate: the same packet once more
        return self

    def lose(self):
        self.cc += 1
        return self

    def no_payload(self, di=0):
        self.out.append(P.ts_packet(self.pid, self.cc - 1, b'', afc=2, di=di))   # the counter does not advance
        return self

    def nulls(self, n):
        self.out += list(P.null_packets(n))
        return self

    def take(self):
        out, self.out = np.array(self.out), []
        return out


def edge_cases():
    """-> [(name, packets [n, 188], the rows behind the first as (kind, flags, closed_bytes) or None)]"""
    ln, cases = Line(), []

    def case(name, want=None):
        cases.append((name, ln.take(), want))

    ln.start()
    for L in (5, 6, 8):
        ln.start(af_len=183 - L)
    for L in (9, 13, 14):
        ln.start(af_len=183 - L, step=0)
    ln.start(af_len=183 - 9, pts=None)                                  # flags 00 needs nine bytes and no more
    for L in (18, 19):
        ln.start(af_len=183 - L, dts=ln.pts + STEP - 1800)
    case('payload lengths 5, 6, 8, 9, 13, 14, 9 without PTS, 18, 19',
         [(SH, CU, 184), (SH, CU, 5), (SH, CU, 6), (SH, CU, 8), (SH, CU, 9), (H, CU, 13), (H, CU, 14), (SH, CU, 9), (H, CU, 18)])
    ln.start().body(af_len=182).start(af_len=182)
    ln.out.append(P.ts_packet(PID, ln.cc, b'', af_len=183, afc=3))      # b4 183 with AFC 3: no payload byte is left
    ln.cc += 1
    ln.start()
    case('b4 182 and 183', [(SH, CU, 185), (H, CG, 1)])
    ln.start()
    for sid in P.PLAIN_IDS:
        ln.start(stream_id=sid, declared=178, pts=None)
    ln.start()
    case('the eight stream ids without a header', [(PL, CU, 184)] + [(PL, C, 184)] * 7 + [(H, C, 184)])
    ln.start().start(pts=None).start(flags=1).start().start(dts=ln.pts + STEP - 900)
    case('PTS_DTS_flags 00, 01, 10, 11', [(H, CU, 184), (MAL, CU, 184), (H, CU, 184), (H, CU, 184)])
    ln.start()
    for m in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        ln.start(pts_markers=m, step=0)
    for m in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        ln.start(dts=ln.pts - 5, dts_markers=m, step=0)
    ln.start(pts_prefix=3, step=0).start(dts=ln.pts, pts_prefix=2, step=0).start(dts=ln.pts, dts_prefix=3, step=0)
    ln.start(hdl=4, step=0).start(dts=ln.pts, hdl=9, step=0).start(b6=0xC0, step=0).start(start=b'\x00\x00\x02', step=0)
    case('marker bits, prefixes, header lengths, start code', [(MAL, CU, 184)] * 12 + [(BAD, CU, 184)])
    ln.start(pts=(1 << 33) - 1000).start()
    case('PTS wrap across 2^33', [(H, CU, 184)])
    ln.start().start(step=63000).start(step=63001)
    case('dT 63000 and 63001', [(H, CU, 184), (H, CU | P.TS_GAP, 184)])
    ln.start().start(step=(1 << 32) - 1).start(step=1 << 32)
    case('dT 2^32 - 1 and 2^32', [(H, CU | P.TS_GAP, 184), (H, CU | P.TS_BACKWARD, 184)])
    ln.start().start(dts=ln.pts + STEP + 1).start(dts=ln.pts + STEP)
    case('DTS one tick after the PTS, then equal', [(H, CU | P.DTS_AFTER_PTS, 184), (H, CU, 184)])
    ln.start()
    for declared in (362, 363, 361):
        ln.start(declared=declared).body()
    ln.start()
    case('declared + 6 met, one byte short, one byte long', [(H, CU, 184), (H, C, 368), (H, CM, 368), (H, CM, 368)])
    ln.start().start(stream_id=0xE0).start(stream_id=0xC0).start(stream_id=0xC0, declared=178)
    case('declared 0 on video and on audio', [(H, CU, 184), (H, CU | UNB, 184), (H, CU, 184)])
    ln.start().start(declared=546).body().lose().start().start(declared=362).body(af_len=1, di=1).start()
    case('a lost packet and a DI packet inside a PES packet', [(H, CU, 184), (H, CG, 368), (H, CU, 184), (H, CG, 366)])
    ln.start().start(declared=546).again().body().again().body().start()
    case('a duplicate of a start and of a middle packet', [(H, CU, 184), (H, C, 552)])
    ln.start().start(declared=362).body().again().again().start()
    case('three equal counters in a row', [(H, CU, 184), (H, CG, 552)])    # the third is a continuity error, and its payload counts
    ln.start().start(declared=362).no_payload().body().no_payload().start()
    case('packets without payload in between', [(H, CU, 184), (H, C, 368)])
    ln.start().start(tsc=2).body().start(declared=362).body(tsc=1).start()
    case('a scrambled start and a scrambled middle', [(SCR, CU, 184), (H, CU, 368), (H, C, 368)])
    ln.start().nulls(LATE - 1).start(step=63000).nulls(LATE).start(step=63000)
    case('dN 210 and 211', [(H, CU, 184), (H, CU | P.PTS_LATE, 184)])
    ln.start()
    ln.out.append(P.pes_packet(OTHER, 0, pts=5))                        # an unwatched PID, TEI and a bad sync byte: not looked at
    ln.out.append(P.ts_packet(PID, 9, b'', pusi=1, tei=1))
    ln.out.append(P.ts_packet(PID, 9, b'', pusi=1, sync=0x48))
    ln.start()
    case('packets that are not looked at', [(H, CU, 184)])
    return cases


def whole_stream():
    return np.concatenate([ts for _, ts, _ in edge_cases()])


def same(bank, model, stream=0):
    """a bank (device or host) and the model agree on everything the last call of `stream` left"""
    assert bank.row_table(stream) == model.table, stream
    for slot in range(-1, 16):
        assert bank.stats(stream, slot) == model.stats(slot), (stream, slot)
    assert bank.stream_stats(stream) == model.stream_stats(), stream
