"""Python model of the IP output bank's rules, written from the header comment (include/dvbs2gpu.h, IP output bank) in plain integers and
`struct`.  It is not the sequential form of csrc/ipout_rules.h: a call first lists the packets that every slot takes, then cuts held +
taken into groups of P; the clock is one unbounded sum of the rates, divided when a tick is asked for; a checksum is a remainder modulo
65535.  The yardstick of the bank's tests."""
import copy
import struct

TS = 188
SLOTS = 4
RAW, RTP_MODE = 0, 1
RTP, SHORT, CARRIED = 1, 2, 4
D = 300 << 24
STREAM_KEYS = ('packets', 'bad_sync')
SLOT_KEYS = ('passed', 'datagrams', 'short_datagrams', 'ts_packets', 'bytes_delivered', 'held')
STAT_KEYS = STREAM_KEYS + SLOT_KEYS
ROW_KEYS = ('offset', 'bytes', 'rtp_timestamp', 'rtp_seq', 'packets', 'flags', 'first_packet', 'udp_checksum')
LAYOUT = dict(ipv4_version_ihl=0x45, ipv4_tos_at=1, ipv4_id_at=4, ipv4_dont_fragment=0x4000, ipv4_ttl_at=8, ipv4_checksum_at=10, ipv6_hop_limit_at=7,
              rtp_first_byte=0x80, tick_divisor=300, max_packets_per_datagram=7, held_packets=6, pid_map_bytes=1024, slots=4, row_bytes=24, flow_bytes=56)
FLOW_DEFAULTS = dict(family=0, src=None, dst=None, src_port=0, dst_port=0, ttl=64, dscp=0, mode=RTP_MODE, ssrc=0, seq_base=0, timestamp_base=0,
                     packets_per_datagram=7, pid_mode=0, pids=(), drop_null=False)


def complement_sum(data):
    """the ones'-complement sum of the big-endian 16-bit words of an even number of bytes: the remainder modulo 65535 of the number they
    spell, 0xFFFF standing for a non-zero multiple"""
    assert len(data) % 2 == 0
    n = int.from_bytes(data, 'big')
    return 0 if n == 0 else (n % 0xFFFF or 0xFFFF)


def selects(flow, packet):
    """does a flow (a dict of FLOW_DEFAULTS' keys) take a packet"""
    if packet[0] != 0x47:
        return False
    pid = (packet[1] & 0x1F) << 8 | packet[2]
    if pid == 0x1FFF and flow['drop_null']:
        return False
    return {0: True, 1: pid in flow['pids'], 2: pid not in flow['pids']}[flow['pid_mode']]


def build(flow, packets, seq, timestamp):
    """one datagram -> (bytes, the UDP checksum as computed, before 0 becomes 0xFFFF)"""
    payload = b''.join(packets)
    if flow['mode'] == RTP_MODE:
        payload = struct.pack('>BBHII', 0x80, 33, seq, timestamp, flow['ssrc']) + payload
    L = 8 + len(payload)
    udp = struct.pack('>HHHH', flow['src_port'], flow['dst_port'], L, 0) + payload
    if flow['family'] == 4:
        pseudo = flow['src'] + flow['dst'] + struct.pack('>BBH', 0, 17, L)
    else:
        pseudo = flow['src'] + flow['dst'] + struct.pack('>IBBBB', L, 0, 0, 0, 17)
    computed = 0xFFFF ^ complement_sum(pseudo + udp)
    udp = udp[:6] + struct.pack('>H', computed or 0xFFFF) + udp[8:]
    if flow['family'] == 4:
        ip = struct.pack('>BBHHHBBH', 0x45, flow['dscp'] << 2, 20 + L, 0, 0x4000, flow['ttl'], 17, 0) + flow['src'] + flow['dst']
        ip = ip[:10] + struct.pack('>H', 0xFFFF ^ complement_sum(ip)) + ip[12:]
    else:
        ip = struct.pack('>IHBB', 6 << 28 | flow['dscp'] << 2 << 20, L, 17, flow['ttl']) + flow['src'] + flow['dst']
    return ip + udp, computed


class Stream:
    """one stream: four flows or None, the clock, what the slots hold, counters"""

    def __init__(self):
        self.flows = [None] * SLOTS
        self.rate = 0
        self.reset()

    def reset(self):
        self.ticks_q24 = 0                                             # the rates of all packets so far, summed
        self.held = [[] for _ in range(SLOTS)]                         # per slot: (packet, tick)
        self.made = [0] * SLOTS                                        # datagrams since set_flow
        self.st = dict.fromkeys(STREAM_KEYS, 0)
        self.slot_st = [dict.fromkeys(SLOT_KEYS, 0) for _ in range(SLOTS)]
        self.table = [[] for _ in range(SLOTS)]
        self.computed = [[] for _ in range(SLOTS)]

    def set_flow(self, slot, **kw):
        f = dict(FLOW_DEFAULTS, **kw)
        f['pids'] = frozenset(f['pids'])
        self.flows[slot] = f if f['family'] else None
        self.held[slot], self.made[slot] = [], 0
        self.slot_st[slot] = dict.fromkeys(SLOT_KEYS, 0)

    def set_rate(self, ticks_per_packet_q24):
        self.rate = ticks_per_packet_q24

    def sizes(self, ts, flush=False):
        """the bytes per slot that process() would deliver, with nothing advanced"""
        return [len(o) for o in copy.deepcopy(self).process(ts, flush)]

    def process(self, ts, flush=False):
        """ts: whole packets -> the datagrams per slot (four bytes objects); self.table[slot]: the call's rows as IpOutBank.row_table gives
        them; self.computed[slot]: every datagram's UDP checksum as computed"""
        ts = bytes(ts)
        assert len(ts) % TS == 0
        packets = [ts[i:i + TS] for i in range(0, len(ts), TS)]
        ticks = [(self.ticks_q24 + k * self.rate) // D % 2 ** 32 for k in range(len(packets))]
        self.ticks_q24 += len(packets) * self.rate
        self.st['packets'] += len(packets)
        self.st['bad_sync'] += sum(p[0] != 0x47 for p in packets)
        out = []
        for slot, f in enumerate(self.flows):
            self.table[slot], self.computed[slot] = [], []
            if f is None:
                out.append(b'')
                continue
            P, st = f['packets_per_datagram'], self.slot_st[slot]
            # (packet, tick, index in this call or None)
            queue = [(p, t, None) for p, t in self.held[slot]] + [(p, ticks[k], k) for k, p in enumerate(packets) if selects(f, p)]
            st['passed'] += len(queue) - len(self.held[slot])
            keep = 0 if flush else len(queue) % P
            groups = [queue[i:i + P] for i in range(0, len(queue) - keep, P)]
            self.held[slot] = [(p, t) for p, t, _ in queue[len(queue) - keep:]]
            buf = b''
            for g in groups:
                rtp = f['mode'] == RTP_MODE
                seq = (f['seq_base'] + self.made[slot]) % 65536 if rtp else 0
                stamp = (f['timestamp_base'] + g[0][1]) % 2 ** 32 if rtp else 0
                d, computed = build(f, [p for p, _, _ in g], seq, stamp)
                from_call = [k for _, _, k in g if k is not None]
                self.table[slot].append(dict(offset=len(buf), bytes=len(d), rtp_timestamp=stamp, rtp_seq=seq, packets=len(g),
                                             flags=(RTP if rtp else 0) | (SHORT if len(g) < P else 0) | (CARRIED if g[0][2] is None else 0),
                                             first_packet=from_call[0] if from_call else -1, udp_checksum=computed or 0xFFFF))
                self.computed[slot].append(computed)
                self.made[slot] += 1
                st['datagrams'] += 1
                st['short_datagrams'] += len(g) < P
                st['ts_packets'] += len(g)
                buf += d
            st['bytes_delivered'] += len(buf)
            st['held'] = len(self.held[slot])
            out.append(buf)
        return out

    def stats(self, slot=-1):
        """as IpOutBank.stats: a slot's counters (the stream's own 0), or with -1 the stream's own and the sum over the slots"""
        res = dict.fromkeys(STAT_KEYS, 0)
        if slot < 0:
            res.update(self.st)
        for s in (self.slot_st if slot < 0 else [self.slot_st[slot]]):
            for k in SLOT_KEYS:
                res[k] += s[k]
        return res
