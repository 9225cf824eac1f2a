"""Python model of the PCR bank's rules (include/dvbs2gpu.h, PCR bank): the sequential definition, packet by packet, in Python's
unbounded integers.  With it a PCR packet builder and a small multiplex builder that stamps PCRs from the packet position at a
chosen rate.  The yardstick of the bank's tests."""
import numpy as np

TS = 188
SLOTS = 16
MOD = (1 << 33) * 300
LATE_TICKS, JUMP_TICKS = 1080000, 2700000
MAX_DN = 32767
DEFAULT_LIMIT_Q6 = 864
FIRST, ANNOUNCED, REPEATED, OK, LATE, JUMP = range(6)
ACCURACY_ERROR, SATURATED = 1, 2
STAT_KEYS = ('pcr_packets', 'first', 'announced', 'repeated', 'jumps', 'late', 'ok', 'malformed', 'accuracy_measured', 'accuracy_errors',
             'sum_ticks', 'sum_packets', 'max_delta_ticks', 'max_abs_accuracy')
MAX_KEYS = ('max_delta_ticks', 'max_abs_accuracy')
ROW_KEYS = ('pid', 'slot', 'kind', 'flags', 'packet', 'pcr', 'delta_ticks', 'delta_packets', 'accuracy')
KIND_KEY = {FIRST: 'first', ANNOUNCED: 'announced', REPEATED: 'repeated', OK: 'ok', LATE: 'late', JUMP: 'jumps'}
U32 = (1 << 32) - 1


class Clock:
    """one stream"""

    def __init__(self, max_rows=1 << 30):
        self.max_rows = max_rows
        self.watch = [-1] * SLOTS
        self.tpp, self.limit = 0, DEFAULT_LIMIT_Q6
        self.reset()

    def reset(self):
        self.slot = [None] * SLOTS                  # None: not seen; else [last_pcr, ref_n]
        self.st = [dict.fromkeys(STAT_KEYS, 0) for _ in range(SLOTS)]
        self.last_n = [-1] * SLOTS
        self.packets = self.unwatched = self.rows_dropped = 0
        self.first_unwatched_pid = -1
        self.table, self.records = [], 0

    def set_watch(self, slot, pid):
        self.watch[slot] = pid
        self.slot[slot], self.st[slot], self.last_n[slot] = None, dict.fromkeys(STAT_KEYS, 0), -1

    def set_rate(self, tpp, limit=DEFAULT_LIMIT_Q6):
        self.tpp, self.limit = tpp, limit

    def _step(self, i, P, n, di):
        """-> (kind, flags, delta_ticks, delta_packets, accuracy)"""
        s, st = self.slot[i], self.st[i]
        if s is None or di:
            self.slot[i] = [P, n]
            return (FIRST if s is None else ANNOUNCED), 0, 0, 0, 0
        if P == s[0]:
            return REPEATED, 0, 0, 0, 0
        dP, dN = (P - s[0]) % MOD, n - s[1]
        self.slot[i] = [P, n]
        if dP > JUMP_TICKS:
            return JUMP, 0, min(dP, U32), min(dN, U32), 0
        kind, flags, acc = (LATE if dP > LATE_TICKS else OK), 0, 0
        if self.tpp:
            acc = max(-(2 ** 31 - 1), min(2 ** 31 - 1, ((dP << 24) - min(dN, MAX_DN) * self.tpp) >> 18))
            flags = (ACCURACY_ERROR if abs(acc) > self.limit else 0) | (SATURATED if dN > MAX_DN else 0)
            st['accuracy_measured'] += 1
            st['accuracy_errors'] += flags & ACCURACY_ERROR
            st['max_abs_accuracy'] = max(st['max_abs_accuracy'], abs(acc))
        st['max_delta_ticks'] = max(st['max_delta_ticks'], dP)
        if not flags & SATURATED:
            st['sum_ticks'] += dP
            st['sum_packets'] += dN
        return kind, flags, dP, min(dN, U32), acc

    def process(self, ts):
        """ts: uint8, whole packets -> the records of the call; self.table: the call's first max_rows rows"""
        ts = np.asarray(ts, np.uint8).reshape(-1, TS)
        self.table, self.records, self.first_unwatched_pid = [], 0, -1
        slots = {p: i for i, p in enumerate(self.watch) if p >= 0}
        for k, pk in enumerate(ts):
            p = bytes(pk[:12])
            pid, afc = (p[1] & 0x1f) << 8 | p[2], (p[3] >> 4) & 3
            if p[0] != 0x47 or p[1] >> 7 or pid == 0x1FFF or not afc & 2 or p[4] < 1 or not p[5] & 0x10:
                continue
            base, ext = p[6] << 25 | p[7] << 17 | p[8] << 9 | p[9] << 1 | p[10] >> 7, (p[10] & 1) << 8 | p[11]
            malformed = p[4] < 7 or p[4] > (182 if afc == 3 else 183) or ext > 299
            if pid not in slots:
                if not malformed:
                    if self.first_unwatched_pid < 0:
                        self.first_unwatched_pid = pid
                    self.unwatched += 1
                continue
            i = slots[pid]
            if malformed:
                self.st[i]['malformed'] += 1
                continue
            P = base * 300 + ext
            kind, flags, dt, dn, acc = self._step(i, P, self.packets + k, p[5] >> 7)
            self.st[i]['pcr_packets'] += 1
            self.st[i][KIND_KEY[kind]] += 1
            self.last_n[i] = self.packets + k
            self.records += 1
            if len(self.table) < self.max_rows:
                self.table.append(dict(pid=pid, slot=i, kind=kind, flags=flags, packet=k, pcr=P, delta_ticks=dt, delta_packets=dn, accuracy=acc))
            else:
                self.rows_dropped += 1
        self.packets += len(ts)
        return self.records

    def stats(self, slot=-1):
        sel = self.st if slot < 0 else [self.st[slot]]
        return {k: int(max(s[k] for s in sel) if k in MAX_KEYS else sum(s[k] for s in sel)) for k in STAT_KEYS}

    def stream_stats(self):
        return dict(packets=self.packets, unwatched_pcr_packets=self.unwatched, rows_dropped=self.rows_dropped, first_unwatched_pid=self.first_unwatched_pid,
                    packets_since_pcr=[self.packets - n if n >= 0 else -1 for n in self.last_n])

    def rate(self, slot=-1):
        st = self.stats(slot)
        return 1504.0 * 27e6 * float(st['sum_packets']) / float(st['sum_ticks']) if st['sum_ticks'] else 0.0


# ------------------------------------------------------------------------------------------------- builders
def pcr_packet(pid, P, cc=0, af_len=7, afc=3, di=0, flag=0x10, tei=0, sync=0x47, ext=None, fill=0xAB):
    """one TS packet with a PCR field: P modulo MOD as base * 300 + ext (ext overrides the extension: a fault); af_len, afc, flag (byte 5
    without DI), tei and sync make the malformed and the look-alike forms.  Bytes behind the PCR are `fill`."""
    base, e = divmod(int(P) % MOD, 300)
    e = e if ext is None else ext
    p = bytearray([sync, tei << 7 | pid >> 8, pid & 255, afc << 4 | cc & 15, af_len, di << 7 | flag,
                   base >> 25 & 255, base >> 17 & 255, base >> 9 & 255, base >> 1 & 255, (base & 1) << 7 | 0x7E | e >> 8, e & 255])
    return np.frombuffer(bytes(p) + bytes([fill]) * (TS - len(p)), np.uint8)


def null_packets(n):
    out = np.full((n, TS), 0xFF, np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = 0x47, 0x1F, 0xFF, 0x10
    return out


def payload_packets(pid, n, rng, cc0=0):
    """n packets of a PID with random payload and no adaptation field"""
    out = rng.integers(0, 256, (n, TS), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = 0x47, pid >> 8, pid & 255
    out[:, 3] = 0x10 | ((cc0 + np.arange(n)) & 15)
    return out


def stamped_mux(rng, n, pids, tpp=1000.0, gap=(7, 40), start=0, jitter=0, other=0x300):
    """n packets: for every PID of `pids` a PCR packet every gap[0]..gap[1] packets (random), stamped start + position * tpp ticks plus
    a random jitter of up to +-jitter ticks; payload packets of PID `other` fill the rest -> [n, 188]"""
    out = payload_packets(other, n, rng)
    taken = set()
    for pid in pids:
        k = int(rng.integers(0, gap[0]))
        while k < n:
            while k in taken:
                k += 1
            if k >= n:
                break
            taken.add(k)
            out[k] = pcr_packet(pid, int(start + k * tpp) + int(rng.integers(-jitter, jitter + 1)), cc=k)
            k += int(rng.integers(gap[0], gap[1] + 1))
    return out
