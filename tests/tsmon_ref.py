"""Python model of the TS monitor's rules (include/dvbs2gpu.h, TS monitor bank): the sequential definition, packet by packet.  With
it a generator of legal multiplexes and fault injectors that say what each fault must cost.  The yardstick of the monitor's tests."""
import numpy as np

TS = 188
NULL_PID = 0x1FFF
FIRST_SEEN, DISCONTINUITY = 1, 2
STAT_KEYS = ('packets', 'null_packets', 'tei_packets', 'sync_byte_errors', 'cc_errors', 'duplicates', 'discontinuities', 'scrambled_packets',
             'passed_packets', 'pids_seen')


class Monitor:
    """one stream"""

    def __init__(self):
        self.state = {}                                            # pid -> [last, dup_used]
        self.st = dict.fromkeys(STAT_KEYS, 0)
        self.table = []
        self.set_filter()

    def set_filter(self, mode=0, pids=(), drop_null=False, drop_tei=False, drop_bad_sync=False):
        self.mode, self.pids, self.drop = mode, set(int(p) for p in pids), (drop_null, drop_tei, drop_bad_sync)

    def process(self, ts):
        """ts: uint8, whole packets -> the passing packets; self.table: the call's rows, as TsMonitorBank.pid_table gives them"""
        ts = np.asarray(ts, np.uint8).reshape(-1, TS)
        rows, keep, st = {}, [], self.st
        for k, p in enumerate(ts):
            st['packets'] += 1
            b = [int(x) for x in p[:6]]
            pid, tsc, afc, cc, pusi = (b[1] & 0x1f) << 8 | b[2], b[3] >> 6, (b[3] >> 4) & 3, b[3] & 15, (b[1] >> 6) & 1
            di = b[5] >> 7 if (afc & 2) and b[4] > 0 else 0
            if b[0] != 0x47:
                st['sync_byte_errors'] += 1
                if not self.drop[2]:
                    keep.append(k)
                continue
            if b[1] >> 7:
                st['tei_packets'] += 1
                if not self.drop[1]:
                    keep.append(k)
                continue
            listed = pid in self.pids
            if not (pid == NULL_PID and self.drop[0]) and (self.mode == 0 or (self.mode == 1) == listed):
                keep.append(k)
            r = rows.setdefault(pid, [pid, 0, 0, 0, 0, 0, 0])       # pid, flags, packets, cc_errors, duplicates, scrambled, pusi
            r[2] += 1
            r[5] += tsc != 0
            r[6] += pusi
            st['scrambled_packets'] += tsc != 0
            if pid == NULL_PID:
                st['null_packets'] += 1
                continue
            s = self.state.get(pid)
            if s is None:
                self.state[pid] = [cc, 0]
                r[1] |= FIRST_SEEN
                st['pids_seen'] += 1
            elif di:
                self.state[pid] = [cc, 0]
                r[1] |= DISCONTINUITY
                st['discontinuities'] += 1
            elif not afc & 1:
                r[3] += cc != s[0]
                st['cc_errors'] += cc != s[0]
                self.state[pid] = [cc, 0]
            elif cc == (s[0] + 1) & 15:
                self.state[pid] = [cc, 0]
            elif cc == s[0] and not s[1]:
                r[4] += 1
                st['duplicates'] += 1
                self.state[pid] = [cc, 1]
            else:
                r[3] += 1
                st['cc_errors'] += 1
                self.state[pid] = [cc, 0]
        st['passed_packets'] += len(keep)
        self.table = [tuple(int(v) for v in rows[p]) for p in sorted(rows)]
        return ts[keep].reshape(-1)

    def stats(self):
        return {k: int(v) for k, v in self.st.items()}


# ------------------------------------------------------------------------------------------------- generator
P, A, D, N = 0, 1, 2, 3          # kinds: payload, adaptation field only, the legal duplicate of the packet before it on its PID, null


def packet(pid, cc, afc=1, rng=None, pusi=0, tsc=0, di=0):
    p = np.full(TS, 0xff, np.uint8) if rng is None else rng.integers(0, 256, TS, dtype=np.uint8)
    p[0], p[1], p[2], p[3] = 0x47, pusi << 6 | pid >> 8, pid & 0xff, tsc << 6 | afc << 4 | cc
    if afc & 2:
        p[4], p[5] = (183 if afc == 2 else 1 + int(p[4]) % 20), di << 7 | (int(p[5]) & 0x40)
    return p


def make_mux(rng, npackets, pids, null_frac=0.15, adapt_frac=0.08, dup_frac=0.05, scr_frac=0.2, pusi_frac=0.1, af_frac=0.2):
    """a legal multiplex of `npackets` packets on `pids` (never 0x1FFF) with null runs -> (ts [n, 188], info); info: pid and kind of
    every packet, and the number of legal duplicates"""
    pids = [int(p) for p in pids]
    cc = {p: int(rng.integers(0, 16)) for p in pids}
    scr = {p: rng.random() < scr_frac for p in pids}
    out, opid, kind = [], [], []
    started = set()
    while len(out) < npackets:
        if rng.random() < null_frac:
            for _ in range(int(rng.integers(1, 5))):
                out.append(packet(NULL_PID, 0)); opid.append(NULL_PID); kind.append(N)
            continue
        p = pids[int(rng.integers(0, len(pids)))]
        if p in started and rng.random() < adapt_frac:
            out.append(packet(p, cc[p], afc=2, rng=rng)); opid.append(p); kind.append(A)
            continue
        cc[p] = (cc[p] + 1) & 15
        started.add(p)
        pk = packet(p, cc[p], afc=3 if rng.random() < af_frac else 1, rng=rng, pusi=int(rng.random() < pusi_frac), tsc=2 if scr[p] else 0)
        out.append(pk); opid.append(p); kind.append(P)
        if rng.random() < dup_frac:
            out.append(pk.copy()); opid.append(p); kind.append(D)
    ts = np.array(out[:npackets], np.uint8).reshape(-1, TS)
    info = dict(pid=np.array(opid[:npackets]), kind=np.array(kind[:npackets]))
    info['duplicates'] = int((info['kind'] == D).sum())
    return ts, info


# ------------------------------------------------------------------------------------------------- fault injectors
def _target(rng, info):
    """a payload packet that is neither the first nor the last of its PID, has no duplicate, and whose successor on the PID is a payload
    packet without a duplicate of its own position: removing it from the chain costs exactly one continuity error"""
    pid, kind = info['pid'], info['kind']
    ok = []
    for k in np.flatnonzero(kind == P):
        same = np.flatnonzero(pid == pid[k])
        i = int(np.searchsorted(same, k))
        if 0 < i < len(same) - 1 and kind[same[i + 1]] == P and kind[same[i - 1]] != D:
            ok.append(int(k))
    return ok[int(rng.integers(0, len(ok)))]


def _without(info, k):
    return dict(info, pid=np.delete(info['pid'], k), kind=np.delete(info['kind'], k))


def drop_packet(rng, ts, info):
    k = _target(rng, info)
    return np.delete(ts, k, axis=0), _without(info, k), dict(packets=-1, cc_errors=1, scrambled_packets=-int(ts[k, 3] >> 6 != 0))


def repeat_twice(rng, ts, info):
    """the packet three times in a row: its first repetition is a duplicate, the second a continuity error"""
    k = _target(rng, info)
    ts = np.insert(ts, [k + 1, k + 1], ts[k], axis=0)
    info = dict(info, pid=np.insert(info['pid'], [k + 1, k + 1], info['pid'][k]), kind=np.insert(info['kind'], [k + 1, k + 1], D))
    return ts, info, dict(packets=2, duplicates=1, cc_errors=1, scrambled_packets=2 * int(ts[k, 3] >> 6 != 0))


def flip_tei(rng, ts, info):
    k = _target(rng, info)
    ts = ts.copy()
    ts[k, 1] |= 0x80
    return ts, info, dict(tei_packets=1, cc_errors=1, scrambled_packets=-int(ts[k, 3] >> 6 != 0))


def break_sync(rng, ts, info):
    k = _target(rng, info)
    ts = ts.copy()
    ts[k, 0] ^= 0x10
    return ts, info, dict(sync_byte_errors=1, cc_errors=1, scrambled_packets=-int(ts[k, 3] >> 6 != 0))


def discontinuity(rng, ts, info):
    """a CC jump announced by the discontinuity indicator: costs no continuity error"""
    k = _target(rng, info)
    ts = ts.copy()
    later = np.flatnonzero(info['pid'] == info['pid'][k])
    later = later[later >= k]
    ts[later, 3] = (ts[later, 3] & 0xf0) | ((ts[later, 3] + 5) & 15)
    ts[k, 3] |= 0x30
    ts[k, 4], ts[k, 5] = 1, 0x80
    return ts, info, dict(discontinuities=1)


INJECTORS = (drop_packet, repeat_twice, flip_tei, break_sync, discontinuity)
