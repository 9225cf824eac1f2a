"""ctypes helpers for the DVB-S part of the CPU oracle (oracle/dvbs.cpp) + a small DVB-S inner-code transmitter
(convolutional encoder of the oracle, puncturing derived from the oracle's own de-puncturers).  Test infrastructure only."""
import ctypes as C
import numpy as np
from orc import lib, ref

VP = C.c_void_p
RATE_NAMES = ['1/2', '2/3', '3/4', '5/6', '7/8']


def P(a):
    return a.ctypes.data_as(VP)


_bound = False


def L():
    global _bound
    l = lib()
    if not _bound:
        for n in ('orc_dvbs_slicer_create', 'orc_depunc_create', 'orc_ccdec_create', 'orc_ccenc_create', 'orc_vitdvbs_create', 'orc_forney_create'):
            getattr(l, n).restype = VP
        l.orc_vitdvbs_create.argtypes = [C.c_float, C.c_int, C.c_int]
        for n in ('orc_dvbs_slicer_destroy', 'orc_depunc_destroy', 'orc_ccdec_destroy', 'orc_ccenc_destroy', 'orc_vitdvbs_destroy', 'orc_forney_destroy'):
            getattr(l, n).restype = None
            getattr(l, n).argtypes = [VP]
        l.orc_dvbs_slicer_process.argtypes = [VP, C.c_int, VP, VP]
        l.orc_rotate_soft.argtypes = [VP, C.c_int, C.c_int, C.c_int]
        l.orc_signed_to_unsigned.argtypes = [VP, VP, C.c_int]
        l.orc_depuncture_34.argtypes = [VP, VP, C.c_int, C.c_int]
        l.orc_depuncture_78.argtypes = [VP, VP, C.c_int, C.c_int]
        l.orc_depunc_static.argtypes = [VP, VP, VP, C.c_int, C.c_int]
        l.orc_depunc_set_shift.argtypes = [VP, C.c_int]
        l.orc_depunc_cont.argtypes = [VP, VP, VP, C.c_int]
        l.orc_ccdec_work.argtypes = [VP, VP, VP]
        l.orc_ccenc_work.argtypes = [VP, VP, VP]
        l.orc_vitdvbs_work.argtypes = [VP, VP, C.c_int, VP, VP]
        l.orc_forney_deinterleave.argtypes = [VP, VP, VP]
        _bound = True
    return l


def cc_encode(bits):
    """r=1/2 K=7 mother code (X = poly 79, Y = poly 109 in the reference's bit order); returns [2n] bits"""
    l = L()
    bits = np.ascontiguousarray(bits, np.uint8)
    h = VP(l.orc_ccenc_create(len(bits)))
    out = np.zeros(2 * len(bits), np.uint8)
    l.orc_ccenc_work(h, P(bits), P(out))
    l.orc_ccenc_destroy(h)
    return out


def puncture_keep_mask(rate, n_tx):
    """mask over mother-code positions that are transmitted for `rate`, derived by de-puncturing n_tx dummy softs with the
    oracle's own de-puncturer at shift 0 (erasures = 128 mark the punctured positions)"""
    l = L()
    x = np.ones(n_tx, np.uint8)
    out = np.full(4 * n_tx + 16, 255, np.uint8)
    if rate == 0:
        return np.ones(n_tx, bool)
    if rate == 1 or rate == 3:
        h = VP(l.orc_depunc_create(3 if rate == 1 else 6))
        n = l.orc_depunc_static(h, P(x), P(out), n_tx, 0)
        l.orc_depunc_destroy(h)
    elif rate == 2:
        n = l.orc_depuncture_34(P(x), P(out), n_tx, 0)
    else:
        n = l.orc_depuncture_78(P(x), P(out), n_tx, 0)
    return out[:n] != 128


def dvbs_tx(rate, n_soft, seed, amp=40.0, sigma=8.0, drop=0, rot90=False):
    """n_soft int8 soft bits of a DVB-S inner-coded random bit stream at puncturing `rate`, with `drop` leading softs
    removed (decoder must find the shift) and optionally rotated so that the decoder needs PHASE_90.  Returns (soft, bits)."""
    rng = np.random.default_rng(seed)
    need = n_soft + drop + 64
    keep = puncture_keep_mask(rate, need)
    nbits = len(keep) // 2 + 8
    bits = rng.integers(0, 2, nbits, dtype=np.uint8)
    mother = cc_encode(bits)[:len(keep)]
    tx = mother[keep][drop:drop + n_soft].astype(np.float64)
    soft = (2 * tx - 1) * amp + rng.normal(0, sigma, n_soft)
    soft = np.clip(np.trunc(soft), -127, 127).astype(np.int8)
    if rot90:
        # the decoder's PHASE_90 maps (a, b) -> (b, -a); pre-rotate with the inverse: (I, Q) -> (-Q, I)
        s2 = soft.reshape(-1, 2)
        soft = np.stack([-s2[:, 1], s2[:, 0]], axis=1).reshape(-1).astype(np.int8)
    return soft, bits


class OracleViterbi:
    def __init__(self, thr=0.15, max_outsync=20):
        self.l = L()
        self.h = VP(self.l.orc_vitdvbs_create(thr, max_outsync, 8192))

    def __del__(self):
        try:
            self.l.orc_vitdvbs_destroy(self.h)
        except Exception:
            pass

    def work(self, soft_blocks, fill=0):
        """soft_blocks int8 [nblocks, 8192] -> bits uint8 [nblocks, 8192] (`fill` where the decoder wrote nothing), nbits [nblocks],
        stats [nblocks, 5] = BER as float bits, state, rate, phase, shift"""
        nb = soft_blocks.shape[0]
        bits = np.zeros((nb, 8192), np.uint8)
        nbits = np.zeros(nb, np.int32)
        stats = np.zeros((nb, 5), np.int32)
        st = np.zeros(4, np.float32)
        for b in range(nb):
            x = np.ascontiguousarray(soft_blocks[b]).copy()
            o = np.full(8192 + 64, fill, np.uint8)
            nbits[b] = self.l.orc_vitdvbs_work(self.h, P(x), 8192, P(o), P(st))
            bits[b] = o[:8192]
            ps = int(st[3])
            stats[b] = [np.float32(st[0]).view(np.int32), int(st[1]), int(st[2]), ps // 16, ps % 16]
        return bits, nbits, stats


def R():
    """the compiled reference (oracle/_ref) with its DVB-S inner-code entry points bound, or None when it is not built"""
    r = ref()
    if r is None or not hasattr(r, 'ref_viterbi_create'):
        return None
    if not getattr(r, '_dvbs_inner_bound', False):
        for n in ('ref_viterbi_create', 'ref_ccdec_create', 'ref_ccenc_create'):
            getattr(r, n).restype = VP
        r.ref_viterbi_create.argtypes = [C.c_float, C.c_int]
        r.ref_ccdec_create.argtypes = r.ref_ccenc_create.argtypes = [C.c_int]
        for n in ('ref_viterbi_destroy', 'ref_ccdec_destroy', 'ref_ccenc_destroy'):
            getattr(r, n).restype = None
            getattr(r, n).argtypes = [VP]
        r.ref_viterbi_work.argtypes = [VP, VP, C.c_int, VP]
        r.ref_viterbi_ber.restype = r.ref_viterbi_d_ber.restype = C.c_float
        for n in ('ref_viterbi_ber', 'ref_viterbi_d_ber', 'ref_viterbi_state', 'ref_viterbi_rate', 'ref_viterbi_getshift', 'ref_viterbi_phase', 'ref_viterbi_shift'):
            getattr(r, n).argtypes = [VP]
        r.ref_ccdec_work.argtypes = r.ref_ccenc_work.argtypes = [VP, VP, VP]
        r.ref_ccdec_work.restype = r.ref_ccenc_work.restype = None
        r._dvbs_inner_bound = True
    return r


class RefViterbi:
    """the reference's Viterbi_DVBS, constructed as the plugin does (8192-soft blocks, phases 0 and 90 degrees)"""

    def __init__(self, thr=0.15, max_outsync=20):
        self.r = R()
        assert self.r.ref_viterbi_buf_size() == 8192
        self.h = VP(self.r.ref_viterbi_create(thr, max_outsync))

    def __del__(self):
        try:
            self.r.ref_viterbi_destroy(self.h)
        except Exception:
            pass

    def work(self, soft_blocks, fill=0):
        """as OracleViterbi.work (rate, phase and shift read 0 until the first lock: see ref_viterbi_create in oracle/ref_shim.cpp)"""
        r, nb = self.r, soft_blocks.shape[0]
        bits = np.zeros((nb, 8192), np.uint8)
        nbits = np.zeros(nb, np.int32)
        stats = np.zeros((nb, 5), np.int32)
        for b in range(nb):
            x = np.ascontiguousarray(soft_blocks[b]).copy()
            o = np.full(8192 + 64, fill, np.uint8)
            nbits[b] = r.ref_viterbi_work(self.h, P(x), 8192, P(o))
            bits[b] = o[:8192]
            # the BER of the stats row is the member d_ber; the public ber() is that member while locked, and in IDLE the smallest
            # BER of the last search (viterbi_all.cpp:278-313), a display value that the oracle and the engine do not offer
            ber = np.float32(r.ref_viterbi_d_ber(self.h)).view(np.int32)
            if r.ref_viterbi_state(self.h) == 1:
                assert np.float32(r.ref_viterbi_ber(self.h)).view(np.int32) == ber
            assert r.ref_viterbi_getshift(self.h) == int(r.ref_viterbi_shift(self.h) != 0)
            stats[b] = [ber, r.ref_viterbi_state(self.h), r.ref_viterbi_rate(self.h), r.ref_viterbi_phase(self.h), r.ref_viterbi_shift(self.h)]
        return bits, nbits, stats


def viterbi_written_bits(bits, nbits, stats):
    """the bits the decoder wrote, block after block: [0, count) of each block, at rate 5/6 [0, 6799) (the reference's main decoder
    of that rate handles 6799 bits and leaves the rest of the count unwritten)"""
    return np.concatenate([bits[b, :min(int(nbits[b]), 6799) if stats[b, 2] == 3 else int(nbits[b])] for b in range(len(nbits))] + [np.zeros(0, np.uint8)])


def viterbi_case_streams(nb):
    """the Viterbi_DVBS test streams, list of (name, soft int8 [nb, 8192]), nb >= 6: five rates x puncturing shifts x 90 degree rotation,
    noise, marginal SNR at 1/2 and 7/8, and lock -> noise -> re-lock at another rate"""
    rng = np.random.default_rng(77)
    cases = []
    for rate in range(5):
        for drop, rot in ((0, False), (1, True), (3, False)):
            if rate in (2, 4):
                drop = 2 * (drop > 0)
            soft, _ = dvbs_tx(rate, nb * 8192, seed=300 + 10 * rate + drop + rot, drop=drop, rot90=rot, sigma=12.0)
            cases.append((f'rate{rate}_d{drop}_r{int(rot)}', soft.reshape(nb, 8192)))
    cases.append(('noise', rng.integers(-70, 71, (nb, 8192)).astype(np.int8)))
    cases.append(('full_range_noise', rng.integers(-128, 128, (nb, 8192)).astype(np.int8)))
    # marginal SNR: BER hovers around the threshold, watchdog counting matters
    soft, _ = dvbs_tx(0, nb * 8192, seed=501, sigma=30.0)
    cases.append(('marginal_12', soft.reshape(nb, 8192)))
    soft, _ = dvbs_tx(4, nb * 8192, seed=502, sigma=17.0)
    cases.append(('marginal_78', soft.reshape(nb, 8192)))
    # signal, then noise, then a different rate: lock -> watchdog -> IDLE -> re-lock
    a, _ = dvbs_tx(1, nb * 8192, seed=503)
    b, _ = dvbs_tx(3, nb * 8192, seed=504, rot90=True)
    x = a.reshape(nb, 8192).copy()
    x[2:5] = rng.integers(-70, 71, (3, 8192))
    x[5:] = b.reshape(nb, 8192)[5:]
    cases.append(('relock', x))
    return cases


# the leading softs to drop from a stream of each rate so that the search ends on each (rate, phase, shift) it can end on: drop -> shift
LOCK_DROPS = {0: {0: 0, 1: 1}, 1: {0: 0, 1: 4, 2: 5}, 2: {0: 0, 2: 1}, 3: {0: 0, 3: 3, 4: 4, 5: 5, 1: 7, 2: 8}, 4: {0: 0, 2: 1, 4: 2, 6: 3}}
VITERBI_LOCK_BLOCKS = 8
VITERBI_LOCK_WATCHDOG = 2          # max_outsync of the decoders these streams are made for
RELOCK_BLOCK = 5                   # the block in which a 'relock' stream locks for the second time


def viterbi_lock_streams():
    """streams for the lock search of Viterbi_DVBS (ST_IDLE: 2 phases x 26 (rate, shift) hypotheses in the order 1/2 x 2, 2/3 x 6, 3/4 x 2,
    5/6 x 12, 7/8 x 4; the LAST one under the threshold wins), for decoders with max_outsync = VITERBI_LOCK_WATCHDOG.
    List of (name, soft int8 [VITERBI_LOCK_BLOCKS, 8192], kind, lock): lock = (rate, phase, shift) the oracle is to end on, None for 'idle'.

      'lock'    one stream per final lock that a coded stream can produce: 34 of the 52 hypotheses.  A sweep over dvbs_tx(rate, drop = 0 .. 27,
                both rotations, sigma 8) on the oracle ends on exactly these and on nothing else; LOCK_DROPS lists the smallest drop for each.
                The other 18 never end a search: rate 2/3 shifts 1, 2, 3 and rate 5/6 shifts 1, 2, 6, 9, 10, 11, each in both phases.  Shifts s
                and s + period stand for the same puncturing phase of the first soft, without and with one erasure in front of it
                (depunc_static, depunc.h:16-38,108-137), so one of the two starts the de-punctured stream on the first half of a mother-code
                pair and the other on the second half.  A stream received at that puncturing phase locks on the pair-aligned one -- 0, 4, 5
                of 2/3 and 0, 3, 4, 5, 7, 8 of 5/6 -- which shadows its twin; six phases of the first soft are all a 5/6 stream can have,
                three all a 2/3 stream can.  Should a sweep ever end on one of the 18, it belongs into LOCK_DROPS and REACHABLE_LOCKS.
      'idle'    coded streams that never lock: rates 3/4 and 7/8 with an odd number of dropped softs (their hypotheses move by whole I/Q
                pairs, viterbi_all.h:92-150): state 0 and count 0 in every block
      'late'    2 blocks of noise, then rate 2/3 / 5/6 at a shift > period - 1: the lock and the de-puncturer's leading erasure come in the middle of a call
      'relock'  signal, 3 blocks of noise (the watchdog gives up in the third), the same rate again at another drop and rotation.  Depunc23/56::set_shift
                resets neither got_extra nor buf (depunc.h), so the continuous de-puncturer starts the second lock with what the noise left in them:
                the counts from RELOCK_BLOCK on differ from those of a fresh decoder fed the same blocks."""
    nb = VITERBI_LOCK_BLOCKS
    rng = np.random.default_rng(78)
    out = []
    for rate, drops in LOCK_DROPS.items():
        for rot in (False, True):
            for drop, shift in drops.items():
                soft, _ = dvbs_tx(rate, nb * 8192, seed=7000 + 100 * rate + 20 * rot + drop, drop=drop, rot90=rot)
                out.append((f'lock_r{rate}_p{int(rot)}_s{shift}', soft.reshape(nb, 8192), 'lock', (rate, int(rot), shift)))
    for rate, drop, rot in ((2, 1, False), (2, 3, True), (4, 1, True), (4, 3, False), (4, 5, False), (4, 7, True)):
        soft, _ = dvbs_tx(rate, nb * 8192, seed=7600 + 10 * rate + drop, drop=drop, rot90=rot)
        out.append((f'idle_r{rate}_d{drop}_p{int(rot)}', soft.reshape(nb, 8192), 'idle', None))
    for rate, drop, rot in ((1, 1, True), (1, 2, False), (3, 1, False), (3, 2, True)):
        soft, _ = dvbs_tx(rate, (nb - 2) * 8192, seed=7700 + 10 * rate + drop, drop=drop, rot90=rot)
        x = np.concatenate([rng.integers(-70, 71, (2, 8192)).astype(np.int8), soft.reshape(nb - 2, 8192)])
        out.append((f'late_r{rate}_p{int(rot)}_s{LOCK_DROPS[rate][drop]}', x, 'late', (rate, int(rot), LOCK_DROPS[rate][drop])))
    for rate, (da, db) in ((1, (1, 0)), (3, (3, 5))):
        a, _ = dvbs_tx(rate, 2 * 8192, seed=7800 + rate, drop=da, rot90=False)
        b, _ = dvbs_tx(rate, (nb - RELOCK_BLOCK) * 8192, seed=7810 + rate, drop=db, rot90=True)
        x = np.concatenate([a.reshape(2, 8192), rng.integers(-70, 71, (RELOCK_BLOCK - 2, 8192)).astype(np.int8), b.reshape(-1, 8192)])
        out.append((f'relock_r{rate}_d{da}_d{db}', x, 'relock', (rate, 1, LOCK_DROPS[rate][db])))
    return out


REACHABLE_LOCKS = {(r, p, s) for r, shifts in ((0, (0, 1)), (1, (0, 4, 5)), (2, (0, 1)), (3, (0, 3, 4, 5, 7, 8)), (4, (0, 1, 2, 3))) for p in (0, 1) for s in shifts}


def check_viterbi_lock_streams(streams, results):
    """the preconditions of viterbi_lock_streams() on the oracle's (or the reference's) own results [(bits, counts, stats)] -- what makes the
    streams worth comparing: the 34 final locks, the streams that stay IDLE, the late locks, and the stale de-puncturer state after a re-lock"""
    locks = set()
    for (name, soft, kind, lock), (_, n, st) in zip(streams, results):
        if kind == 'lock':
            assert (st[:, 1] == 1).all() and (n > 0).all(), (name, st[:, 1], n)
            assert tuple(st[-1, 2:5]) == lock and (st[:, 2:5] == st[-1, 2:5]).all(), (name, st[:, 2:5])
            locks.add(tuple(int(v) for v in st[-1, 2:5]))
        elif kind == 'idle':
            assert (st[:, 1] == 0).all() and (n == 0).all(), (name, st[:, 1], n)
        elif kind == 'late':
            assert (st[:2, 1] == 0).all() and (n[:2] == 0).all() and (st[2:, 1] == 1).all() and (n[2:] > 0).all(), (name, st[:, 1], n)
            assert (st[2:, 2:5] == np.asarray(lock)).all() and lock[2] > (2 if lock[0] == 1 else 5), (name, st[:, 2:5])
        else:
            k = RELOCK_BLOCK
            assert list(st[:k, 1]) == [1] * (k - 1) + [0] and st[k, 1] == 1, (name, st[:, 1])               # locked, watchdog, IDLE after block k - 1, locked again in block k
            assert tuple(st[0, 2:5]) != tuple(st[k, 2:5]) and tuple(st[k, 2:5]) == lock and st[0, 2] == lock[0], (name, st[:, 2:5])
            fresh = OracleViterbi(0.15, VITERBI_LOCK_WATCHDOG).work(soft[k:])
            assert tuple(fresh[2][0, 1:5]) == (1,) + lock, (name, fresh[2])
            assert list(n[k:]) != list(fresh[1]), (name, n[k:], fresh[1])                                    # the stale got_extra / buf shows in the counts
    assert locks == REACHABLE_LOCKS and len(locks) == 34, sorted(REACHABLE_LOCKS ^ locks)


CCDEC_FRAMES = [54, 56, 57, 59, 114, 1024, 1366, 1699, 4096, 6799]     # (frame + 6 steps in chunks of 60 = 10 rotations of the state layout: every remainder 0..5, a chunk that is exactly full)


def ccdec_case_softs(frame, S=6, nblk=4):
    """unsigned softs uint8 [S, 2 * frame * nblk + 64] for chained CCDecoder blocks of `frame` bits: five noise levels (one with
    erasures) and pure garbage; consecutive blocks start 2 * frame apart and overlap by the 12-byte tail, like the reference's buffers"""
    rng = np.random.default_rng(frame)
    stride = 2 * frame
    Lb = stride * nblk + 64
    soft = np.zeros((S, Lb), np.uint8)
    for s in range(S):
        bits = rng.integers(0, 2, frame * nblk + 64, dtype=np.uint8)
        enc = cc_encode(bits)[:Lb]
        sigma = [10, 25, 40, 60, 90, 1e-3][s]
        x = np.where(enc > 0, 127 + 35, 127 - 35) + rng.normal(0, sigma, Lb)
        x = np.clip(np.rint(x), 0, 255).astype(np.uint8)
        if s == 4:
            x[rng.random(Lb) < 0.3] = 128   # erasures
        soft[s] = x
    soft[5] = rng.integers(0, 256, Lb, dtype=np.uint8)   # pure garbage: exercises the uint8 wrap-around of the metrics
    return soft


# ------------------------------------------------------------------ DVB-S front end (oracle/dvbs_fe.cpp)
class QpskAltCfg(C.Structure):
    _fields_ = [('symbolrate', C.c_double), ('samplerate', C.c_double), ('rrc_taps', C.c_int), ('rrc_alpha', C.c_float),
                ('agc_rate', C.c_float), ('costas_bw', C.c_float), ('fll_bw', C.c_float), ('omega_gain', C.c_float),
                ('mu_gain', C.c_float), ('omega_rel_limit', C.c_float)]


_fe_bound = False


def LF():
    global _fe_bound
    l = L()
    if not _fe_bound:
        l.orc_qpskalt_default_cfg.argtypes = [C.POINTER(QpskAltCfg)]
        l.orc_qpskalt_default_cfg.restype = None
        l.orc_qpskalt_create.argtypes = [C.POINTER(QpskAltCfg)]
        l.orc_qpskalt_create.restype = VP
        l.orc_qpskalt_destroy.argtypes = [VP]
        l.orc_qpskalt_destroy.restype = None
        l.orc_qpskalt_process.argtypes = [VP, C.c_int, VP, VP]
        l.orc_qpskalt_stage.argtypes = [VP, C.c_int, C.c_int, VP, VP]
        l.orc_qpskalt_state.argtypes = [VP, VP]
        l.orc_qpskalt_state.restype = None
        l.orc_dvbs_modulate.argtypes = [VP, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint64, VP]
        l.orc_dvbs_modulate.restype = None
        _fe_bound = True
    return l


def qpsk_alt_default_cfg(**kw):
    c = QpskAltCfg()
    LF().orc_qpskalt_default_cfg(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def dvbs_tx_bits(rate, n_tx_bits, seed):
    """transmitted (punctured) bit stream of a random message: returns (tx bits uint8 [n_tx_bits], info bits)"""
    rng = np.random.default_rng(seed)
    keep = puncture_keep_mask(rate, n_tx_bits + 64)
    nbits = len(keep) // 2 + 8
    bits = rng.integers(0, 2, nbits, dtype=np.uint8)
    mother = cc_encode(bits)[:len(keep)]
    return np.ascontiguousarray(mother[keep][:n_tx_bits]), bits


def dvbs_iq(rate, nsym, seed, esn0_db=12.0, cfo=0.0, timing=0.0, phase0=0.0):
    """complex64 [2*nsym] at 2 sps of a DVB-S inner-coded QPSK stream (no RS / interleaver: inner code only)"""
    tx, bits = dvbs_tx_bits(rate, 2 * nsym, seed)
    out = np.zeros(2 * nsym, np.complex64)
    LF().orc_dvbs_modulate(P(tx), nsym, esn0_db, cfo, timing, phase0, seed, P(out))
    return out, bits


class OracleQpskAlt:
    def __init__(self, cfg=None):
        self.l = LF()
        self.cfg = cfg or qpsk_alt_default_cfg()
        self.h = VP(self.l.orc_qpskalt_create(C.byref(self.cfg)))

    def __del__(self):
        try:
            self.l.orc_qpskalt_destroy(self.h)
        except Exception:
            pass

    def process(self, iq):
        iq = np.ascontiguousarray(iq, np.complex64)
        # (one symbol per `freq + mu_gain * e` samples, any ratio: a configuration the engine accepts never steps by less than a sample -- csrc/rx_cfg_rules.h)
        out = np.zeros(iq.size + 64, np.complex64)
        n = self.l.orc_qpskalt_process(self.h, iq.size, P(iq), P(out))
        return out[:n]

    def stage(self, which, x):
        x = np.ascontiguousarray(x, np.complex64)
        out = np.zeros(x.size + 64, np.complex64)
        n = self.l.orc_qpskalt_stage(self.h, which, x.size, P(x), P(out))
        return out[:n]

    def state(self):
        s = np.zeros(8, np.float32)
        self.l.orc_qpskalt_state(self.h, P(s))
        return s
