"""Shared by tests/test_s2_tx_cpu.py and tests/test_gpu_s2_tx.py: the code words the oracle transmitter modulates, its symbols buffer, the PLS codes."""
import ctypes as C
import functools

import numpy as np

import orc

RATE_OF_MODCOD = ([None] + list(range(11)) + [4, 5, 6, 8, 9, 10] + [5, 6, 7, 8, 9, 10] + [6, 7, 8, 9, 10])    # modcod -> rate index (EN 302 307-1 table 12)


def pls_code(modcod, short=0, pilots=0):
    return modcod << 2 | (2 if short else 0) | (1 if pilots else 0)


def pls_valid(pls):
    modcod, short = pls >> 2, (pls >> 1) & 1
    return modcod == 0 or (modcod <= 28 and not (short and RATE_OF_MODCOD[modcod] == 10))


VALID_PLS = [p for p in range(128) if pls_valid(p)]
INVALID_PLS = [p for p in range(128) if not pls_valid(p)]


@functools.lru_cache(maxsize=None)
def frame_code(rate, short, frame_seed):
    """(BBFRAME bytes, packed code word N/8 bytes) of the oracle's frame with that seed"""
    bb, bits = orc.encode_frame(rate, short, frame_seed)
    return bb, np.packbits(bits)


def code_words(pls_list, seed):
    """what orc.transmit / orc.transmit_vcm with `seed` modulates in frame f (its BBFRAME is make_bbframe(seed * 1000003 + f)), encoded by the oracle's FEC
    -> (code bytes of all frames one behind the other, [BBFRAME or None per frame])"""
    code, bbs = [], []
    for f, pls in enumerate(pls_list):
        if pls >> 2 == 0:
            bbs.append(None)
            continue
        bb, cw = frame_code(RATE_OF_MODCOD[pls >> 2], (pls >> 1) & 1, seed * 1000003 + f)
        code.append(cw)
        bbs.append(bb)
    return (np.concatenate(code) if code else np.zeros(0, np.uint8)), bbs


def transmit_vcm_symbols(pls_list, nframes, seed=1, timing=0.0):
    """orc.transmit_vcm with the symbols buffer bound (tests/orc.py passes none) -> (iq, symbols)"""
    L = orc._bind_chain()
    t = orc.TxCfg(0, 0, 0, nframes, seed, 200.0, 0.0, timing, 0.0, 0, 0, 0, len(pls_list), (C.c_int * 64)(*pls_list))
    nsym = sum(orc.pls_info(pls_list[f % len(pls_list)])[0] for f in range(nframes))
    iq, syms = np.zeros(2 * nsym, np.complex64), np.zeros(nsym, np.complex64)
    bb = np.zeros(sum(orc.pls_info(pls_list[f % len(pls_list)])[1] for f in range(nframes)) + 8, np.uint8)
    n = L.orc_s2_transmit(C.byref(t), iq.ctypes.data, iq.size, bb.ctypes.data, syms.ctypes.data, syms.size)
    assert n == iq.size
    return iq, syms


def same_bits(a, b):
    """bit-for-bit equality of two complex64 / float32 arrays (a -0.0 is not a 0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
