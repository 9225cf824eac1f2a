"""The T2-MI bank's CRC takes a lane per piece of a packet (its bytes in one TS payload), 64 pieces a round (csrc/t2mi.hip, phase D).  A
packet whose TS packets carry adaptation fields has many small pieces: packets of 63, 64, 65 and more than 128 pieces, whole and with a
bit error in a piece of the second and of the third round, device against host bank and model."""
import numpy as np
import pytest

import t2mi_cases as K
import t2mi_ref as T
from test_gpu_t2mi import Rig, eng  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def test_packets_of_more_pieces_than_a_wave_has_lanes(pkg, eng):  # noqa: F811
    rng = np.random.default_rng(21)
    z, af = T.Packetiser(K.PID), 172                                 # 11 payload bytes in a TS packet, 10 behind a pointer
    parts, want_pieces = [], [63, 64, 65, 66, 131, 140]
    for k, n in enumerate(want_pieces):
        total = 10 + 11 * (n - 1)                                    # the PUSI packet's 10 bytes, then n - 1 packets filled to the last byte
        parts.append(z.lay([T.bb_packet(k, 3, bytes(rng.integers(0, 256, total - 13, dtype=np.uint8)), frame_idx=k)], af_len=af))
        assert len(parts[-1]) == n
    ts = np.concatenate(parts)
    rig = Rig(pkg, eng, 1, 1024, 64)
    rig.call([ts], shift=1)
    rows = rig.models[0].table(0)
    assert [r['last_packet'] - r['first_packet'] + 1 for r in rows] == want_pieces and all(r['flags'] == T.BBFRAME for r in rows)
    bad = ts.copy()
    at = np.cumsum([0] + want_pieces)
    bad[at[3] + 65, 185] ^= 0x10                                     # the 66th piece of a packet: the second round's second lane
    bad[at[4] + 129, 180] ^= 0x01                                    # the 130th: the third round
    bad[at[5] + 5, 187] ^= 0x80                                      # and one in the first round
    rig = Rig(pkg, eng, 1, 1024, 64)
    rig.call([bad], shift=2)
    assert [r['flags'] for r in rig.models[0].table(0)] == [T.BBFRAME] * 3 + [T.CRC_ERROR] * 3
    rig = Rig(pkg, eng, 1, 1024, 64)
    rig.call([ts[:at[5] + 70]]), rig.call([ts[at[5] + 70:]], shift=3)    # carried in: the buffer is the first piece
    assert rig.models[0].table(0)[0]['first_packet'] == -1 and rig.models[0].table(0)[0]['flags'] == T.BBFRAME
