"""sdrpp-dvbs-demodulator_amd -- Python plumbing over libdvbs2gpu.so (C ABI: include/dvbs2gpu.h).

The product is the HIP library; this module only loads it (ctypes), hands it device pointers of torch
tensors and the current HIP stream, and raises if the library or a GPU is missing -- there is no CPU
fallback and nothing here touches oracle/.

Import with  importlib.import_module("sdrpp-dvbs-demodulator_amd")  (the directory name has hyphens),
or use the helper  `from __graft_entry__ import load_package`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DVBS2GPU_LIB: development aid (tools/ab.sh runs the bench against a variant build under /tmp without touching the in-tree library)
LIB_PATH = os.environ.get('DVBS2GPU_LIB') or os.path.join(_HERE, 'libdvbs2gpu.so')

ERR_ARG, ERR_MODCOD, ERR_HIP, ERR_NODEVICE, ERR_CAPACITY = -1, -2, -3, -4, -5
ERR_NAMES = {-1: 'ERR_ARG', -2: 'ERR_MODCOD', -3: 'ERR_HIP', -4: 'ERR_NODEVICE', -5: 'ERR_CAPACITY'}


class Dvbs2GpuError(RuntimeError):
    def __init__(self, code, text):
        super().__init__('dvbs2gpu %s (%d): %s' % (ERR_NAMES.get(code, '?'), code, text))
        self.code = code


class ModcodInfo(C.Structure):
    _fields_ = [('constellation', C.c_int32), ('bits_per_symbol', C.c_int32), ('rate', C.c_int32), ('slots', C.c_int32),
                ('pilot_blocks', C.c_int32), ('plframe_symbols', C.c_int32), ('ldpc_n', C.c_int32), ('ldpc_k', C.c_int32),
                ('kbch', C.c_int32), ('bch_t', C.c_int32), ('ldpc_edges', C.c_int32), ('g1', C.c_float), ('g2', C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DemodCfg(C.Structure):
    """dvbs2gpu_demod_cfg"""
    _fields_ = [('symbolrate', C.c_double), ('samplerate', C.c_double), ('agc_rate', C.c_float), ('rrc_alpha', C.c_float),
                ('rrc_taps', C.c_int32), ('loop_bw', C.c_float), ('fll_bw', C.c_float), ('clock_omega_gain', C.c_float),
                ('clock_mu_gain', C.c_float), ('omega_rel_limit', C.c_float), ('modcod', C.c_int32), ('shortframes', C.c_int32),
                ('pilots', C.c_int32), ('sof_threshold', C.c_float), ('max_ldpc_trials', C.c_int32), ('force_ldpc_iters', C.c_int32),
                ('acm_vcm', C.c_int32), ('soft_plsc', C.c_int32), ('pilot_aided', C.c_int32)]


STAGE_NAMES = ('frontend', 'rrc', 'plsync', 'loops', 'demap', 'ldpc', 'bch', 'deliver')


class StageTimes(C.Structure):
    """dvbs2gpu_stage_times"""
    _fields_ = [('ms', C.c_double * 8), ('launches', C.c_int64 * 8), ('units', C.c_int64 * 8)]


class FrameStats(C.Structure):
    """dvbs2gpu_frame_stats"""
    _fields_ = [('pl_sync_best_match', C.c_float), ('detected_modcod', C.c_int32), ('detected_shortframes', C.c_int32),
                ('detected_pilots', C.c_int32), ('coarse_freq_err', C.c_float), ('ldpc_trials', C.c_int32), ('bch_corrections', C.c_int32),
                ('bbframe_bytes', C.c_int32)]


class BbtsMaCfg(C.Structure):
    """dvbs2gpu_bbts_ma_cfg"""
    _fields_ = [('issy_bytes', C.c_int32), ('crc_span', C.c_int32), ('reinsert_nulls', C.c_int32), ('check_crc', C.c_int32)]


class BbtsMaStats(C.Structure):
    """dvbs2gpu_bbts_ma_stats"""
    _fields_ = [('packets', C.c_int64), ('nulls', C.c_int64), ('ts_errs', C.c_int64), ('broken_joins', C.c_int32), ('undecided', C.c_int32),
                ('frames', C.c_int32), ('skipped_frames', C.c_int32), ('rejected_frames', C.c_int32), ('issy_bytes', C.c_int32),
                ('iscr_valid', C.c_int32), ('last_iscr', C.c_uint32), ('carried', C.c_int32), ('selected', C.c_int32), ('isi', C.c_int32),
                ('hem_frames', C.c_int32)]


class GseStats(C.Structure):
    """dvbs2gpu_gse_stats"""
    _fields_ = [(k, C.c_int64) for k in ('frames', 'packets', 'complete_pdus', 'reassembled_pdus', 'crc_failures', 'dropped_no_slot', 'dropped_overflow',
                                         'dropped_no_fit', 'bytes_delivered', 'host_fallback_calls', 'fallback_records', 'fallback_capacity')]


class BbtsMaGseStats(C.Structure):
    """dvbs2gpu_bbts_ma_gse_stats"""
    _fields_ = [(k, C.c_int64) for k in ('frames', 'packets', 'complete_pdus', 'reassembled_pdus', 'crc_failures', 'dropped_no_slot', 'dropped_overflow',
                                         'dropped_no_fit', 'bytes_delivered', 'malformed_frames', 'host_fallback_calls')] + \
               [('open_slots', C.c_int32), ('last_crc_err', C.c_int32)]


class GsePdu(C.Structure):
    """dvbs2gpu_gse_pdu"""
    _fields_ = [('offset', C.c_uint32), ('bytes', C.c_uint32), ('protocol', C.c_uint16), ('flags', C.c_uint16), ('reserved', C.c_uint32)]


class TsMonFilter(C.Structure):
    """dvbs2gpu_tsmon_filter"""
    _fields_ = [('mode', C.c_int32), ('drop_null', C.c_int32), ('drop_tei', C.c_int32), ('drop_bad_sync', C.c_int32)]


class TsMonStats(C.Structure):
    """dvbs2gpu_tsmon_stats"""
    _fields_ = [(k, C.c_int64) for k in ('packets', 'null_packets', 'tei_packets', 'sync_byte_errors', 'cc_errors', 'duplicates', 'discontinuities',
                                         'scrambled_packets', 'passed_packets', 'pids_seen')]


class TsMonPid(C.Structure):
    """dvbs2gpu_tsmon_pid"""
    _fields_ = [('pid', C.c_uint16), ('flags', C.c_uint16), ('packets', C.c_uint32), ('cc_errors', C.c_uint32), ('duplicates', C.c_uint32),
                ('scrambled', C.c_uint32), ('pusi', C.c_uint32)]


class PsiLayout(C.Structure):
    """dvbs2gpu_psi_layout"""
    _fields_ = [(k, C.c_int32) for k in ('header_bytes', 'length_mask', 'max_section_length', 'max_section_bytes', 'min_long_section', 'ext_at',
                                         'version_at', 'section_number_at', 'last_section_number_at', 'long_header_bytes', 'crc_bytes', 'pat_loop_at',
                                         'pat_stride', 'pmt_pcr_at', 'pmt_info_length_at', 'pmt_loop_at', 'pmt_stride')]


class PsiStats(C.Structure):
    """dvbs2gpu_psi_stats"""
    _fields_ = [(k, C.c_int64) for k in ('packets', 'sections', 'valid', 'changed', 'crc_errors', 'dropped_sections', 'malformed_sections',
                                         'malformed_packets', 'scrambled_packets', 'unexpected_table_id', 'bytes_delivered')]


class PsiSection(C.Structure):
    """dvbs2gpu_psi_section"""
    _fields_ = [('pid', C.c_uint16), ('flags', C.c_uint16), ('table_id', C.c_uint8), ('ssi', C.c_uint8), ('version', C.c_uint8), ('current_next', C.c_uint8),
                ('section_number', C.c_uint8), ('last_section_number', C.c_uint8), ('table_id_ext', C.c_uint16), ('length', C.c_int32),
                ('offset', C.c_int32), ('first_packet', C.c_int32)]


class PsiProgram(C.Structure):
    """dvbs2gpu_psi_program"""
    _fields_ = [('program_number', C.c_uint16), ('pid', C.c_uint16)]


class PsiPat(C.Structure):
    """dvbs2gpu_psi_pat"""
    _fields_ = [('transport_stream_id', C.c_int32), ('version', C.c_int32), ('malformed', C.c_int32)]


class PsiEs(C.Structure):
    """dvbs2gpu_psi_es"""
    _fields_ = [('stream_type', C.c_uint16), ('elementary_pid', C.c_uint16)]


class PsiPmt(C.Structure):
    """dvbs2gpu_psi_pmt"""
    _fields_ = [('program_number', C.c_int32), ('version', C.c_int32), ('pcr_pid', C.c_int32), ('malformed', C.c_int32)]


class PcrStats(C.Structure):
    """dvbs2gpu_pcr_stats"""
    _fields_ = [(k, C.c_int64) for k in ('pcr_packets', 'first', 'announced', 'repeated', 'jumps', 'late', 'ok', 'malformed', 'accuracy_measured',
                                         'accuracy_errors', 'sum_ticks', 'sum_packets', 'max_delta_ticks', 'max_abs_accuracy')]


class PcrStreamStats(C.Structure):
    """dvbs2gpu_pcr_stream_stats"""
    _fields_ = [('packets', C.c_int64), ('unwatched_pcr_packets', C.c_int64), ('rows_dropped', C.c_int64), ('first_unwatched_pid', C.c_int32),
                ('reserved', C.c_int32), ('packets_since_pcr', C.c_int64 * 16)]


class PcrRow(C.Structure):
    """dvbs2gpu_pcr_row"""
    _pack_ = 4
    _fields_ = [('pid', C.c_uint16), ('slot', C.c_uint8), ('kind', C.c_uint8), ('flags', C.c_uint16), ('reserved', C.c_uint16), ('packet', C.c_int32),
                ('pcr', C.c_uint64), ('delta_ticks', C.c_uint32), ('delta_packets', C.c_uint32), ('accuracy', C.c_int32)]


class PesStats(C.Structure):
    """dvbs2gpu_pes_stats"""
    _fields_ = [(k, C.c_int64) for k in ('packets', 'payload_bytes', 'duplicates', 'cc_errors', 'scrambled_packets', 'malformed_packets', 'starts',
                                         'starts_scrambled', 'starts_short', 'starts_bad_start', 'starts_plain', 'starts_malformed', 'starts_header',
                                         'with_pts', 'with_dts', 'closed_ok', 'closed_mismatch', 'closed_gap', 'closed_unchecked', 'ts_backward', 'ts_gap',
                                         'pts_late', 'dts_after_pts', 'max_delta_packets')]


class PesStreamStats(C.Structure):
    """dvbs2gpu_pes_stream_stats"""
    _fields_ = [('packets', C.c_int64), ('rows_dropped', C.c_int64), ('packets_since_start', C.c_int64 * 16)]


class PesRow(C.Structure):
    """dvbs2gpu_pes_row"""
    _pack_ = 4
    _fields_ = [('pid', C.c_uint16), ('slot', C.c_uint8), ('kind', C.c_uint8), ('flags', C.c_uint16), ('stream_id', C.c_uint8), ('reserved', C.c_uint8),
                ('packet', C.c_int32), ('declared', C.c_uint32), ('pts', C.c_uint64), ('dts', C.c_uint64), ('closed_bytes', C.c_uint32),
                ('closed_packets', C.c_uint32), ('delta_packets', C.c_uint32), ('delta_ts', C.c_int32)]


class EsStats(C.Structure):
    """dvbs2gpu_es_stats"""
    _fields_ = [(k, C.c_int64) for k in ('packets', 'payload_bytes', 'es_bytes', 'bytes_unsynced', 'duplicates', 'cc_errors', 'scrambled_packets',
                                         'malformed_packets', 'resets', 'pes_starts', 'pes_invalid', 'split_headers', 'codes', 'pictures', 'pictures_i',
                                         'pictures_p', 'pictures_b', 'key_pictures', 'sequences', 'gops', 'params', 'auds', 'ends', 'slices', 'other_codes',
                                         'bad_codes')]


class EsStreamStats(C.Structure):
    """dvbs2gpu_es_stream_stats"""
    _fields_ = [('packets', C.c_int64), ('rows_dropped', C.c_int64)]


class EsRow(C.Structure):
    """dvbs2gpu_es_row"""
    _pack_ = 4
    _fields_ = [('pid', C.c_uint16), ('slot', C.c_uint8), ('unit', C.c_uint8), ('code', C.c_uint8), ('detail', C.c_uint8), ('flags', C.c_uint16),
                ('packet', C.c_int32), ('head', C.c_uint32), ('es_offset', C.c_uint64), ('pts', C.c_uint64), ('dts', C.c_uint64), ('reserved', C.c_uint64)]


class AudStats(C.Structure):
    """dvbs2gpu_aud_stats"""
    _fields_ = [(k, C.c_int64) for k in ('packets', 'payload_bytes', 'es_bytes', 'bytes_unsynced', 'duplicates', 'cc_errors', 'scrambled_packets',
                                         'malformed_packets', 'resets', 'pes_starts', 'pes_invalid', 'split_headers', 'frames', 'frame_bytes_total',
                                         'samples_total', 'acquisitions', 'sync_losses', 'param_changes', 'unaligned_starts', 'bytes_unlocked')]


class AudStreamStats(C.Structure):
    """dvbs2gpu_aud_stream_stats"""
    _fields_ = [('packets', C.c_int64), ('rows_dropped', C.c_int64)]


class AudRow(C.Structure):
    """dvbs2gpu_aud_row"""
    _pack_ = 4
    _fields_ = [('pid', C.c_uint16), ('slot', C.c_uint8), ('unit', C.c_uint8), ('code', C.c_uint8), ('detail', C.c_uint8), ('flags', C.c_uint16),
                ('packet', C.c_uint16), ('kbps', C.c_uint16), ('head', C.c_uint32), ('es_offset', C.c_uint64), ('pts', C.c_uint64), ('dts', C.c_uint64),
                ('sample_rate', C.c_uint32), ('frame_bytes', C.c_uint16), ('samples', C.c_uint16)]


class T2miLayout(C.Structure):
    """dvbs2gpu_t2mi_layout"""
    _fields_ = [(k, C.c_int32) for k in ('header_bytes', 'crc_bytes', 'min_packet_bytes', 'max_packet_bytes', 'bbframe_type', 'bbframe_prefix_bytes',
                                         'min_bbframe_bytes', 'max_bbframe_bytes', 'stream_id_mask')]


class T2miStats(C.Structure):
    """dvbs2gpu_t2mi_stats"""
    _fields_ = [(k, C.c_int64) for k in ('packets', 't2mi_packets', 'crc_errors', 'count_errors', 'bbframes', 'bad_payload', 'bbframes_delivered',
                                         'bytes_delivered', 'dropped_packets', 'malformed_packets', 'scrambled_packets', 'pointer_slack')]


class T2miRow(C.Structure):
    """dvbs2gpu_t2mi_row"""
    _fields_ = [('packet_type', C.c_uint8), ('packet_count', C.c_uint8), ('superframe_idx', C.c_uint8), ('stream_id', C.c_uint8), ('flags', C.c_uint16),
                ('plp_id', C.c_uint8), ('frame_idx', C.c_uint8), ('payload_bits', C.c_uint32), ('length', C.c_int32), ('offset', C.c_int32),
                ('bbframe_bytes', C.c_int32), ('first_packet', C.c_int32), ('last_packet', C.c_int32)]


class MpeLayout(C.Structure):
    """dvbs2gpu_mpe_layout"""
    _fields_ = ([(k, C.c_int32) for k in ('header_bytes', 'length_mask', 'max_section_length', 'max_section_bytes', 'table_id', 'mpe_header_bytes', 'crc_bytes',
                                          'min_section_bytes')] + [('mac_at', C.c_int32 * 6)] +
                [(k, C.c_int32) for k in ('flags_at', 'section_number_at', 'last_section_number_at', 'llc_snap_bytes', 'ethertype_at', 'ethertype_ipv4',
                                          'ethertype_ipv6', 'ipv4_min_header', 'ipv4_total_length_at', 'ipv4_fragment_at', 'ipv4_protocol_at', 'ipv4_src_at',
                                          'ipv4_dst_at', 'ipv6_header', 'ipv6_payload_length_at', 'ipv6_next_header_at', 'head_bytes')])


class MpeStats(C.Structure):
    """dvbs2gpu_mpe_stats"""
    _fields_ = [(k, C.c_int64) for k in ('packets', 'sections', 'other_table', 'crc_errors', 'unchecked', 'scrambled_sections', 'filtered', 'fragments',
                                         'other_protocol', 'bad_ip', 'datagrams', 'datagrams_delivered', 'bytes_delivered', 'dropped_sections',
                                         'malformed_sections', 'malformed_packets', 'scrambled_packets')]


class MpeRow(C.Structure):
    """dvbs2gpu_mpe_row"""
    _fields_ = [('flags', C.c_uint16), ('family', C.c_uint8), ('protocol', C.c_uint8), ('mac', C.c_uint8 * 6), ('section_number', C.c_uint8),
                ('last_section_number', C.c_uint8), ('src_port', C.c_uint16), ('dst_port', C.c_uint16), ('src4', C.c_uint32), ('dst4', C.c_uint32),
                ('length', C.c_int32), ('offset', C.c_int32), ('bytes', C.c_int32), ('first_packet', C.c_int32), ('last_packet', C.c_int32),
                ('ethertype', C.c_uint16), ('stuffing', C.c_uint16)]


class UleLayout(C.Structure):
    """dvbs2gpu_ule_layout"""
    _fields_ = [(k, C.c_int32) for k in ('header_bytes', 'length_bytes', 'd_bit', 'length_mask', 'max_length', 'max_sndu_bytes', 'type_at', 'npa_bytes', 'crc_bytes',
                                         'min_length_d1', 'min_length_d0', 'type_test', 'type_bridged', 'type_ts_concat', 'type_priv_concat', 'ethertype_floor',
                                         'hlen_shift', 'hlen_mask', 'max_hlen', 'max_extension_bytes', 'mac_header_bytes', 'bridged_ethertype_at', 'ethertype_ipv4',
                                         'ethertype_ipv6', 'ipv4_min_header', 'ipv4_total_length_at', 'ipv4_fragment_at', 'ipv4_protocol_at', 'ipv4_src_at',
                                         'ipv4_dst_at', 'ipv6_header', 'ipv6_payload_length_at', 'ipv6_next_header_at', 'head_bytes')]


class UleStats(C.Structure):
    """dvbs2gpu_ule_stats"""
    _fields_ = [(k, C.c_int64) for k in ('packets', 'sndus', 'crc_errors', 'filtered', 'no_address', 'test', 'bridged', 'extension', 'other_protocol', 'bad_ip',
                                         'datagrams', 'datagrams_delivered', 'bytes_delivered', 'dropped_sndus', 'malformed_sndus', 'slack', 'malformed_packets',
                                         'scrambled_packets')]


class UleRow(C.Structure):
    """dvbs2gpu_ule_row"""
    _fields_ = [('flags', C.c_uint16), ('family', C.c_uint8), ('protocol', C.c_uint8), ('mac', C.c_uint8 * 6), ('ip_at', C.c_uint8), ('extension_bytes', C.c_uint8),
                ('src_port', C.c_uint16), ('dst_port', C.c_uint16), ('src4', C.c_uint32), ('dst4', C.c_uint32), ('length', C.c_int32), ('offset', C.c_int32),
                ('bytes', C.c_int32), ('first_packet', C.c_int32), ('last_packet', C.c_int32), ('ethertype', C.c_uint16), ('stuffing', C.c_uint16)]


class IptsView(C.Structure):
    """dvbs2gpu_ipts_view"""
    _fields_ = [('bytes', C.c_void_p), ('rows', C.c_void_p), ('stride', C.c_int32), ('offset_at', C.c_int32), ('bytes_at', C.c_int32), ('kind', C.c_int32),
                ('n', C.c_int32), ('reserved', C.c_int32)]


class IptsLayout(C.Structure):
    """dvbs2gpu_ipts_layout"""
    _fields_ = [(k, C.c_int32) for k in ('gre_header_bytes', 'ipv4_src_at', 'ipv6_src_at', 'ipv6_dst_at', 'ipv4_more_fragments', 'udp_protocol', 'udp_header_bytes',
                                         'udp_length_at', 'udp_checksum_at', 'ts_packet_bytes', 'ts_sync', 'rtp_min_header', 'rtp_version', 'rtp_payload_type_mp2t',
                                         'rtp_seq_at', 'rtp_timestamp_at', 'rtp_ssrc_at', 'late_from', 'head_bytes', 'slots', 'row_bytes', 'view_bytes')]


class IptsStats(C.Structure):
    """dvbs2gpu_ipts_stats"""
    _fields_ = [(k, C.c_int64) for k in ('rows', 'not_delivered', 'not_ip', 'bad_ip', 'fragments', 'other_protocol', 'bad_udp', 'unwatched', 'matched', 'bad_checksum',
                                         'no_checksum', 'bad_payload', 'other_payload', 'raw', 'rtp', 'new_source', 'loss_events', 'late', 'ts', 'ts_packets',
                                         'bytes_delivered', 'lost')]


class IptsRow(C.Structure):
    """dvbs2gpu_ipts_row"""
    _fields_ = [('flags', C.c_uint32), ('slot', C.c_int8), ('family', C.c_uint8), ('payload_type', C.c_uint8), ('reserved', C.c_uint8), ('src_port', C.c_uint16),
                ('dst_port', C.c_uint16), ('rtp_seq', C.c_uint16), ('ts_at', C.c_uint16), ('rtp_timestamp', C.c_uint32), ('rtp_ssrc', C.c_uint32),
                ('packets', C.c_int32), ('lost', C.c_int32), ('offset', C.c_int32), ('bytes', C.c_int32)]


class IpoutFlow(C.Structure):
    """dvbs2gpu_ipout_flow"""
    _fields_ = [('family', C.c_int32), ('src_addr', C.c_uint8 * 16), ('dst_addr', C.c_uint8 * 16), ('src_port', C.c_uint16), ('dst_port', C.c_uint16),
                ('ttl', C.c_uint8), ('dscp', C.c_uint8), ('mode', C.c_uint8), ('packets_per_datagram', C.c_uint8), ('ssrc', C.c_uint32),
                ('timestamp_base', C.c_uint32), ('seq_base', C.c_uint16), ('pid_mode', C.c_uint8), ('drop_null', C.c_uint8)]


class IpoutLayout(C.Structure):
    """dvbs2gpu_ipout_layout"""
    _fields_ = [(k, C.c_int32) for k in ('ipv4_version_ihl', 'ipv4_tos_at', 'ipv4_id_at', 'ipv4_dont_fragment', 'ipv4_ttl_at', 'ipv4_checksum_at', 'ipv6_hop_limit_at',
                                         'rtp_first_byte', 'tick_divisor', 'max_packets_per_datagram', 'held_packets', 'pid_map_bytes', 'slots', 'row_bytes',
                                         'flow_bytes')]


class IpoutStats(C.Structure):
    """dvbs2gpu_ipout_stats"""
    _fields_ = [(k, C.c_int64) for k in ('packets', 'bad_sync', 'passed', 'datagrams', 'short_datagrams', 'ts_packets', 'bytes_delivered', 'held')]


class IpoutRow(C.Structure):
    """dvbs2gpu_ipout_row"""
    _fields_ = [('offset', C.c_int32), ('bytes', C.c_int32), ('rtp_timestamp', C.c_uint32), ('rtp_seq', C.c_uint16), ('packets', C.c_uint8), ('flags', C.c_uint8),
                ('first_packet', C.c_int32), ('udp_checksum', C.c_uint16), ('reserved', C.c_uint16)]


class FrameQuality(C.Structure):
    """dvbs2gpu_frame_quality"""
    _fields_ = [('esn0_db', C.c_float), ('mer_db', C.c_float), ('gain', C.c_float), ('phase', C.c_float), ('known_symbols', C.c_int32),
                ('payload_symbols', C.c_int32)]


class DvbsQuality(C.Structure):
    """dvbs2gpu_dvbs_quality"""
    _fields_ = [('esn0_db', C.c_float), ('mer_db', C.c_float), ('amplitude', C.c_float), ('symbols', C.c_int32)]


def _quality_dtype(st):
    """numpy structured dtype with the fields of a ctypes record"""
    import numpy as np
    return np.dtype([(k, np.float32 if t is C.c_float else np.int32) for k, t in st._fields_])


# name -> (restype, argtypes); every symbol declared in include/dvbs2gpu.h
_vp = C.c_void_p
_i = C.c_int
PROTOTYPES = {
    'dvbs2gpu_version': (C.c_char_p, []),
    'dvbs2gpu_last_error': (C.c_char_p, []),
    'dvbs2gpu_create': (_i, [_i, C.POINTER(_vp)]),
    'dvbs2gpu_destroy': (None, [_vp]),
    'dvbs2gpu_modcod_info_get': (_i, [_i, _i, _i, C.POINTER(ModcodInfo)]),
    'dvbs2gpu_fec_info_get': (_i, [_i, _i, C.POINTER(ModcodInfo)]),
    'dvbs2gpu_set_option': (_i, [_vp, C.c_char_p, _i]),
    'dvbs2gpu_preinit': (_i, []),
    'dvbs2gpu_device_count': (_i, []),
    'dvbs2gpu_fleet_plan': (_i, [C.POINTER(C.c_int32), C.POINTER(C.c_double), _i, _i, C.c_double, C.POINTER(C.c_int32)]),
    'dvbs2gpu_fleet_create': (_i, [C.POINTER(_i), _i, C.POINTER(_vp)]),
    'dvbs2gpu_fleet_destroy': (None, [_vp]),
    'dvbs2gpu_fleet_size': (_i, [_vp]),
    'dvbs2gpu_fleet_assign': (_i, [_vp, _vp, _i, _i, C.c_double, C.POINTER(C.c_int32)]),
    'dvbs2gpu_fleet_set_pipelined': (_i, [_vp, _i]),
    'dvbs2gpu_fleet_reset': (_i, [_vp]),
    'dvbs2gpu_fleet_process_batch': (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, C.POINTER(_i)]),
    'dvbs2gpu_fleet_get_stats': (_i, [_vp, _i, C.POINTER(FrameStats), _i]),
    'dvbs2gpu_get_state': (_i, [_vp, C.c_char_p, C.POINTER(C.c_longlong)]),
    'dvbs2gpu_debug_last_fec_job': (_i, [_vp, _i, C.POINTER(C.c_longlong), C.POINTER(C.c_int32), C.POINTER(_vp), _i]),
    'dvbs2gpu_ldpc_plan_dump': (_i, [_i, _i, _vp, _vp, _vp, C.POINTER(C.c_int32)]),
    'dvbs2gpu_ldpc_plan_info': (_i, [_vp, _i, _i, C.POINTER(C.c_int32)]),
    'dvbs2gpu_ldpc_decoder_form': (_i, [_vp, _i, _i]),
    'dvbs2gpu_ldpc_wave_plan_dump': (_i, [_i, _i, _vp, _vp, _vp, C.POINTER(C.c_int32)]),
    'dvbs2gpu_ldpc_addr_table_dump': (_i, [_i, _i, _vp, C.POINTER(C.c_int32)]),
    'dvbs2gpu_ldpc_split_plan_dump': (_i, [_i, _i, _vp, _vp, _vp, _vp, C.POINTER(C.c_int32)]),
    'dvbs2gpu_ldpc_decode_batch': (_i, [_vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    'dvbs2gpu_bch_decode_batch': (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    'dvbs2gpu_bb_descramble_batch': (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    'dvbs2gpu_fec_decode_batch': (_i, [_vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    'dvbs2gpu_bb_scramble_batch': (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    'dvbs2gpu_bch_encode_batch': (_i, [_vp, _i, _i, _vp, _i, _vp]),
    'dvbs2gpu_ldpc_encode_batch': (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    'dvbs2gpu_fec_encode_batch': (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _i, _vp]),
    'dvbs2gpu_fec_channel_ber_batch': (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    'dvbs2gpu_fec_encode_plan_dump': (_i, [_i, _i, _vp, C.POINTER(C.c_int32)]),
    'dvbs2gpu_s2_tx_sizes': (_i, [_vp, _i, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    'dvbs2gpu_pl_frame_batch': (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    'dvbs2gpu_pulse_shape_batch': (_i, [_vp, _vp, _i, C.c_longlong, C.c_double, C.c_double, _i, _vp, _vp]),
    'dvbs2gpu_channel_batch': (_i, [_vp, _vp, _i, C.c_longlong, _vp, _vp, _vp, _vp, _vp]),
    'dvbs2gpu_s2_modulate_batch': (_i, [_vp, _vp, _i, _vp, _i, C.c_double, C.c_double, _i, _vp, _vp, _vp]),
    'dvbs2gpu_s2_tx_host': (_i, [_vp, _i, _vp, C.c_double, C.c_double, _i, _vp, C.c_longlong, _vp, _vp]),
    'dvbs2gpu_pulse_shape_host': (_i, [_vp, C.c_longlong, C.c_double, C.c_double, _i, _vp]),
    'dvbs2gpu_channel_host': (_i, [_vp, C.c_longlong, _vp, C.c_longlong]),
    'dvbs2gpu_demap_batch': (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    'dvbs2gpu_deinterleave_batch': (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    'dvbs2gpu_set_stage_timing': (_i, [_vp, _i]),
    'dvbs2gpu_get_stage_times': (_i, [_vp, _vp]),
    'dvbs2gpu_pl_tables_dump': (_i, [_vp, _vp, _vp, _vp]),
    'dvbs2gpu_math_eval': (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'dvbs2gpu_demod_default_cfg': (None, [_i, _i, _i, C.POINTER(DemodCfg)]),
    'dvbs2gpu_demod_create': (_i, [_vp, C.POINTER(DemodCfg), _i, C.POINTER(_vp)]),
    'dvbs2gpu_demod_destroy': (None, [_vp]),
    'dvbs2gpu_demod_reset': (_i, [_vp]),
    'dvbs2gpu_demod_set_params': (_i, [_vp, _i, _i, _i, C.c_float, _i]),
    'dvbs2gpu_demod_get_kbch': (_i, [_vp]),
    'dvbs2gpu_demod_process': (_i, [_vp, _i, _vp, _vp, _i]),
    'dvbs2gpu_demod_process_batch': (_i, [C.POINTER(_vp), _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, C.POINTER(_i)]),
    'dvbs2gpu_set_pipelined': (_i, [_vp, _i]),
    'dvbs2gpu_demod_get_stats': (_i, [_vp, C.POINTER(FrameStats), _i]),
    'dvbs2gpu_demod_get_nco_freq': (C.c_float, [_vp]),
    'dvbs2gpu_demod_get_tap': (_i, [_vp, _i, _vp, _i]),
    'dvbs2gpu_demod_set_quality': (_i, [_vp, _i]),
    'dvbs2gpu_demod_get_quality': (_i, [_vp, C.POINTER(FrameQuality), _i]),
    # DVB-S inner code
    'dvbs2gpu_dvbs_slice': (_i, [_vp, _vp, _i, _vp, _vp]),
    'dvbs2gpu_ccdec_create': (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_ccdec_destroy': (None, [_vp]),
    'dvbs2gpu_ccdec_work_batch': (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, _vp]),
    'dvbs2gpu_viterbi_create': (_i, [_vp, _i, C.c_float, _i, C.POINTER(_vp)]),
    'dvbs2gpu_viterbi_reset': (_i, [_vp]),
    'dvbs2gpu_viterbi_destroy': (None, [_vp]),
    'dvbs2gpu_viterbi_work_batch': (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    'dvbs2gpu_forney_create': (_i, [_vp, _i, C.POINTER(_vp)]),
    'dvbs2gpu_forney_destroy': (None, [_vp]),
    'dvbs2gpu_forney_deinterleave_batch': (_i, [_vp, _vp, _i, _vp, _vp]),
    'dvbs2gpu_dvbs_demod_default_cfg': (None, [_vp]),
    'dvbs2gpu_dvbs_demod_create': (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_dvbs_demod_reset': (_i, [_vp]),
    'dvbs2gpu_dvbs_demod_destroy': (None, [_vp]),
    'dvbs2gpu_dvbs_demod_process': (_i, [_vp, _i, _vp, _vp, _i]),
    'dvbs2gpu_dvbs_demod_process_batch': (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, C.POINTER(_i)]),
    'dvbs2gpu_dvbs_demod_get_stats': (_i, [_vp, _vp]),
    'dvbs2gpu_dvbs_demod_get_tap': (_i, [_vp, _i, _i, _vp, _i]),
    'dvbs2gpu_dvbs_demod_set_quality': (_i, [_vp, _i]),
    'dvbs2gpu_dvbs_demod_get_quality': (_i, [_vp, C.POINTER(DvbsQuality)]),
    'dvbs2gpu_dvbs_tail_create': (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_dvbs_tail_reset': (_i, [_vp]),
    'dvbs2gpu_dvbs_tail_destroy': (None, [_vp]),
    'dvbs2gpu_dvbs_tail_process_batch': (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, C.POINTER(_i), _vp]),
    'dvbs2gpu_dvbs_tail_get_stats': (_i, [_vp, _i, C.POINTER(C.c_int32)]),
    'dvbs2gpu_dvbs_tail_get_dropped': (_i, [_vp, _i, C.POINTER(C.c_int32)]),
    'dvbs2gpu_dvbs_tail_get_tap': (_i, [_vp, _i, _i, _vp, _i]),
    'dvbs2gpu_dvbs_tail_rs_stage': (_i, [_vp, _vp, _i, _i, _vp, _i]),
    'dvbs2gpu_dvbs_depuncture': (_i, [_vp, _i, _i, _vp, _i, _vp, _i, C.POINTER(C.c_int32)]),
    'dvbs2gpu_demod_get_frame_positions': (_i, [_vp, C.POINTER(C.c_int64), _i]),
    'dvbs2gpu_segrx_create': (_i, [_vp, C.POINTER(DemodCfg), _i, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_segrx_reset': (_i, [_vp]),
    'dvbs2gpu_segrx_destroy': (None, [_vp]),
    'dvbs2gpu_segrx_chunk_samples': (C.c_longlong, [_vp]),
    'dvbs2gpu_segrx_process': (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong]),
    'dvbs2gpu_segrx_get_stats': (_i, [_vp, C.POINTER(C.c_int32)]),
    'dvbs2gpu_dvbs_segrx_create': (_i, [_vp, _vp, _i, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_dvbs_segrx_reset': (_i, [_vp]),
    'dvbs2gpu_dvbs_segrx_destroy': (None, [_vp]),
    'dvbs2gpu_dvbs_segrx_chunk_samples': (C.c_longlong, [_vp]),
    'dvbs2gpu_dvbs_segrx_process': (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong]),
    'dvbs2gpu_dvbs_segrx_get_stats': (_i, [_vp, C.POINTER(C.c_int32)]),
    'dvbs2gpu_dvbs_process_ts': (_i, [_vp, _vp, _i, _vp, _vp, _i]),
    'dvbs2gpu_dvbs_segrx_find_join': (C.c_longlong, [_vp, C.c_longlong, _vp, C.c_longlong, C.POINTER(C.c_int)]),
    'dvbs2gpu_bbts_create': (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_bbts_set_frame_size': (_i, [_vp, _i]),
    'dvbs2gpu_bbts_destroy': (None, [_vp]),
    'dvbs2gpu_bbts_process_batch': (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, C.POINTER(_i), _vp]),
    'dvbs2gpu_bbts_work': (_i, [_vp, _vp, _i, _vp, _i]),
    'dvbs2gpu_bbts_get_stats': (_i, [_vp, _i, C.POINTER(C.c_int32), _i]),
    'dvbs2gpu_bbts_set_gse_path': (_i, [_vp, _i]),
    'dvbs2gpu_bbts_get_gse_stats': (_i, [_vp, _i, C.POINTER(GseStats)]),
    'dvbs2gpu_bbts_get_pdu_table': (_i, [_vp, _i, C.POINTER(GsePdu), _i, C.POINTER(_i)]),
    'dvbs2gpu_bbts_get_pdu_table_device': (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i)]),
    'dvbs2gpu_crc32_mpeg_shift': (C.c_uint32, [C.c_uint32, C.c_uint32]),
    'dvbs2gpu_bbts_ma_default_cfg': (None, [C.POINTER(BbtsMaCfg)]),
    'dvbs2gpu_bbts_ma_get_layout': (_i, [C.POINTER(C.c_int32)]),
    'dvbs2gpu_bbts_create_host': (_i, [_i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_bbts_set_mode_adaptation': (_i, [_vp, C.POINTER(BbtsMaCfg)]),
    'dvbs2gpu_bbts_select_isi': (_i, [_vp, _i, C.POINTER(C.c_uint8), _i]),
    'dvbs2gpu_bbts_process_ma_batch': (_i, [_vp, C.POINTER(_vp), C.POINTER(C.POINTER(_i)), C.POINTER(_i), C.POINTER(_vp), _i, C.POINTER(_i),
                                            C.POINTER(_i), _vp]),
    'dvbs2gpu_bbts_ma_work': (_i, [_vp, _vp, C.POINTER(_i), _i, C.POINTER(_vp), _i, C.POINTER(_i), C.POINTER(_i)]),
    'dvbs2gpu_bbts_ma_flush': (_i, [_vp, C.POINTER(_vp), _i, C.POINTER(_i)]),
    'dvbs2gpu_bbts_ma_flush_host': (_i, [_vp, C.POINTER(_vp), _i, C.POINTER(_i)]),
    'dvbs2gpu_bbts_ma_get_stats': (_i, [_vp, _i, _i, C.POINTER(BbtsMaStats)]),
    'dvbs2gpu_bbts_get_isi_seen': (_i, [_vp, _i, C.POINTER(C.c_uint32)]),
    'dvbs2gpu_bbts_ma_set_gse': (_i, [_vp, _i]),
    'dvbs2gpu_bbts_ma_set_t2_hem': (_i, [_vp, _i]),
    'dvbs2gpu_bbts_ma_get_hem_layout': (_i, [C.POINTER(C.c_int32)]),
    'dvbs2gpu_bbts_ma_get_gse_stats': (_i, [_vp, _i, _i, C.POINTER(BbtsMaGseStats)]),
    'dvbs2gpu_bbts_ma_get_pdu_table': (_i, [_vp, _i, _i, C.POINTER(GsePdu), _i, C.POINTER(_i)]),
    'dvbs2gpu_bbts_ma_get_pdu_table_device': (_i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_i)]),
    'dvbs2gpu_tsmon_create': (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_tsmon_create_host': (_i, [_i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_tsmon_reset': (_i, [_vp]),
    'dvbs2gpu_tsmon_destroy': (None, [_vp]),
    'dvbs2gpu_tsmon_set_filter': (_i, [_vp, _i, C.POINTER(TsMonFilter), C.POINTER(C.c_uint16), _i]),
    'dvbs2gpu_tsmon_process_batch': (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, C.POINTER(_i), _vp]),
    'dvbs2gpu_tsmon_work': (_i, [_vp, _i, _vp, _i, _vp, _i]),
    'dvbs2gpu_tsmon_get_stats': (_i, [_vp, _i, C.POINTER(TsMonStats)]),
    'dvbs2gpu_tsmon_get_pid_table': (_i, [_vp, _i, C.POINTER(TsMonPid), _i, C.POINTER(_i)]),
    'dvbs2gpu_tsmon_get_pid_table_device': (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i)]),
    'dvbs2gpu_psi_create': (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_psi_create_host': (_i, [_i, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_psi_reset': (_i, [_vp]),
    'dvbs2gpu_psi_destroy': (None, [_vp]),
    'dvbs2gpu_psi_get_layout': (_i, [C.POINTER(PsiLayout)]),
    'dvbs2gpu_psi_set_watch': (_i, [_vp, _i, _i, _i, _i]),
    'dvbs2gpu_psi_set_deliver': (_i, [_vp, _i, _i]),
    'dvbs2gpu_psi_process_batch': (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    'dvbs2gpu_psi_work': (_i, [_vp, _i, _vp, _i, _vp, _i]),
    'dvbs2gpu_psi_get_needed': (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i)]),
    'dvbs2gpu_psi_get_stats': (_i, [_vp, _i, _i, C.POINTER(PsiStats)]),
    'dvbs2gpu_psi_get_section_table': (_i, [_vp, _i, C.POINTER(PsiSection), _i, C.POINTER(_i)]),
    'dvbs2gpu_psi_get_section_table_device': (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i)]),
    'dvbs2gpu_psi_get_programs': (_i, [_vp, _i, C.POINTER(PsiPat), C.POINTER(PsiProgram), _i, C.POINTER(_i)]),
    'dvbs2gpu_psi_get_program_map': (_i, [_vp, _i, _i, C.POINTER(PsiPmt), C.POINTER(PsiEs), _i, C.POINTER(_i)]),
}
# the four watched-PID banks (csrc/watch_bank.h): the same functions but for the prefix, the structures, what set_watch takes behind the
# PID and the rate functions
for _p, _St, _SSt, _Row, _watch, _own in (
        ('pcr', PcrStats, PcrStreamStats, PcrRow, [], {'set_rate': (_i, [_vp, _i, C.c_uint64, _i]), 'get_rate': (_i, [_vp, _i, _i, C.POINTER(C.c_double)])}),
        ('pes', PesStats, PesStreamStats, PesRow, [], {'set_rate': (_i, [_vp, _i, C.c_uint64])}),
        ('es', EsStats, EsStreamStats, EsRow, [_i], {}),
        ('aud', AudStats, AudStreamStats, AudRow, [_i], {})):
    PROTOTYPES.update({'dvbs2gpu_%s_%s' % (_p, _k): _v for _k, _v in {
        'create': (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
        'create_host': (_i, [_i, _i, _i, C.POINTER(_vp)]),
        'reset': (_i, [_vp]),
        'destroy': (None, [_vp]),
        'set_watch': (_i, [_vp, _i, _i, _i] + _watch),
        'process_batch': (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), _vp]),
        'work': (_i, [_vp, _i, _vp, _i]),
        'get_stats': (_i, [_vp, _i, _i, C.POINTER(_St)]),
        'get_stream_stats': (_i, [_vp, _i, C.POINTER(_SSt)]),
        'get_row_table': (_i, [_vp, _i, C.POINTER(_Row), _i, C.POINTER(_i)]),
        'get_row_table_device': (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i)]),
        **_own,
    }.items()})
PROTOTYPES.update({
    'dvbs2gpu_t2mi_create': (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_t2mi_create_host': (_i, [_i, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_t2mi_reset': (_i, [_vp]),
    'dvbs2gpu_t2mi_destroy': (None, [_vp]),
    'dvbs2gpu_t2mi_get_layout': (_i, [C.POINTER(T2miLayout)]),
    'dvbs2gpu_t2mi_set_watch': (_i, [_vp, _i, _i, _i, _i]),
    'dvbs2gpu_t2mi_process_batch': (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    'dvbs2gpu_t2mi_work': (_i, [_vp, _i, _i, _vp, _i, _vp, _i]),
    'dvbs2gpu_t2mi_get_needed': (_i, [_vp, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    'dvbs2gpu_t2mi_get_stats': (_i, [_vp, _i, _i, C.POINTER(T2miStats)]),
    'dvbs2gpu_t2mi_get_row_table': (_i, [_vp, _i, _i, C.POINTER(T2miRow), _i, C.POINTER(_i)]),
    'dvbs2gpu_t2mi_get_row_table_device': (_i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_i)]),
    'dvbs2gpu_t2mi_get_frame_bytes': (_i, [_vp, _i, _i, C.POINTER(_i), _i, C.POINTER(_i)]),
})
# the two datagram banks (csrc/dgram_bank.h): the same functions but for the prefix, the structures and what set_watch takes behind the mask
for _p, _Lay, _St, _Row, _watch in (('mpe', MpeLayout, MpeStats, MpeRow, []), ('ule', UleLayout, UleStats, UleRow, [_i])):
    PROTOTYPES.update({'dvbs2gpu_%s_%s' % (_p, _k): _v for _k, _v in {
        'create': (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
        'create_host': (_i, [_i, _i, _i, C.POINTER(_vp)]),
        'reset': (_i, [_vp]),
        'destroy': (None, [_vp]),
        'get_layout': (_i, [C.POINTER(_Lay)]),
        'set_watch': (_i, [_vp, _i, _i, _i, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)] + _watch),
        'process_batch': (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, C.POINTER(_i), C.POINTER(_i), _vp]),
        'work': (_i, [_vp, _i, _i, _vp, _i, _vp, _i]),
        'get_needed': (_i, [_vp, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
        'get_stats': (_i, [_vp, _i, _i, C.POINTER(_St)]),
        'get_row_table': (_i, [_vp, _i, _i, C.POINTER(_Row), _i, C.POINTER(_i)]),
        'get_row_table_device': (_i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_i)]),
    }.items()})
PROTOTYPES.update({
    'dvbs2gpu_ipts_create': (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_ipts_create_host': (_i, [_i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_ipts_reset': (_i, [_vp]),
    'dvbs2gpu_ipts_destroy': (None, [_vp]),
    'dvbs2gpu_ipts_get_layout': (_i, [C.POINTER(IptsLayout)]),
    'dvbs2gpu_ipts_set_flow': (_i, [_vp, _i, _i, _i, C.POINTER(C.c_uint8), _i]),
    'dvbs2gpu_ipts_process_batch': (_i, [_vp, C.POINTER(IptsView), C.POINTER(_vp), _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    'dvbs2gpu_ipts_work': (_i, [_vp, _i, C.POINTER(IptsView), C.POINTER(_vp), _i, C.POINTER(_i)]),
    'dvbs2gpu_ipts_get_needed': (_i, [_vp, _i, _i, C.POINTER(_i)]),
    'dvbs2gpu_ipts_get_stats': (_i, [_vp, _i, _i, C.POINTER(IptsStats)]),
    'dvbs2gpu_ipts_get_row_table': (_i, [_vp, _i, C.POINTER(IptsRow), _i, C.POINTER(_i)]),
    'dvbs2gpu_ipts_get_row_table_device': (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i)]),
    'dvbs2gpu_ipout_create': (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_ipout_create_host': (_i, [_i, _i, C.POINTER(_vp)]),
    'dvbs2gpu_ipout_reset': (_i, [_vp]),
    'dvbs2gpu_ipout_destroy': (None, [_vp]),
    'dvbs2gpu_ipout_get_layout': (_i, [C.POINTER(IpoutLayout)]),
    'dvbs2gpu_ipout_set_flow': (_i, [_vp, _i, _i, C.POINTER(IpoutFlow), C.POINTER(C.c_uint16), _i]),
    'dvbs2gpu_ipout_set_rate': (_i, [_vp, _i, C.c_uint64]),
    'dvbs2gpu_ipout_process_batch': (_i, [_vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, C.POINTER(_i), C.POINTER(_i), _i, _vp]),
    'dvbs2gpu_ipout_work': (_i, [_vp, _i, _vp, _i, C.POINTER(_vp), _i, C.POINTER(_i), _i]),
    'dvbs2gpu_ipout_get_needed': (_i, [_vp, _i, _i, C.POINTER(_i)]),
    'dvbs2gpu_ipout_get_stats': (_i, [_vp, _i, _i, C.POINTER(IpoutStats)]),
    'dvbs2gpu_ipout_get_row_table': (_i, [_vp, _i, _i, C.POINTER(IpoutRow), _i, C.POINTER(_i)]),
    'dvbs2gpu_ipout_get_row_table_device': (_i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_i)]),
})

_lib = None


def load_library():
    """dlopen libdvbs2gpu.so (built in-tree by __graft_entry__.build()).  Fails loudly if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError('%s not found: run `python -c "import __graft_entry__ as g; g.build()"` '
                              '(hipcc --offload-arch=gfx950); there is no CPU fallback' % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def modcod_info(modcod, shortframes=False, pilots=False):
    info = ModcodInfo()
    rc = load_library().dvbs2gpu_modcod_info_get(int(modcod), int(bool(shortframes)), int(bool(pilots)), C.byref(info))
    if rc != 0:
        raise Dvbs2GpuError(rc, load_library().dvbs2gpu_last_error().decode())
    return info.as_dict()


def pl_tables():
    """Host-only: the physical-layer tables a receiver uploads -> (sof complex64 [26], plsc symbols complex64 [128, 64], codewords uint64 [128], Rn uint8 [131072])"""
    import numpy as np
    sof, sym = np.zeros(26, np.complex64), np.zeros((128, 64), np.complex64)
    codes, rn = np.zeros(128, np.uint64), np.zeros(131072, np.uint8)
    rc = load_library().dvbs2gpu_pl_tables_dump(sof.ctypes.data, sym.ctypes.data, codes.ctypes.data, rn.ctypes.data)
    if rc != 0:
        raise Dvbs2GpuError(rc, load_library().dvbs2gpu_last_error().decode())
    return sof, sym, codes, rn


def fec_info(rate, shortframes=False):
    info = ModcodInfo()
    rc = load_library().dvbs2gpu_fec_info_get(int(rate), int(bool(shortframes)), C.byref(info))
    if rc != 0:
        raise Dvbs2GpuError(rc, load_library().dvbs2gpu_last_error().decode())
    return info.as_dict()


def ldpc_split_plan(rate, shortframes=False):
    """Host-only: the half-row LDPC decoder's plan (csrc/ldpc_split_plan.h) as numpy arrays; None for codes that decoder does not take."""
    import numpy as np
    lib = load_library()
    cnt = (C.c_int32 * 6)()
    rc = lib.dvbs2gpu_ldpc_split_plan_dump(int(rate), int(bool(shortframes)), None, None, None, None, cnt)
    if rc != 0:
        raise Dvbs2GpuError(rc, lib.dvbs2gpu_last_error().decode())
    npl, npw, hs, rec_total, nwords, rec_dw = list(cnt)
    if npl == 0:
        return None
    layers = np.zeros((npl, 4), np.uint32); table = np.zeros(nwords, np.uint32)
    row_of = np.zeros((npl, 384), np.int32); layer_of = np.zeros(npl, np.int32)
    rc = lib.dvbs2gpu_ldpc_split_plan_dump(int(rate), int(bool(shortframes)), layers.ctypes.data, table.ctypes.data, row_of.ctypes.data, layer_of.ctypes.data, cnt)
    if rc != 0:
        raise Dvbs2GpuError(rc, lib.dvbs2gpu_last_error().decode())
    return {'npl': npl, 'npw': npw, 'hs': hs, 'rec_total': rec_total, 'rec_dwords': rec_dw, 'kind': (layers[:, 0] & 0xff).astype(int), 'nw': ((layers[:, 0] >> 8) & 0xff).astype(int),
            'nc': ((layers[:, 0] >> 16) & 15).astype(int), 'noprev': ((layers[:, 0] >> 20) & 1).astype(int), 'aux': layers[:, 1].astype(int), 'rec_off': layers[:, 2].astype(int),
            'ent_off': layers[:, 3].astype(int), 'table': table[:npl * 768 * npw].reshape(npl, 768, npw), 'words': table, 'row_of': row_of, 'layer': layer_of}


def fec_encode_plan(rate, shortframes=False):
    """Host-only: the FEC encoder's rules for one code (csrc/fec_encode_rules.h) -> dict: 'generator' the BCH generator polynomial as uint8 coefficients, x^0
    first; 'parity_bits', 'bch_chunks', 'chunk_bytes', 'bch_frames_per_workgroup', 'ldpc_frames_per_workgroup', 'layers', 'links', 'max_workgroups',
    'ber_chunk_frames'; 'seams': the frame bits at which a chunk of the BCH kernel begins inside the message"""
    import numpy as np
    lib = load_library()
    cnt = (C.c_int32 * 80)()
    rc = lib.dvbs2gpu_fec_encode_plan_dump(int(rate), int(bool(shortframes)), None, cnt)
    if rc != 0:
        raise Dvbs2GpuError(rc, lib.dvbs2gpu_last_error().decode())
    gen = np.zeros(cnt[0] + 1, np.uint8)
    rc = lib.dvbs2gpu_fec_encode_plan_dump(int(rate), int(bool(shortframes)), gen.ctypes.data, cnt)
    if rc != 0:
        raise Dvbs2GpuError(rc, lib.dvbs2gpu_last_error().decode())
    keys = ['parity_bits', 'bch_chunks', 'chunk_bytes', 'bch_frames_per_workgroup', 'ldpc_frames_per_workgroup', 'layers', 'links', 'max_workgroups', 'ber_chunk_frames']
    d = dict(zip(keys, list(cnt)[:9]))
    d['generator'] = gen
    d['seams'] = [int(x) for x in list(cnt)[16:16 + cnt[9]]]
    return d


class TxChannel(C.Structure):
    """dvbs2gpu_tx_channel: pointers to the channel's host arrays"""
    _fields_ = [('esn0_db', _vp), ('cfo', _vp), ('phase0', _vp), ('seed', _vp)]


def _tx_channel(esn0_db, cfo, phase0, seed, nstreams):
    """-> (TxChannel, the numpy arrays it points to); scalars are repeated for every stream"""
    import numpy as np
    arrs = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (nstreams,))) for v, dt in
            ((esn0_db, np.float64), (cfo, np.float64), (phase0, np.float64), (seed, np.uint64))]
    return TxChannel(*[a.ctypes.data for a in arrs]), arrs


def _pls_array(pls):
    import numpy as np
    return np.ascontiguousarray(np.asarray(pls, np.int32).reshape(-1))


def s2_tx_sizes(pls):
    """Host-only: the sizes of one stream's block for a PLS list (pls = modcod << 2 | short << 1 | pilots, modcod 0 = dummy PLFRAME)
    -> dict 'symbols', 'bbframe_bytes', 'code_bytes'"""
    lib = load_library()
    a = _pls_array(pls)
    o = [C.c_longlong() for _ in range(3)]
    rc = lib.dvbs2gpu_s2_tx_sizes(a.ctypes.data, a.size, C.byref(o[0]), C.byref(o[1]), C.byref(o[2]))
    if rc != 0:
        raise Dvbs2GpuError(rc, lib.dvbs2gpu_last_error().decode())
    return {'symbols': int(o[0].value), 'bbframe_bytes': int(o[1].value), 'code_bytes': int(o[2].value)}


def s2_tx_host(pls, code, rolloff=0.35, timing=0.0, circular=False, esn0_db=None, cfo=0.0, phase0=0.0, seed=0, stream=0, want_iq=True):
    """Host-only: the modulator's rules (csrc/s2_tx_rules.h) on the CPU for one stream.  code: uint8, the frames' code words one behind the other.
    -> (symbols complex64 [symbols], iq complex64 [2 * symbols] or None); the channel is applied when esn0_db is given"""
    import numpy as np
    lib = load_library()
    a = _pls_array(pls)
    sz = s2_tx_sizes(a)
    code = np.ascontiguousarray(np.asarray(code, np.uint8).reshape(-1))
    assert code.size == sz['code_bytes'], (code.size, sz['code_bytes'])
    sym = np.zeros(sz['symbols'], np.complex64)
    iq = np.zeros(2 * sz['symbols'], np.complex64) if want_iq else None
    ch, keep = (None, None) if esn0_db is None else _tx_channel(esn0_db, cfo, phase0, seed, 1)
    rc = lib.dvbs2gpu_s2_tx_host(a.ctypes.data, a.size, code.ctypes.data if code.size else None, float(rolloff), float(timing), int(bool(circular)),
                                 C.addressof(ch) if ch is not None else None, int(stream), sym.ctypes.data, iq.ctypes.data if want_iq else None)
    if rc != 0:
        raise Dvbs2GpuError(rc, lib.dvbs2gpu_last_error().decode())
    return sym, iq


def pulse_shape_host(symbols, rolloff=0.35, timing=0.0, circular=False):
    """Host-only: the shaping stage of s2_tx_host for any block of symbols, complex64 [n] -> iq complex64 [2 n]"""
    import numpy as np
    lib = load_library()
    symbols = np.ascontiguousarray(np.asarray(symbols, np.complex64).reshape(-1))
    iq = np.zeros(2 * symbols.size, np.complex64)
    rc = lib.dvbs2gpu_pulse_shape_host(symbols.ctypes.data, symbols.size, float(rolloff), float(timing), int(bool(circular)), iq.ctypes.data)
    if rc != 0:
        raise Dvbs2GpuError(rc, lib.dvbs2gpu_last_error().decode())
    return iq


def channel_host(iq, esn0_db=200.0, cfo=0.0, phase0=0.0, seed=0, stream=0):
    """Host-only: the channel stage of s2_tx_host for any block, complex64 [n] -> a changed copy; `stream` is the stream's index in a device call"""
    import numpy as np
    lib = load_library()
    out = np.array(np.asarray(iq, np.complex64).reshape(-1), copy=True, order='C')
    ch, keep = _tx_channel(esn0_db, cfo, phase0, seed, 1)
    rc = lib.dvbs2gpu_channel_host(out.ctypes.data, out.size, C.addressof(ch), int(stream))
    if rc != 0:
        raise Dvbs2GpuError(rc, lib.dvbs2gpu_last_error().decode())
    return out


class FleetEntry(C.Structure):
    """dvbs2gpu_fleet_entry"""
    _fields_ = [('cfg', DemodCfg), ('weight', C.c_double), ('max_samples', C.c_int32), ('reserved', C.c_int32)]


def fleet_plan(modcods, weights, world, tolerance=0.25):
    """Host-only: the fleet's placement rule (dvbs2gpu_fleet_plan) -> member index of every transponder"""
    lib = load_library()
    n = len(modcods)
    m = (C.c_int32 * max(n, 1))(*[int(x) for x in modcods])
    w = (C.c_double * max(n, 1))(*[float(x) for x in weights])
    out = (C.c_int32 * max(n, 1))()
    rc = lib.dvbs2gpu_fleet_plan(m, w, n, int(world), float(tolerance), out)
    if rc != 0:
        raise Dvbs2GpuError(rc, lib.dvbs2gpu_last_error().decode())
    return [int(out[i]) for i in range(n)]


class Fleet:
    """dvbs2gpu_fleet_*: a transponder table over several (logical) devices behind the C ABI; host buffers in, BBFRAMEs out in table order"""

    def __init__(self, devices):
        self.lib = load_library()
        h = _vp()
        d = (_i * len(devices))(*[int(x) for x in devices])
        rc = self.lib.dvbs2gpu_fleet_create(d, len(devices), C.byref(h))
        if rc != 0:
            raise Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
        self.h, self.nt, self.cap = h, 0, 0

    def _check(self, rc):
        if rc < 0:
            raise Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
        return rc

    def assign(self, cfgs, max_samples, out_cap, weights=None, tolerance=0.25):
        """cfgs: one DemodCfg per transponder -> member index of every transponder"""
        n = len(cfgs)
        tab = (FleetEntry * max(n, 1))()
        for i, c in enumerate(cfgs):
            tab[i].cfg = c
            tab[i].weight = float(weights[i]) if weights is not None else 0.0
            tab[i].max_samples = int(max_samples)
        out = (C.c_int32 * max(n, 1))()
        self._check(self.lib.dvbs2gpu_fleet_assign(self.h, C.cast(tab, _vp), n, int(out_cap), float(tolerance), out))
        self.nt, self.cap = n, int(out_cap)
        return [int(out[i]) for i in range(n)]

    def set_pipelined(self, on):
        self._check(self.lib.dvbs2gpu_fleet_set_pipelined(self.h, int(bool(on))))

    def process(self, iqs):
        """iqs: one numpy complex64 array per transponder (may be empty) -> list of numpy uint8 arrays (BBFRAME bytes, table order)"""
        import numpy as np
        iqs = [np.ascontiguousarray(x, np.complex64) for x in iqs]
        outs = [np.zeros(self.cap, np.uint8) for _ in range(self.nt)]
        pin = (_vp * self.nt)(*[x.ctypes.data for x in iqs])
        cnt = (_i * self.nt)(*[int(x.size) for x in iqs])
        pout = (_vp * self.nt)(*[o.ctypes.data for o in outs])
        nb = (_i * self.nt)()
        self._check(self.lib.dvbs2gpu_fleet_process_batch(self.h, pin, cnt, pout, self.cap, nb))
        return [outs[i][:nb[i]] for i in range(self.nt)]

    def close(self):
        if getattr(self, 'h', None):
            self.lib.dvbs2gpu_fleet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Engine:
    """One engine context on one GPU.  All tensor arguments are torch CUDA tensors on that GPU."""

    def __init__(self, device=0, options=None):
        """options: development / test options of the context, {name: int} (dvbs2gpu_set_option)"""
        import torch
        self.torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise Dvbs2GpuError(-4, 'no GPU visible to torch; the engine has no CPU fallback')
        self.device = torch.device('cuda', device)
        h = C.c_void_p()
        self._check(self.lib.dvbs2gpu_create(int(device), C.byref(h)))
        self.h = h
        for name, value in (options or {}).items():
            self.set_option(name, value)

    def set_option(self, name, value):
        self._check(self.lib.dvbs2gpu_set_option(self.h, str(name).encode(), int(value)))

    def get_state(self, name):
        """read-only introspection (dvbs2gpu_get_state): 'kernel_launches', 'g_prio_duty', 'stage_pipeline_on', 'pipelined', ..."""
        v = C.c_longlong()
        self._check(self.lib.dvbs2gpu_get_state(self.h, str(name).encode(), C.byref(v)))
        return int(v.value)

    def last_fec_job(self, slot=0):
        """the pipelined CCM decoder job group `slot` delivered last (dvbs2gpu_debug_last_fec_job): dict with the device pointers of its LLRs / BBFRAMEs, the
        frame count, N, kb, the code, and `first` (first pooled frame of every stream of the job) + `handles` (the streams' demod handles)"""
        import numpy as np
        o = (C.c_longlong * 10)()
        self._check(self.lib.dvbs2gpu_debug_last_fec_job(self.h, int(slot), o, None, None, 0))
        n = int(o[3])
        first = (C.c_int32 * (n + 1))()
        hs = (_vp * max(n, 1))()
        self._check(self.lib.dvbs2gpu_debug_last_fec_job(self.h, int(slot), o, first, hs, n + 1))
        return dict(d_llr=int(o[0]), d_bb=int(o[1]), nf=int(o[2]), n=n, N=int(o[4]), kb=int(o[5]), rate=int(o[6]), short=int(o[7]), max_trials=int(o[8]), force=int(o[9]),
                    first=np.array(first[:n + 1], dtype=np.int64), handles=[hs[i] for i in range(n)])

    def close(self):
        if getattr(self, 'h', None):
            self.lib.dvbs2gpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
        return rc

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def ldpc_plan_info(self, rate, shortframes=False):
        out = (C.c_int32 * 8)()
        self._check(self.lib.dvbs2gpu_ldpc_plan_info(self.h, int(rate), int(bool(shortframes)), out))
        keys = ['layers', 'max_deg', 'rec_dwords', 'sum_depth', 'blocks_per_cu', 'cus', 'edges', 'conflict_layers']
        return dict(zip(keys, list(out)))

    def ldpc_decoder_form(self, rate, shortframes=False):
        """0 lane per row, 1 wave per frame, 2 half a row per lane: the kernel that serves the code under this engine's options"""
        r = self.lib.dvbs2gpu_ldpc_decoder_form(self.h, int(rate), int(bool(shortframes)))
        if r < 0:
            self._check(r)
        return r

    def ldpc_split_plan(self, rate, shortframes=False):
        return ldpc_split_plan(rate, shortframes)

    # ---- FEC stages --------------------------------------------------------------------------------
    def ldpc_decode(self, llr, rate, shortframes=False, max_trials=25, force=False, want_post=False):
        """llr int8 [F, N] -> (hard uint8 [F, K/8], trials int32 [F], post int8 [F, N] or None)"""
        t = self.torch
        fi = fec_info(rate, shortframes)
        assert llr.dtype == t.int8 and llr.is_cuda and llr.is_contiguous() and llr.shape[1] == fi['ldpc_n']
        F = llr.shape[0]
        hard = t.empty((F, fi['ldpc_k'] // 8), dtype=t.uint8, device=llr.device)
        trials = t.empty((F,), dtype=t.int32, device=llr.device)
        post = t.empty_like(llr) if want_post else None
        self._check(self.lib.dvbs2gpu_ldpc_decode_batch(self.h, int(rate), int(bool(shortframes)), _ptr(llr), F, int(max_trials),
                                                        int(bool(force)), _ptr(hard), _ptr(post), _ptr(trials), self._stream()))
        return hard, trials, post

    def bch_decode(self, frames, rate, shortframes=False):
        """frames uint8 [F, K/8], corrected in place -> corrections int32 [F]"""
        t = self.torch
        fi = fec_info(rate, shortframes)
        assert frames.dtype == t.uint8 and frames.is_cuda and frames.is_contiguous() and frames.shape[1] == fi['ldpc_k'] // 8
        corr = t.empty((frames.shape[0],), dtype=t.int32, device=frames.device)
        self._check(self.lib.dvbs2gpu_bch_decode_batch(self.h, int(rate), int(bool(shortframes)), _ptr(frames), frames.shape[0],
                                                       _ptr(corr), self._stream()))
        return corr

    def bb_descramble(self, frames, rate, shortframes=False):
        t = self.torch
        fi = fec_info(rate, shortframes)
        assert frames.dtype == t.uint8 and frames.is_cuda and frames.is_contiguous() and frames.shape[1] == fi['ldpc_k'] // 8
        out = t.empty((frames.shape[0], fi['kbch'] // 8), dtype=t.uint8, device=frames.device)
        self._check(self.lib.dvbs2gpu_bb_descramble_batch(self.h, int(rate), int(bool(shortframes)), _ptr(frames), frames.shape[0],
                                                          _ptr(out), self._stream()))
        return out

    def fec_decode(self, llr, rate, shortframes=False, max_trials=25, force=False, out=None, trials=None, corr=None):
        """llr int8 [F, N] -> (bbframes uint8 [F, kbch/8], trials int32 [F], bch corrections int32 [F])"""
        t = self.torch
        fi = fec_info(rate, shortframes)
        assert llr.dtype == t.int8 and llr.is_cuda and llr.is_contiguous() and llr.shape[1] == fi['ldpc_n']
        F = llr.shape[0]
        if out is None:
            out = t.empty((F, fi['kbch'] // 8), dtype=t.uint8, device=llr.device)
        if trials is None:
            trials = t.empty((F,), dtype=t.int32, device=llr.device)
        if corr is None:
            corr = t.empty((F,), dtype=t.int32, device=llr.device)
        self._check(self.lib.dvbs2gpu_fec_decode_batch(self.h, int(rate), int(bool(shortframes)), _ptr(llr), F, int(max_trials),
                                                       int(bool(force)), _ptr(out), _ptr(trials), _ptr(corr), self._stream()))
        return out, trials, corr

    # ---- FEC encoder: the inverses of the stages above, and the per-frame channel BER made from them
    def bb_scramble(self, bbframes, rate, shortframes=False):
        """bbframes uint8 [F, kbch/8] -> scrambled frames uint8 [F, K/8], the BCH parity area zeroed"""
        t = self.torch
        fi = fec_info(rate, shortframes)
        assert bbframes.dtype == t.uint8 and bbframes.is_cuda and bbframes.is_contiguous() and bbframes.shape[1] == fi['kbch'] // 8
        out = t.empty((bbframes.shape[0], fi['ldpc_k'] // 8), dtype=t.uint8, device=bbframes.device)
        self._check(self.lib.dvbs2gpu_bb_scramble_batch(self.h, int(rate), int(bool(shortframes)), _ptr(bbframes), bbframes.shape[0], _ptr(out), self._stream()))
        return out

    def bch_encode(self, frames, rate, shortframes=False):
        """frames uint8 [F, K/8]: the BCH parity of the first kbch bits is written behind them in place -> frames"""
        t = self.torch
        fi = fec_info(rate, shortframes)
        assert frames.dtype == t.uint8 and frames.is_cuda and frames.is_contiguous() and frames.shape[1] == fi['ldpc_k'] // 8
        self._check(self.lib.dvbs2gpu_bch_encode_batch(self.h, int(rate), int(bool(shortframes)), _ptr(frames), frames.shape[0], self._stream()))
        return frames

    def ldpc_encode(self, info, rate, shortframes=False, out=None):
        """info uint8 [F, K/8] -> code words uint8 [F, N/8]"""
        t = self.torch
        fi = fec_info(rate, shortframes)
        assert info.dtype == t.uint8 and info.is_cuda and info.is_contiguous() and info.shape[1] == fi['ldpc_k'] // 8
        if out is None:
            out = t.empty((info.shape[0], fi['ldpc_n'] // 8), dtype=t.uint8, device=info.device)
        assert out.dtype == t.uint8 and out.is_cuda and out.is_contiguous() and out.shape[1] == fi['ldpc_n'] // 8 and out.shape[0] >= info.shape[0]
        self._check(self.lib.dvbs2gpu_ldpc_encode_batch(self.h, int(rate), int(bool(shortframes)), _ptr(info), info.shape[0], _ptr(out), self._stream()))
        return out

    def fec_encode(self, bbframes, rate, shortframes=False, amplitude=None, out=None, llr=None):
        """bbframes uint8 [F, kbch/8] -> (code words uint8 [F, N/8], LLRs int8 [F, N] of +-amplitude, or None without an amplitude)"""
        t = self.torch
        fi = fec_info(rate, shortframes)
        assert bbframes.dtype == t.uint8 and bbframes.is_cuda and bbframes.is_contiguous() and bbframes.shape[1] == fi['kbch'] // 8
        F = bbframes.shape[0]
        if out is None:
            out = t.empty((F, fi['ldpc_n'] // 8), dtype=t.uint8, device=bbframes.device)
        assert out.dtype == t.uint8 and out.is_cuda and out.is_contiguous() and out.shape[1] == fi['ldpc_n'] // 8 and out.shape[0] >= F
        if amplitude is not None and llr is None:
            llr = t.empty((F, fi['ldpc_n']), dtype=t.int8, device=bbframes.device)
        if amplitude is not None:
            assert llr.dtype == t.int8 and llr.is_cuda and llr.is_contiguous() and llr.shape[1] == fi['ldpc_n'] and llr.shape[0] >= F
        self._check(self.lib.dvbs2gpu_fec_encode_batch(self.h, int(rate), int(bool(shortframes)), _ptr(bbframes), F, _ptr(out),
                                                       _ptr(llr) if amplitude is not None else None, int(amplitude or 0), self._stream()))
        return out, (llr if amplitude is not None else None)

    def channel_ber(self, llr, bbframes, rate, shortframes=False, corrections=None):
        """llr int8 [F, N] (what the decoder read), bbframes uint8 [F, kbch/8] (what it delivered), corrections int32 [F] (its BCH results) or None
        -> (errors int32 [F], counted int32 [F]); a frame with a negative correction count gives (-1, 0)"""
        t = self.torch
        fi = fec_info(rate, shortframes)
        assert llr.dtype == t.int8 and llr.is_cuda and llr.is_contiguous() and llr.shape[1] == fi['ldpc_n']
        F = llr.shape[0]
        assert bbframes.dtype == t.uint8 and bbframes.is_cuda and bbframes.is_contiguous() and bbframes.shape == (F, fi['kbch'] // 8)
        if corrections is not None:
            assert corrections.dtype == t.int32 and corrections.is_cuda and corrections.is_contiguous() and corrections.shape == (F,)
        errors = t.empty((F,), dtype=t.int32, device=llr.device)
        counted = t.empty((F,), dtype=t.int32, device=llr.device)
        self._check(self.lib.dvbs2gpu_fec_channel_ber_batch(self.h, int(rate), int(bool(shortframes)), _ptr(llr), _ptr(bbframes), _ptr(corrections), F,
                                                            _ptr(errors), _ptr(counted), self._stream()))
        return errors, counted

    # ---- modulator: code words -> PL symbols -> 2-sps IQ -> channel (csrc/s2_tx.hip)
    def pl_frame(self, code, pls, nstreams=None, code_off=None, code_stride=None, out=None):
        """code uint8: the code words of the PLS list `pls`, by default [nstreams, code_bytes] (a stream's code words one behind the other); with code_off /
        code_stride (bytes, one per frame) frame f of stream s is read at code_off[f] + s * code_stride[f] -> symbols complex64 [nstreams, symbols]"""
        import numpy as np
        t = self.torch
        a = _pls_array(pls)
        sz = s2_tx_sizes(a)
        assert code.dtype == t.uint8 and code.is_cuda and code.is_contiguous()
        if code_off is None:
            assert code.dim() == 2 and code.shape[1] == sz['code_bytes']
            nstreams = code.shape[0]
            off = stride = None
        else:
            off = np.ascontiguousarray(np.asarray(code_off, np.int64))
            stride = np.ascontiguousarray(np.asarray(code_stride, np.int64))
            assert off.shape == (a.size,) and stride.shape == (a.size,) and nstreams is not None
            for f in range(a.size):     # the last byte read lies inside `code`
                if a[f] >> 2:
                    assert off[f] >= 0 and stride[f] >= 0 and off[f] + (nstreams - 1) * stride[f] + s2_tx_sizes([a[f]])['code_bytes'] <= code.numel()
        if out is None:
            out = t.empty((nstreams, sz['symbols']), dtype=t.complex64, device=code.device)
        assert out.dtype == t.complex64 and out.is_cuda and out.is_contiguous() and out.shape == (nstreams, sz['symbols'])
        self._check(self.lib.dvbs2gpu_pl_frame_batch(self.h, a.ctypes.data, a.size, _ptr(code), off.ctypes.data if off is not None else None,
                                                     stride.ctypes.data if stride is not None else None, int(nstreams), _ptr(out), self._stream()))
        return out

    def pulse_shape(self, symbols, rolloff=0.35, timing=0.0, circular=False, out=None):
        """symbols complex64 [nstreams, symbols] -> IQ complex64 [nstreams, 2 * symbols]"""
        t = self.torch
        assert symbols.dtype == t.complex64 and symbols.is_cuda and symbols.is_contiguous() and symbols.dim() == 2
        S, n = symbols.shape
        if out is None:
            out = t.empty((S, 2 * n), dtype=t.complex64, device=symbols.device)
        assert out.dtype == t.complex64 and out.is_cuda and out.is_contiguous() and out.shape == (S, 2 * n)
        self._check(self.lib.dvbs2gpu_pulse_shape_batch(self.h, _ptr(symbols), S, n, float(rolloff), float(timing), int(bool(circular)), _ptr(out), self._stream()))
        return out

    def channel(self, iq, esn0_db=200.0, cfo=0.0, phase0=0.0, seed=0):
        """iq complex64 [nstreams, nsamples], changed in place: rotation by phase0 + cfo * n, AWGN at esn0_db (>= 100: none); each parameter a scalar or one
        value per stream -> iq"""
        t = self.torch
        assert iq.dtype == t.complex64 and iq.is_cuda and iq.is_contiguous() and iq.dim() == 2
        ch, keep = _tx_channel(esn0_db, cfo, phase0, seed, iq.shape[0])
        self._check(self.lib.dvbs2gpu_channel_batch(self.h, _ptr(iq), iq.shape[0], iq.shape[1], ch.esn0_db, ch.cfo, ch.phase0, ch.seed, self._stream()))
        return iq

    def modulate(self, bbframes, pls, nstreams, rolloff=0.35, timing=0.0, circular=False, esn0_db=None, cfo=0.0, phase0=0.0, seed=0, out=None):
        """bbframes uint8, frame-major: for every frame of the PLS list its nstreams BBFRAMEs of kbch/8 bytes (dummy frames take none), one flat tensor of
        nstreams * bbframe_bytes -> IQ complex64 [nstreams, 2 * symbols]; the channel is applied when esn0_db is given"""
        t = self.torch
        a = _pls_array(pls)
        sz = s2_tx_sizes(a)
        assert bbframes.dtype == t.uint8 and bbframes.is_cuda and bbframes.is_contiguous() and bbframes.numel() == nstreams * sz['bbframe_bytes']
        if out is None:
            out = t.empty((nstreams, 2 * sz['symbols']), dtype=t.complex64, device=bbframes.device)
        assert out.dtype == t.complex64 and out.is_cuda and out.is_contiguous() and out.shape == (nstreams, 2 * sz['symbols'])
        ch, keep = (None, None) if esn0_db is None else _tx_channel(esn0_db, cfo, phase0, seed, nstreams)
        self._check(self.lib.dvbs2gpu_s2_modulate_batch(self.h, a.ctypes.data, a.size, _ptr(bbframes), int(nstreams), float(rolloff), float(timing),
                                                        int(bool(circular)), C.addressof(ch) if ch is not None else None, _ptr(out), self._stream()))
        return out

    def demap(self, frames, modcod, shortframes=False, pilots=False):
        """frames complex64 [F, plframe] (PLL output) -> LLR int8 [F, N]"""
        t = self.torch
        mi = modcod_info(modcod, shortframes, pilots)
        assert frames.dtype == t.complex64 and frames.is_cuda and frames.is_contiguous() and frames.shape[1] == mi['plframe_symbols']
        llr = t.empty((frames.shape[0], mi['ldpc_n']), dtype=t.int8, device=frames.device)
        self._check(self.lib.dvbs2gpu_demap_batch(self.h, int(modcod), int(bool(shortframes)), int(bool(pilots)), _ptr(frames),
                                                  frames.shape[0], _ptr(llr), self._stream()))
        return llr

    def deinterleave(self, llr, modcod, shortframes=False):
        """S2Deinterleaver::deinterleave on int8 [F, N] frames (the demapper's index function as its own stage)"""
        t = self.torch
        assert llr.dtype == t.int8 and llr.is_cuda and llr.is_contiguous() and llr.dim() == 2
        out = t.empty_like(llr)
        self._check(self.lib.dvbs2gpu_deinterleave_batch(self.h, int(modcod), int(bool(shortframes)), _ptr(llr), llr.shape[0], _ptr(out), self._stream()))
        return out

    def dvbs_depuncture(self, period, mode, data, state4, fill=0):
        """stage entry: the Viterbi kernel's de-puncturers / soft rotation on host bytes -> (output bytes incl. one byte beyond the
        returned count, count, new state4)"""
        import numpy as np
        data = np.ascontiguousarray(data).view(np.uint8)
        out = np.full(2 * data.size + 64, fill, np.uint8)
        st = (C.c_int32 * 4)(*[int(x) for x in state4])
        n = self._check(self.lib.dvbs2gpu_dvbs_depuncture(self.h, int(period), int(mode), C.c_void_p(data.ctypes.data), data.size,
                                                          C.c_void_p(out.ctypes.data), out.size, st))
        return out, n, list(st)

    def math_eval(self, func, a, b=None):
        """include/dvbs2gpu_math.h evaluated on the device (0 sincos, 1 atan2(a, b), 2 exp, 3 log, 4 LLR clamp) -> (out0, out1)"""
        t = self.torch
        assert a.dtype == t.float32 and a.is_cuda and a.is_contiguous()
        o0, o1 = t.empty_like(a), t.empty_like(a)
        self._check(self.lib.dvbs2gpu_math_eval(self.h, int(func), a.numel(), _ptr(a), _ptr(b) if b is not None else None, _ptr(o0),
                                                _ptr(o1), self._stream()))
        return o0, o1

    def set_stage_timing(self, on):
        self._check(self.lib.dvbs2gpu_set_stage_timing(self.h, int(bool(on))))

    def stage_times(self):
        """per-stage device times since the previous call: {stage: (ms, launches, units)}"""
        st = StageTimes()
        self._check(self.lib.dvbs2gpu_get_stage_times(self.h, C.byref(st)))
        return {STAGE_NAMES[i]: (st.ms[i], st.launches[i], st.units[i]) for i in range(8)}

    def set_pipelined(self, on):
        """FEC of call k overlaps the front end of call k+1; BBFRAMEs are delivered one process_batch call later"""
        self._check(self.lib.dvbs2gpu_set_pipelined(self.h, int(bool(on))))

    def default_cfg(self, modcod, shortframes=False, pilots=False, **kw):
        c = DemodCfg()
        self.lib.dvbs2gpu_demod_default_cfg(int(modcod), int(bool(shortframes)), int(bool(pilots)), C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def demod(self, cfg, max_samples=1000000):
        return Demod(self, cfg, max_samples)

    def process_batch(self, demods, iq_tensors, out_tensors):
        """One call for many streams: iq_tensors[i] complex64 CUDA 1-D, out_tensors[i] uint8 CUDA buffers.
        Returns the list of byte counts."""
        n = len(demods)
        hs = (C.c_void_p * n)(*[d.h for d in demods])
        iq = (C.c_void_p * n)(*[t.data_ptr() for t in iq_tensors])
        cnt = (C.c_int * n)(*[int(t.numel()) for t in iq_tensors])
        out = (C.c_void_p * n)(*[t.data_ptr() for t in out_tensors])
        nb = (C.c_int * n)()
        cap = min(int(t.numel()) for t in out_tensors)
        self._check(self.lib.dvbs2gpu_demod_process_batch(hs, n, iq, cnt, out, cap, nb))
        return list(nb)

    def prepare_batch(self, demods, iq_tensors, out_tensors):
        """the argument arrays of process_batch built once for a fixed set of buffers (thousands of streams: building them per call costs
        tens of milliseconds of Python); returns a callable that runs one call and returns the byte counts (numpy int32)"""
        import numpy as np
        n = len(demods)
        hs = (C.c_void_p * n)(*[d.h for d in demods])
        iq = (C.c_void_p * n)(*[t.data_ptr() for t in iq_tensors])
        cnt = (C.c_int * n)(*[int(t.numel()) for t in iq_tensors])
        out = (C.c_void_p * n)(*[t.data_ptr() for t in out_tensors])
        nb = (C.c_int * n)()
        cap = min(int(t.numel()) for t in out_tensors)
        keep = (list(iq_tensors), list(out_tensors))

        def run(_keep=keep):
            self._check(self.lib.dvbs2gpu_demod_process_batch(hs, n, iq, cnt, out, cap, nb))
            return np.frombuffer(nb, dtype=np.int32).copy()
        return run


class Demod:
    """One DVB-S2 transponder stream: mirror of DVBS2Demod (init/process/reset/setDemodParams/getKBCH)."""

    def __init__(self, engine, cfg, max_samples=1000000):
        self.eng = engine
        self.lib = engine.lib
        self.cfg = cfg
        self.info = modcod_info(cfg.modcod, cfg.shortframes, cfg.pilots)
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_demod_create(engine.h, C.byref(cfg), int(max_samples), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None):
            self.lib.dvbs2gpu_demod_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.eng._check(self.lib.dvbs2gpu_demod_reset(self.h))

    def get_kbch(self):
        return self.lib.dvbs2gpu_demod_get_kbch(self.h)

    def set_params(self, modcod, shortframes, pilots, sof_threshold=0.6, max_ldpc_trials=16):
        """DVBS2Demod::setDemodParams (module_dvbs2_demod.cpp:118-168)"""
        self.eng._check(self.lib.dvbs2gpu_demod_set_params(self.h, int(modcod), int(bool(shortframes)), int(bool(pilots)), float(sof_threshold), int(max_ldpc_trials)))
        self.info = modcod_info(modcod, bool(shortframes), bool(pilots))

    def process(self, iq):
        """iq: numpy complex64 1-D (host, 2 sps) -> numpy uint8 [frames, kbch/8]"""
        import numpy as np
        iq = np.ascontiguousarray(iq, np.complex64)
        if self.cfg.acm_vcm:
            return self.process_vcm(iq)
        kb = self.info['kbch'] // 8
        cap = (iq.size // (2 * self.info['plframe_symbols']) + 4) * kb
        out = np.zeros(cap, np.uint8)
        n = self.lib.dvbs2gpu_demod_process(self.h, int(iq.size), C.c_void_p(iq.ctypes.data), C.c_void_p(out.ctypes.data), cap)
        self.eng._check(n)
        return out[:n].reshape(-1, kb)

    def process_vcm(self, iq):
        """ACM/VCM mode: -> list of BBFRAMEs (numpy uint8, sizes from the per-frame statistics' bbframe_bytes)"""
        import numpy as np
        iq = np.ascontiguousarray(iq, np.complex64)
        cap = iq.size // 2 + 65536 + 40000
        out = np.zeros(cap, np.uint8)
        n = self.eng._check(self.lib.dvbs2gpu_demod_process(self.h, int(iq.size), C.c_void_p(iq.ctypes.data), C.c_void_p(out.ctypes.data), cap))
        frames, pos = [], 0
        for st in self.stats():
            if st.bbframe_bytes:
                frames.append(out[pos:pos + st.bbframe_bytes].copy())
                pos += st.bbframe_bytes
        assert pos == n, (pos, n)
        return frames

    def stats(self):
        n = self.lib.dvbs2gpu_demod_get_stats(self.h, None, 0)
        arr = (FrameStats * max(n, 1))()
        self.lib.dvbs2gpu_demod_get_stats(self.h, arr, n)
        return [arr[i] for i in range(n)]

    def nco_freq(self):
        return float(self.lib.dvbs2gpu_demod_get_nco_freq(self.h))

    def set_quality(self, on):
        """per-frame Es/N0 and MER estimates (dvbs2gpu_demod_set_quality; off by default)"""
        self.eng._check(self.lib.dvbs2gpu_demod_set_quality(self.h, int(bool(on))))

    def quality(self):
        """numpy structured array, one record per stats() record (esn0_db, mer_db, gain, phase, known_symbols, payload_symbols)"""
        import numpy as np
        n = self.eng._check(self.lib.dvbs2gpu_demod_get_quality(self.h, None, 0))
        a = np.zeros(n, _quality_dtype(FrameQuality))
        if n:
            self.eng._check(self.lib.dvbs2gpu_demod_get_quality(self.h, C.cast(a.ctypes.data, C.POINTER(FrameQuality)), n))
        return a

    def tap(self, which):
        import numpy as np
        n = self.eng._check(self.lib.dvbs2gpu_demod_get_tap(self.h, which, None, 0))
        a = np.zeros(n, np.int8 if which == 3 else np.complex64)
        if n:
            self.eng._check(self.lib.dvbs2gpu_demod_get_tap(self.h, which, C.c_void_p(a.ctypes.data), n))
        return a


class _Handle:
    _destroy = None

    def close(self):
        if getattr(self, 'h', None):
            getattr(self.lib, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CcDecoderBatch(_Handle):
    """`nstreams` chained CCDecoder objects (dvbs/viterbi/cc_decoder.cpp) of `frame_size` bits."""
    _destroy = 'dvbs2gpu_ccdec_destroy'

    def __init__(self, engine, nstreams, frame_size):
        self.eng, self.lib, self.nstreams, self.frame_size = engine, engine.lib, nstreams, frame_size
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_ccdec_create(engine.h, nstreams, frame_size, C.byref(h)))
        self.h = h

    def work(self, soft, nblocks, block_stride):
        """soft uint8 CUDA [nstreams, L]; block b of a stream starts at b*block_stride.  -> bits uint8 [nstreams, nblocks, frame]"""
        t = self.eng.torch
        assert soft.dtype == t.uint8 and soft.is_cuda and soft.is_contiguous() and soft.shape[0] == self.nstreams
        assert (nblocks - 1) * block_stride + 2 * (self.frame_size + 6) <= soft.shape[1]
        bits = t.empty((self.nstreams, nblocks, self.frame_size), dtype=t.uint8, device=soft.device)
        self.eng._check(self.lib.dvbs2gpu_ccdec_work_batch(self.h, _ptr(soft), soft.shape[1], block_stride, nblocks, _ptr(bits), self.eng._stream()))
        return bits


class ViterbiStats(C.Structure):
    _fields_ = [('ber', C.c_float), ('state', C.c_int32), ('rate', C.c_int32), ('phase', C.c_int32), ('shift', C.c_int32)]


class ViterbiBatch(_Handle):
    """`nstreams` Viterbi_DVBS objects (dvbs/viterbi_all.cpp) as DVBSDemod::init creates them."""
    _destroy = 'dvbs2gpu_viterbi_destroy'

    def __init__(self, engine, nstreams, ber_threshold=0.15, max_outsync=20):
        self.eng, self.lib, self.nstreams = engine, engine.lib, nstreams
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_viterbi_create(engine.h, nstreams, ber_threshold, max_outsync, C.byref(h)))
        self.h = h

    def reset(self):
        self.eng._check(self.lib.dvbs2gpu_viterbi_reset(self.h))

    def work(self, soft):
        """soft int8 CUDA [nstreams, nblocks, 8192] -> (bits uint8 [nstreams, nblocks, 8192], nbits int32 [nstreams, nblocks],
        stats int32 [nstreams, nblocks, 5] (ber as float bits, state, rate, phase, shift))"""
        t = self.eng.torch
        assert soft.dtype == t.int8 and soft.is_cuda and soft.is_contiguous() and soft.shape[0] == self.nstreams and soft.shape[2] == 8192
        nb = soft.shape[1]
        bits = t.zeros((self.nstreams, nb, 8192), dtype=t.uint8, device=soft.device)
        nbits = t.zeros((self.nstreams, nb), dtype=t.int32, device=soft.device)
        stats = t.zeros((self.nstreams, nb, 5), dtype=t.int32, device=soft.device)
        self.eng._check(self.lib.dvbs2gpu_viterbi_work_batch(self.h, _ptr(soft), nb, _ptr(bits), _ptr(nbits), _ptr(stats), self.eng._stream()))
        return bits, nbits, stats


class ForneyBatch(_Handle):
    """`nstreams` DVBSInterleaving de-interleavers (dvbs/dvbs_interleaving.h)."""
    _destroy = 'dvbs2gpu_forney_destroy'

    def __init__(self, engine, nstreams):
        self.eng, self.lib, self.nstreams = engine, engine.lib, nstreams
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_forney_create(engine.h, nstreams, C.byref(h)))
        self.h = h

    def deinterleave(self, data):
        """data uint8 CUDA [nstreams, nbytes] -> same shape"""
        t = self.eng.torch
        assert data.dtype == t.uint8 and data.is_cuda and data.is_contiguous() and data.shape[0] == self.nstreams
        out = t.empty_like(data)
        self.eng._check(self.lib.dvbs2gpu_forney_deinterleave_batch(self.h, _ptr(data), data.shape[1], _ptr(out), self.eng._stream()))
        return out


def dvbs_slice(engine, iq):
    """iq complex64 CUDA 1-D -> int8 [2n] soft bits (DVBSymToSoftBlock conversion)"""
    t = engine.torch
    assert iq.dtype == t.complex64 and iq.is_cuda and iq.is_contiguous()
    out = t.empty(2 * iq.numel(), dtype=t.int8, device=iq.device)
    engine._check(engine.lib.dvbs2gpu_dvbs_slice(engine.h, _ptr(iq), iq.numel(), _ptr(out), engine._stream()))
    return out


class DvbsCfg(C.Structure):
    _fields_ = [('symbolrate', C.c_double), ('samplerate', C.c_double), ('agc_rate', C.c_float), ('rrc_alpha', C.c_float),
                ('rrc_taps', C.c_int32), ('loop_bw', C.c_float), ('fll_bw', C.c_float), ('clock_omega_gain', C.c_float),
                ('clock_mu_gain', C.c_float), ('omega_rel_limit', C.c_float), ('viterbi_ber_threshold', C.c_float),
                ('viterbi_max_outsync', C.c_int32)]


class DvbsDemodBank(_Handle):
    """`nstreams` DVB-S receivers: mirror of DVBSDemod from the input samples to the Viterbi output (module_dvbs_demod.cpp:78-81)."""
    _destroy = 'dvbs2gpu_dvbs_demod_destroy'

    def __init__(self, engine, nstreams=1, max_samples=1 << 20, **kw):
        self.eng, self.lib, self.nstreams, self.max_samples = engine, engine.lib, nstreams, max_samples
        self.cfg = DvbsCfg()
        self.lib.dvbs2gpu_dvbs_demod_default_cfg(C.byref(self.cfg))
        for k, v in kw.items():
            setattr(self.cfg, k, v)
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_dvbs_demod_create(engine.h, C.byref(self.cfg), nstreams, max_samples, C.byref(h)))
        self.h = h

    def reset(self):
        self.eng._check(self.lib.dvbs2gpu_dvbs_demod_reset(self.h))

    def process(self, iq):
        """single-stream bank: numpy complex64 (host) -> numpy uint8 decoded bits"""
        import numpy as np
        iq = np.ascontiguousarray(iq, np.complex64)
        out = np.zeros(iq.size + 4 * 8192, np.uint8)
        n = self.eng._check(self.lib.dvbs2gpu_dvbs_demod_process(self.h, int(iq.size), C.c_void_p(iq.ctypes.data), C.c_void_p(out.ctypes.data), out.size))
        return out[:n]

    def process_batch(self, iq_tensors, out_tensors):
        n = self.nstreams
        iq = (C.c_void_p * n)(*[t.data_ptr() for t in iq_tensors])
        cnt = (C.c_int * n)(*[int(t.numel()) for t in iq_tensors])
        out = (C.c_void_p * n)(*[t.data_ptr() for t in out_tensors])
        nb = (C.c_int * n)()
        cap = min(int(t.numel()) for t in out_tensors)
        self.eng._check(self.lib.dvbs2gpu_dvbs_demod_process_batch(self.h, iq, cnt, out, cap, nb))
        return list(nb)

    def stats(self):
        arr = (ViterbiStats * self.nstreams)()
        self.eng._check(self.lib.dvbs2gpu_dvbs_demod_get_stats(self.h, arr))
        return [arr[i] for i in range(self.nstreams)]

    def symbols(self, stream=0):
        import numpy as np
        n = self.eng._check(self.lib.dvbs2gpu_dvbs_demod_get_tap(self.h, stream, 0, None, 0))
        a = np.zeros(n, np.complex64)
        if n:
            self.eng._check(self.lib.dvbs2gpu_dvbs_demod_get_tap(self.h, stream, 0, C.c_void_p(a.ctypes.data), n))
        return a

    def loop_state(self, stream=0):
        import numpy as np
        a = np.zeros(8, np.float32)
        self.eng._check(self.lib.dvbs2gpu_dvbs_demod_get_tap(self.h, stream, 1, C.c_void_p(a.ctypes.data), 8))
        return a

    def set_quality(self, on):
        """per-stream Es/N0 (M2M4) and MER of every call (dvbs2gpu_dvbs_demod_set_quality; off by default)"""
        self.eng._check(self.lib.dvbs2gpu_dvbs_demod_set_quality(self.h, int(bool(on))))

    def quality(self):
        """numpy structured array [nstreams] of the last call (esn0_db, mer_db, amplitude, symbols); empty when it ran with quality off"""
        import numpy as np
        a = np.zeros(self.nstreams, _quality_dtype(DvbsQuality))
        n = self.eng._check(self.lib.dvbs2gpu_dvbs_demod_get_quality(self.h, C.cast(a.ctypes.data, C.POINTER(DvbsQuality))))
        return a[:n]


class DvbsTailBank(_Handle):
    """TS deframer + Forney de-interleaver + RS(204,188) + energy dispersal for `nstreams` DVB-S streams (module_dvbs_demod.cpp:82-99)."""
    _destroy = 'dvbs2gpu_dvbs_tail_destroy'

    def __init__(self, engine, nstreams=1, max_bits=1 << 18):
        self.eng, self.lib, self.nstreams, self.max_bits = engine, engine.lib, nstreams, max_bits
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_dvbs_tail_create(engine.h, nstreams, max_bits, C.byref(h)))
        self.h = h

    def reset(self):
        self.eng._check(self.lib.dvbs2gpu_dvbs_tail_reset(self.h))

    def process_batch(self, bit_tensors, out_tensors):
        """bit_tensors[i]: uint8 CUDA 1-D (one bit per byte); out_tensors[i]: uint8 CUDA buffers -> list of byte counts"""
        n = self.nstreams
        pin = (C.c_void_p * n)(*[t.data_ptr() for t in bit_tensors])
        cnt = (C.c_int * n)(*[int(t.numel()) for t in bit_tensors])
        pout = (C.c_void_p * n)(*[t.data_ptr() for t in out_tensors])
        nb = (C.c_int * n)()
        cap = min(int(t.numel()) for t in out_tensors)
        self.eng._check(self.lib.dvbs2gpu_dvbs_tail_process_batch(self.h, pin, cnt, pout, cap, nb, self.eng._stream()))
        return list(nb)

    def stats(self, stream=0):
        a = (C.c_int32 * 11)()
        self.eng._check(self.lib.dvbs2gpu_dvbs_tail_get_stats(self.h, stream, a))
        return {'frames': a[0], 'errors_nor': a[1], 'errors_inv': a[2], 'rs_errors': list(a[3:11])}

    @property
    def max_frames(self):
        """frames one call can deliver per stream: the handle's capacity (include/dvbs2gpu.h)"""
        return self.max_bits // 13056 + 3

    def dropped(self, stream=0):
        """sync-pattern hits of the last process_batch call found beyond max_frames and not delivered"""
        a = C.c_int32()
        self.eng._check(self.lib.dvbs2gpu_dvbs_tail_get_dropped(self.h, stream, C.byref(a)))
        return a.value

    def tap(self, which, stream=0):
        """stage taps of the last call: 0 deframed frames, 1 packets after Forney + RS, 2 RS status, 3 RS error counts (int32)"""
        import numpy as np
        n = self.eng._check(self.lib.dvbs2gpu_dvbs_tail_get_tap(self.h, stream, which, None, 0))
        a = np.zeros(n, np.uint8)
        if n:
            self.eng._check(self.lib.dvbs2gpu_dvbs_tail_get_tap(self.h, stream, which, C.c_void_p(a.ctypes.data), n))
        return a.view(np.int32) if which == 3 else a

    def rs_stage(self, packets, skip_rs=False):
        """packets: numpy uint8 [n, 204] (n a multiple of 8) -> TS bytes uint8 [n, 188] (stage entry, stream 0)"""
        import numpy as np
        packets = np.ascontiguousarray(packets, np.uint8)
        out = np.zeros(packets.shape[0] * 188, np.uint8)
        n = self.eng._check(self.lib.dvbs2gpu_dvbs_tail_rs_stage(self.h, C.c_void_p(packets.ctypes.data), packets.shape[0], int(bool(skip_rs)),
                                                                 C.c_void_p(out.ctypes.data), out.size))
        return out[:n].reshape(-1, 188)


class BbTsParserBank(_Handle):
    """BBFRAME -> MPEG-TS / GSE parser for `nstreams` DVB-S2 streams: dsp::dvbs2::BBFrameTSParser (bbframe_ts_parser.cpp:104-390),
    the consumer of DVBS2Demod's output in the reference's sink handler (main.cpp:532-558)."""
    _destroy = 'dvbs2gpu_bbts_destroy'
    HEADER_FIELDS = ('ts_gs', 'sis_mis', 'ccm_acm', 'issyi', 'npd', 'ro', 'isi', 'upl', 'dfl', 'sync', 'syncd')

    def __init__(self, engine, nstreams=1, kbch_bits=48408, max_frames=16):
        self.eng, self.lib, self.nstreams, self.kbch, self.max_frames = engine, engine.lib, nstreams, kbch_bits, max_frames
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_bbts_create(engine.h, nstreams, kbch_bits, max_frames, C.byref(h)))
        self.h = h

    def set_frame_size(self, kbch_bits):
        self.eng._check(self.lib.dvbs2gpu_bbts_set_frame_size(self.h, kbch_bits))
        self.kbch = kbch_bits

    def process_batch(self, bb_tensors, out_tensors):
        """bb_tensors[i]: uint8 CUDA, a whole number of kbch/8-byte BBFRAMEs; out_tensors[i]: uint8 CUDA buffers -> byte counts"""
        n, fb = self.nstreams, self.kbch // 8
        pin = (C.c_void_p * n)(*[t.data_ptr() for t in bb_tensors])
        cnt = (C.c_int * n)(*[int(t.numel()) // fb for t in bb_tensors])
        pout = (C.c_void_p * n)(*[t.data_ptr() for t in out_tensors])
        nb = (C.c_int * n)()
        cap = min(int(t.numel()) for t in out_tensors)
        self.eng._check(self.lib.dvbs2gpu_bbts_process_batch(self.h, pin, cnt, pout, cap, nb, self.eng._stream()))
        return list(nb)

    def work(self, bbframes, cap=None):
        """BBFrameTSParser::work on host buffers (bank of one stream): numpy uint8 in -> numpy uint8 out"""
        import numpy as np
        bb = np.ascontiguousarray(bbframes, np.uint8).reshape(-1)
        cnt = bb.size // (self.kbch // 8)
        cap = cap if cap is not None else bb.size + 376
        out = np.zeros(max(cap, 1), np.uint8)
        n = self.eng._check(self.lib.dvbs2gpu_bbts_work(self.h, C.c_void_p(bb.ctypes.data), cnt, C.c_void_p(out.ctypes.data), cap))
        return out[:n].copy()

    def stats(self, stream=0):
        a = (C.c_int32 * 17)()
        self.eng._check(self.lib.dvbs2gpu_bbts_get_stats(self.h, stream, a, 17))
        d = {k: a[i] for i, k in enumerate(self.HEADER_FIELDS)}
        d.update(last_gse_crc_err=a[11], last_bb_cnt=a[12], last_bb_proc=a[13], last_ts_errs=a[14], synched=a[15], count=a[16])
        return d

    # ---- GSE (include/dvbs2gpu.h): where GSE frames are parsed, the counters, and one row per GRE packet of the last call
    GSE_DEVICE, GSE_HOST = 0, 1
    PDU_REASSEMBLED, PDU_LABEL = 1, 2

    def set_gse_path(self, mode):
        """0: the GPU kernels (default); 1: the library's host parser, for comparison"""
        self.eng._check(self.lib.dvbs2gpu_bbts_set_gse_path(self.h, int(mode)))

    def gse_stats(self, stream=0):
        st = GseStats()
        self.eng._check(self.lib.dvbs2gpu_bbts_get_gse_stats(self.h, int(stream), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in GseStats._fields_}

    def pdu_table(self, stream=0):
        """[(offset in the stream's output, bytes, protocol type, flags)] of the last call, in output order"""
        n = C.c_int()
        self.eng._check(self.lib.dvbs2gpu_bbts_get_pdu_table(self.h, int(stream), None, 0, C.byref(n)))
        rows = (GsePdu * max(n.value, 1))()
        self.eng._check(self.lib.dvbs2gpu_bbts_get_pdu_table(self.h, int(stream), rows, n.value, C.byref(n)))
        return [(r.offset, r.bytes, r.protocol, r.flags) for r in rows[:n.value]]

    def pdu_table_device(self, stream=0):
        """(device pointer or None, rows): the same table as dvbs2gpu_gse_pdu records in HBM, valid until the next call"""
        p, n = C.c_void_p(), C.c_int()
        self.eng._check(self.lib.dvbs2gpu_bbts_get_pdu_table_device(self.h, int(stream), C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- mode-adaptation mode (include/dvbs2gpu.h): ISI demultiplexing, ISSY / DNP, null-packet reinsertion, CRC-8, per-frame sizes
    MA_SLOTS = 8

    @classmethod
    def host(cls, kbch_bits=58192, max_frames=64):
        """a one-stream bank without a device: the library's host parser behind ma_work / ma_flush"""
        self = cls.__new__(cls)
        self.eng, self.lib, self.nstreams, self.kbch, self.max_frames = None, load_library(), 1, kbch_bits, max_frames
        h = C.c_void_p()
        self._check(self.lib.dvbs2gpu_bbts_create_host(kbch_bits, max_frames, C.byref(h)))
        self.h = h
        return self

    def _check(self, rc):
        if rc < 0:
            raise Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
        return rc

    def set_mode_adaptation(self, on=True, **kw):
        """on: issy_bytes (0 auto, 2, 3), crc_span, reinsert_nulls, check_crc as keywords; off: back to a fresh reference-mode bank"""
        if not on:
            return self._check(self.lib.dvbs2gpu_bbts_set_mode_adaptation(self.h, None))
        cfg = BbtsMaCfg()
        self.lib.dvbs2gpu_bbts_ma_default_cfg(C.byref(cfg))
        for k, v in kw.items():
            if k not in dict(BbtsMaCfg._fields_):
                raise TypeError(k)
            setattr(cfg, k, int(v))
        self._check(self.lib.dvbs2gpu_bbts_set_mode_adaptation(self.h, C.byref(cfg)))

    def select_isi(self, stream, isis):
        a = (C.c_uint8 * max(len(isis), 1))(*[int(x) for x in isis])
        self._check(self.lib.dvbs2gpu_bbts_select_isi(self.h, int(stream), a, len(isis)))

    def _sizes(self, frame_bytes, n):
        if frame_bytes is None:
            return None, None
        keep = [(C.c_int * max(len(x), 1))(*[int(v) for v in x]) if x is not None else None for x in frame_bytes]
        ptrs = (C.POINTER(C.c_int) * n)(*[C.cast(k, C.POINTER(C.c_int)) if k is not None else C.POINTER(C.c_int)() for k in keep])
        return ptrs, keep

    def process_ma(self, bb_tensors, out_tensors, frame_bytes=None, nframes=None):
        """bb_tensors[i]: uint8 CUDA, the BBFRAMEs of stream i back to back; frame_bytes[i]: their sizes (None: kbch/8 each);
        out_tensors[i][k]: uint8 CUDA buffer of slot k of stream i (a list per stream, at least as many as ISIs selected).
        -> byte counts [nstreams][8].  Dvbs2GpuError -5 carries .needed when a buffer is too small (nothing has advanced then)."""
        n, S = self.nstreams, self.MA_SLOTS
        pin = (C.c_void_p * n)(*[t.data_ptr() for t in bb_tensors])
        if nframes is None:
            nframes = [len(frame_bytes[i]) if frame_bytes is not None and frame_bytes[i] is not None else int(bb_tensors[i].numel()) // (self.kbch // 8)
                       for i in range(n)]
        cnt = (C.c_int * n)(*[int(x) for x in nframes])
        flat = [None] * (n * S)
        for i, row in enumerate(out_tensors):
            flat[i * S:i * S + len(row)] = list(row)
        pout = (C.c_void_p * (n * S))(*[t.data_ptr() if t is not None else None for t in flat])
        cap = min([int(t.numel()) for t in flat if t is not None] or [0])
        nb, need = (C.c_int * (n * S))(), (C.c_int * (n * S))()
        sizes, _keep = self._sizes(frame_bytes, n)
        rc = self.lib.dvbs2gpu_bbts_process_ma_batch(self.h, pin, sizes, cnt, pout, cap, nb, need, self.eng._stream())
        if rc < 0:
            e = Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
            e.needed = [list(need[i * S:(i + 1) * S]) for i in range(n)]
            raise e
        return [list(nb[i * S:(i + 1) * S]) for i in range(n)]

    def process_ma_from_demods(self, demods, bb_tensors, out_tensors):
        """the BBFRAMEs an Engine.process_batch call left in bb_tensors (device), stream i of this bank = demods[i]: the sizes come
        from the handles' per-frame statistics (ACM/VCM: bbframe_bytes, dummy frames left out), the bytes stay where they are"""
        sizes = [[st.bbframe_bytes for st in d.stats() if st.bbframe_bytes] for d in demods]
        return self.process_ma(bb_tensors, out_tensors, frame_bytes=sizes)

    def ma_work(self, frames, cap=1 << 20):
        """one stream, host buffers: frames = list of numpy uint8 BBFRAMEs (any sizes) -> list of 8 numpy arrays (TS per slot)"""
        import numpy as np
        S = self.MA_SLOTS
        bb = np.ascontiguousarray(np.concatenate([np.asarray(f, np.uint8).reshape(-1) for f in frames]) if len(frames) else np.zeros(0, np.uint8))
        sizes = (C.c_int * max(len(frames), 1))(*[int(np.asarray(f).size) for f in frames])
        outs = [np.zeros(max(cap, 1), np.uint8) for _ in range(S)]
        pout = (C.c_void_p * S)(*[o.ctypes.data for o in outs])
        nb, need = (C.c_int * S)(), (C.c_int * S)()
        rc = self.lib.dvbs2gpu_bbts_ma_work(self.h, C.c_void_p(bb.ctypes.data), sizes, len(frames), pout, cap, nb, need)
        if rc < 0:
            e = Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
            e.needed = list(need)
            raise e
        return [outs[k][:nb[k]].copy() for k in range(S)]

    def ma_flush(self, cap=256 * 188):
        """-> [nstreams][8] numpy arrays: the packets that were held back for the CRC-8 after them"""
        import numpy as np
        n, S = self.nstreams, self.MA_SLOTS
        nb = (C.c_int * (n * S))()
        if self.eng is None:
            outs = [np.zeros(cap, np.uint8) for _ in range(n * S)]
            pout = (C.c_void_p * (n * S))(*[o.ctypes.data for o in outs])
            self._check(self.lib.dvbs2gpu_bbts_ma_flush(self.h, pout, cap, nb))
            res = [outs[i][:nb[i]].copy() for i in range(n * S)]
        else:
            import torch
            buf = torch.zeros((n * S, cap), dtype=torch.uint8, device='cuda')
            pout = (C.c_void_p * (n * S))(*[buf[i].data_ptr() for i in range(n * S)])
            self._check(self.lib.dvbs2gpu_bbts_ma_flush(self.h, pout, cap, nb))
            host = buf.cpu().numpy()
            res = [host[i, :nb[i]].copy() for i in range(n * S)]
        return [res[i * S:(i + 1) * S] for i in range(n)]

    def ma_stats(self, stream=0, slot=0):
        st = BbtsMaStats()
        self._check(self.lib.dvbs2gpu_bbts_ma_get_stats(self.h, int(stream), int(slot), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in BbtsMaStats._fields_}

    # ---- DVB-T2 high-efficiency-mode BBFRAMEs (those of a T2-MI feed): [187 UP bytes][DNP], the ISSY field in the header
    def ma_set_t2_hem(self, on=True):
        """HEM frames are parsed by their own rules (off: rejected, as before); needs the mode on; every lane starts afresh"""
        self._check(self.lib.dvbs2gpu_bbts_ma_set_t2_hem(self.h, int(bool(on))))

    @staticmethod
    def ma_hem_layout():
        """the compiled-in HEM slot layout: {'up_off', 'up_len', 'dnp_off', 'mode'}"""
        a = (C.c_int32 * 4)()
        rc = load_library().dvbs2gpu_bbts_ma_get_hem_layout(a)
        if rc < 0:
            raise Dvbs2GpuError(rc, 'dvbs2gpu_bbts_ma_get_hem_layout')
        return dict(zip(('up_off', 'up_len', 'dnp_off', 'mode'), a))

    # ---- GSE in the mode-adaptation mode: one reassembly context per (stream, selected ISI); GRE packets in the slot's own buffer
    def ma_set_gse(self, on=True):
        """GSE frames of the selected ISIs are decapsulated (off: skipped, the slots' GSE state dropped); needs the mode on"""
        self._check(self.lib.dvbs2gpu_bbts_ma_set_gse(self.h, int(bool(on))))

    def ma_gse_stats(self, stream=0, slot=0):
        st = BbtsMaGseStats()
        self._check(self.lib.dvbs2gpu_bbts_ma_get_gse_stats(self.h, int(stream), int(slot), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in BbtsMaGseStats._fields_}

    def ma_pdu_table(self, stream=0, slot=0):
        """[(offset in the slot's output, bytes, protocol type, flags)] of the last call, in output order"""
        n = C.c_int()
        self._check(self.lib.dvbs2gpu_bbts_ma_get_pdu_table(self.h, int(stream), int(slot), None, 0, C.byref(n)))
        rows = (GsePdu * max(n.value, 1))()
        self._check(self.lib.dvbs2gpu_bbts_ma_get_pdu_table(self.h, int(stream), int(slot), rows, n.value, C.byref(n)))
        return [(r.offset, r.bytes, r.protocol, r.flags) for r in rows[:n.value]]

    def ma_pdu_table_device(self, stream=0, slot=0):
        """(device pointer or None, rows): the same table as dvbs2gpu_gse_pdu records in HBM, valid until the next call"""
        p, n = C.c_void_p(), C.c_int()
        self._check(self.lib.dvbs2gpu_bbts_ma_get_pdu_table_device(self.h, int(stream), int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value

    def isi_seen(self, stream=0):
        """-> sorted list of the ISIs seen on `stream` since the mode was switched on"""
        m = (C.c_uint32 * 8)()
        self._check(self.lib.dvbs2gpu_bbts_get_isi_seen(self.h, int(stream), m))
        return [i for i in range(256) if m[i >> 5] >> (i & 31) & 1]


class _TsBank(_Handle):
    """what the banks on transport streams in HBM share (csrc/ts_bank.h): error check, host-bank construction, the pointer tables of a
    batch call and the two-call table read"""

    def _check(self, rc):
        if rc < 0:
            raise Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
        return rc

    @classmethod
    def _host(cls, create, **dims):
        self = cls.__new__(cls)
        self.eng, self.lib = None, load_library()
        self.__dict__.update(dims)
        h = C.c_void_p()
        self._check(getattr(self.lib, create)(*dims.values(), C.byref(h)))
        self.h = h
        return self

    def _marshal(self, ts_tensors, out_tensors, nbytes):
        """-> (input pointers, byte counts, output pointers or None, cap: the smallest output buffer)"""
        n = self.nstreams
        pin = (C.c_void_p * n)(*[t.data_ptr() for t in ts_tensors])
        cnt = (C.c_int * n)(*[int(t.numel()) if nbytes is None else int(nbytes[i]) for i, t in enumerate(ts_tensors)])
        if out_tensors is None:
            return pin, cnt, None, 0
        return pin, cnt, (C.c_void_p * n)(*[t.data_ptr() for t in out_tensors]), min(int(t.numel()) for t in out_tensors)

    def _rows(self, getter, Row, *args):
        """ask how many rows there are, then fetch them: getter(h, *args, rows, cap, &n) -> the rows"""
        n = C.c_int()
        self._check(getter(self.h, *args, None, 0, C.byref(n)))
        rows = (Row * max(n.value, 1))()
        self._check(getter(self.h, *args, rows, n.value, C.byref(n)))
        return rows[:n.value]


class TsMonitorBank(_TsBank):
    """TS monitor for `nstreams` transport streams (own extension; include/dvbs2gpu.h, TS monitor bank): per-PID continuity checks, the
    PID table of the last call and a PID filter that compacts the passing packets on the GPU.  Its input is what BbTsParserBank or
    DvbsTailBank left in HBM."""
    _destroy = 'dvbs2gpu_tsmon_destroy'
    PASS_ALL, PASS_LISTED, DROP_LISTED = 0, 1, 2
    PID_FIRST_SEEN, PID_DISCONTINUITY = 1, 2

    def __init__(self, engine, nstreams=1, max_packets=4096):
        self.eng, self.lib, self.nstreams, self.max_packets = engine, engine.lib, nstreams, max_packets
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_tsmon_create(engine.h, nstreams, max_packets, C.byref(h)))
        self.h = h

    @classmethod
    def host(cls, nstreams=1, max_packets=4096):
        """a bank without a device: the library's host implementation of the same rules, behind work()"""
        return cls._host('dvbs2gpu_tsmon_create_host', nstreams=nstreams, max_packets=max_packets)

    def reset(self):
        self._check(self.lib.dvbs2gpu_tsmon_reset(self.h))

    def set_filter(self, stream, mode=0, pids=(), drop_null=False, drop_tei=False, drop_bad_sync=False):
        f = TsMonFilter(int(mode), int(bool(drop_null)), int(bool(drop_tei)), int(bool(drop_bad_sync)))
        a = (C.c_uint16 * max(len(pids), 1))(*[int(p) for p in pids])
        self._check(self.lib.dvbs2gpu_tsmon_set_filter(self.h, int(stream), C.byref(f), a, len(pids)))

    def process(self, ts_tensors, out_tensors=None, nbytes=None):
        """ts_tensors[i]: uint8 CUDA, whole 188-byte packets (nbytes[i] of them, default all); out_tensors: None for statistics and
        table only, else uint8 CUDA buffers that receive the passing packets -> byte counts.  Dvbs2GpuError -5 carries .needed when a
        buffer is too small (nothing has advanced then)."""
        pin, cnt, pout, cap = self._marshal(ts_tensors, out_tensors, nbytes)
        nb = (C.c_int * self.nstreams)()
        rc = self.lib.dvbs2gpu_tsmon_process_batch(self.h, pin, cnt, pout, cap, nb, self.eng._stream())
        if rc < 0:
            e = Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
            e.needed = list(nb)
            raise e
        return list(nb)

    def work(self, ts, stream=0, cap=None, filtered=True):
        """one stream, host buffers: numpy uint8 packets in -> the passing packets (numpy uint8), or None with filtered=False"""
        import numpy as np
        ts = np.ascontiguousarray(ts, np.uint8).reshape(-1)
        if not filtered:
            self._check(self.lib.dvbs2gpu_tsmon_work(self.h, int(stream), C.c_void_p(ts.ctypes.data), ts.size, None, 0))
            return None
        cap = ts.size if cap is None else cap
        out = np.zeros(max(cap, 1), np.uint8)
        n = self._check(self.lib.dvbs2gpu_tsmon_work(self.h, int(stream), C.c_void_p(ts.ctypes.data), ts.size, C.c_void_p(out.ctypes.data), cap))
        return out[:n].copy()

    def stats(self, stream=0):
        st = TsMonStats()
        self._check(self.lib.dvbs2gpu_tsmon_get_stats(self.h, int(stream), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in TsMonStats._fields_}

    def pid_table(self, stream=0):
        """[(pid, flags, packets, cc_errors, duplicates, scrambled, pusi)] of the last call, ascending by PID"""
        rows = self._rows(self.lib.dvbs2gpu_tsmon_get_pid_table, TsMonPid, int(stream))
        return [(r.pid, r.flags, r.packets, r.cc_errors, r.duplicates, r.scrambled, r.pusi) for r in rows]

    def pid_table_device(self, stream=0):
        """(device pointer or None, rows): the same table as dvbs2gpu_tsmon_pid records in HBM, valid until the next call"""
        p, n = C.c_void_p(), C.c_int()
        self._check(self.lib.dvbs2gpu_tsmon_get_pid_table_device(self.h, int(stream), C.byref(p), C.byref(n)))
        return p.value, n.value


class PsiBank(_TsBank):
    """PSI section bank for `nstreams` transport streams (own extension; include/dvbs2gpu.h, PSI section bank): PAT / PMT / SI section
    reassembly with CRC-32 on up to 16 watched PIDs per stream, one table row per section, the decoded PAT and PMTs on the host."""
    _destroy = 'dvbs2gpu_psi_destroy'
    SLOTS = 16
    CRC_ERROR, CHANGED = 1, 2
    ROW_KEYS = tuple(k for k, _ in PsiSection._fields_)

    def __init__(self, engine, nstreams=1, max_packets=4096, max_sections=1024):
        self.eng, self.lib, self.nstreams, self.max_packets, self.max_sections = engine, engine.lib, nstreams, max_packets, max_sections
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_psi_create(engine.h, nstreams, max_packets, max_sections, C.byref(h)))
        self.h = h
        self._watched = [{0: 0} for _ in range(nstreams)]           # per stream: slot -> PID, as set_watch left them

    @classmethod
    def host(cls, nstreams=1, max_packets=4096, max_sections=1024):
        """a bank without a device: the library's host implementation of the same rules, behind work()"""
        self = cls._host('dvbs2gpu_psi_create_host', nstreams=nstreams, max_packets=max_packets, max_sections=max_sections)
        self._watched = [{0: 0} for _ in range(nstreams)]
        return self

    @staticmethod
    def layout():
        """the section syntax the library relies on (dvbs2gpu_psi_layout) as a dict"""
        lay = PsiLayout()
        load_library().dvbs2gpu_psi_get_layout(C.byref(lay))
        return {k: int(getattr(lay, k)) for k, _ in PsiLayout._fields_}

    def reset(self):
        self._check(self.lib.dvbs2gpu_psi_reset(self.h))

    def set_watch(self, stream, slot, pid, expect_table_id=-1):
        """pid -1 clears the slot; the slot starts afresh"""
        self._check(self.lib.dvbs2gpu_psi_set_watch(self.h, int(stream), int(slot), int(pid), int(expect_table_id)))
        self._watched[int(stream)].pop(int(slot), None)
        if pid >= 0:
            self._watched[int(stream)][int(slot)] = int(pid)

    def set_deliver(self, stream, mode):
        self._check(self.lib.dvbs2gpu_psi_set_deliver(self.h, int(stream), int(mode)))

    def follow_pat(self, stream=0):
        """slots 1..15 of the stream start afresh and watch the PMT PIDs of the programs of the stream's PAT (program 0, the network PID,
        is no program), in the PAT's order and expecting table_id 2, as far as the slots go -> [(program_number, pid)] of the programs
        that did not fit.  Programs that share a PMT PID share its slot; a PMT PID that slot 0 watches already stays there."""
        free, left, seen = list(range(1, self.SLOTS)), [], {self._watched[int(stream)].get(0, -1)}
        for slot in free:
            self.set_watch(stream, slot, -1)
        for n, p in self.programs(stream)[1]:
            if n == 0 or p in seen:
                continue
            if not free:
                left.append((n, p))
                continue
            seen.add(p)
            self.set_watch(stream, free.pop(0), p, 2)
        return left

    def process(self, ts_tensors, out_tensors=None, nbytes=None):
        """ts_tensors[i]: uint8 CUDA, whole 188-byte packets (nbytes[i] of them, default all); out_tensors: None for rows and counters
        only, else uint8 CUDA buffers that receive the delivered sections -> byte counts.  Dvbs2GpuError -5 carries .needed and .rows
        when a buffer or max_sections is too small (nothing has advanced then)."""
        pin, cnt, pout, cap = self._marshal(ts_tensors, out_tensors, nbytes)
        nb, nr = (C.c_int * self.nstreams)(), (C.c_int * self.nstreams)()
        rc = self.lib.dvbs2gpu_psi_process_batch(self.h, pin, cnt, pout, cap, nb, nr, self.eng._stream())
        if rc < 0:
            e = Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
            e.needed, e.rows = list(nb), list(nr)
            raise e
        return list(nb)

    def work(self, ts, stream=0, cap=None, deliver=True):
        """one stream, host buffers: numpy uint8 packets in -> the delivered sections back to back (numpy uint8), or None with
        deliver=False (rows and counters only)"""
        import numpy as np
        ts = np.ascontiguousarray(ts, np.uint8).reshape(-1)
        cap = ts.size + self.SLOTS * 4096 if cap is None else cap
        out = np.zeros(max(cap, 1), np.uint8) if deliver else None
        rc = self.lib.dvbs2gpu_psi_work(self.h, int(stream), C.c_void_p(ts.ctypes.data), ts.size, C.c_void_p(out.ctypes.data) if deliver else None,
                                        cap if deliver else 0)
        if rc < 0:
            e = Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
            nb, nr = C.c_int(), C.c_int()
            self.lib.dvbs2gpu_psi_get_needed(self.h, int(stream), C.byref(nb), C.byref(nr))
            e.needed, e.rows = nb.value, nr.value
            raise e
        return out[:rc].copy() if deliver else None

    def stats(self, stream=0, slot=-1):
        st = PsiStats()
        self._check(self.lib.dvbs2gpu_psi_get_stats(self.h, int(stream), int(slot), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in PsiStats._fields_}

    def section_table(self, stream=0):
        """one dict per section of the last call (the fields of dvbs2gpu_psi_section), in row order"""
        rows = self._rows(self.lib.dvbs2gpu_psi_get_section_table, PsiSection, int(stream))
        return [{k: int(getattr(r, k)) for k in self.ROW_KEYS} for r in rows]

    def section_table_device(self, stream=0):
        """(device pointer or None, rows): the same table as dvbs2gpu_psi_section records in HBM, valid until the next call"""
        p, n = C.c_void_p(), C.c_int()
        self._check(self.lib.dvbs2gpu_psi_get_section_table_device(self.h, int(stream), C.byref(p), C.byref(n)))
        return p.value, n.value

    def programs(self, stream=0):
        """-> ({transport_stream_id, version, malformed}, [(program_number, pid)]) from the PAT the stream holds (-1, -1: none)"""
        hdr = PsiPat()
        rows = self._rows(self.lib.dvbs2gpu_psi_get_programs, PsiProgram, int(stream), C.byref(hdr))
        return {k: int(getattr(hdr, k)) for k, _ in PsiPat._fields_}, [(r.program_number, r.pid) for r in rows]

    def program_map(self, stream=0, slot=1):
        """-> ({program_number, version, pcr_pid, malformed}, [(stream_type, elementary_pid)]) from the slot's PMT (program_number -1: none)"""
        hdr = PsiPmt()
        rows = self._rows(self.lib.dvbs2gpu_psi_get_program_map, PsiEs, int(stream), int(slot), C.byref(hdr))
        return {k: int(getattr(hdr, k)) for k, _ in PsiPmt._fields_}, [(r.stream_type, r.elementary_pid) for r in rows]


class _WatchBank(_TsBank):
    """what the banks share that judge up to 16 watched PIDs per stream and write one row table per stream (csrc/watch_bank.h; PcrBank,
    PesBank, and under _CodecBank EsBank and AudBank).  A bank names its C prefix (_c) and its row and statistics structures (_Row, _Stats, _StreamStats), gives the row
    table its public names and adds stream_stats(), follow_pmts() and what it is told beyond the watch list."""
    SLOTS = 16
    _c = _Row = _Stats = _StreamStats = None

    def _fn(self, name):
        return getattr(self.lib, '%s_%s' % (self._c, name))

    def __init__(self, engine, nstreams=1, max_packets=4096, max_rows=1024):
        self.eng, self.lib, self.nstreams, self.max_packets, self.max_rows = engine, engine.lib, nstreams, max_packets, max_rows
        h = C.c_void_p()
        engine._check(self._fn('create')(engine.h, nstreams, max_packets, max_rows, C.byref(h)))
        self.h = h
        self._watched = [{} for _ in range(nstreams)]               # per stream: slot -> PID (EsBank: (PID, codec)), as set_watch left them

    @classmethod
    def host(cls, nstreams=1, max_packets=4096, max_rows=1024):
        """a bank without a device: the library's host implementation of the same rules, behind work()"""
        self = cls._host(cls._c + '_create_host', nstreams=nstreams, max_packets=max_packets, max_rows=max_rows)
        self._watched = [{} for _ in range(nstreams)]
        return self

    def reset(self):
        """forgets states, positions and counters; watches, rates and codecs stay"""
        self._check(self._fn('reset')(self.h))

    def set_watch(self, stream, slot, pid, *extra):
        """pid -1 clears the slot; the slot starts afresh"""
        self._check(self._fn('set_watch')(self.h, int(stream), int(slot), int(pid), *[int(x) for x in extra]))
        self._watched[int(stream)].pop(int(slot), None)
        if pid >= 0:
            self._watched[int(stream)][int(slot)] = (int(pid), *[int(x) for x in extra]) if extra else int(pid)

    def _follow(self, psi_bank, stream, pick):
        """watches, in free slots, the PIDs that pick(hdr, es) yields as (pid, what set_watch takes behind it) for each PMT that `psi_bank`
        holds decoded, in the order of its slots; 0x1FFF and above and PIDs watched already are skipped -> the PIDs that found no free slot"""
        watched = self._watched[int(stream)]
        left = []
        for slot in range(psi_bank.SLOTS):
            hdr, es = psi_bank.program_map(stream, slot)
            if hdr['program_number'] < 0:
                continue
            for pid, *extra in pick(hdr, es):
                if pid >= 0x1FFF or pid in [w[0] if extra else w for w in watched.values()] or pid in left:
                    continue
                free = [s for s in range(self.SLOTS) if s not in watched]
                if free:
                    self.set_watch(stream, free[0], pid, *extra)
                else:
                    left.append(pid)
        return left

    def process(self, ts_tensors, nbytes=None):
        """ts_tensors[i]: uint8 CUDA, whole 188-byte packets (nbytes[i] of them, default all), of any alignment -> the rows (PCR records,
        PES starts, ES rows) of the call per stream (the table holds the first max_rows of them)"""
        pin, cnt, _, _ = self._marshal(ts_tensors, None, nbytes)
        nr = (C.c_int * self.nstreams)()
        self._check(self._fn('process_batch')(self.h, pin, cnt, nr, self.eng._stream()))
        return list(nr)

    def work(self, ts, stream=0):
        """one stream, a host buffer: numpy uint8 packets in -> the rows of the call"""
        import numpy as np
        ts = np.ascontiguousarray(ts, np.uint8).reshape(-1)
        return self._check(self._fn('work')(self.h, int(stream), C.c_void_p(ts.ctypes.data), ts.size))

    def stats(self, stream=0, slot=-1):
        st = self._Stats()
        self._check(self._fn('get_stats')(self.h, int(stream), int(slot), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in self._Stats._fields_}

    def _stream_stats(self, stream):
        st = self._StreamStats()
        self._check(self._fn('get_stream_stats')(self.h, int(stream), C.byref(st)))
        return st

    def _table(self, stream=0):
        """one dict per row of the last call (the fields of the bank's row structure but `reserved`), in row order"""
        rows = self._rows(self._fn('get_row_table'), self._Row, int(stream))
        return [{k: int(getattr(r, k)) for k in self.ROW_KEYS if k != 'reserved'} for r in rows]

    def _table_device(self, stream=0):
        """(device pointer or None, rows): the same table as the bank's row records in HBM, valid until the next call"""
        p, n = C.c_void_p(), C.c_int()
        self._check(self._fn('get_row_table_device')(self.h, int(stream), C.byref(p), C.byref(n)))
        return p.value, n.value


class PcrBank(_WatchBank):
    """PCR bank for `nstreams` transport streams (own extension; include/dvbs2gpu.h, PCR bank): PCR repetition, discontinuity and
    accuracy checks on up to 16 watched PIDs per stream, one table row per PCR, in integers on (PCR value, packet position)."""
    _c, _Row, _Stats, _StreamStats = 'dvbs2gpu_pcr', PcrRow, PcrStats, PcrStreamStats
    _destroy = 'dvbs2gpu_pcr_destroy'
    SLOTS = 16
    FIRST, ANNOUNCED, REPEATED, OK, LATE, JUMP = range(6)
    ACCURACY_ERROR, SATURATED = 1, 2
    DEFAULT_LIMIT_Q6 = 864
    ROW_KEYS = tuple(k for k, _ in PcrRow._fields_)
    row_table, row_table_device = _WatchBank._table, _WatchBank._table_device

    def set_rate(self, stream, ticks_per_packet_q24, limit_q6=DEFAULT_LIMIT_Q6):
        """27 MHz ticks per 188-byte packet in Q24.24 (0: no accuracy check) and the accuracy limit in 1/64 tick"""
        self._check(self.lib.dvbs2gpu_pcr_set_rate(self.h, int(stream), int(ticks_per_packet_q24), int(limit_q6)))

    def follow_pmts(self, psi_bank, stream=0):
        """watches the PCR PIDs of the PMTs that `psi_bank` (a PsiBank that read the same stream) holds decoded, in free slots, in the
        order of its slots; 0x1FFF (a programme without a PCR) and PIDs watched already are skipped -> the PIDs that found no free slot"""
        return self._follow(psi_bank, stream, lambda hdr, es: [(hdr['pcr_pid'],)] if hdr['pcr_pid'] >= 0 else [])

    def stream_stats(self, stream=0):
        st = self._stream_stats(stream)
        return dict(packets=int(st.packets), unwatched_pcr_packets=int(st.unwatched_pcr_packets), rows_dropped=int(st.rows_dropped),
                    first_unwatched_pid=int(st.first_unwatched_pid), packets_since_pcr=[int(v) for v in st.packets_since_pcr])

    def rate(self, stream=0, slot=-1):
        """the transport-stream rate in bit/s as the slot's PCRs give it (0.0: no pairs yet)"""
        v = C.c_double()
        self._check(self.lib.dvbs2gpu_pcr_get_rate(self.h, int(stream), int(slot), C.byref(v)))
        return v.value


class PesBank(_WatchBank):
    """PES bank for `nstreams` transport streams (own extension; include/dvbs2gpu.h, PES bank): PES packet starts, PES length checks and
    PTS / DTS checks on up to 16 watched PIDs per stream, one table row per PES packet start."""
    _c, _Row, _Stats, _StreamStats = 'dvbs2gpu_pes', PesRow, PesStats, PesStreamStats
    _destroy = 'dvbs2gpu_pes_destroy'
    SLOTS = 16
    SCRAMBLED, SHORT, BAD_START, PLAIN, MALFORMED, HEADER = range(6)
    CLOSED, CLOSED_GAP, CLOSED_MISMATCH, CLOSED_UNCHECKED, UNBOUNDED_NONVIDEO = 1, 2, 4, 8, 16
    TS_FIRST, TS_BACKWARD, TS_GAP, PTS_LATE, DTS_AFTER_PTS = 32, 64, 128, 256, 512
    NO_TS = (1 << 64) - 1
    SECTION_STREAM_TYPES = (0x05, 0x0A, 0x0B, 0x0C, 0x0D, 0x86)     # private sections, DSM-CC (four types), SCTE 35: they carry sections
    ROW_KEYS = tuple(k for k, _ in PesRow._fields_)
    row_table, row_table_device = _WatchBank._table, _WatchBank._table_device

    def set_rate(self, stream, ticks_per_packet_q24):
        """27 MHz ticks per 188-byte packet in Q24.24, the PCR bank's quantity (0: no PTS_LATE)"""
        self._check(self.lib.dvbs2gpu_pes_set_rate(self.h, int(stream), int(ticks_per_packet_q24)))

    def follow_pmts(self, psi_bank, stream=0, skip_types=SECTION_STREAM_TYPES):
        """watches the elementary PIDs of the PMTs that `psi_bank` (a PsiBank that read the same stream) holds decoded, in free slots, in
        the order of its slots and then of each PMT's elementary streams; stream types that carry sections (skip_types) and PIDs watched
        already are skipped -> the PIDs that found no free slot"""
        return self._follow(psi_bank, stream, lambda hdr, es: [(pid,) for stream_type, pid in es if stream_type not in skip_types])

    def stream_stats(self, stream=0):
        st = self._stream_stats(stream)
        return dict(packets=int(st.packets), rows_dropped=int(st.rows_dropped), packets_since_start=[int(v) for v in st.packets_since_start])


class _CodecBank(_WatchBank):
    """what the watched-PID banks share that read the elementary streams of their PIDs and are told a codec per slot (csrc/es_stream.h;
    EsBank, AudBank): a larger row table by default, set_watch() with the codec, follow_pmts() by the bank's STREAM_TYPE_CODECS (PMT
    stream_type -> codec) and the row table as rows() / rows_device()."""
    STREAM_TYPE_CODECS = {}
    rows, rows_device = _WatchBank._table, _WatchBank._table_device

    def __init__(self, engine, nstreams=1, max_packets=4096, max_rows=4096):
        super().__init__(engine, nstreams, max_packets, max_rows)

    @classmethod
    def host(cls, nstreams=1, max_packets=4096, max_rows=4096):
        """a bank without a device: the library's host implementation of the same rules, behind work()"""
        return super().host(nstreams, max_packets, max_rows)

    def set_watch(self, stream, slot, pid, codec=0):
        """pid -1 clears the slot; the slot starts afresh"""
        super().set_watch(stream, slot, pid, codec)

    def follow_pmts(self, psi_bank, stream=0):
        """watches the PIDs of the PMTs that `psi_bank` (a PsiBank that read the same stream) holds decoded whose stream type the bank's
        STREAM_TYPE_CODECS names, with that codec, everything else skipped -- in free slots, in the order of its slots and then of each
        PMT's elementary streams; PIDs watched already are skipped -> the PIDs that found no free slot"""
        codecs = self.STREAM_TYPE_CODECS
        return self._follow(psi_bank, stream, lambda hdr, es: [(pid, codecs[stream_type]) for stream_type, pid in es if stream_type in codecs])

    def stream_stats(self, stream=0):
        st = self._stream_stats(stream)
        return dict(packets=int(st.packets), rows_dropped=int(st.rows_dropped))


class EsBank(_CodecBank):
    """ES bank for `nstreams` transport streams (own extension; include/dvbs2gpu.h, ES bank): every payload byte of up to 16 watched video
    PIDs per stream is scanned for start codes; one table row per PES packet start and per picture, sequence header / SPS, GOP header,
    parameter set, access unit delimiter and sequence end, with its position in the elementary stream.  follow_pmts() takes stream
    types 0x01 and 0x02 as MPEG2, 0x1B as H264, 0x24 as H265."""
    _c, _Row, _Stats, _StreamStats = 'dvbs2gpu_es', EsRow, EsStats, EsStreamStats
    _destroy = 'dvbs2gpu_es_destroy'
    SLOTS = 16
    MPEG2, H264, H265 = 1, 2, 3
    PES, PICTURE, SEQUENCE, GOP, PARAM, AUD, END = range(7)
    PIC_I, PIC_P, PIC_B = 1, 2, 3
    KEY, RESYNC, UNSYNCED, SPLIT_HEADER = 1, 2, 4, 8
    NO_TS = (1 << 64) - 1
    STREAM_TYPE_CODECS = {0x01: 1, 0x02: 1, 0x1B: 2, 0x24: 3}       # PMT stream_type -> codec
    ROW_KEYS = tuple(k for k, _ in EsRow._fields_)


class AudBank(_CodecBank):
    """Audio bank for `nstreams` transport streams (own extension; include/dvbs2gpu.h, audio bank): the frames of up to 16 watched audio
    PIDs per stream (MPEG audio, ADTS, AC-3 / E-AC-3) are followed header by header from PES payload starts on; one table row per PES
    packet start, per frame (codec sub-kind, channel mode, sample rate, samples, bitrate, size, position in the elementary stream) and
    per loss of framing.  follow_pmts() takes stream types 0x03 and 0x04 as MPA, 0x0F as ADTS, 0x81 and 0x87 as AC3; the PMT views
    carry no descriptors: DVB's AC-3 in private stream type 0x06 cannot be followed, the caller names such a PID with set_watch()."""
    _c, _Row, _Stats, _StreamStats = 'dvbs2gpu_aud', AudRow, AudStats, AudStreamStats
    _destroy = 'dvbs2gpu_aud_destroy'
    SLOTS = 16
    MPA, ADTS, AC3 = 1, 2, 3
    PES, FRAME, LOSS = range(3)
    ACQUIRED, RESYNC, UNSYNCED, SPLIT_HEADER, CHANGE = 1, 2, 4, 8, 16
    NO_TS = (1 << 64) - 1
    STREAM_TYPE_CODECS = {0x03: 1, 0x04: 1, 0x0F: 2, 0x81: 3, 0x87: 3}      # PMT stream_type -> codec
    ROW_KEYS = tuple(k for k, _ in AudRow._fields_)


class _DatagramBank(_TsBank):
    """what the banks share that deliver the payloads of the units of a PID (csrc/dgram_bank.h; MpeBank: the IP datagrams of sections,
    UleBank: of SNDUs, T2miBank: the BBFRAMEs of T2-MI packets): four slots per stream, each a watch and a reassembler of its own, one
    table row per unit, the payloads back to back.  A bank names its C prefix (_c), its row and statistics structures (_Row, _Stats)
    and the longest payload (_WORK_SLACK: what work() allows beyond the input's size) and adds layout() and set_watch()."""
    SLOTS = 4
    _c = _Row = _Stats = None
    _WORK_SLACK = 4096

    def _fn(self, name):
        return getattr(self.lib, '%s_%s' % (self._c, name))

    def __init__(self, engine, nstreams=1, max_packets=4096, max_rows=1024):
        self.eng, self.lib, self.nstreams, self.max_packets, self.max_rows = engine, engine.lib, nstreams, max_packets, max_rows
        h = C.c_void_p()
        engine._check(self._fn('create')(engine.h, nstreams, max_packets, max_rows, C.byref(h)))
        self.h = h

    @classmethod
    def host(cls, nstreams=1, max_packets=4096, max_rows=1024):
        """a bank without a device: the library's host implementation of the same rules, behind work()"""
        return cls._host(cls._c + '_create_host', nstreams=nstreams, max_packets=max_packets, max_rows=max_rows)

    def reset(self):
        self._check(self._fn('reset')(self.h))

    def process(self, ts_tensors, out_tensors=None, nbytes=None):
        """ts_tensors[i]: uint8 CUDA, whole 188-byte packets (nbytes[i] of them, default all); out_tensors: None for rows and counters
        only, else out_tensors[i][k]: the uint8 CUDA buffer that receives the datagrams (BBFRAMEs) of slot k of stream i (None for an empty slot)
        -> byte counts [i][k].  Dvbs2GpuError -5 carries .needed and .rows ([i][k] each) when a buffer or max_rows is too small
        (nothing has advanced then)."""
        n, S = self.nstreams, self.SLOTS
        pin, cnt, _, _ = self._marshal(ts_tensors, None, nbytes)
        pout, cap = None, 0
        if out_tensors is not None:
            flat = [t for per in out_tensors for t in (list(per) + [None] * S)[:S]]
            pout = (C.c_void_p * (n * S))(*[None if t is None else t.data_ptr() for t in flat])
            cap = min([int(t.numel()) for t in flat if t is not None] or [0])
        nb, nr = (C.c_int * (n * S))(), (C.c_int * (n * S))()
        rc = self._fn('process_batch')(self.h, pin, cnt, pout, cap, nb, nr, self.eng._stream())
        split = lambda a: [list(a[i * S:(i + 1) * S]) for i in range(n)]
        if rc < 0:
            e = Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
            e.needed, e.rows = split(nb), split(nr)
            raise e
        return split(nb)

    def work(self, ts, stream=0, slot=0, cap=None, deliver=True):
        """one stream and slot, host buffers: numpy uint8 packets in -> the delivered datagrams (BBFRAMEs) back to back (numpy uint8), or None with
        deliver=False (rows and counters only)"""
        import numpy as np
        ts = np.ascontiguousarray(ts, np.uint8).reshape(-1)
        cap = ts.size + self._WORK_SLACK if cap is None else cap
        out = np.zeros(max(cap, 1), np.uint8) if deliver else None
        rc = self._fn('work')(self.h, int(stream), int(slot), C.c_void_p(ts.ctypes.data), ts.size,
                              C.c_void_p(out.ctypes.data) if deliver else None, cap if deliver else 0)
        if rc < 0:
            e = Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
            nb, nr = C.c_int(), C.c_int()
            self._fn('get_needed')(self.h, int(stream), int(slot), C.byref(nb), C.byref(nr))
            e.needed, e.rows = nb.value, nr.value
            raise e
        return out[:rc].copy() if deliver else None

    def needed(self, stream=0, slot=0):
        """(bytes, rows) that the slot's last call needed, whether it succeeded or failed for capacity (bytes -1: the rows did not fit)"""
        nb, nr = C.c_int(), C.c_int()
        self._check(self._fn('get_needed')(self.h, int(stream), int(slot), C.byref(nb), C.byref(nr)))
        return nb.value, nr.value

    def stats(self, stream=0, slot=-1):
        st = self._Stats()
        self._check(self._fn('get_stats')(self.h, int(stream), int(slot), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in self._Stats._fields_}

    def row_table(self, stream=0, slot=0):
        """one dict per unit (section, SNDU, T2-MI packet) of the slot's last call (the fields of the bank's row structure; mac: six bytes), in row order"""
        rows = self._rows(self._fn('get_row_table'), self._Row, int(stream), int(slot))
        return [{k: bytes(r.mac) if k == 'mac' else int(getattr(r, k)) for k in self.ROW_KEYS} for r in rows]

    def row_table_device(self, stream=0, slot=0):
        """(device pointer or None, rows): the same table as the bank's row records in HBM, valid until the next call"""
        p, n = C.c_void_p(), C.c_int()
        self._check(self._fn('get_row_table_device')(self.h, int(stream), int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value


class T2miBank(_DatagramBank):
    """T2-MI bank for `nstreams` transport streams (own extension; include/dvbs2gpu.h, T2-MI bank): the T2-MI packets of a PID are
    reassembled, their CRC-32 and packet count checked, one table row per T2-MI packet, and the BBFRAMEs of the chosen PLP laid back
    to back in a device buffer for BbTsParserBank.process_ma.  Four slots per stream, each a (PID, PLP) pair and a reassembler of its
    own: the same PID may sit in several slots."""
    _c, _Row, _Stats = 'dvbs2gpu_t2mi', T2miRow, T2miStats
    _destroy = 'dvbs2gpu_t2mi_destroy'
    _WORK_SLACK = 8208
    SLOTS = 4
    CRC_ERROR, COUNT_ERROR, BBFRAME, INTL_FRAME_START, BAD_PAYLOAD = 1, 2, 4, 8, 16
    ROW_KEYS = tuple(k for k, _ in T2miRow._fields_)

    @staticmethod
    def layout():
        """the T2-MI syntax the library relies on (dvbs2gpu_t2mi_layout) as a dict"""
        lay = T2miLayout()
        load_library().dvbs2gpu_t2mi_get_layout(C.byref(lay))
        return {k: int(getattr(lay, k)) for k, _ in T2miLayout._fields_}

    def set_watch(self, stream, slot, pid, plp=-1):
        """pid -1 empties the slot; plp -1: every PLP; the slot starts afresh"""
        self._check(self.lib.dvbs2gpu_t2mi_set_watch(self.h, int(stream), int(slot), int(pid), int(plp)))

    def frame_bytes(self, stream=0, slot=0):
        """the sizes of the BBFRAMEs that the slot's last call delivered, in order: with the slot's output buffer, the frame_bytes and
        nframes of BbTsParserBank.process_ma"""
        return [int(v) for v in self._rows(self.lib.dvbs2gpu_t2mi_get_frame_bytes, C.c_int, int(stream), int(slot))]


class MpeBank(_DatagramBank):
    """MPE bank for `nstreams` transport streams (own extension; include/dvbs2gpu.h, MPE bank): the DSM-CC datagram_sections of a PID are
    reassembled, their CRC-32 checked, a MAC filter applied and the IPv4 / IPv6 header behind the MPE header (and LLC/SNAP) checked, one
    table row per section, and the IP datagrams laid back to back in a device buffer.  Four slots per stream, each a (PID, MAC value,
    MAC mask) and a reassembler of its own: the same PID may sit in several slots."""
    _c, _Row, _Stats = 'dvbs2gpu_mpe', MpeRow, MpeStats
    _destroy = 'dvbs2gpu_mpe_destroy'
    SLOTS = 4
    OTHER_TABLE, MALFORMED, CRC_ERROR, UNCHECKED, SCRAMBLED, FILTERED, FRAGMENT, OTHER_PROTOCOL, BAD_IP, DATAGRAM = (1 << k for k in range(10))
    DSMCC_STREAM_TYPES = (0x0A, 0x0D)                                # multi-protocol encapsulation, DSM-CC sections
    ROW_KEYS = tuple(k for k, _ in MpeRow._fields_)

    def __init__(self, engine, nstreams=1, max_packets=4096, max_rows=1024):
        super().__init__(engine, nstreams, max_packets, max_rows)
        self._watched = [{} for _ in range(nstreams)]               # per stream: slot -> PID, as set_watch left them

    @classmethod
    def host(cls, nstreams=1, max_packets=4096, max_rows=1024):
        """a bank without a device: the library's host implementation of the same rules, behind work()"""
        self = super().host(nstreams, max_packets, max_rows)
        self._watched = [{} for _ in range(nstreams)]
        return self

    @staticmethod
    def layout():
        """the section and IP syntax the library relies on (dvbs2gpu_mpe_layout) as a dict; mac_at: a list of six"""
        lay = MpeLayout()
        load_library().dvbs2gpu_mpe_get_layout(C.byref(lay))
        return {k: [int(v) for v in getattr(lay, k)] if k == 'mac_at' else int(getattr(lay, k)) for k, _ in MpeLayout._fields_}

    def set_watch(self, stream, slot, pid, mac=None, mask=None):
        """pid -1 empties the slot; mac / mask: six bytes each in network order (None: all zero; an all-zero mask takes every address);
        the slot starts afresh"""
        six = lambda v: None if v is None else (C.c_uint8 * 6)(*bytes(v))
        if any(v is not None and len(bytes(v)) != 6 for v in (mac, mask)):
            raise ValueError('a MAC address or mask has six bytes')
        self._check(self.lib.dvbs2gpu_mpe_set_watch(self.h, int(stream), int(slot), int(pid), six(mac), six(mask)))
        self._watched[int(stream)].pop(int(slot), None)
        if pid >= 0:
            self._watched[int(stream)][int(slot)] = int(pid)

    def follow_pmts(self, psi_bank, stream=0, stream_types=DSMCC_STREAM_TYPES):
        """watches the elementary PIDs with one of `stream_types` in the PMTs that `psi_bank` (a PsiBank that read the same stream) holds
        decoded, in free slots and with no MAC filter, in the order of its slots and then of each PMT's elementary streams; PIDs watched
        already are skipped -> the PIDs that found no free slot.  The PMT views carry no descriptors, so a data_broadcast_id is not
        looked at: an object-carousel PID caught this way only yields OTHER_TABLE rows."""
        watched = self._watched[int(stream)]
        left = []
        for slot in range(psi_bank.SLOTS):
            hdr, es = psi_bank.program_map(stream, slot)
            if hdr['program_number'] < 0:
                continue
            for stream_type, pid in es:
                if stream_type not in stream_types or pid >= 0x1FFF or pid in watched.values() or pid in left:
                    continue
                free = [s for s in range(self.SLOTS) if s not in watched]
                if free:
                    self.set_watch(stream, free[0], pid)
                else:
                    left.append(pid)
        return left


class UleBank(_DatagramBank):
    """ULE bank for `nstreams` transport streams (own extension; include/dvbs2gpu.h, ULE bank): the SNDUs of a PID (Unidirectional
    Lightweight Encapsulation, RFC 4326) are reassembled, their CRC-32 checked, a filter on the destination NPA address applied,
    optional extension headers and a bridged frame's MAC header followed and the IPv4 / IPv6 header behind them checked, one table row
    per SNDU, and the IP datagrams laid back to back in a device buffer.  Four slots per stream, each a (PID, NPA value, NPA mask,
    accept_unaddressed) and a reassembler of its own: the same PID may sit in several slots.  There is no follow_pmts: ULE has no
    dependable PMT signalling, the caller names the PID."""
    _c, _Row, _Stats = 'dvbs2gpu_ule', UleRow, UleStats
    _destroy = 'dvbs2gpu_ule_destroy'
    SLOTS = 4
    MALFORMED, CRC_ERROR, FILTERED, NO_ADDRESS, TEST, BRIDGED, EXTENSION, OTHER_PROTOCOL, BAD_IP, DATAGRAM = (1 << k for k in range(10))
    ROW_KEYS = tuple(k for k, _ in UleRow._fields_)

    @staticmethod
    def layout():
        """the SNDU and IP syntax the library relies on (dvbs2gpu_ule_layout) as a dict"""
        lay = UleLayout()
        load_library().dvbs2gpu_ule_get_layout(C.byref(lay))
        return {k: int(getattr(lay, k)) for k, _ in UleLayout._fields_}

    def set_watch(self, stream, slot, pid, npa=None, mask=None, accept_unaddressed=False):
        """pid -1 empties the slot; npa / mask: six bytes each (None: all zero; an all-zero mask takes every address);
        accept_unaddressed: SNDUs without a destination address (D = 1) pass the filter; the slot starts afresh"""
        six = lambda v: None if v is None else (C.c_uint8 * 6)(*bytes(v))
        if any(v is not None and len(bytes(v)) != 6 for v in (npa, mask)):
            raise ValueError('an NPA address or mask has six bytes')
        self._check(self.lib.dvbs2gpu_ule_set_watch(self.h, int(stream), int(slot), int(pid), six(npa), six(mask), int(bool(accept_unaddressed))))


class IpTsBank(_TsBank):
    """IP-TS bank for `nstreams` streams (own extension; include/dvbs2gpu.h, IP-TS bank): among the IP datagrams that an MpeBank, a
    UleBank or a GSE path left in HBM with one table row each, the UDP datagrams of up to four flows (family, destination address,
    destination port) per stream have their UDP checksum verified, their payload recognised as raw TS or RTP/MP2T and an RTP sequence
    rule applied; one row per input row, and the TS packets of each flow slot back to back in a device buffer that TsMonitorBank,
    PsiBank, PcrBank, PesBank and T2miBank take as input.  The input is a view (IptsView): view_from_mpe / view_from_ule /
    view_from_pdu_table / view_from_ma_pdu_table build it from the source bank's table in HBM."""
    _destroy = 'dvbs2gpu_ipts_destroy'
    SLOTS = 4
    KIND_RAW_IP, KIND_GRE = 0, 1
    (NOT_DELIVERED, NOT_IP, BAD_IP, FRAGMENT, OTHER_PROTOCOL, BAD_UDP, UNWATCHED, BAD_CHECKSUM, NO_CHECKSUM, BAD_PAYLOAD, OTHER_PAYLOAD, RAW, RTP, NEW_SOURCE, LOSS,
     LATE, TS) = (1 << k for k in range(17))
    ROW_KEYS = tuple(k for k, _ in IptsRow._fields_ if k != 'reserved')

    def __init__(self, engine, nstreams=1, max_rows=1024):
        self.eng, self.lib, self.nstreams, self.max_rows = engine, engine.lib, nstreams, max_rows
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_ipts_create(engine.h, nstreams, max_rows, C.byref(h)))
        self.h = h

    @classmethod
    def host(cls, nstreams=1, max_rows=1024):
        """a bank without a device: the library's host implementation of the same rules, behind work()"""
        return cls._host('dvbs2gpu_ipts_create_host', nstreams=nstreams, max_rows=max_rows)

    @staticmethod
    def layout():
        """the UDP, RTP and TS syntax the library relies on (dvbs2gpu_ipts_layout) as a dict"""
        lay = IptsLayout()
        load_library().dvbs2gpu_ipts_get_layout(C.byref(lay))
        return {k: int(getattr(lay, k)) for k, _ in IptsLayout._fields_}

    def reset(self):
        self._check(self.lib.dvbs2gpu_ipts_reset(self.h))

    def set_flow(self, stream, slot, family, addr=None, port=0):
        """family 4 or 6 with the destination address (4 or 16 bytes, network order) and UDP port; family 0 empties the slot; the slot's
        counters and RTP state start afresh"""
        a = None
        if family:
            if addr is None or len(bytes(addr)) != (4 if family == 4 else 16):
                raise ValueError('an IPv4 address has four bytes, an IPv6 address sixteen')
            a = (C.c_uint8 * 16)(*bytes(addr))
        self._check(self.lib.dvbs2gpu_ipts_set_flow(self.h, int(stream), int(slot), int(family), a, int(port)))

    # ---- views
    @staticmethod
    def _view(data_ptr, rows_ptr, n, Row, kind):
        return IptsView(data_ptr if n else None, rows_ptr if n else None, C.sizeof(Row), getattr(Row, 'offset').offset, getattr(Row, 'bytes').offset, kind, n, 0)

    @classmethod
    def _view_from_datagram_bank(cls, bank, out_tensor, stream, slot):
        p, n = bank.row_table_device(stream, slot)
        return cls._view(out_tensor.data_ptr(), p, n, bank._Row, cls.KIND_RAW_IP), out_tensor

    @classmethod
    def view_from_mpe(cls, bank, out_tensor, stream=0, slot=0):
        """(view, out_tensor): the datagrams of (stream, slot) of an MpeBank's last process() call, which wrote them into out_tensor"""
        return cls._view_from_datagram_bank(bank, out_tensor, stream, slot)

    @classmethod
    def view_from_ule(cls, bank, out_tensor, stream=0, slot=0):
        """(view, out_tensor): the datagrams of (stream, slot) of a UleBank's last process() call, which wrote them into out_tensor"""
        return cls._view_from_datagram_bank(bank, out_tensor, stream, slot)

    @classmethod
    def view_from_pdu_table(cls, bank, out_tensor, stream=0):
        """(view, out_tensor): the GRE packets of a stream of a BbTsParserBank's last process_batch() call (GSE frames), kind GRE"""
        p, n = bank.pdu_table_device(stream)
        return cls._view(out_tensor.data_ptr(), p, n, GsePdu, cls.KIND_GRE), out_tensor

    @classmethod
    def view_from_ma_pdu_table(cls, bank, out_tensor, stream=0, slot=0):
        """(view, out_tensor): the GRE packets of an ISI lane of a BbTsParserBank's last mode-adaptation call (GSE frames), kind GRE"""
        p, n = bank.ma_pdu_table_device(stream, slot)
        return cls._view(out_tensor.data_ptr(), p, n, GsePdu, cls.KIND_GRE), out_tensor

    @classmethod
    def view_from_ipout(cls, bank, out_tensor, stream=0, slot=0):
        """(view, out_tensor): the datagrams of (stream, slot) of an IpOutBank's last process() call, which wrote them into out_tensor"""
        p, n = bank.row_table_device(stream, slot)
        return cls._view(out_tensor.data_ptr(), p, n, IpoutRow, cls.KIND_RAW_IP), out_tensor

    # ---- calls
    def process(self, views, out_tensors=None):
        """views[i]: the IptsView of stream i (None: no row), device pointers; out_tensors: None for rows and counters only, else
        out_tensors[i][k]: the uint8 CUDA buffer that receives the TS packets of slot k of stream i (None for an empty slot) -> byte
        counts [i][k].  Dvbs2GpuError -5 carries .needed ([i][k]) when a buffer is too small (nothing has advanced then)."""
        n, S = self.nstreams, self.SLOTS
        va = (IptsView * n)(*[IptsView() if v is None else v for v in views])
        pout, cap = None, 0
        if out_tensors is not None:
            flat = [t for per in out_tensors for t in (list(per) + [None] * S)[:S]]
            pout = (C.c_void_p * (n * S))(*[None if t is None else t.data_ptr() for t in flat])
            cap = min([int(t.numel()) for t in flat if t is not None] or [0])
        nb, nr = (C.c_int * (n * S))(), (C.c_int * n)()
        rc = self.lib.dvbs2gpu_ipts_process_batch(self.h, va, pout, cap, nb, nr, self.eng._stream())
        split = lambda a: [list(a[i * S:(i + 1) * S]) for i in range(n)]
        if rc < 0:
            e = Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
            e.needed = split(nb)
            raise e
        return split(nb)

    def work(self, data, table, kind=0, stream=0, cap=None, deliver=True):
        """one stream, host buffers: data: numpy uint8 datagram bytes; table: (offset, bytes) per datagram -> the TS packets of the four
        slots (a list of numpy uint8), or None with deliver=False (rows and counters only)"""
        import numpy as np
        data = np.ascontiguousarray(data, np.uint8).reshape(-1)
        tab = np.ascontiguousarray(np.asarray(table, np.int32).reshape(-1, 2))
        v = IptsView(C.c_void_p(data.ctypes.data) if len(tab) else None, C.c_void_p(tab.ctypes.data) if len(tab) else None, 8, 0, 4, int(kind), len(tab), 0)
        S = self.SLOTS
        cap = data.size if cap is None else cap
        outs = [np.zeros(max(cap, 1), np.uint8) for _ in range(S)] if deliver else None
        pout = (C.c_void_p * S)(*[o.ctypes.data for o in outs]) if deliver else None
        nb = (C.c_int * S)()
        rc = self.lib.dvbs2gpu_ipts_work(self.h, int(stream), C.byref(v), pout, cap if deliver else 0, nb)
        if rc < 0:
            e = Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
            e.needed = list(nb)
            raise e
        return [o[:k].copy() for o, k in zip(outs, nb)] if deliver else None

    def needed(self, stream=0, slot=0):
        """the bytes that the slot's last call needed, whether it succeeded or failed for capacity"""
        nb = C.c_int()
        self._check(self.lib.dvbs2gpu_ipts_get_needed(self.h, int(stream), int(slot), C.byref(nb)))
        return nb.value

    def stats(self, stream=0, slot=-1):
        """a slot's counters; slot -1: the stream's own counters and the sum over its slots"""
        st = IptsStats()
        self._check(self.lib.dvbs2gpu_ipts_get_stats(self.h, int(stream), int(slot), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in IptsStats._fields_}

    def row_table(self, stream=0):
        """one dict per input row of the stream's last call (the fields of dvbs2gpu_ipts_row), in row order"""
        rows = self._rows(self.lib.dvbs2gpu_ipts_get_row_table, IptsRow, int(stream))
        return [{k: int(getattr(r, k)) for k in self.ROW_KEYS} for r in rows]

    def row_table_device(self, stream=0):
        """(device pointer or None, rows): the same table as dvbs2gpu_ipts_row records in HBM, valid until the next call"""
        p, n = C.c_void_p(), C.c_int()
        self._check(self.lib.dvbs2gpu_ipts_get_row_table_device(self.h, int(stream), C.byref(p), C.byref(n)))
        return p.value, n.value


class IpOutBank(_TsBank):
    """IP output bank for `nstreams` transport streams (own extension; include/dvbs2gpu.h, IP output bank): the packets of up to four
    flow slots per stream, selected by PID, leave as UDP or RTP/MP2T datagrams with complete IPv4 / IPv6, UDP and RTP headers and
    checksums, back to back per slot in a device buffer with one table row each.  It is IpTsBank's direction reversed:
    IpTsBank.view_from_ipout reads the result back."""
    _destroy = 'dvbs2gpu_ipout_destroy'
    SLOTS = 4
    MODE_RAW, MODE_RTP = 0, 1
    PASS_ALL, PASS_LISTED, DROP_LISTED = 0, 1, 2
    RTP, SHORT, CARRIED = 1, 2, 4
    ROW_KEYS = tuple(k for k, _ in IpoutRow._fields_ if k != 'reserved')

    def __init__(self, engine, nstreams=1, max_packets=4096):
        self.eng, self.lib, self.nstreams, self.max_packets = engine, engine.lib, nstreams, max_packets
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_ipout_create(engine.h, nstreams, max_packets, C.byref(h)))
        self.h = h

    @classmethod
    def host(cls, nstreams=1, max_packets=4096):
        """a bank without a device: the library's host implementation of the same rules, behind work()"""
        return cls._host('dvbs2gpu_ipout_create_host', nstreams=nstreams, max_packets=max_packets)

    @staticmethod
    def layout():
        """what the library's headers rely on beyond IpTsBank.layout() (dvbs2gpu_ipout_layout) as a dict"""
        lay = IpoutLayout()
        load_library().dvbs2gpu_ipout_get_layout(C.byref(lay))
        return {k: int(getattr(lay, k)) for k, _ in IpoutLayout._fields_}

    def reset(self):
        self._check(self.lib.dvbs2gpu_ipout_reset(self.h))

    def set_flow(self, stream, slot, family=0, src=None, dst=None, src_port=0, dst_port=0, ttl=64, dscp=0, mode=1, ssrc=0, seq_base=0, timestamp_base=0,
                 packets_per_datagram=7, pid_mode=0, pids=(), drop_null=False):
        """family 4 or 6 with source and destination address (4 or 16 bytes, network order); family 0 empties the slot.  pids: the list of
        pid_mode 1 (pass listed) and 2 (drop listed).  The slot's counters, held packets and RTP sequence start afresh."""
        f = IpoutFlow()
        if family:
            if any(a is None or len(bytes(a)) != (4 if family == 4 else 16) for a in (src, dst)):
                raise ValueError('an IPv4 address has four bytes, an IPv6 address sixteen')
            for k, v in (('family', family), ('src_port', src_port), ('dst_port', dst_port), ('ttl', ttl), ('mode', mode), ('ssrc', ssrc), ('seq_base', seq_base),
                         ('timestamp_base', timestamp_base), ('pid_mode', pid_mode), ('drop_null', bool(drop_null))):
                setattr(f, k, int(v))
            # (out of range for their bytes: the library refuses 255)
            f.dscp, f.packets_per_datagram = min(max(int(dscp), 0), 255), min(max(int(packets_per_datagram), 0), 255)
            f.src_addr[:len(bytes(src))] = list(bytes(src))
            f.dst_addr[:len(bytes(dst))] = list(bytes(dst))
        if any(not 0 <= int(p) <= 0xFFFF for p in pids):
            raise ValueError('a PID is a 13-bit number')
        a = (C.c_uint16 * max(len(pids), 1))(*[int(p) for p in pids])
        self._check(self.lib.dvbs2gpu_ipout_set_flow(self.h, int(stream), int(slot), C.byref(f), a, len(pids)))

    def set_rate(self, stream, ticks_per_packet_q24):
        """27 MHz ticks per packet in Q24.24 (PcrBank.set_rate's quantity); 0: not set"""
        self._check(self.lib.dvbs2gpu_ipout_set_rate(self.h, int(stream), int(ticks_per_packet_q24)))

    def process(self, ts_tensors, out_tensors, nbytes=None, flush=False):
        """ts_tensors[i]: uint8 CUDA, whole 188-byte packets (nbytes[i] of them, default all); out_tensors[i][k]: the uint8 CUDA buffer
        that receives the datagrams of slot k of stream i (None for an empty slot) -> byte counts [i][k].  Dvbs2GpuError -5 carries
        .needed ([i][k]) when a buffer is too small (nothing has advanced then)."""
        n, S = self.nstreams, self.SLOTS
        pin = (C.c_void_p * n)(*[t.data_ptr() if t is not None and t.numel() else None for t in ts_tensors])
        cnt = (C.c_int * n)(*[(0 if t is None else int(t.numel())) if nbytes is None else int(nbytes[i]) for i, t in enumerate(ts_tensors)])
        flat = [t for per in out_tensors for t in (list(per) + [None] * S)[:S]]
        pout = (C.c_void_p * (n * S))(*[None if t is None else t.data_ptr() for t in flat])
        cap = min([int(t.numel()) for t in flat if t is not None] or [0])
        nb, nr = (C.c_int * (n * S))(), (C.c_int * (n * S))()
        rc = self.lib.dvbs2gpu_ipout_process_batch(self.h, pin, cnt, pout, cap, nb, nr, int(bool(flush)), self.eng._stream())
        split = lambda a: [list(a[i * S:(i + 1) * S]) for i in range(n)]
        if rc < 0:
            e = Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
            e.needed = split(nb)
            raise e
        return split(nb)

    def work(self, ts, stream=0, cap=None, flush=False):
        """one stream, host buffers: numpy uint8 packets in -> the datagrams of the four slots (a list of numpy uint8)"""
        import numpy as np
        ts = np.ascontiguousarray(ts, np.uint8).reshape(-1)
        S = self.SLOTS
        cap = (ts.size // 188 + 7) * (188 + 60) if cap is None else cap
        outs = [np.zeros(max(cap, 1), np.uint8) for _ in range(S)]
        pout = (C.c_void_p * S)(*[o.ctypes.data for o in outs])
        nb = (C.c_int * S)()
        rc = self.lib.dvbs2gpu_ipout_work(self.h, int(stream), C.c_void_p(ts.ctypes.data) if ts.size else None, ts.size, pout, cap, nb, int(bool(flush)))
        if rc < 0:
            e = Dvbs2GpuError(rc, self.lib.dvbs2gpu_last_error().decode())
            e.needed = list(nb)
            raise e
        return [o[:k].copy() for o, k in zip(outs, nb)]

    def needed(self, stream=0, slot=0):
        """the bytes that the slot's last call needed, whether it succeeded or failed for capacity"""
        nb = C.c_int()
        self._check(self.lib.dvbs2gpu_ipout_get_needed(self.h, int(stream), int(slot), C.byref(nb)))
        return nb.value

    def stats(self, stream=0, slot=-1):
        """a slot's counters; slot -1: the stream's own counters and the sum over its slots"""
        st = IpoutStats()
        self._check(self.lib.dvbs2gpu_ipout_get_stats(self.h, int(stream), int(slot), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in IpoutStats._fields_}

    def row_table(self, stream=0, slot=0):
        """one dict per datagram of the slot's last call (the fields of dvbs2gpu_ipout_row), in output order"""
        rows = self._rows(self.lib.dvbs2gpu_ipout_get_row_table, IpoutRow, int(stream), int(slot))
        return [{k: int(getattr(r, k)) for k in self.ROW_KEYS} for r in rows]

    def row_table_device(self, stream=0, slot=0):
        """(device pointer or None, rows): the same table as dvbs2gpu_ipout_row records in HBM, valid until the next call"""
        p, n = C.c_void_p(), C.c_int()
        self._check(self.lib.dvbs2gpu_ipout_get_row_table_device(self.h, int(stream), int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value


class SegmentReceiver(_Handle):
    """One fast transponder on the many-stream engine: a long chunk of one continuous IQ stream is cut into overlapping segments
    that run as independent streams and are stitched back in order (include/dvbs2gpu.h, segment receiver)."""
    _destroy = 'dvbs2gpu_segrx_destroy'

    def __init__(self, engine, cfg, nsegments, own_frames, warm_frames):
        self.eng, self.lib = engine, engine.lib
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_segrx_create(engine.h, C.byref(cfg), nsegments, own_frames, warm_frames, C.byref(h)))
        self.h = h
        self.chunk_samples = int(self.lib.dvbs2gpu_segrx_chunk_samples(self.h))

    def reset(self):
        self.eng._check(self.lib.dvbs2gpu_segrx_reset(self.h))

    def process(self, iq, out):
        """iq: complex64 CUDA 1-D (continues the stream), out: uint8 CUDA buffer -> bytes written"""
        return self.eng._check(self.lib.dvbs2gpu_segrx_process(self.h, C.c_void_p(iq.data_ptr()), int(iq.numel()), C.c_void_p(out.data_ptr()), int(out.numel())))

    def stats(self):
        a = (C.c_int32 * 3)()
        self.eng._check(self.lib.dvbs2gpu_segrx_get_stats(self.h, a))
        return {'sightings': a[0], 'returned': a[1], 'warmup_only': a[2]}


class DvbsSegmentReceiver(_Handle):
    """One fast DVB-S carrier: overlapping segments through the receiver bank, decoded bit streams joined in order
    (include/dvbs2gpu.h, DVB-S segment receiver)."""
    _destroy = 'dvbs2gpu_dvbs_segrx_destroy'

    def __init__(self, engine, nsegments, own_symbols, warm_symbols, **kw):
        self.eng, self.lib = engine, engine.lib
        self.cfg = DvbsCfg()
        self.lib.dvbs2gpu_dvbs_demod_default_cfg(C.byref(self.cfg))
        for k, v in kw.items():
            setattr(self.cfg, k, v)
        h = C.c_void_p()
        engine._check(self.lib.dvbs2gpu_dvbs_segrx_create(engine.h, C.byref(self.cfg), nsegments, own_symbols, warm_symbols, C.byref(h)))
        self.h = h
        self.chunk_samples = int(self.lib.dvbs2gpu_dvbs_segrx_chunk_samples(self.h))

    def reset(self):
        self.eng._check(self.lib.dvbs2gpu_dvbs_segrx_reset(self.h))

    def process(self, iq, out):
        """iq: complex64 CUDA 1-D (continues the stream), out: uint8 CUDA buffer -> number of bits written (one per byte)"""
        return self.eng._check(self.lib.dvbs2gpu_dvbs_segrx_process(self.h, C.c_void_p(iq.data_ptr()), int(iq.numel()), C.c_void_p(out.data_ptr()), int(out.numel())))

    def stats(self):
        a = (C.c_int32 * 4)()
        self.eng._check(self.lib.dvbs2gpu_dvbs_segrx_get_stats(self.h, a))
        return {'segments': a[0], 'matched': a[1], 'unmatched': a[2], 'bits': a[3]}
