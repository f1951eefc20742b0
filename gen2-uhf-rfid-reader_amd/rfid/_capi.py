"""ctypes binding of librfid_mi355x.so (include/rfid_mi355x.h).

The library is the product: there is no Python or CPU implementation of the receive
path behind it.  If the shared object is missing or no gfx950 GPU is usable, loading /
context creation raises RfidError -- nothing falls back.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.path.join(PKG_ROOT, "lib", "librfid_mi355x.so")
HEADER_PATH = os.path.join(REPO_ROOT, "include", "rfid_mi355x.h")

# enums (include/rfid_mi355x.h; numeric values of gr-rfid/include/rfid/global_vars.h:31-34)
RUNNING, TERMINATED = 0, 1
(SEND_QUERY, SEND_ACK, SEND_QUERY_REP, IDLE, SEND_CW, START, SEND_QUERY_ADJUST, SEND_NAK_QR,
 SEND_NAK_Q, POWER_DOWN) = range(10)
GATE_OPEN, GATE_CLOSED, GATE_SEEK_RN16, GATE_SEEK_EPC = range(4)
DECODE_RN16, DECODE_EPC = 0, 1

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED, ERR_CAPACITY, ERR_STATE = 0, -1, -2, -3, -4, -5, -6


class RfidError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"rfid_mi355x status {status}: {msg}")
        self.status = status


class Params(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("decim", C.c_int32), ("n_taps", C.c_int32),
                ("fixed_q", C.c_int32), ("max_num_queries", C.c_int32), ("number_unique_tags", C.c_int32)]


class ReaderState(C.Structure):
    _fields_ = [("status", C.c_int32), ("gen2_logic_status", C.c_int32), ("gate_status", C.c_int32),
                ("decoder_status", C.c_int32), ("n_samples_to_ungate", C.c_int32),
                ("n_queries_sent", C.c_int32), ("cur_inventory_round", C.c_int32),
                ("cur_slot_number", C.c_int32), ("max_slot_number", C.c_int32), ("n_epc_correct", C.c_int32),
                ("n_unique_tags", C.c_int32), ("tag_reads", C.c_int32 * 256)]


class SynthGen2Params(C.Structure):
    _fields_ = [("leak_re", C.c_float), ("leak_im", C.c_float), ("h_re", C.c_float * 16), ("h_im", C.c_float * 16),
                ("n_tags", C.c_int32), ("tail_us", C.c_int32)]


class LsReport(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("pieces", "units", "chunk", "avg_rounds", "avg_reruns", "fsm_rounds", "dc_rounds",
                                         "dc_reruns", "verified", "gave_up", "cuts_dropped", "windows", "dc_finished")]


class BatchTiming(C.Structure):
    _fields_ = [("mf_ms", C.c_float), ("gate_ms", C.c_float), ("decode_ms", C.c_float),
                ("stats_ms", C.c_float), ("total_ms", C.c_float), ("front_ms", C.c_float),
                ("front_chunks", C.c_int32), ("decode_launches", C.c_int32),
                ("fused_front", C.c_int32), ("reserved_", C.c_int32)]


WINDOW_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("start", "<i4"), ("type", "<i4"),
                         ("dc_re", "<f4"), ("dc_im", "<f4")])
RESULT_DTYPE = np.dtype([("type", "<i4"), ("index", "<i4"), ("h_re", "<f4"), ("h_im", "<f4"), ("T", "<f4"),
                         ("bits", "<u4", (4,)), ("n_bits", "<i4"), ("crc_ok", "<i4"), ("tag_id", "<i4")])
SCORES_DTYPE = np.dtype([("corr", "<f4", (15,)), ("energy", "<f4", (20,)), ("pad_", "<f4")])
STATS_DTYPE = np.dtype([("n_queries_sent", "<i4"), ("cur_inventory_round", "<i4"), ("cur_slot_number", "<i4"),
                        ("n_epc_correct", "<i4"), ("n_unique_tags", "<i4"), ("n_windows", "<i4"),
                        ("n_windows_used", "<i4"), ("status", "<i4"), ("tag_reads", "<i4", (256,))])
STREAM_WINDOW_DTYPE = np.dtype([("start", "<i8"), ("type", "<i4"), ("reserved_", "<i4"), ("dc_re", "<f4"), ("dc_im", "<f4")])
TAG_ENTRY_DTYPE = np.dtype([("stream", "<i4"), ("reads", "<i4"), ("frame", "<u4", (4,)), ("first_seq", "<i4"),
                            ("last_seq", "<i4"), ("best_seq", "<i4"), ("best_h_re", "<f4"), ("best_h_im", "<f4"),
                            ("tag_id", "<i4")])
TAG_READ_DTYPE = np.dtype([("stream", "<i4"), ("entry", "<i4"), ("seq", "<i4"), ("start", "<i4"), ("h_re", "<f4"),
                           ("h_im", "<f4"), ("T", "<f4"), ("index", "<i4")])
assert STREAM_WINDOW_DTYPE.itemsize == 24 and TAG_ENTRY_DTYPE.itemsize == 48
QUALITY_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("sig_abs", "<f4"), ("sig_sq", "<f4"), ("quad_sq", "<f4"),
                          ("margin_min", "<f4"), ("margin_bit", "<i4"), ("flags", "<i4")])
assert TAG_READ_DTYPE.itemsize == 32 and QUALITY_DTYPE.itemsize == 32
REPAIR_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("start", "<i4"), ("flags", "<i4"), ("n_flips", "<i4"),
                         ("flips", "<i4"), ("cost", "<f4"), ("entry", "<i4"), ("frame", "<u4", (4,))])
REPAIR_CANDIDATES, REPAIR_MAX_FLIPS = 8, 3
assert REPAIR_DTYPE.itemsize == 48
MOMENTS_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("sx", "<f4"), ("sy", "<f4"), ("sxx", "<f4"), ("sxy", "<f4"),
                          ("syy", "<f4"), ("flags", "<i4")])
MOMENTS_SAMPLES = 240
assert MOMENTS_DTYPE.itemsize == 32
COMMAND_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("cmd", "<i4"), ("n_edges", "<i4"), ("n_syms", "<i4"), ("end", "<i4"),
                          ("d0", "<i4"), ("rtcal", "<i4"), ("trcal", "<i4"), ("n_bits", "<i4"), ("bits", "<u4"), ("flags", "<i4")])
CMD_SPAN, CMD_MAX_EDGES, CMD_GAP = 704, 64, 120
CMD_NONE, CMD_QUERY, CMD_QUERY_REP, CMD_ACK, CMD_NAK, CMD_QUERY_ADJUST, CMD_UNKNOWN = range(7)
assert COMMAND_DTYPE.itemsize == 48
FINE_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("start", "<i4"), ("flags", "<i4"), ("sum_re", "<f4"), ("sum_im", "<f4"),
                       ("pow", "<f4"), ("reserved_", "<i4"), ("seg_re", "<f4", (8,)), ("seg_im", "<f4", (8,)), ("seg_pow", "<f4", (8,))])
FINE_SEGMENTS, FINE_SEGMENT_BITS = 8, 16
assert FINE_DTYPE.itemsize == 128
RETUNE_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("start", "<i4"), ("flags", "<i4"), ("t_index", "<i4"), ("T", "<f4"),
                         ("h_re", "<f4"), ("h_im", "<f4"), ("energy", "<f4"), ("frame", "<u4", (4,)), ("reserved_", "<i4", (3,))])
RETUNE_SPAN, RETUNE_CANDIDATES = 1408, 81
assert RETUNE_DTYPE.itemsize == 64
COLLISION_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("flags", "<i4"), ("n_same", "<i4"), ("n_diff", "<i4"), ("rn16_a", "<i4"),
                            ("rn16_b", "<i4"), ("ha_re", "<f4"), ("ha_im", "<f4"), ("hb_re", "<f4"), ("hb_im", "<f4"), ("resid", "<f4"),
                            ("sum_sq", "<f4"), ("c_re", "<f4"), ("c_im", "<f4"), ("reserved_", "<i4")])
RN16_WINDOW = 250         # the gated samples of an RN16 window
assert COLLISION_DTYPE.itemsize == 64
SIZED_FRAME_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("start", "<i4"), ("flags", "<i4"), ("words", "<i4"), ("n_bits", "<i4"),
                              ("crc_rcvd", "<i4"), ("crc_calc", "<i4"), ("frame", "<u4", (5,)), ("reserved_", "<i4", (3,))])
LENGTHS_SPAN, LENGTHS_MAX_WORDS = 1728, 8
assert SIZED_FRAME_DTYPE.itemsize == 64
DIVERSITY_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("start", "<i4"), ("flags", "<i4"), ("present", "<i4"), ("reads", "<i4"),
                            ("frame", "<u4", (4,)), ("crc_rcvd", "<i4"), ("crc_calc", "<i4"), ("h_sq", "<f4"), ("margin_min", "<f4"),
                            ("weakest", "<i4"), ("reserved_", "<i4")])
DIVERSITY_MAX_MEMBERS, DIVERSITY_SLACK = 8, 4
assert DIVERSITY_DTYPE.itemsize == 64
MATCH_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("start", "<i4"), ("flags", "<i4"), ("n_cand", "<i4"), ("best", "<i4"),
                        ("second", "<i4"), ("score_best", "<f4"), ("score_second", "<f4"), ("sig_abs", "<f4"), ("dist_best", "<i4"),
                        ("diff", "<i4"), ("frame", "<u4", (4,))])
MATCH_MAX_LIST = 1024
assert MATCH_DTYPE.itemsize == 64
STACK_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("start", "<i4"), ("flags", "<i4"), ("ordinal", "<i4"), ("n_partners", "<i4"),
                        ("member_mask", "<u8"), ("sig_abs", "<f4"), ("margin_min", "<f4"), ("weakest", "<i4"), ("reserved_", "<i4"),
                        ("frame", "<u4", (4,))])
STACK_BLOCK, STACK_MAX_WINDOWS = 64, 64
assert STACK_DTYPE.itemsize == 64
GATE_FSM_IN_DTYPE = np.dtype([("mode", "<i4"), ("n_samples", "<i4"), ("signal_state", "<i4"), ("num_pulses", "<i4"),
                              ("gate_open", "<i4"), ("n_to_ungate", "<i4"), ("wtype", "<i4"), ("nvalid", "<i4"), ("pos", "<i4"),
                              ("reserved_", "<i4"), ("below", "<u8"), ("above", "<u8")])
GATE_FSM_OUT_DTYPE = np.dtype([("n_samples", "<i4"), ("signal_state", "<i4"), ("num_pulses", "<i4"), ("gate_open", "<i4"),
                               ("n_to_ungate", "<i4"), ("wtype", "<i4"), ("nvalid", "<i4"), ("stop", "<i4"), ("consumed", "<i4"),
                               ("open_lane", "<i4"), ("open_type", "<i4"), ("reserved_", "<i4"), ("closedmask", "<u8"),
                               ("openmask", "<u8")])
assert GATE_FSM_IN_DTYPE.itemsize == 56 and GATE_FSM_OUT_DTYPE.itemsize == 64
# rfid_selftest_arith: the operands of one wave, and what every arithmetic primitive made of them
ARITH_IN_DTYPE = np.dtype([("carry", "<f4"), ("carry_b", "<f4"), ("fill", "<i4"), ("reserved_", "<i4"), ("x0", "<f4", (64,)),
                           ("x1", "<f4", (64,)), ("iv", "<i4", (64,)), ("tile", "<f4", (680,))])
ARITH_OUT_DTYPE = np.dtype([(k, "<f4", (64,)) for k in ("chain", "scan", "autosum", "pair0", "pair1", "pair_fb0", "pair_fb1", "auto2_a",
                                                          "auto2_b", "chain2_a", "chain2_b", "div100", "div48", "fast100", "fast48",
                                                          "fdiv", "hypot", "shr1", "rint")] +
                           [("f2i", "<i4", (64,)), ("sum25", "<f4", (128,)), ("mf", "<f4", (128,))] +
                           [(k, "<i4", (64,)) for k in ("scan_add", "row_shr1", "row_shr2", "row_shr4", "row_shr8", "row_bcast15",
                                                         "row_bcast31", "wave_shr1")] +
                           [("div_bad", "<u8"), ("div_ok", "<u8"), ("scan_flag", "<i4"), ("pair_flag", "<i4"), ("auto2_flag", "<i4"),
                            ("reserved_", "<i4"), ("ends_a", "<f4"), ("ends_b", "<f4")])
assert ARITH_IN_DTYPE.itemsize == 3504 and ARITH_OUT_DTYPE.itemsize == 8232
assert WINDOW_DTYPE.itemsize == 24 and RESULT_DTYPE.itemsize == 48
assert SCORES_DTYPE.itemsize == 144 and STATS_DTYPE.itemsize == 1056

# the output arrays of rfid_selftest_inventory, in the order of its arguments
INVENTORY_SELFTEST_OUTPUTS = ("rows", "counts", "overflow", "head", "ent_off", "packed", "base", "reads_head", "offsets", "reads")


def inventory_selftest_outputs(n_streams: int, max_tags: int, reads_len: int, prefill: int = 0) -> dict:
    """the arrays rfid_selftest_inventory fills, every 32-bit word of them `prefill`"""
    n_rows = max(0, n_streams * max_tags)

    def arr(dtype, n, shape=None):
        a = np.full(max(0, n) * np.dtype(dtype).itemsize // 4, prefill, dtype=np.int32).view(dtype)
        return a if shape is None else a.reshape(shape)
    return dict(rows=arr(TAG_ENTRY_DTYPE, n_rows, (n_streams, max(0, max_tags))), counts=arr(np.int32, n_streams), overflow=arr(np.int32, n_streams),
                head=arr(np.int32, 2), ent_off=arr(np.int32, n_streams), packed=arr(TAG_ENTRY_DTYPE, n_rows), base=arr(np.int32, n_streams),
                reads_head=arr(np.int32, 1), offsets=arr(np.int64, n_rows + 1), reads=arr(TAG_READ_DTYPE, reads_len))


# every symbol include/rfid_mi355x.h declares: name -> (restype, argtypes)
_vp, _i, _i64, _ip = C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_int)
SIGNATURES = {
    "rfid_params_default": (_i, [C.POINTER(Params)]),
    "rfid_ctx_create": (_i, [C.POINTER(Params), _i, C.POINTER(_vp)]),
    "rfid_ctx_destroy": (_i, [_vp]),
    "rfid_ctx_reset": (_i, [_vp]),
    "rfid_strerror": (C.c_char_p, [_i]),
    "rfid_last_error": (C.c_char_p, [_vp]),
    "rfid_version": (C.c_char_p, []),
    "rfid_selftest": (_i, [_vp, _ip]),
    "rfid_selftest_gate_fsm": (_i, [_vp, _vp, _i, _vp, _vp]),
    "rfid_selftest_arith": (_i, [_vp, _vp, _i, _vp]),
    "rfid_selftest_stats": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "rfid_selftest_inventory": (_i, [_vp] * 5 + [_i] * 5 + [_i64, _i64] + [_vp] * 10),
    "rfid_mf_work": (_i, [_vp, _vp, _i, _vp, _i, _ip]),
    "rfid_gate_work": (_i, [_vp, _vp, _i, _vp, _i, _ip, _ip]),
    "rfid_decoder_work": (_i, [_vp, _vp, _i, _vp, _i, _ip, _ip, _vp, _vp]),
    "rfid_reader_work": (_i, [_vp, _i, _ip]),
    "rfid_reader_work_tx": (_i, [_vp, _i, _vp, _i, _vp, _i, _ip, _ip]),
    "rfid_reader_tx_max": (_i, [_i]),
    "rfid_get_state": (_i, [_vp, C.POINTER(ReaderState)]),
    "rfid_print_results": (_i, [_vp, C.c_char_p, _i, _ip]),
    "rfid_synth_gen2_size": (_i, [_vp, _vp, _i64, C.POINTER(C.c_int64)]),
    "rfid_synth_gen2": (_i, [_vp, _vp, _vp, _i64, _vp, _i64, C.c_float, C.c_uint64, _i64, C.POINTER(C.c_int64)]),
    "rfid_stream_begin": (_i, [_vp, _i64]),
    "rfid_stream_staging": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(C.c_int64)]),
    "rfid_stream_work": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _i64, C.POINTER(C.c_int64)]),
    "rfid_stream_end": (_i, [_vp]),
    "rfid_lookahead_enable": (_i, [_vp, _i64]),
    "rfid_lookahead_enable_gate": (_i, [_vp, _i64]),
    "rfid_lookahead_pending": (_i, [_vp, _ip, _ip]),
    "rfid_lookahead_set_coalesce": (_i, [_vp, _i64]),
    "rfid_lookahead_drain": (_i, [_vp]),
    "rfid_lookahead_set_late_outputs": (_i, [_vp, _i]),
    "rfid_mf_pending": (_i, [_vp, _ip]),
    "rfid_mf_must_fetch": (_i, [_vp, _ip]),
    "rfid_lookahead_set_consume_ahead": (_i, [_vp, _i]),
    "rfid_gate_forecast": (_i, [_vp, _i, _ip]),
    "rfid_lookahead_set_scheduler": (_i, [_vp, _i64]),
    "rfid_abi_version": (_i, []),
    "rfid_lookahead_flush": (_i, [_vp]),
    "rfid_host_alloc": (_vp, [C.c_size_t]),
    "rfid_host_free": (None, [_vp]),
    "rfid_gate_magn_squared": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "rfid_batch_get_gated": (_i, [_vp, _i, _i, _vp, _i64, C.POINTER(C.c_int64)]),
    "rfid_batch_plan": (_i, [_vp, _i, _i64]),
    "rfid_batch_set_streams": (_i, [_vp, _i]),
    "rfid_batch_set_long_stream": (_i, [_vp, _i]),
    "rfid_batch_ls_report": (_i, [_vp, _vp]),
    "rfid_ctx_set_knob": (_i, [_vp, C.c_char_p, _i]),
    "rfid_ctx_get_knob": (_i, [_vp, C.c_char_p, _ip]),
    "rfid_batch_mf": (_i, [_vp, _vp, _i64, _i64, _vp]),
    "rfid_batch_gate": (_i, [_vp]),
    "rfid_batch_decode": (_i, [_vp, _i]),
    "rfid_batch_stats": (_i, [_vp]),
    "rfid_batch_process": (_i, [_vp, _vp, _i64, _i64, _vp, _i]),
    "rfid_batch_plan_inventory": (_i, [_vp, _i]),
    "rfid_batch_inventory": (_i, [_vp]),
    "rfid_batch_get_inventory": (_i, [_vp, _vp, _i64, C.POINTER(_i64), _vp]),
    "rfid_batch_inventory_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_batch_plan_tracks": (_i, [_vp]),
    "rfid_batch_tracks": (_i, [_vp]),
    "rfid_batch_get_tracks": (_i, [_vp, _vp, _i64, C.POINTER(_i64), _vp]),
    "rfid_batch_tracks_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_batch_plan_quality": (_i, [_vp]),
    "rfid_batch_quality": (_i, [_vp]),
    "rfid_batch_get_quality": (_i, [_vp, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_get_window_quality": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_quality_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_batch_plan_repair": (_i, [_vp]),
    "rfid_batch_repair": (_i, [_vp]),
    "rfid_batch_get_repairs": (_i, [_vp, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_get_window_repairs": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_repair_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_repair_window": (_i, [_vp, _vp, _vp, _vp]),
    "rfid_batch_plan_slots": (_i, [_vp]),
    "rfid_batch_slots": (_i, [_vp]),
    "rfid_batch_get_window_moments": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_slots_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_window_moments_of": (_i, [_vp, _vp, _i, _vp]),
    "rfid_batch_plan_commands": (_i, [_vp]),
    "rfid_batch_commands": (_i, [_vp]),
    "rfid_batch_get_window_commands": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_commands_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_commands_of": (_i, [_vp, _vp, _vp, _i, _vp]),
    "rfid_batch_plan_fine": (_i, [_vp]),
    "rfid_batch_fine": (_i, [_vp]),
    "rfid_batch_get_fine": (_i, [_vp, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_get_window_fine": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_fine_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_fine_window": (_i, [_vp, _vp, _vp, _vp]),
    "rfid_batch_plan_retune": (_i, [_vp]),
    "rfid_batch_retune": (_i, [_vp]),
    "rfid_batch_get_window_retunes": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_retune_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_retune_window": (_i, [_vp, _vp, _i, _vp, _vp]),
    "rfid_batch_plan_collisions": (_i, [_vp]),
    "rfid_batch_collisions": (_i, [_vp]),
    "rfid_batch_get_window_collisions": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_collisions_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_collisions_of": (_i, [_vp, _vp, _vp, _i, _vp]),
    "rfid_batch_plan_lengths": (_i, [_vp]),
    "rfid_batch_lengths": (_i, [_vp]),
    "rfid_batch_get_window_lengths": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_lengths_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_length_window": (_i, [_vp, _vp, _i, _vp, _vp]),
    "rfid_batch_plan_diversity": (_i, [_vp, _i]),
    "rfid_batch_diversity": (_i, [_vp]),
    "rfid_batch_get_window_diversity": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_diversity_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_diversity_window": (_i, [_vp, _vp, _i, _vp, _vp]),
    "rfid_batch_plan_match": (_i, [_vp]),
    "rfid_batch_match_set_list": (_i, [_vp, _vp, _i]),
    "rfid_batch_match": (_i, [_vp]),
    "rfid_batch_get_window_matches": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_match_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_match_window": (_i, [_vp, _vp, _vp, _vp, _i, _vp]),
    "rfid_batch_plan_stack": (_i, [_vp]),
    "rfid_batch_stack": (_i, [_vp, C.c_float]),
    "rfid_batch_get_window_stacks": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_stack_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rfid_stack_windows": (_i, [_vp, _vp, _vp, _i, C.c_float, _vp]),
    "rfid_batch_sync": (_i, [_vp]),
    "rfid_batch_timing_get": (_i, [_vp, C.POINTER(BatchTiming)]),
    "rfid_batch_get_stats": (_i, [_vp, _vp, _i]),
    "rfid_batch_get_windows": (_i, [_vp, _vp, _vp, _vp, _i64, C.POINTER(_i64)]),
    "rfid_batch_device_ptrs": (_i, [_vp, C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_vp), C.POINTER(_vp)]),
    "rfid_batch_get_mf": (_i, [_vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "rfid_ctx_stream": (_vp, [_vp]),
    "rfid_synth_replicas": (_i, [_vp, _vp, _i64, _vp, _i64, _i, C.c_float, C.c_uint64, _i64]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load librfid_mi355x.so and bind every declared symbol.  Raises RfidError when the
    library has not been built (run `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RfidError(ERR_NO_DEVICE, f"{LIB_PATH} is missing: the HIP library has not been built; "
                                       "there is no CPU fallback")
    # Callers own HBM through PyTorch, whose wheel bundles its own HIP runtime (same soname as /opt/rocm's):
    # whichever copy is loaded first serves the whole process, and torch finds no device when it comes second
    # (measured on the MI355X box).  So let torch load and initialise its runtime first when it is installed.
    try:
        import torch
        torch.cuda.is_available()
    except ImportError:
        pass
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 not found
        raise RfidError(ERR_NO_DEVICE, f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, ctx: Optional[int] = None) -> None:
    if status != OK:
        lib = load()
        msg = lib.rfid_strerror(status).decode()
        if ctx:
            detail = lib.rfid_last_error(ctx).decode()
            if detail:
                msg += f" ({detail})"
        raise RfidError(status, msg)


def default_params(**overrides) -> Params:
    p = Params()
    check(load().rfid_params_default(C.byref(p)))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown rfid_params field {k!r}")
        setattr(p, k, int(v))
    return p
