"""The reader's statistics of a trace, replayed window by window: the plain reference of stream_stats_kernel (TEST
INFRASTRUCTURE).  Written from the reference's lines, one decoded window after the other, with Python integers and a dict:

  before every window  gate_impl.cc:101-109         n_queries_sent > MAX_NUM_QUERIES || tag_reads.size() > NUMBER_UNIQUE_TAGS
                                                    -> TERMINATED: the gate passes nothing on any more, this window and all
                                                    behind it are not decoded (n_windows_used = its index)
  an RN16 window       tag_decoder_impl.cc:256-268  decoded -> SEND_ACK; the reader's ACK (reader_impl.cc:290-320) counts nothing
  an EPC window        tag_decoder_impl.cc:295      cur_slot_number++
                       :327-365 (CRC good)          past max_slot_number: slot 1, next round; n_epc_correct++, tag_reads[id]++
                       :366-383 (CRC bad)           past max_slot_number: slot 1, next round
                       reader_impl.cc:261,335       the SEND_QUERY / SEND_QUERY_REP that follows: n_queries_sent++
  behind the last one  the same check once more (the gate runs on over the rest of the trace)

and in front of it all START -> SEND_QUERY (reader_impl.cc:218-261): n_queries_sent = 1 before the first sample.
tests/test_stats_emu.py pins this replay to the oracle's final reader state on synthesised traces before any kernel is compared
with it."""
from collections import namedtuple

RUNNING, TERMINATED = 0, 1
RN16, EPC = 0, 1

Stats = namedtuple("Stats", "n_queries_sent cur_inventory_round cur_slot_number n_epc_correct n_unique_tags n_windows "
                            "n_windows_used status tag_reads")


def _over(n_queries_sent, tag_reads, max_num_queries, number_unique_tags):
    return n_queries_sent > max_num_queries or len(tag_reads) > number_unique_tags       # gate_impl.cc:101-102


def replay(windows, max_slot_number, max_num_queries, number_unique_tags):
    """windows: (type, crc_ok, tag_id) per decoded window, in order -> Stats (tag_reads: {id: reads})"""
    windows = list(windows)
    n_queries_sent = 0                    # global_vars.cc:37
    n_epc_correct = 0
    cur_inventory_round = 1
    cur_slot_number = 1
    tag_reads = {}
    status = RUNNING
    n_queries_sent += 1                   # START -> SEND_QUERY, reader_impl.cc:261
    used = len(windows)
    for k, (wtype, crc_ok, tag_id) in enumerate(windows):
        if _over(n_queries_sent, tag_reads, max_num_queries, number_unique_tags):
            status = TERMINATED
            used = k
            break
        if int(wtype) == EPC:
            cur_slot_number += 1                                   # tag_decoder_impl.cc:295
            if int(crc_ok):
                if cur_slot_number > max_slot_number:              # :330-340
                    cur_slot_number = 1
                    cur_inventory_round += 1
                n_epc_correct += 1                                 # :346
                tag_id = int(tag_id)
                if tag_id in tag_reads:                            # :356-364
                    tag_reads[tag_id] += 1
                else:
                    tag_reads[tag_id] = 1
            else:
                if cur_slot_number > max_slot_number:              # :369-378
                    cur_slot_number = 1
                    cur_inventory_round += 1
            n_queries_sent += 1                                    # reader_impl.cc:261 / :335
    else:
        if _over(n_queries_sent, tag_reads, max_num_queries, number_unique_tags):
            status = TERMINATED
    return Stats(n_queries_sent, cur_inventory_round, cur_slot_number, n_epc_correct, len(tag_reads), len(windows), used, status,
                 tag_reads)


def windows_of(records):
    """(type, crc_ok, tag_id) of result records (capi.RESULT_DTYPE) or of the oracle's dumps"""
    return list(zip(records["type"].tolist(), records["crc_ok"].tolist(), records["tag_id"].tolist()))
