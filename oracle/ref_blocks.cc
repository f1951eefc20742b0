// oracle/ref_blocks.cc -- TEST INFRASTRUCTURE, own code.  Runs the REFERENCE's own gate, tag_decoder and reader blocks
// (lib/{gate,tag_decoder,reader,global_vars}_impl.cc compiled untouched against oracle/refshim, see oracle/Makefile
// `refblocks`) on a decimated trace, in the single-threaded order that oracle/rfid_oracle.c models
// (orc_stream_feed):
//
//   * the gate runs on up to --chunk items at a time (honouring its forecast); it breaks at every window close;
//   * whatever it wrote is appended to the decoder's queue, and the decoder is called on the whole queue (honouring its
//     forecast) until it consumes nothing;
//   * after every decoder call its port-0 items are appended to the reader's queue and the reader is run until it is
//     quiescent (IDLE, or a call that neither writes nor changes gen2_logic_status).
//
// The blocks are made in the order of apps/reader.py:75-78 (gate, tag_decoder, reader) with adc_rate/decim = 400000
// and --dac-rate (default 1000000); the reader is first run to quiescence before the gate sees a sample (START ->
// SEND_QUERY -> IDLE), as in the oracle.  The matched filter is not part of this run: the input is already filtered
// (tests use oracle.fir(raw)).
//
//   ref_blocks --in Y.c64 --out DIR [--chunk N] [--dac-rate R]     trace mode (N = 0: the whole trace in one call)
//   ref_blocks --state S --out DIR [--dac-rate R] [--bits 0101...]  set gen2_logic_status = S, call the reader once
//
// Output files in DIR (little-endian, no headers):
//   gated.c64    complex64: every sample the gate wrote, in order
//   tx.f32       float32: every sample the reader wrote, in order
//   magn.f32     float32: reader_state->magn_squared_samples at the end
//   windows.i32  int32 records of WIN_FIELDS, one per decoder call that consumed input (layout: WIN_* below)
//   reader.i32   int32 records of 4, one per reader call: gen2_logic_status before, ninput, written, status after
//   result.json  final reader_state: status words, counters, tag_reads, unique_tags_round, record counts
// and reader::print_results() on stdout (after the gate's own "| Execution time" line, if the run terminated).
//
// tag_decoder_impl's h_est, T_global and char_bits are private.  This translation unit -- and no other -- includes the block
// headers with `private` defined as `public` (after every standard header they pull in, so only the blocks' own
// access specifiers change; the Itanium C++ ABI lays members out the same either way) and reads them after each call.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <numeric>
#include <queue>
#include <sstream>
#include <string>
#include <vector>
#include <sys/time.h>
#include <time.h>

#include <gnuradio/block.h>
#include <gnuradio/io_signature.h>

#define private public
#include "gate_impl.h"
#include "reader_impl.h"
#include "tag_decoder_impl.h"
#undef private

using namespace gr::rfid;

namespace {

enum {
  WIN_GATED_START = 0,  // index into gated.c64 of the window's first sample
  WIN_OPEN_IDX,         // decimated input index of the window's first sample
  WIN_TYPE,             // decoder_status before the call (0 RN16, 1 EPC)
  WIN_CONSUMED,         // items the decoder consumed
  WIN_N_OUT0,           // items it produced on port 0
  WIN_BITS,             // WIN_BITS .. +15: the port-0 items (RN16 bits, 0 / 1)
  WIN_STATUS = WIN_BITS + 16,  // reader_state after the reader is quiescent again:
  WIN_GEN2,
  WIN_GATE,
  WIN_DECODER,
  WIN_N_QUERIES,
  WIN_ROUND,
  WIN_SLOT,
  WIN_N_EPC,
  WIN_N_TAGS,           // tag_reads.size()
  WIN_H_RE,             // tag_decoder_impl::h_est after the call, binary32 bits
  WIN_H_IM,
  WIN_T,                // tag_decoder_impl::T_global after the call, binary32 bits
  WIN_EPC_BITS,         // EPC calls: tag_decoder_impl::char_bits, the 128 decided bits, packed 32 per word MSB first
  WIN_FIELDS = WIN_EPC_BITS + 4
};

[[noreturn]] void die(const std::string &msg) {
  std::cerr << "ref_blocks: " << msg << std::endl;
  std::exit(2);
}

int f32_bits(float f) {
  int i;
  std::memcpy(&i, &f, sizeof i);
  return i;
}

template <class T>
void write_vec(const std::string &path, const std::vector<T> &v) {
  std::FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) die("cannot write " + path);
  if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) die("short write " + path);
  std::fclose(f);
}

struct Driver {
  gate::sptr g;
  tag_decoder::sptr d;
  reader::sptr r;
  gate_impl *gi;
  tag_decoder_impl *di;
  reader_impl *ri;

  std::vector<gr_complex> gated, dq;  // all gated samples; the decoder's input queue
  std::vector<float> rq, tx;          // the reader's input queue; all reader output
  std::vector<int> windows, reader_calls;
  long gated_consumed = 0;            // gated samples the decoder has consumed so far
  long cur_open = -1;                 // decimated index of the first sample of the window in the decoder's queue

  Driver(int dac_rate) {
    g = gate::make(400000);            // apps/reader.py:75-78 -- the gate initialises reader_state
    d = tag_decoder::make(400000);
    r = reader::make(400000, dac_rate);
    gi = dynamic_cast<gate_impl *>(g.get());
    di = dynamic_cast<tag_decoder_impl *>(d.get());
    ri = dynamic_cast<reader_impl *>(r.get());
    if (!gi || !di || !ri) die("unexpected block types");
  }

  // one reader call on its whole queue; returns whether it wrote or changed gen2_logic_status
  bool reader_call() {
    const int before = reader_state->gen2_logic_status;
    const int noutput = 1 << 16;
    std::vector<float> out((size_t)noutput + 64);
    gr_vector_int req(1, -1), nin(1, (int)rq.size());
    r->forecast(noutput, req);
    if (req[0] > nin[0]) die("reader forecast asks for more input than is queued");
    gr_vector_const_void_star in(1, rq.empty() ? nullptr : (const void *)rq.data());
    gr_vector_void_star outv(1, (void *)out.data());
    r->refshim_begin_work(1, 1);
    int ret = r->general_work(noutput, nin, in, outv);
    int written = ret == gr::block::WORK_CALLED_PRODUCE ? r->refshim_produced(0) : ret;
    if (written < 0 || written > noutput) die("reader wrote past noutput_items");
    const int consumed = r->refshim_consumed(0);
    if (consumed < 0 || consumed > nin[0]) die("reader consumed more than its input");
    reader_calls.insert(reader_calls.end(), {before, nin[0], written, (int)reader_state->gen2_logic_status});
    tx.insert(tx.end(), out.begin(), out.begin() + written);
    rq.erase(rq.begin(), rq.begin() + consumed);
    return written > 0 || reader_state->gen2_logic_status != before;
  }

  void reader_until_quiescent() {
    for (int guard = 0; guard < 8; ++guard) {
      if (reader_state->gen2_logic_status == IDLE) return;
      if (!reader_call()) return;
    }
  }

  // the decoder on its whole queue; returns items consumed
  int decoder_call() {
    if (dq.empty()) return 0;
    const int type = reader_state->decoder_status;
    int noutput = (int)dq.size();
    gr_vector_int req(1, -1), nin(1, (int)dq.size());
    d->forecast(noutput, req);
    if (req[0] > nin[0]) die("decoder forecast asks for more input than is queued");
    std::vector<float> out0((size_t)noutput + 64);
    std::vector<gr_complex> out1((size_t)noutput + 64);
    gr_vector_const_void_star in(1, (const void *)dq.data());
    gr_vector_void_star outv;
    outv.push_back(out0.data());
    outv.push_back(out1.data());
    d->refshim_begin_work(1, 2);
    int ret = d->general_work(noutput, nin, in, outv);
    int p0 = ret == gr::block::WORK_CALLED_PRODUCE ? d->refshim_produced(0) : ret;
    int p1 = ret == gr::block::WORK_CALLED_PRODUCE ? d->refshim_produced(1) : ret;
    if (p0 < 0 || p0 > noutput || p1 < 0 || p1 > noutput) die("decoder wrote past noutput_items");
    const int consumed = d->refshim_consumed(0);
    if (consumed < 0 || consumed > nin[0]) die("decoder consumed more than its input");
    if (consumed == 0) {
      if (p0 || p1) die("decoder produced without consuming");
      return 0;
    }
    std::vector<int> rec(WIN_FIELDS, 0);
    rec[WIN_GATED_START] = (int)gated_consumed;
    rec[WIN_OPEN_IDX] = (int)cur_open;
    rec[WIN_TYPE] = type;
    rec[WIN_CONSUMED] = consumed;
    rec[WIN_N_OUT0] = p0;
    if (p0 > 16) die("more than 16 port-0 items in one call");
    for (int k = 0; k < p0; ++k) rec[WIN_BITS + k] = (int)out0[(size_t)k];
    rq.insert(rq.end(), out0.begin(), out0.begin() + p0);
    dq.erase(dq.begin(), dq.begin() + consumed);
    gated_consumed += consumed;
    reader_until_quiescent();
    const READER_STATS &s = reader_state->reader_stats;
    rec[WIN_STATUS] = reader_state->status;
    rec[WIN_GEN2] = reader_state->gen2_logic_status;
    rec[WIN_GATE] = reader_state->gate_status;
    rec[WIN_DECODER] = reader_state->decoder_status;
    rec[WIN_N_QUERIES] = s.n_queries_sent;
    rec[WIN_ROUND] = s.cur_inventory_round;
    rec[WIN_SLOT] = s.cur_slot_number;
    rec[WIN_N_EPC] = s.n_epc_correct;
    rec[WIN_N_TAGS] = (int)s.tag_reads.size();
    rec[WIN_H_RE] = f32_bits(di->h_est.real());
    rec[WIN_H_IM] = f32_bits(di->h_est.imag());
    rec[WIN_T] = f32_bits(di->T_global);
    if (type == DECODER_DECODE_EPC)
      for (int b = 0; b < 128; ++b)
        if (di->char_bits[b] == '1') rec[WIN_EPC_BITS + b / 32] |= (int)(1u << (31 - b % 32));
    windows.insert(windows.end(), rec.begin(), rec.end());
    return consumed;
  }

  void run(const std::vector<gr_complex> &y, long chunk) {
    reader_until_quiescent();
    long pos = 0;
    const long n = (long)y.size();
    while (pos < n) {
      const int n_items = (int)std::min(chunk > 0 ? chunk : n, n - pos);
      int noutput = n_items;
      gr_vector_int req(1, -1);
      g->forecast(noutput, req);
      if (req[0] > n_items) die("gate forecast asks for more input than is offered");
      gr_vector_int nin(1, n_items);
      std::vector<gr_complex> out((size_t)noutput + 64);
      gr_vector_const_void_star in(1, (const void *)(y.data() + pos));
      gr_vector_void_star outv(1, (void *)out.data());
      g->refshim_begin_work(1, 1);
      int ret = g->general_work(noutput, nin, in, outv);
      int written = ret == gr::block::WORK_CALLED_PRODUCE ? g->refshim_produced(0) : ret;
      if (written < 0 || written > noutput) die("gate wrote past noutput_items");
      const int consumed = g->refshim_consumed(0);
      if (consumed <= 0 || consumed > n_items) die("gate consumed nothing or more than its input");
      if (written > 0) {
        // a window's samples are contiguous in the input; the last one written is the last consumed (the gate closed
        // in this call) or the last offered (it is still open)
        const long last = (reader_state->gate_status == GATE_OPEN) ? pos + n_items - 1 : pos + consumed - 1;
        if (dq.empty()) cur_open = last - (written - 1);
        gated.insert(gated.end(), out.begin(), out.begin() + written);
        dq.insert(dq.end(), out.begin(), out.begin() + written);
      }
      pos += consumed;
      while (decoder_call() > 0) {
      }
    }
  }

  void dump(const std::string &dir) {
    write_vec(dir + "/gated.c64", gated);
    write_vec(dir + "/tx.f32", tx);
    write_vec(dir + "/magn.f32", reader_state->magn_squared_samples);
    write_vec(dir + "/windows.i32", windows);
    write_vec(dir + "/reader.i32", reader_calls);
    const READER_STATS &s = reader_state->reader_stats;
    std::ofstream j((dir + "/result.json").c_str());
    j << "{\"status\": " << reader_state->status << ", \"gen2_logic_status\": " << reader_state->gen2_logic_status
      << ", \"gate_status\": " << reader_state->gate_status << ", \"decoder_status\": " << reader_state->decoder_status
      << ", \"n_queries_sent\": " << s.n_queries_sent << ", \"cur_inventory_round\": " << s.cur_inventory_round
      << ", \"cur_slot_number\": " << s.cur_slot_number << ", \"max_slot_number\": " << s.max_slot_number
      << ", \"n_epc_correct\": " << s.n_epc_correct << ", \"win_fields\": " << (int)WIN_FIELDS
      << ", \"n_windows\": " << windows.size() / WIN_FIELDS << ", \"n_reader_calls\": " << reader_calls.size() / 4
      << ", \"n_gated\": " << gated.size() << ", \"n_tx\": " << tx.size() << ", \"tag_reads\": {";
    bool first = true;
    for (std::map<int, int>::const_iterator it = s.tag_reads.begin(); it != s.tag_reads.end(); ++it) {
      j << (first ? "" : ", ") << "\"" << it->first << "\": " << it->second;
      first = false;
    }
    j << "}, \"unique_tags_round\": [";
    for (size_t k = 0; k < s.unique_tags_round.size(); ++k) j << (k ? ", " : "") << s.unique_tags_round[k];
    j << "]}\n";
    if (!j) die("cannot write result.json");
  }
};

}  // namespace

int main(int argc, char **argv) {
  std::string in_path, out_dir, bits;
  long chunk = 4096;
  int dac_rate = 1000000, state = -1;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (i + 1 >= argc) die("missing value after " + a);
    const std::string v = argv[++i];
    if (a == "--in") in_path = v;
    else if (a == "--out") out_dir = v;
    else if (a == "--chunk") chunk = std::atol(v.c_str());
    else if (a == "--dac-rate") dac_rate = std::atoi(v.c_str());
    else if (a == "--state") state = std::atoi(v.c_str());
    else if (a == "--bits") bits = v;
    else die("unknown option " + a);
  }
  if (out_dir.empty() || (in_path.empty() == (state < 0))) die("usage: --in Y.c64 | --state S, and --out DIR");
  if (chunk < 0 || dac_rate <= 0) die("bad --chunk / --dac-rate");

  Driver drv(dac_rate);
  if (state >= 0) {
    if (state > POWER_DOWN) die("no such gen2_logic_status");
    reader_state->gen2_logic_status = (GEN2_LOGIC_STATUS)state;
    for (size_t k = 0; k < bits.size(); ++k) drv.rq.push_back(bits[k] == '1' ? 1.0f : 0.0f);
    drv.reader_call();
  } else {
    std::FILE *f = std::fopen(in_path.c_str(), "rb");
    if (!f) die("cannot read " + in_path);
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % (long)sizeof(gr_complex)) die("input is not complex64");
    std::vector<gr_complex> y((size_t)bytes / sizeof(gr_complex));
    if (!y.empty() && std::fread(y.data(), sizeof(gr_complex), y.size(), f) != y.size()) die("short read");
    std::fclose(f);
    drv.run(y, chunk);
  }
  drv.dump(out_dir);
  drv.r->print_results();
  return 0;
}
