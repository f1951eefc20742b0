// refshim/gnuradio/block.h -- stand-in for the part of GNU Radio 3.7's gr::block interface that the reference's
// gate, tag_decoder and reader blocks are written against, so that their sources compile untouched and run under
// oracle/ref_blocks.cc (own code, test infrastructure; see oracle/Makefile `refblocks`).
//
// Interface names only: the constructor, forecast, general_work, consume_each / consume, produce,
// WORK_CALLED_PRODUCE, d_logger / d_debug_logger, gnuradio::get_initial_sptr, gr_complex and gr_vector_*.  There is no
// scheduler here: the driver calls forecast / general_work itself and reads back, through the refshim_* members, what
// the block consumed and produced.  This directory is self-contained on purpose -- it does not share the product's
// model of gr::block (gen2-uhf-rfid-reader_amd/cxx/minigr), which the reference's blocks are meant to check.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include <boost/shared_ptr.hpp>
#include <gnuradio/attributes.h>
#include <gnuradio/io_signature.h>
#include <gnuradio/logger.h>

typedef std::complex<float> gr_complex;
typedef std::vector<int> gr_vector_int;
typedef std::vector<const void *> gr_vector_const_void_star;
typedef std::vector<void *> gr_vector_void_star;

namespace gr {

class block {
 public:
  enum { WORK_CALLED_PRODUCE = -2, WORK_DONE = -1 };
  virtual ~block() {}
  const std::string &name() const { return d_name; }
  virtual void forecast(int noutput_items, gr_vector_int &ninput_items_required) {
    for (size_t i = 0; i < ninput_items_required.size(); ++i) ninput_items_required[i] = noutput_items;
  }
  virtual int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &input_items,
                           gr_vector_void_star &output_items) = 0;
  void consume_each(int how_many_items) {
    for (size_t i = 0; i < d_consumed.size(); ++i) d_consumed[i] = how_many_items;
  }
  void consume(int which_input, int how_many_items) { d_consumed.at((size_t)which_input) = how_many_items; }
  void produce(int which_output, int how_many_items) { d_produced.at((size_t)which_output) = how_many_items; }

  // the driver's side: clear the counters before general_work, read them after
  void refshim_begin_work(int n_inputs, int n_outputs) {
    d_consumed.assign((size_t)n_inputs, 0);
    d_produced.assign((size_t)n_outputs, 0);
  }
  int refshim_consumed(int port) const { return d_consumed.at((size_t)port); }
  int refshim_produced(int port) const { return d_produced.at((size_t)port); }

 protected:
  block() {}  // for `class X : virtual public gr::block`
  block(const std::string &name, io_signature::sptr in, io_signature::sptr out)
      : d_logger(0), d_debug_logger(0), d_name(name), d_in(in), d_out(out) {}
  logger_ptr d_logger, d_debug_logger;

 private:
  std::string d_name;
  io_signature::sptr d_in, d_out;
  std::vector<int> d_consumed, d_produced;
};

}  // namespace gr

namespace gnuradio {
template <class T>
boost::shared_ptr<T> get_initial_sptr(T *p) {
  return boost::shared_ptr<T>(p);
}
}  // namespace gnuradio
