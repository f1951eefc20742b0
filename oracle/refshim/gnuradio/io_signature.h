// refshim/gnuradio/io_signature.h -- gr::io_signature::make / makev (own code, test infrastructure).
#pragma once
#include <cmath>
#include <vector>

#include <boost/shared_ptr.hpp>

namespace gr {

class io_signature {
 public:
  typedef boost::shared_ptr<io_signature> sptr;
  static sptr make(int min_streams, int max_streams, int sizeof_stream_item) {
    return sptr(new io_signature(min_streams, max_streams, std::vector<int>(1, sizeof_stream_item)));
  }
  static sptr makev(int min_streams, int max_streams, const std::vector<int> &sizeof_stream_items) {
    return sptr(new io_signature(min_streams, max_streams, sizeof_stream_items));
  }
  int min_streams() const { return d_min; }
  int max_streams() const { return d_max; }
  // the item size of stream i; streams past the list repeat its last entry
  int sizeof_stream_item(int i) const {
    return d_sizes[(size_t)i < d_sizes.size() ? (size_t)i : d_sizes.size() - 1];
  }

 private:
  io_signature(int mn, int mx, const std::vector<int> &s) : d_min(mn), d_max(mx), d_sizes(s) {}
  int d_min, d_max;
  std::vector<int> d_sizes;
};

}  // namespace gr
