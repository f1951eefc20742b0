// refshim/boost/shared_ptr.hpp -- boost::shared_ptr as std::shared_ptr (own code, test infrastructure).
#pragma once
#include <memory>
namespace boost {
using std::shared_ptr;
}
