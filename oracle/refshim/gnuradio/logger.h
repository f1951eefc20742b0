// refshim/gnuradio/logger.h -- GR_LOG_* (own code, test infrastructure).  Each macro evaluates its stream expression
// into an std::ostringstream that is then thrown away: the blocks' own log expressions are still compiled and run,
// nothing is printed.
#pragma once
#include <sstream>

namespace gr {
typedef void *logger_ptr;
}

#define GR_RFID_REFSHIM_LOG(logger, msg)   \
  do {                                     \
    (void)(logger);                        \
    std::ostringstream gr_refshim_discard; \
    gr_refshim_discard << msg;             \
  } while (0)
#define GR_LOG_DEBUG(logger, msg) GR_RFID_REFSHIM_LOG(logger, msg)
#define GR_LOG_INFO(logger, msg) GR_RFID_REFSHIM_LOG(logger, msg)
#define GR_LOG_WARN(logger, msg) GR_RFID_REFSHIM_LOG(logger, msg)
#define GR_LOG_ERROR(logger, msg) GR_RFID_REFSHIM_LOG(logger, msg)
#define GR_LOG_EMERG(logger, msg) GR_RFID_REFSHIM_LOG(logger, msg)
