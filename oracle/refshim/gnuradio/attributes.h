// refshim/gnuradio/attributes.h -- stand-in for GNU Radio's symbol-visibility macros (own code, test infrastructure).
// See refshim/gnuradio/block.h for what this directory is.
#pragma once
#define __GR_ATTR_EXPORT __attribute__((visibility("default")))
#define __GR_ATTR_IMPORT __attribute__((visibility("default")))
