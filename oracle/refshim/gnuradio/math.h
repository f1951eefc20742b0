// refshim/gnuradio/math.h -- included by the blocks under test, nothing of it is used (own code, test infrastructure).
#pragma once
