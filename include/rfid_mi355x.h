/*
 * rfid_mi355x.h -- C-ABI of the MI355X-native Gen2 RFID receive path
 *                  (matched filter -> gate -> tag_decoder), librfid_mi355x.so.
 *
 * This is the drop-in boundary for the hot path of nkargas/Gen2-UHF-RFID-Reader.
 * Every entry point names the reference interface it replaces (paths relative to
 * /root/reference/gr-rfid/).  Plain C: pointers and sizes only, no C++/torch types,
 * no exceptions; every function returns an rfid_status (0 = ok, <0 = error) and never
 * aborts.  There is NO CPU fallback: if no gfx950 device / HIP runtime is usable,
 * rfid_ctx_create fails with RFID_ERR_NO_DEVICE.
 *
 * Sample format everywhere: interleaved little-endian float32 I,Q (= gr_complex =
 * the reference's file_source format, misc/code/plot_signal.m:5-9).
 *
 * Two families of entry points:
 *   (1) per-block streaming calls on HOST buffers -- one per reference work():
 *         rfid_mf_work       <- filter.fir_filter_ccc(5,[1]*25)      apps/reader.py:65,75
 *         rfid_gate_work     <- gate_impl::general_work               lib/gate_impl.cc:85-200
 *         rfid_decoder_work  <- tag_decoder_impl::general_work        lib/tag_decoder_impl.cc:196-397
 *         rfid_reader_work_tx <- reader_impl::general_work (state transitions + transmit waveform)
 *         rfid_reader_work    <- its state transitions alone
 *                                                                     lib/reader_impl.cc:200-380
 *   (2) batched offline calls on DEVICE buffers (many independent traces per launch):
 *         rfid_batch_mf / rfid_batch_gate / rfid_batch_decode / rfid_batch_stats and the
 *         fused driver rfid_batch_process -- the same arithmetic, all windows of all
 *         traces decoded in one launch.
 *
 * Threading: one rfid_ctx = one GPU + one HIP stream.  Calls on a ctx must be
 * serialised by the caller; distinct contexts are independent (multi-GPU = one ctx,
 * one process, per device; no collective).
 */
#ifndef RFID_MI355X_H
#define RFID_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RFID_API __attribute__((visibility("default")))
#define RFID_MI355X_ABI 7   /* see rfid_abi_version() */

typedef enum rfid_status {
  RFID_OK = 0,
  RFID_ERR_INVALID = -1,      /* bad argument */
  RFID_ERR_NO_DEVICE = -2,    /* no usable gfx950 device / HIP runtime */
  RFID_ERR_HIP = -3,          /* a HIP call failed: see rfid_last_error() */
  RFID_ERR_UNSUPPORTED = -4,  /* parameter combination the kernels are not built for */
  RFID_ERR_CAPACITY = -5,     /* caller buffer or planned workspace too small */
  RFID_ERR_STATE = -6         /* call not valid in the current state (e.g. no plan) */
} rfid_status;

/* gr_complex */
typedef struct rfid_cf32 { float re, im; } rfid_cf32;

/* enums of include/rfid/global_vars.h:31-34, same numeric values */
enum { RFID_RUNNING = 0, RFID_TERMINATED = 1 };
enum { RFID_SEND_QUERY = 0, RFID_SEND_ACK, RFID_SEND_QUERY_REP, RFID_IDLE, RFID_SEND_CW, RFID_START,
       RFID_SEND_QUERY_ADJUST, RFID_SEND_NAK_QR, RFID_SEND_NAK_Q, RFID_POWER_DOWN };
enum { RFID_GATE_OPEN = 0, RFID_GATE_CLOSED, RFID_GATE_SEEK_RN16, RFID_GATE_SEEK_EPC };
enum { RFID_DECODE_RN16 = 0, RFID_DECODE_EPC = 1 };

/* Construction parameters.  Replaces the ctor arguments gate::make(int sample_rate)
 * (include/rfid/gate.h:51), tag_decoder::make(int sample_rate) (include/rfid/tag_decoder.h:48),
 * the flowgraph's decim / num_taps (apps/reader.py:54,65) and the compile-time constants
 * FIXED_Q, MAX_NUM_QUERIES, NUMBER_UNIQUE_TAGS (include/rfid/global_vars.h:72,76,100). */
typedef struct rfid_params {
  int32_t sample_rate;        /* rate after decimation; only 400000 is supported */
  int32_t decim;              /* 5  */
  int32_t n_taps;             /* 25, all-ones */
  int32_t fixed_q;            /* 0..15 */
  int32_t max_num_queries;    /* 1000 */
  int32_t number_unique_tags; /* 100 */
} rfid_params;

/* READER_STATE / READER_STATS view (include/rfid/global_vars.h:36-67) */
typedef struct rfid_reader_state {
  int32_t status, gen2_logic_status, gate_status, decoder_status;
  int32_t n_samples_to_ungate;
  int32_t n_queries_sent, cur_inventory_round, cur_slot_number, max_slot_number, n_epc_correct;
  int32_t n_unique_tags;
  int32_t tag_reads[256];     /* std::map<int,int> tag_reads, key = EPC bits 104..111 */
} rfid_reader_state;

/* one gate opening, produced by the batched gate scan */
typedef struct rfid_window {
  int32_t stream;   /* trace index in the batch */
  int32_t seq;      /* 0,1,2,... per trace; type = seq & 1 */
  int32_t start;    /* index (400 ksps domain) of the first gated sample */
  int32_t type;     /* RFID_DECODE_RN16 / RFID_DECODE_EPC */
  float dc_re, dc_im; /* gate_impl::dc_est at the opening (lib/gate_impl.cc:141,176) */
} rfid_window;

/* what tag_decoder computes for one window */
typedef struct rfid_decode_result {
  int32_t type;       /* RFID_DECODE_RN16 / RFID_DECODE_EPC */
  int32_t index;      /* value returned by tag_sync (lib/tag_decoder_impl.cc:107-108) */
  float h_re, h_im;   /* h_est (:103) */
  float T;            /* T_global (:166-169); 0 for RN16 */
  uint32_t bits[4];   /* decoded bits, bit j of the frame at bits[j>>5] bit (j&31) */
  int32_t n_bits;     /* 16 or 128 */
  int32_t crc_ok;     /* EPC: 1 if check_crc()==1 (:401-445), else 0 */
  int32_t tag_id;     /* EPC bits 104..111, MSB first (:348-352); -1 unless crc_ok */
} rfid_decode_result;

/* optional per-window scores for tolerance checks (correlation / energy values) */
typedef struct rfid_scores {
  float corr[15];     /* std::norm(corr2) per candidate offset (lib/tag_decoder_impl.cc:85-99) */
  float energy[20];   /* per half-period candidate (:157-164); zeros for RN16 */
  float pad_;
} rfid_scores;

/* per-trace statistics after the decode of a batch (READER_STATS per trace) */
typedef struct rfid_stream_stats {
  int32_t n_queries_sent, cur_inventory_round, cur_slot_number, n_epc_correct, n_unique_tags;
  int32_t n_windows;       /* complete windows the gate produced */
  int32_t n_windows_used;  /* windows consumed before TERMINATED (lib/gate_impl.cc:101-109) */
  int32_t status;          /* RFID_RUNNING / RFID_TERMINATED */
  int32_t tag_reads[256];
} rfid_stream_stats;

/* one DISTINCT EPC frame of one trace: what the inventory stage (rfid_batch_inventory) lists.  The reads it covers are
 * those tag_reads[] counts -- EPC windows with a verified CRC before the TERMINATED cut-off (window index <
 * n_windows_used) -- keyed by all 128 frame bits instead of the one byte tag_reads[] is keyed by. */
typedef struct rfid_tag_entry {      /* 48 bytes */
  int32_t  stream;                   /* trace index */
  int32_t  reads;                    /* CRC-verified reads of this frame before the cut-off */
  uint32_t frame[4];                 /* the 128 frame bits, packed as rfid_decode_result::bits
                                        (PC 0..15, EPC 16..111, CRC-16 112..127) */
  int32_t  first_seq, last_seq;      /* window seq of the first / last such read */
  int32_t  best_seq;                 /* the read with the largest h_re*h_re + h_im*h_im (binary32, this expression,
                                        no fused multiply-add; earliest seq on ties) */
  float    best_h_re, best_h_im;     /* its h_est, copied bit for bit */
  int32_t  tag_id;                   /* frame bits 104..111, as rfid_decode_result::tag_id */
} rfid_tag_entry;

/* one CRC-verified EPC read before the TERMINATED cut-off: what the tracks stage (rfid_batch_tracks) lists for every
 * read the inventory counts -- when it happened and the channel estimate the decoder formed for it */
typedef struct rfid_tag_read {       /* 32 bytes */
  int32_t stream;                    /* trace index */
  int32_t entry;                     /* which tag: index into THIS trace's inventory list (order of first_seq), 0-based */
  int32_t seq;                       /* the EPC window's seq (rfid_window::seq) */
  int32_t start;                     /* rfid_window::start of that window: 400 ksps index of its first gated sample */
  float   h_re, h_im;                /* rfid_decode_result::h_re / h_im of that window, copied bit for bit */
  float   T;                         /* rfid_decode_result::T, bit for bit */
  int32_t index;                     /* rfid_decode_result::index (tag_sync's return value) */
} rfid_tag_read;

/* how good the decision of one EPC window was: what the quality stage (rfid_batch_quality) works out for EVERY EPC window
 * before the TERMINATED cut-off, CRC-verified or not, from the 128 decision values of tag_detection_EPC
 * (lib/tag_decoder_impl.cc:171-190) and their quadrature counterparts.  THE DEFINITION (the contract; binary32 throughout,
 * every operation rounded by itself, no fused multiply-add):
 *   from the window's own rfid_decode_result (h_re, h_im, T, index) and its gated samples
 *   s[i] = y[start + i] - dc per component (y: the matched filter's output, start / dc: the window's rfid_window),
 *   for j = 0 .. 127:
 *     ia  = (int)((float)j * (2.0f * T) + (float)index)
 *     ib  = (int)(((float)(j * 2) * T + T) + (float)index)
 *     dx  = s[ia].x - s[ib].x,  dy = s[ia].y - s[ib].y
 *     r_j = dx * h_re - dy * (-h_im)         the decoder's decision value, Re((s_a - s_b) conj(h_est))
 *     q_j = dy * h_re - dx * h_im            the imaginary part of the same product: noise and interference only
 *   the three sums are IN-ORDER sums (((0.0f + t_0) + t_1) + ...) + t_127: a record is a function of the input alone and
 *   is compared by bit pattern.  (A window with a non-finite sample: unspecified, as its decoding is.)
 * What a host makes of it (rfid.batch.quality_fields, in binary64): snr_db = 10 log10(sig_sq / quad_sq) -- CRC-verified
 * reads lie some 6 dB per halving of the noise above the ~0 dB of an empty or collided slot -- and
 * margin = margin_min / (sig_abs / 128), the weakest decision relative to the mean one. */
typedef struct rfid_read_quality {   /* 32 bytes */
  int32_t stream, seq;               /* the EPC window (rfid_window::stream / seq) */
  float   sig_abs;                   /* sum_j |r_j|      j = 0..127, ascending, from 0.0f, binary32 */
  float   sig_sq;                    /* sum_j r_j * r_j  same order */
  float   quad_sq;                   /* sum_j q_j * q_j  same order */
  float   margin_min;                /* min_j |r_j| */
  int32_t margin_bit;                /* the first j that attains it (a = |r_0|; j = 1..127: if (|r_j| < a) take j) */
  int32_t flags;                     /* bit 0: crc_ok of the window's result */
} rfid_read_quality;

/* what the repair stage (rfid_batch_repair, rfid_repair_window) finds for one EPC window: the cheapest way to make a frame
 * whose CRC-16 failed pass by reversing up to RFID_REPAIR_MAX_FLIPS of its RFID_REPAIR_CANDIDATES weakest sign decisions.
 * The decoder is differential (lib/tag_decoder_impl.cc:171-190: bit = "sign equals previous sign"), so reversing decision j
 * toggles frame bits j and j + 1, and for j = 127 bit 127 only.  A repair is NOT a read: nothing else the library reports
 * changes, and with 92 masks tried against a 16-bit CRC about one hopeless window in 700 is "repaired" by chance -- `entry`
 * says whether the repaired frame is one the same trace's inventory already holds.
 * THE DEFINITION (the contract; binary32 throughout, every operation rounded by itself, no fused multiply-add), for an EPC
 * window with seq < n_windows_used and crc_ok == 0:
 *   1. r_j, j = 0 .. 127, exactly as in the rfid_read_quality definition above (from the window's own result h_re, h_im, T,
 *      index and s[i] = y[start + i] - dc); a_j = |r_j|; the frame bits b are rfid_decode_result::bits.
 *   2. candidates c_0 .. c_7: the RFID_REPAIR_CANDIDATES decisions with the smallest (a_j, j) in that order -- a compared as
 *      binary32 values, the smaller j first on equal a.
 *   3. for every mask m in 1 .. 255 with at most RFID_REPAIR_MAX_FLIPS bits set: frame(m) = b XOR the toggles of all c_i with
 *      bit i of m set (two neighbouring candidates toggle the bit they share twice).
 *   4. m passes when the reference's check_crc (lib/tag_decoder_impl.cc:401-445) accepts frame(m).
 *   5. cost(m) = ((0.0f + a_{c_i1}) + a_{c_i2}) + a_{c_i3}, i ascending.  The winner is the passing mask with the smallest
 *      cost (binary32 <), the smaller m on equal cost.
 * A window with a non-finite sample: unspecified, as its decoding is. */
#define RFID_REPAIR_CANDIDATES 8
#define RFID_REPAIR_MAX_FLIPS 3
typedef struct rfid_repair {         /* 48 bytes */
  int32_t  stream, seq;              /* the EPC window (rfid_window::stream / seq) */
  int32_t  start;                    /* rfid_window::start of that window */
  int32_t  flags;                    /* bit 0: crc_ok of the window's result (then nothing is searched);
                                        bit 1: this trace's inventory overflowed, entry not looked up */
  int32_t  n_flips;                  /* 0: not repaired; 1 .. 3: decisions reversed */
  int32_t  flips;                    /* byte k (k < n_flips): decision index j of the k-th flip, ascending j;
                                        unused bytes 0xFF; -1 when n_flips == 0 */
  float    cost;                     /* cost of the winner; 0.0f when n_flips == 0 */
  int32_t  entry;                    /* index into THIS trace's inventory list (as rfid_tag_read::entry) of the entry whose
                                        128 frame bits equal the repaired frame; -1: none, or n_flips == 0 */
  uint32_t frame[4];                 /* the repaired frame, packed as rfid_decode_result::bits; zeros when n_flips == 0 */
} rfid_repair;

/* the data-aided channel estimate of one EPC window: what the fine stage (rfid_batch_fine, rfid_fine_window) works out for EVERY
 * EPC window before the TERMINATED cut-off, CRC-verified or not.  rfid_decode_result::h_est is the mean of six matched-filter
 * samples of the preamble relative to the gate's dc_est; the frame behind it carries 256 more half-bit samples of the same
 * channel, and with the frame bits known so are their polarities.  Their signed sum does not depend on dc_est, its noise is some
 * 3.3 times smaller, and taken over 16 bits (400 us) at a time it gives the channel at eight points inside the read.
 * THE DEFINITION (the contract; binary32 throughout, every operation rounded by itself, no fused multiply-add):
 *   from the window's own rfid_decode_result (T, index, bits; h_re / h_im are NOT used) and its gated samples
 *   s[i] = y[start + i] - dc per component, with ia, ib of the rfid_read_quality definition above (clamped into 0 .. 1369),
 *   for j = 0 .. 127:
 *     dx_j = s[ia].x - s[ib].x,  dy_j = s[ia].y - s[ib].y
 *     g_j  = +1.0f when the number of set bits among frame bits 0 .. j is even, else -1.0f   (the decoder's sign chain:
 *            lib/tag_decoder_impl.cc:171-190, prev = 1 at the start; taken from the BITS, so the per-call form works on a
 *            frame whose bits a caller has corrected)
 *   segment k = 0 .. 7 covers j = 16 k .. 16 k + 15, its three sums IN-ORDER sums (((0.0f + t_16k) + t_16k+1) + ...):
 *     seg_re[k] = sum g_j * dx_j,  seg_im[k] = sum g_j * dy_j,  seg_pow[k] = sum (dx_j * dx_j + dy_j * dy_j)
 *   sum_re, sum_im, pow are the in-order sums of the eight segment values from 0.0f (the longest dependent chain is 16 + 8
 *   additions, not 128).  A record is a function of the input alone and is compared by bit pattern.  For a window whose CRC
 *   failed the record is decision-directed, and flags says so.  (A window with a non-finite sample: unspecified.)
 * What a host makes of it (rfid.batch.fine_fields, in binary64): h = (sum_re + j sum_im) / 128 -- in the units of h_est -- the
 * noise per difference (pow - |sum|^2 / 128) / 127, snr_db, the segments' h_k = seg / 16 and the drift of their phase. */
typedef struct rfid_read_fine {      /* 128 bytes */
  int32_t stream, seq;               /* the EPC window (rfid_window::stream / seq) */
  int32_t start;                     /* rfid_window::start of that window */
  int32_t flags;                     /* bit 0: crc_ok of the window's result */
  float   sum_re, sum_im;            /* the eight seg_re / seg_im, added in order from 0.0f */
  float   pow;                       /* the eight seg_pow, likewise */
  int32_t reserved_;                 /* 0 */
  float   seg_re[8], seg_im[8], seg_pow[8];
} rfid_read_fine;

/* what the retune stage (rfid_batch_retune, rfid_retune_window) finds for one EPC window whose CRC-16 failed: the frame decoded
 * again with the half-bit period searched over the whole tolerance Gen2 allows a tag's backscatter link frequency at this link
 * setting (DR = 8, TRcal = 200 us: 40 kHz +- 4 %, Gen2 table 6.9) -- 81 candidates over 5.0 +- 4 % samples, where the decoder
 * searches 20 over +- 1 % (lib/tag_decoder_impl.cc:150-166).  A tag further off than that fails every CRC and is otherwise absent
 * from everything a pass reports.  A retuned frame is NOT a read: nothing else the library reports changes.
 * THE DEFINITION (the contract; binary32 throughout, every operation rounded by itself, no fused multiply-add, every sum in order
 * from 0.0f), for an EPC window with seq < n_windows_used and crc_ok == 0:
 *   span   s[i] = y[start + min(i, last)] - dc per component, 0 <= i < RFID_RETUNE_SPAN: the gate's output and what follows it --
 *          a slow tag's frame ends up to 38 samples behind the window (the furthest index is 14 + 268 x 5.2 = 1407.6).  last: the
 *          trace's own last matched-filter output relative to start; no sample behind it is read.  p[i] = s.x * s.x + s.y * s.y.
 *   sync   the decoder's: m = rfid_decode_result::index - 65, in 0 .. 14.
 *   grid   t = 0 .. 80:  T_t = 4.8f + (float)t * ((5.2f - 4.8f) / 80.0f),  idx_t = (float)m + 13.0f * T_t   (at T = 5: m + 65)
 *   energy[t] = sum over i = 0 .. 255 of p[(int)((float)i * T_t + idx_t)]     (the decoder's metric); t* = the first maximum
 *   at T = T_t*, idx = idx_t*:
 *     h    = the sum, left to right, of s[(int)((float)m + (float)j * T)], j = 0, 1, 3, 6, 10, 11 (the preamble's ones), each
 *            component divided by 6.0f
 *     bits = the decoder's 128 decisions (tag_decoder_impl.cc:171-190) on s with that h, T and idx: samples at
 *            (int)((float)j * (2.0f * T) + idx) and (int)(((float)(2 j) * T + T) + idx), the same sign chain
 *     the frame passes when the reference's check_crc (:401-445) accepts it
 * A window with a non-finite sample: unspecified, as its decoding is. */
#define RFID_RETUNE_SPAN 1408
#define RFID_RETUNE_CANDIDATES 81
typedef struct rfid_retune {         /* 64 bytes */
  int32_t  stream, seq;              /* the EPC window (rfid_window::stream / seq) */
  int32_t  start;                    /* rfid_window::start of that window */
  int32_t  flags;                    /* bit 0: crc_ok of the window's result (then nothing is searched: every field below is 0);
                                        bit 1: the frame decoded again passes the CRC; bit 2: an index the search used lay behind
                                        the trace's (the span's) last sample and was held there */
  int32_t  t_index;                  /* t* */
  float    T;                        /* T_t* */
  float    h_re, h_im;               /* h at T_t* */
  float    energy;                   /* energy[t*] */
  uint32_t frame[4];                 /* the bits decoded at T_t*, packed as rfid_decode_result::bits, whether they pass or not */
  int32_t  reserved_[3];             /* 0 */
} rfid_retune;

/* what the lengths stage (rfid_batch_lengths, rfid_length_window) finds for one EPC window whose CRC-16 failed: the frame read at the
 * length its own PC word announces.  A tag answers an ACK with PC (16 bits) + EPC + CRC-16, and the first five PC bits give the EPC's
 * length L in 16-bit words (Gen2 6.3.2.1.2.2).  The decoder takes every reply for 128 bits (EPC_BITS = 129, check_crc over 14 bytes:
 * L = 6, a 96-bit EPC); a tag with a 128- or a 64-bit EPC fails every CRC and is otherwise absent from everything a pass reports.
 * A frame of L < 6 lies inside the gate's 1 370-sample window; one of L = 7 or 8 ends behind it, on the reader's carrier, which lasts
 * 1 830 decimated samples after the ACK: the furthest half-bit of a 160-bit frame is at 79 + 319 x 5.05000019 = 1689.95 samples.
 * A frame found here is NOT a read: nothing else the library reports changes.
 * THE DEFINITION (the contract; binary32 throughout, every operation rounded by itself, no fused multiply-add), for an EPC window
 * with seq < n_windows_used and crc_ok == 0:
 *   L      = sum of bit_i << (4 - i) over the result's frame bits i = 0 .. 4.  L == 6 or L > 8: only `words` and the flag bit (4 / 3)
 *            are set.  Else n = 32 + 16 L.
 *   span   s[i] = y[start + min(i, last)] - dc per component, 0 <= i < RFID_LENGTHS_SPAN.  last: the trace's own last
 *          matched-filter output relative to start (as rfid_retune has it); no sample behind it is read.
 *   decisions j = 0 .. n - 1, with the result's own T, index, h_re, h_im -- the decoder's two associations and its sign chain
 *          (tag_decoder_impl.cc:171-190), continued past 127:
 *            ia = (int)((float)j * (2.0f * T) + (float)index),  ib = (int)(((float)(2 j) * T + T) + (float)index), both held
 *            inside 0 .. RFID_LENGTHS_SPAN - 1;  (dx, dy) = s[ia] - s[ib];  r_j = dx * h_re - dy * (-h_im);  cur_j = r_j > 0;
 *            bit_j = (cur_j != cur_(j-1)), cur_(-1) positive.
 *   CRC    the reference's check_crc (:401-445) over n bits instead of 128: the bits packed MSB first into bytes, CRC-16/CCITT
 *          (init 0xFFFF, per byte crc ^= b << 8 and eight shift-xor 0x1021 steps) over the first (n - 16) / 8 bytes, complemented,
 *          compared with the last 16 bits.
 * Decisions 0 .. 127 are the decoder's own: frame words 0 .. 3, as far as n reaches, equal the result's bits.
 * A window with a non-finite sample: unspecified, as its decoding is. */
#define RFID_LENGTHS_SPAN      1728   /* 27 x 64 */
#define RFID_LENGTHS_MAX_WORDS 8      /* EPC words a slot of this link setting holds: a 160-bit frame */
typedef struct rfid_sized_frame {    /* 64 bytes */
  int32_t  stream, seq;              /* the EPC window (rfid_window::stream / seq) */
  int32_t  start;                    /* rfid_window::start of that window */
  int32_t  flags;                    /* bit 0: crc_ok of the window's result (then nothing is done: every field below is 0);
                                        bit 1: the frame at the PC's length passes its CRC-16; bit 2: an index lay behind the
                                        trace's (the span's) last sample and was held there; bit 3: L > 8: does not fit the slot,
                                        nothing decoded; bit 4: L == 6: the decoder's own length, nothing to add */
  int32_t  words;                    /* L */
  int32_t  n_bits;                   /* 32 + 16 L when decoded, else 0 */
  int32_t  crc_rcvd, crc_calc;       /* the last 16 bits MSB first / the CRC computed over the bits before them; 0 when not decoded */
  uint32_t frame[5];                 /* n_bits bits packed as rfid_decode_result::bits; the rest 0 */
  int32_t  reserved_[3];             /* 0 */
} rfid_sized_frame;

/* what the diversity stage (rfid_batch_diversity, rfid_diversity_window) makes of one EPC window of a GROUP of traces: the receive
 * antennas of one reader session, recorded together (a two-channel receiver, or several receivers on a common clock).  The decoder's
 * 128 decisions are the best one receive channel allows; a tag too weak for every antenna alone fails its CRC on each and is absent
 * from everything else a pass reports.  Adding the antennas' decision values before the sign is taken is maximum-ratio combining and
 * gains 10 log10 M dB.  The weights are conj(h_est) -- each antenna's own channel estimate, unnormalised: that is maximum-ratio
 * combining for EQUAL NOISE POWER on every antenna (no noise weighting).  A combined frame is NOT a read: nothing else the library
 * reports changes.
 * THE DEFINITION (the contract; binary32 throughout, every operation rounded by itself, no fused multiply-add):
 *   groups   rfid_batch_plan_diversity(ctx, M), 2 <= M <= RFID_DIVERSITY_MAX_MEMBERS.  The traces of a pass form groups of M consecutive
 *            rows: group g is traces g M .. g M + M - 1, member m of it trace g M + m.  Member 0 is the ANCHOR.
 *   rows     row k of group g is the anchor's EPC window seq = 2 k + 1, for every such window before the anchor's TERMINATED cut-off
 *            (seq < n_windows_used): nrows[g] = n_windows_used(anchor) / 2.  Rows behind it are zero.
 *   present  member m is present in row k when window 2 k + 1 lies before m's own cut-off, its result's type is RFID_DECODE_EPC and
 *            |start_m - start_0| <= RFID_DIVERSITY_SLACK filtered samples.  The slack is a definition, not a measurement: the decoder's
 *            sync absorbs 15 offsets within a window, and gates that opened further apart did not open on the same command edge.  The
 *            anchor is always present.
 *   read by some   a present member's own CRC held (type RFID_DECODE_EPC and crc_ok == 1): flags bit 0, `reads` the mask of such members,
 *            `frame` the four bit words of the lowest of them.  Nothing is combined: every field behind `frame` is 0.
 *   lone     no present member read it and fewer than two are present: flags bit 2.  Nothing is combined.
 *   combined neither.  For each present member, in ascending m, with that member's OWN values -- s = y - dc_est of its own window per
 *            component, its result's T, index, h_re, h_im -- the decoder's decision values (tag_decoder_impl.cc:171-190), j = 0 .. 127:
 *              ia = (int)((float)j * (2.0f * T) + (float)index),  ib = (int)(((float)(2 j) * T + T) + (float)index), both held inside
 *              0 .. 1369;  (dx, dy) = s[ia] - s[ib];  r_j = dx * h_re - dy * (-h_im).
 *            acc_j = r_j of the first present member, then acc_j = acc_j + r_j of each further one in order.  cur_j = acc_j > 0;
 *            bit_j = (cur_j != cur_(j-1)), cur_(-1) positive.  The decoder's CRC-16 (check_crc, :401-445) over bits 0 .. 111 against
 *            bits 112 .. 127: flags bit 1 when it holds.  crc_rcvd / crc_calc: the two words compared.  margin_min = min_j |acc_j|,
 *            weakest = the lowest j attaining it.  h_sq: from 0.0f, over the present members in order, h_sq = h_sq + (h_re * h_re +
 *            h_im * h_im).
 * A window with a non-finite sample: unspecified, as its decoding is. */
#define RFID_DIVERSITY_MAX_MEMBERS 8
#define RFID_DIVERSITY_SLACK       4   /* filtered samples */
typedef struct rfid_diversity {      /* 64 bytes */
  int32_t  stream, seq;              /* the ANCHOR's EPC window (rfid_window::stream / seq) */
  int32_t  start;                    /* rfid_window::start of that window */
  int32_t  flags;                    /* bit 0: read by some member (nothing combined); bit 1: the combined frame passes its CRC-16;
                                        bit 2: lone (nothing combined).  0: combined, and the frame fails */
  int32_t  present, reads;           /* member masks (bit m: member m): present in this row / present and its own CRC held */
  uint32_t frame[4];                 /* bit 0: the lowest reader's bits; combined: the combined frame's, packed as
                                        rfid_decode_result::bits; lone: 0 */
  int32_t  crc_rcvd, crc_calc;       /* combined: bits 112 .. 127 MSB first / the CRC computed over bits 0 .. 111; else 0 */
  float    h_sq;                     /* combined: sum of |h_est|^2 over the present members; else 0 */
  float    margin_min;               /* combined: min |acc_j|; else 0 */
  int32_t  weakest;                  /* combined: the lowest j with |acc_j| == margin_min; else 0 */
  int32_t  reserved_;                /* 0 */
} rfid_diversity;

/* what the match stage (rfid_batch_match, rfid_match_window) finds for one EPC window: which of a set of KNOWN tags' replies the
 * window most resembles.  Repair, retune, lengths and diversity all DECODE: the frame must come out whole and pass a CRC-16.  A tag
 * the pass already knows -- in this trace's inventory, or on a list the caller supplies -- has a known reply of 128 bits, and a known
 * reply is a known pattern of 128 signs: correlating the window's decision values against it is a matched filter over the whole frame
 * and needs no single decision to be right.  An attribution is NOT a read: nothing else the library reports changes, and whether a
 * score amounts to an attribution is the host's to say (rfid.batch.match_fields).
 * THE DEFINITION (the contract; binary32 throughout, every operation rounded by itself, no fused multiply-add), for an EPC window
 * with seq < n_windows_used:
 *   candidates   with a list set (rfid_batch_match_set_list): the list's frames in the caller's order, the same for every trace (flags
 *                bit 3).  Otherwise the entries of THIS trace's inventory of the same pass, in the inventory's order: a candidate's
 *                index is what rfid_tag_read::entry is.  An overflowed inventory: flags bit 1, nothing is searched.  No candidates:
 *                flags bit 2, nothing is searched.  A window whose own CRC held: flags bit 0, nothing is searched.
 *   r_j          j = 0 .. 127, exactly as in the rfid_read_quality definition above (from the window's own result h_re, h_im, T,
 *                index and s[i] = y[start + i] - dc).  sig_abs: the in-order sum of |r_j|, as rfid_read_quality::sig_abs.
 *   pattern      of a candidate frame b: the one sign sequence from which the decoder's own chain (bit_j = c_j XOR c_(j-1), the
 *                sign in front of the first one positive) yields b: c_j = 1 XOR b_0 XOR ... XOR b_j.
 *   score        (((0.0f + t_0) + t_1) + ...) + t_127 with t_j = r_j where c_j = 1 and -r_j otherwise.
 *   best         the candidate with the largest score (binary32 >), the smaller index on equal scores; second: the same rule over
 *                the rest.  Duplicates are allowed.  dist_best: the frame bits in which rfid_decode_result::bits differ from best's
 *                frame; diff: the decisions j on which best's and second's patterns differ.
 * Bits 1 to 3 of flags say what the trace's candidates are and stand in every row before the cut-off.  Where nothing is searched
 * every field behind flags is 0.  A candidate equal to the window's decoded frame scores sig_abs, bit for bit (a -0 term does not
 * disturb an in-order sum that starts from +0); a span negated under the same result record scores -sig_abs.  A window with a
 * non-finite sample: unspecified, as its decoding is. */
#define RFID_MATCH_MAX_LIST 1024
typedef struct rfid_match {          /* 64 bytes */
  int32_t  stream, seq, start;       /* the EPC window */
  int32_t  flags;                    /* bit 0: crc_ok of the window's result (nothing is searched)
                                        bit 1: candidates are this trace's inventory and it overflowed (nothing is searched)
                                        bit 2: no candidates (nothing is searched)
                                        bit 3: the candidates are the caller's list */
  int32_t  n_cand;                   /* candidates looked at */
  int32_t  best, second;             /* candidate indices; -1: none */
  float    score_best, score_second; /* 0.0f when none */
  float    sig_abs;                  /* as rfid_read_quality::sig_abs of the same window, bit for bit */
  int32_t  dist_best;                /* frame bits in which the window's decoded bits differ from best's frame; -1: none */
  int32_t  diff;                     /* decisions on which best's and second's sign patterns differ; -1: no second */
  uint32_t frame[4];                 /* best's frame, packed as rfid_decode_result::bits; zeros when none */
} rfid_match;

/* what the stack stage (rfid_batch_stack, rfid_stack_windows) finds for one EPC window: the CRC-failed windows near it that hold the
 * SAME frame, and what their decision values add up to.  Repair and retune work on one window alone, diversity needs several
 * antennas, match needs the tag's EPC.  A tag too weak in every round that nobody knows is asked for the same 128-bit frame round
 * after round: two failed windows that hold the same frame have strongly correlated decision values, two that hold different
 * frames, noise or collisions uncorrelated ones.  Adding the r_j of the windows that correlate, before the sign is taken, is
 * maximum-ratio combining over rounds (each r_j carries its own conj(h_est)); the CRC-16 then decides whether the sum is a frame.
 * rho_min is a DETECTION threshold; the CRC is the acceptance test.  A stacked frame is NOT a read: nothing else the library
 * reports changes.
 * THE DEFINITION (the contract; binary32 throughout, every operation rounded by itself, no fused multiply-add, every sum in order
 * from 0.0f, every tie to the lower index), for the EPC windows of a trace with seq < n_windows_used:
 *   failed rows  the EPC windows whose result is not a verified read (type EPC and crc_ok = 1 is one), in row order, numbered
 *                f = 0 .. F - 1: the ordinals.
 *   blocks       block q holds ordinals 64 q .. 64 q + 63 (RFID_STACK_BLOCK).  Partners are sought inside a window's own block only:
 *                the work on a trace with 100 000 failed windows stays bounded, and at one reply per tag and round 64
 *                consecutive failed windows span many rounds.
 *   r^f_j        j = 0 .. 127, the decision values of row f exactly as in the rfid_read_quality definition above (from the
 *                window's own start, dc, T, index and h_re, h_im).
 *   partner      for rows f != g of one block: s = sum_j (r^f_j * r^g_j), a = sum_j |r^f_j * r^g_j| (each product rounded once and
 *                used in both sums).  g is a partner of f iff s > 0 and s >= rho_min * a (the product on the right rounded once).
 *                The relation is symmetric bit for bit.
 *   members(f)   f together with its partners: member_mask has bit l set for ordinal 64 q + l, f's own bit included; n_partners
 *                = popcount - 1.  Without a partner nothing is combined: flags = 0 and every field behind member_mask is 0.
 *   combination  R_j = the sum of r^m_j over the members in ascending ordinal, the anchor in its place; the decoder's own sign chain
 *                (bit_j = (R_j > 0) XOR (R_(j-1) > 0), the sign in front of the first one positive) and CRC-16 over R.  sig_abs
 *                = sum_j |R_j|; margin_min = min_j |R_j|, weakest the lowest j that attains it.
 * Rows behind a trace's cut-off are zero.  A window with a non-finite sample: unspecified, as its decoding is. */
#define RFID_STACK_BLOCK 64
#define RFID_STACK_MAX_WINDOWS 64
typedef struct rfid_stack {          /* 64 bytes */
  int32_t  stream, seq, start;       /* the EPC window */
  int32_t  flags;                    /* bit 0: the window is a verified read (ordinal = -1, everything behind it 0)
                                        bit 1: a combination was formed (at least one partner)
                                        bit 2: the combination's CRC holds */
  int32_t  ordinal;                  /* f; -1 for a read */
  int32_t  n_partners;
  uint64_t member_mask;              /* bit l: ordinal 64 (f / 64) + l is a member; the window's own bit included */
  float    sig_abs;                  /* sum |R_j| */
  float    margin_min;               /* min |R_j| */
  int32_t  weakest;                  /* the lowest j with |R_j| = margin_min */
  int32_t  reserved_;                /* 0 */
  uint32_t frame[4];                 /* the combination's 128 bits whenever bit 1 is set, packed as rfid_decode_result::bits */
} rfid_stack;

/* what the collisions stage (rfid_batch_collisions, rfid_collisions_of) works out for one RN16 window: the two RN16s and the two
 * channels of a slot in which two tags replied at once.  The decoder is single-tag by construction (tag_detection_RN16,
 * lib/tag_decoder_impl.cc:114-142, 237-253): decision j is the difference d_j of two adjacent half-bit samples across a bit
 * boundary, and with two synchronous FM0 replies d_j = +-h1 +- h2 -- four points in the I/Q plane.  h1 + h2 is known: it is the
 * decoder's h_est, both tags send the same preamble.  Squared, the d_j fall into two clusters, one around (h1 + h2)^2 and one around
 * (h1 - h2)^2, 4 |h1| |h2| apart.  A record is worked out for EVERY RN16 window before the TERMINATED cut-off, whatever its slot
 * held: which slots collided is the slots stage's to say (rfid.batch.classify_collisions puts the two together, on the host).
 * THE DEFINITION (the contract; binary32 throughout, every operation rounded by itself, no fused multiply-add, every sum in order
 * from 0.0f, every division the correctly rounded binary32 quotient), from the window's rfid_window (start, dc) and its own
 * rfid_decode_result (index, hs = (h_re, h_im), bits[0]):
 *   samples    m = min(max(index - 65, 0), 14);  z_i = y[start + m + 65 + 5 i] - dc per component, i = 0 .. 31: the decoder's 32
 *              half-bit samples (the largest index is 234, inside the 250-sample window);  d_j = z_2j - z_2j+1 per component,
 *              j = 0 .. 15; below (dx, dy) = d_j.
 *   squares    sq(v) = (v.x * v.x - v.y * v.y, (2.0f * v.x) * v.y);  w_j = sq(d_j);  A = sq(hs);
 *              dist(p, q) = (p.x - q.x) * (p.x - q.x) + (p.y - q.y) * (p.y - q.y)
 *   clusters   two, the centre of one held at A.  The other starts at c = w_j*, j* the first j with the largest dist(w_j, A)
 *              (j* = 0; j = 1 .. 15: taken when dist(w_j, A) > the largest so far).  Four rounds: j is a member iff
 *              dist(w_j, c) < dist(w_j, A); with at least one member c becomes (sum of the members' w_j.x / (float)count, the
 *              same of w_j.y), j ascending; with none c stays.  One more assignment with the c of the fourth round gives the members
 *              that count below: n_diff of them, n_same = 16 - n_diff.
 *   channels   hs' = the sum over the NON-members, j ascending, of +d_j when dx * hs.x + dy * hs.y > 0.0f and of -d_j otherwise, per
 *              component, divided by (float)n_same; hs' = hs when n_same == 0.
 *              hd  = the sum over the members, j ascending, of +d_j when dx * r.x + dy * r.y > 0.0f and of -d_j otherwise, r the d_j
 *              of the member of lowest j, divided by (float)n_diff; hd = (0.0f, 0.0f) when n_diff == 0.
 *   decisions  for every j the nearest, by dist(d_j, P), of P0 = hs' (alpha, beta = +, +), P1 = -hs' (-, -), P2 = hd (+, -) and
 *              P3 = -hd (-, +): the first minimum in that order (P_k, k = 1 .. 3, is taken when its distance is < the smallest so
 *              far).  resid = the sum of the 16 smallest distances, sum_sq = the sum of dx * dx + dy * dy, both j ascending.
 *   handles    bit_j of the first tag = (alpha_j != alpha_j-1), alpha_-1 = + (the decoder's sign chain); its handle is the sum of
 *              bit_j << (15 - j): MSB first as sent, the convention of rfid_command's RN16.  The second tag's likewise from beta.
 *              dec = the decoder's own 16 bits in the same convention: the sum of ((bits[0] >> j) & 1) << (15 - j).
 *   labels     h1 = (hs' + hd) / 2.0f, h2 = (hs' - hd) / 2.0f per component.  Tag A is the first tag and tag B the second, unless
 *              h2.x * h2.x + h2.y * h2.y > h1.x * h1.x + h1.y * h1.y: then they swap, channels and handles both (flags bit 3).
 *              A is the stronger tag.
 * A record is a function of the input alone and is compared by bit pattern.  A window with a non-finite sample: unspecified.
 * What a host makes of it (rfid.batch.collision_fields, in binary64): |hA|, |hB| and their ratio in dB, the phase between them,
 * fit = resid / sum_sq -- small when four points explain the window, large when three or more tags replied -- and which of the two
 * handles, if any, the decoder handed to the ACK. */
typedef struct rfid_collision {      /* 64 bytes */
  int32_t  stream, seq;              /* the RN16 window (rfid_window::stream / seq) */
  int32_t  flags;                    /* bit 0: dec == rn16_a; bit 1: dec == rn16_b; bit 2: n_diff == 0 (one cluster: nothing to
                                        separate); bit 3: the two tags were swapped */
  int32_t  n_same, n_diff;           /* decisions around (h1 + h2)^2 / around (h1 - h2)^2 */
  int32_t  rn16_a, rn16_b;           /* the handles of tag A and tag B, 0 .. 65535 */
  float    ha_re, ha_im;             /* the channel of tag A, in the units of h_est */
  float    hb_re, hb_im;             /* ... of tag B */
  float    resid, sum_sq;
  float    c_re, c_im;               /* c of the last assignment: the centre around (h1 - h2)^2 */
  int32_t  reserved_;                /* 0 */
} rfid_collision;

/* the second-order moments of one window's gated samples: what the slots stage (rfid_batch_slots, rfid_window_moments_of)
 * works out for EVERY window before the TERMINATED cut-off, RN16 and EPC alike.  The reference ACKs every slot, so a
 * FIXED_Q > 0 trace yields an RN16 / EPC window pair per slot whatever was on the air; the moments tell an empty slot (an
 * isotropic noise blob) from a single reply (samples on a line along h) from a collision (samples spread over a plane).
 * THE DEFINITION (the contract; binary32 throughout, every operation rounded by itself, no fused multiply-add):
 *   for i = 0 .. RFID_MOMENTS_SAMPLES - 1:
 *     x_i = y[start + i].x - dc_re,  y_i = y[start + i].y - dc_im
 *   (y: the matched filter's output of the pass, start / dc: the window's rfid_window -- the gate's output samples), and the
 *   five sums are IN-ORDER sums (((0.0f + t_0) + t_1) + ...) + t_239 of t_i = x_i, y_i, x_i * x_i, x_i * y_i, y_i * y_i.  They
 *   start from 0.0f: a first term of -0.0 gives +0.0.  A record is a function of the input alone and is compared by bit
 *   pattern.  (A window with a non-finite sample: unspecified.)
 * 240 samples fit both window kinds: an RN16 reply ends by sample 244 of its 250; of an EPC window the preamble and the first
 * 17 bits are used.
 * What a host makes of it (rfid.batch.moment_fields / classify_slots, in binary64): the eigenvalues l1 >= l2 of the scatter
 * matrix per sample; the median l2 of a trace's EPC windows is its noise floor -- noise whether the slot was empty, single or
 * collided. */
#define RFID_MOMENTS_SAMPLES 240
typedef struct rfid_window_moments {   /* 32 bytes */
  int32_t stream, seq;                 /* the window (rfid_window::stream / seq); type = seq & 1 */
  float   sx, sy;                      /* sum x_i, sum y_i */
  float   sxx, sxy, syy;               /* sum x_i*x_i, sum x_i*y_i, sum y_i*y_i */
  int32_t flags;                       /* bit 0: crc_ok of the window's result (0 for RN16); bit 1: the window is an EPC window */
} rfid_window_moments;

/* the reader's own PIE command in front of one window: what the commands stage (rfid_batch_commands, rfid_commands_of) decodes
 * for EVERY window before the TERMINATED cut-off.  Every window the gate opens was opened by a reader command on the same
 * trace -- a Query or QueryRep before an RN16 window, an ACK before an EPC window -- at full carrier depth in the matched
 * filter's output just before the window's start.  The record names the command, its calibration symbols and its data bits,
 * and says whether an ACK echoes the RN16 decoded in the window before: a reader-side ground truth that needs no CRC.
 * THE DEFINITION (the contract; integer apart from one binary32 comparison per sample; a record is a function of the input
 * alone and is compared byte for byte), for a window with seq < n_windows_used, start a and dc (dr, di):
 *   samples  span position p = 0 .. RFID_CMD_SPAN - 1 is sample y[a - RFID_CMD_SPAN + p] of that trace; a position whose index
 *            is below 0 is HIGH (and flag bit 4 is set).  thr = 0.25f * (dr * dr + di * di); low[p] = (re * re + im * im) < thr,
 *            in binary32, every operation rounded by itself, no fused multiply-add: a sample exactly at thr is high, thr == 0
 *            means nothing is low.
 *   edges    a rising edge is at p (1 <= p < RFID_CMD_SPAN) iff low[p - 1] && !low[p].  n_edges counts all of them; only the
 *            last min(n_edges, RFID_CMD_MAX_EDGES) are kept: e_0 < ... < e_(n-1).
 *   command  the longest suffix c_0 .. c_(m-1) of the kept edges whose consecutive distances are all <= RFID_CMD_GAP;
 *            d_k = c_k - c_(k-1); n_syms = m; end = c_(m-1).
 *   m < 3    cmd = RFID_CMD_NONE; d0 = d_1 if m >= 2; everything else 0.
 *   m >= 3   d0 = d_1, rtcal = d_2; if m >= 4 and d_3 > rtcal: trcal = d_3 and the data starts at k = 4, otherwise trcal = 0 and
 *            the data starts at k = 3.  Data bit = (2 * d_k > rtcal); n_bits counts all data symbols, bits keeps the first 32.
 *   cmd      (patterns in the order the bits are sent)
 *            QUERY         trcal > 0, n_bits == 22, the first four bits 1000
 *            QUERY_REP     trcal == 0, n_bits == 4, the bits start with 00
 *            ACK           trcal == 0, n_bits == 18, the bits start with 01
 *            NAK           trcal == 0, n_bits == 8, the bits are 11000000
 *            QUERY_ADJUST  trcal == 0, n_bits == 9, the bits start with 1001
 *            UNKNOWN       anything else
 *   flags    see the field; bits 0, 3 and 4 describe the span and are set whatever m is, bit 5 only when m >= 3.  CRC-5: poly x^5 + x^3 + 1, preset 01001, MSB first, over bits 0..16, equal to bits 17..21.
 * Rows behind the cut-off are zero.  A non-finite sample in the span makes the record unspecified.
 * 704 = 11 x 64: the longest Query is 12 + 24 + 72 + 200 + 22 x 48 = 1 364 us = 546 samples, T1 to the opening adds 98. */
#define RFID_CMD_SPAN 704        /* decimated samples before a window's start that are searched: 11 x 64 */
#define RFID_CMD_MAX_EDGES 64    /* rising edges kept (the last ones) */
#define RFID_CMD_GAP 120         /* a longer distance between rising edges ends a command (1.5 x TRcal of 80) */
enum { RFID_CMD_NONE = 0, RFID_CMD_QUERY, RFID_CMD_QUERY_REP, RFID_CMD_ACK, RFID_CMD_NAK, RFID_CMD_QUERY_ADJUST, RFID_CMD_UNKNOWN };
typedef struct rfid_command {    /* 48 bytes */
  int32_t stream, seq;           /* the window the command opened */
  int32_t cmd;                   /* RFID_CMD_* */
  int32_t n_edges;               /* rising edges in the span, all of them (before the cap) */
  int32_t n_syms;                /* rising edges of the command, m above (0..64) */
  int32_t end;                   /* span position of the command's last rising edge (0 when n_syms == 0);
                                    RFID_CMD_SPAN - end = samples from it to the window's first sample */
  int32_t d0, rtcal, trcal;      /* in samples; 0 when absent */
  int32_t n_bits;                /* data symbols behind the frame-sync / preamble */
  uint32_t bits;                 /* data bit k (k-th sent, k < 32) at bit k -- the packing of rfid_decode_result::bits */
  int32_t flags;                 /* bit 0: EPC window (seq & 1); bit 1: Query whose CRC-5 holds; bit 2: ACK whose 16 RN bits
                                    equal the RN16 decoded in window seq - 1; bit 3: n_edges > 64; bit 4: span clipped at the
                                    trace's start; bit 5: 2 * d0 > rtcal (not a frame-sync) */
} rfid_command;

/* timing of the last rfid_batch_* pass, from HIP events on the ctx stream */
typedef struct rfid_batch_timing {
  float mf_ms, gate_ms, decode_ms, stats_ms; /* kernel time per pass (summed over the launches of a pass) */
  float total_ms;       /* wall time of the pass on the device (front end overlapped) */
  float front_ms;       /* wall time of matched filter + gate scan (they overlap on two streams) */
  int32_t front_chunks; /* launches of each of the two front-end kernels in the pass (1 = not chunked) */
  int32_t decode_launches; /* 2: one EPC launch, one RN16 launch */
  int32_t fused_front;  /* 1: rfid_batch_process ran the fused front end (matched filter inside the gate launch:
                           mf_ms = 0, gate_ms = the fused kernel); 2: the long-stream front end with the matched filter inside
                           its first launch (few, long traces: mf_ms = 0, gate_ms = its whole launch list) */
  int32_t reserved_;
} rfid_batch_timing;

/* what the long-stream front end did in the last rfid_batch_process pass (all zero when it was not used).  The front
 * end cuts each trace along time into pieces at idle points of the gate and processes all pieces at once: avg_ampl, then
 * the state machine -- from guessed start values whose runs are PROVEN to cover the true ones (or run again) -- then dc_est,
 * every unit from 64 neighbouring start values at once and the chain of their tables from the trace's exact start (round 6);
 * see csrc/rfid_ls2.hpp. */
typedef struct rfid_ls_report {
  int32_t pieces;           /* pieces the traces were cut into */
  int32_t units;            /* runs of pieces scanned in one go by the state-machine / dc_est passes (= pieces unless a cut
                             * turned out not to be idle: see cuts_dropped) */
  int32_t chunk;            /* nominal piece length, decimated samples */
  int32_t avg_rounds;       /* avg_ampl: chain rounds that had work (1 = every guess was proven at once) */
  int32_t avg_reruns;       /*   pieces run again from their predicted start because their first run did not cover it */
  int32_t fsm_rounds;       /* state machine: rounds */
  int32_t dc_rounds;        /* dc_est: rounds that had work (2: the first round's centres, the ring means, were off by the rounding
                             * drift; more: the sums hover at a binade edge and the settled prefix grew round by round) */
  int32_t dc_reruns;        /*   unit runs after the first round */
  int32_t verified;         /* 1: accepted -- every piece's latest run is exact or proven: the sequential scan, bit for bit */
  int32_t gave_up;          /* != 0: the sequential scan ran instead (1 no trace could be cut, 2 / 3: avg_ampl / state machine not
                             * settled within the round limit, 5: the first pass met a stretch of 32 nominal piece lengths
                             * without 128 carrier samples in a row).  dc_est never gives a pass up: see dc_finished */
  int32_t cuts_dropped;     /* cut points withdrawn because the state machine (or the dc ring) was not idle there */
  int32_t windows;          /* complete windows found */
  int32_t dc_finished;      /* dc_est units that were not settled when the enqueued rounds were used up and went through the
                             * finishing walk (one after the other from the proven value before them; the settled units kept
                             * their results): the partial fallback.  0: the rounds sufficed */
} rfid_ls_report;

/* One 64-sample step of the gate's edge / pulse / window state machine by itself (rfid_selftest_gate_fsm): the state in front
 * of the step and the two threshold-vote masks (sample i of the step = bit i; disjoint; no bit at or past nvalid) ... */
typedef struct {
  int32_t mode;             /* 0 batch (the gate re-arms behind a window), 1 per call (the scan stops where a window closes) */
  int32_t n_samples, signal_state, num_pulses, gate_open, n_to_ungate, wtype;
  int32_t nvalid;           /* valid samples of the step, 0 .. 64 */
  int32_t pos;              /* the step's first sample within the call (what `consumed` counts from) */
  int32_t reserved_;
  uint64_t below, above;    /* |x| < thresh, |x| > thresh */
} rfid_gate_fsm_in;
/* ... and what the step leaves: the state, which samples were "closed" (they update dc_est) and which lie in a window (the
 * opening sample is both), the opening (open_lane 0xff: none), nvalid as returned (cut where a per-call scan stops) */
typedef struct {
  int32_t n_samples, signal_state, num_pulses, gate_open, n_to_ungate, wtype;
  int32_t nvalid, stop;
  int32_t consumed;         /* pos + samples taken when stop is set, else 0 */
  int32_t open_lane, open_type;
  int32_t reserved_;
  uint64_t closedmask, openmask;
} rfid_gate_fsm_out;

/* The arithmetic primitives by themselves (rfid_selftest_arith): the operands of one 64-lane wave -- lane L takes x0[L], x1[L],
 * iv[L]; tile holds the 5 * 63 + 25 complex samples (re, im interleaved) of one matched-filter step ... */
typedef struct {
  float carry, carry_b;     /* the carries of the in-order sums */
  int32_t fill;             /* what the DPP building blocks leave in lanes without a source */
  int32_t reserved_;
  float x0[64], x1[64];
  int32_t iv[64];
  float tile[680];
} rfid_arith_in;
/* ... and what every routine made of them.  Flags are 0 / 1, vote masks have bit L = lane L.  Every field is stored over what
 * the caller put there, except f2i[L] where |x0[L]| >= 2^31 and reserved_, which keep the caller's words. */
typedef struct {
  float chain[64];          /* chain_add(carry, x0) */
  float scan[64];           /* chain_add_scan(carry, x0): the value as returned, whatever scan_flag says */
  float autosum[64];        /* chain_add_auto(carry, x0) */
  float pair0[64], pair1[64];       /* chain_add_scan_pair(carry, x0, x1), as returned */
  float pair_fb0[64], pair_fb1[64]; /* what the pair body falls back to: chain_add_auto(carry, x0), then from its lane 63 over x1 */
  float auto2_a[64], auto2_b[64];   /* chain_add_auto2(carry, carry_b, x0) */
  float chain2_a[64], chain2_b[64]; /* chain_add2(carry, x0, carry_b, x1) */
  float div100[64], div48[64];      /* div_const<100>(x0), div_const<48>(x0) */
  float fast100[64], fast48[64];    /* div_const_fast<100>(x0), div_const_fast<48>(x0), unguarded */
  float fdiv[64];           /* wv::fdiv(x0, x1) */
  float hypot[64];          /* wv::hypot_f(x0, x1) */
  float shr1[64];           /* wv::shr1(x0) */
  float rint[64];           /* wv::rint_f(x0) */
  int32_t f2i[64];          /* wv::f2i(rint[L]) where |x0[L]| < 2^31 */
  float sum25[128];         /* wv::lds_sum25_in_order(&tile[5 L]) from the tile staged in LDS as the filter wave stages it: re, im of lane L at [2 L], [2 L + 1] */
  float mf[128];            /* the stage kernel's (mf_boxcar25_decim5_kernel) plain 25-term loop over the same tile, likewise */
  int32_t scan_add[64];     /* wv::scan_add(iv) */
  int32_t row_shr1[64], row_shr2[64], row_shr4[64], row_shr8[64];   /* wv::dpp_row_shr<N>(iv, fill) */
  int32_t row_bcast15[64], row_bcast31[64], wave_shr1[64];          /* wv::dpp_row_bcast15 / 31, wv::dpp_wave_shr1 (iv, fill) */
  uint64_t div_bad;         /* div_const_bad(x0) */
  uint64_t div_ok;          /* the vote of div_const_ok(x0) */
  int32_t scan_flag, pair_flag, auto2_flag;   /* what chain_add_scan, chain_add_scan_pair, chain_add_auto2 returned */
  int32_t reserved_;
  float ends_a, ends_b;     /* chain_add2_ends from (carry, carry_b) over x0 / x1 staged in LDS */
} rfid_arith_out;

typedef struct rfid_ctx rfid_ctx;

/* ---- lifetime ------------------------------------------------------------------------ */
RFID_API int rfid_params_default(rfid_params *p);
/* device = HIP device ordinal.  Fails (RFID_ERR_NO_DEVICE) when it is not a gfx950 GPU. */
RFID_API int rfid_ctx_create(const rfid_params *p, int device, rfid_ctx **out);
RFID_API int rfid_ctx_destroy(rfid_ctx *ctx);
/* resets gate/decoder/reader state as the block constructors + initialize_reader_state()
 * do (lib/gate_impl.cc:41-70, lib/global_vars.cc:34-54) */
RFID_API int rfid_ctx_reset(rfid_ctx *ctx);
RFID_API const char *rfid_strerror(int status);
RFID_API const char *rfid_last_error(const rfid_ctx *ctx);
RFID_API const char *rfid_version(void);
/* RFID_MI355X_ABI of the library that was loaded: it changes whenever a struct of this header changes size or layout
 * (4: rfid_ls_report has 13 fields since round 3; 5: its last field is dc_finished since round 6; 6: rfid_repair and the repair stage; 7: rfid_window_moments and the slots stage; still 7 with rfid_command and the commands stage, which only add functions and one struct, and with the test entries rfid_selftest_inventory, a function, and rfid_selftest_arith, a function and two structs of its own).  A caller built against another value must not pass structs. */
RFID_API int rfid_abi_version(void);
/* device self-test of the wave-level primitives the kernels rely on (DPP wave shift,
 * IEEE division, double sqrt).  0 = all good, >0 = number of failing checks. */
RFID_API int rfid_selftest(rfid_ctx *ctx, int *n_failed);
/* test entry: the gate's step function on `n` caller-given records (host memory), each from its own state, in both forms the
 * kernels call it in: out_wave[k] with wave-uniform arguments (scalar unit), out_lane[k] with one record per lane.  The
 * caller holds the expected values (tests/gate_ref.py); nothing is judged here. */
RFID_API int rfid_selftest_gate_fsm(rfid_ctx *ctx, const rfid_gate_fsm_in *in, int n, rfid_gate_fsm_out *out_wave,
                                    rfid_gate_fsm_out *out_lane);
/* test entry: the arithmetic primitives under every kernel -- the in-order binary32 sums and their integer-scan shortcuts, the
 * three-instruction constant divisions and their admission votes, wv::fdiv / hypot_f / shr1 / rint_f / f2i, the matched filter's
 * in-order sum out of LDS, the integer wave scan and its DPP building blocks -- on `n` caller-given records (host memory), one
 * 64-lane workgroup per record.  out[n + 1] is copied to the device before the launches and back after them: every field is
 * stored over the caller's prefill, and out[n], a guard record, must come back as it went.  The caller holds the expected
 * values (tests/arith_ref.py); nothing is judged here. */
RFID_API int rfid_selftest_arith(rfid_ctx *ctx, const rfid_arith_in *in, int n, rfid_arith_out *out);
/* test entry: the per-trace statistics kernel by itself on a caller-given result table res[n_streams][wmax] (host memory;
 * wcount[s] <= wmax records of row s count), one workgroup of `waves` (1 .. 16) wavefronts per trace -- the batch path launches
 * 1, or 16 for wmax > 2048.  from_summaries != 0: the kernel reads the results' one-word summaries, made on the device as the
 * decoders make them, from an array sized as a plan's (n_streams * wmax + 4 words), instead of the records.  max_slot_number
 * (>= 1) is 2^fixed_q.  out[n_streams] is copied to the device before the launch and back after it.  The caller holds the
 * expected values (tests/stats_ref.py); nothing is judged here. */
RFID_API int rfid_selftest_stats(rfid_ctx *ctx, const rfid_decode_result *res, const int32_t *wcount, int n_streams, int wmax,
                                 int waves, int from_summaries, int max_slot_number, int max_num_queries,
                                 int number_unique_tags, rfid_stream_stats *out);
/* test entry: the inventory's and the tracks' kernels by themselves on a caller-given result table res[n_streams][wmax] (host
 * memory), in the launch sequence of rfid_batch_inventory + rfid_batch_tracks and with their choice of instantiation (a table of up
 * to 128 slots or of 1024; rows of up to 64 entries or of 512): the inventory, its offsets, its packed copy, the tracks' offsets, the
 * tracks.  wcount[s] (0 .. wmax) and n_windows_used[s] (any value) are what the statistics of a pass would hold for trace s: the
 * records before the smaller of the two count.  start[n_streams][wmax]: rfid_window::start of every window (stream, seq and type =
 * seq & 1 are filled in here).  waves: 1 or 16 wavefronts per trace -- the batch path launches 16 for wmax > 2048.  max_tags
 * (1 .. 512) and slots (a power of two in 2 .. 1024) as rfid_batch_plan_inventory and the inventory_slots knob set them; unlike a
 * plan's, slots may be smaller than 2 max_tags.  reads_cap: the capacity the tracks kernel is given; reads_len >= reads_cap (and
 * >= 1): the records of `reads`.
 * Outputs, every one copied to the device before the launches and back behind them, so that what the kernels leave alone comes back
 * as the caller filled it: rows[n_streams][max_tags], counts[n_streams], overflow[n_streams], head[2] (entries in all; the first
 * trace that overflowed, INT32_MAX when none did), ent_off[n_streams], packed[n_streams * max_tags], base[n_streams],
 * reads_head[1], offsets[n_streams * max_tags + 1], reads[reads_len].  The caller holds the expected values
 * (tests/inventory_ref.py, tests/tracks_ref.py); nothing is judged here.  RFID_ERR_INVALID / RFID_ERR_UNSUPPORTED for arguments
 * outside these ranges, as the planning calls answer. */
RFID_API int rfid_selftest_inventory(rfid_ctx *ctx, const rfid_decode_result *res, const int32_t *wcount,
                                     const int32_t *n_windows_used, const int32_t *start, int n_streams, int wmax, int waves,
                                     int max_tags, int slots, int64_t reads_cap, int64_t reads_len, rfid_tag_entry *rows,
                                     int32_t *counts, int32_t *overflow, int32_t *head, int32_t *ent_off, rfid_tag_entry *packed,
                                     int32_t *base, int32_t *reads_head, int64_t *offsets, rfid_tag_read *reads);

/* ---- (1) streaming, host buffers: one call per reference work() ----------------------- */
/* fir_filter_ccc(5,[1]*25): consumes all n_in samples, keeps the filter history and the decimation
 * phase inside ctx.  y[n] = sum_{k=0..24} x[5n-24+k], k ascending; output n is written by the call
 * that completes its decimation group x[5n .. 5n+4] (GNU Radio's sync_decimator: noutput =
 * ninput / decim), so a stream of N samples yields floor(N/5) outputs whatever the call sizes --
 * the same outputs as rfid_batch_mf / rfid_batch_process on the same samples. */
RFID_API int rfid_mf_work(rfid_ctx *ctx, const rfid_cf32 *in, int n_in, rfid_cf32 *out, int out_cap,
                          int *n_produced);
/* gate_impl::general_work: scans in[0..n_in), writes gated, DC-removed samples to out and
 * stops right after a window closes (consume_each(i+1), lib/gate_impl.cc:189-194).
 * *n_consumed / *n_written are the values the block passes to consume_each() / returns. */
RFID_API int rfid_gate_work(rfid_ctx *ctx, const rfid_cf32 *in, int n_in, rfid_cf32 *out, int out_cap,
                            int *n_consumed, int *n_written);
/* tag_decoder_impl::general_work: acts only when n_in >= n_samples_to_ungate.  RN16: writes 16
 * floats (0.0/1.0) to out_bits (port 0) and sets gen2_logic_status = SEND_ACK.  EPC: decodes,
 * checks CRC, updates the statistics.  *n_consumed as consume_each(); *n_produced = items
 * produced on port 0.  `res`/`scores` (nullable) receive the per-window details. */
RFID_API int rfid_decoder_work(rfid_ctx *ctx, const rfid_cf32 *in, int n_in, float *out_bits,
                               int out_cap, int *n_consumed, int *n_produced,
                               rfid_decode_result *res, rfid_scores *scores);
/* Look-ahead for the three per-block calls above.  Called block by block, every rfid_gate_work / rfid_decoder_work is
 * a host <-> device round trip for a few hundred samples (~6 per inventory slot: slower than one CPU core).  With the
 * look-ahead on, rfid_mf_work runs the WHOLE chain for the buffer it is handed (matched filter -> gate -> tag_decoder in
 * one submission, the machinery of rfid_stream_work, state carried on the device) and keeps the filter output, the
 * gate's windows -- their gated, DC-removed samples included -- and the decoder's results on the host; the gate / decoder
 * calls that follow are answered from there when their input is the data this library itself handed out (the gate's
 * input must be the matched filter's output, the decoder's input the gate's output: first and last sample of every
 * call are compared; anything else is RFID_ERR_STATE), with the same consume / produce counts, outputs and READER_STATE
 * transitions as without it (lib/gate_impl.cc:189-199, lib/tag_decoder_impl.cc:223,266,289,393-396).  The window types
 * are those of the reference's own control flow (RN16, EPC, RN16, ...: after an RN16 the reader always ACKs).
 * Since round 5 the calls GATHER: a rfid_mf_work call uploads and filters its own samples (its outputs are what it
 * returns) and a whole-chain pass over everything pending is submitted once 65 536 decimated samples have gathered
 * (rfid_lookahead_set_coalesce) -- a pass per 8 192-item scheduler buffer was a third of one CPU core's speed.  The pass
 * stays on the device while the next calls upload into the other buffer.
 * What lies behind the last idle point of the gate in the samples the passes have seen is not decided yet: a gate call
 * consumes up to there and no further.  A gate call that can decide nothing returns (0 consumed, 0 written) ONCE per
 * arrival of new samples -- the scheduler brings more; asked again without anything new (the input has paused or ended:
 * a scheduler calls a block again when its upstream neighbour is done), or shown 2 x the gathering threshold or more
 * (a bounded buffer must drain), it makes the device decide at once: the pass under way is waited for, a pass goes
 * over whatever is pending, and what even that leaves undecided goes through the exact per-call scan (the streaming
 * gate_scan_kernel from the carried state: gate_impl.cc:127-196 sample by sample, as without the look-ahead).  Every
 * sample is consumed and every window handed out whether or not rfid_lookahead_flush is ever called.
 * max_chunk_raw: the largest rfid_mf_work call to expect (a larger one goes through in pieces); the staging holds what
 * gathers + one such call.  Call before the first sample; rfid_ctx_reset switches it off.  Like rfid_stream_begin it runs
 * on a one-trace plan of its own: any rfid_batch_plan of the context is replaced.  (A reader that answers tags in
 * real time cannot wait for 164 ms of signal to gather: RFID_LOOKAHEAD=0 / no rfid_lookahead_enable is the path for that.) */
RFID_API int rfid_lookahead_enable(rfid_ctx *ctx, int64_t max_chunk_raw);
/* The same look-ahead keyed on the GATE's input, for a flowgraph whose matched filter is not this library's --
 * apps/reader.py:75 instantiates GNU Radio's own filter.fir_filter_ccc, so with that file unchanged the first buffer
 * this library sees is the gate's (apps/reader.py:76,106-107).  rfid_gate_work then uploads whatever part of its input
 * the device has not seen yet (a scheduler shows unconsumed samples again; the new ones lie behind them), runs
 * gate -> tag_decoder over it in one submission from the carried state, and answers this and the following gate /
 * decoder calls from the cache, exactly as above (same consume / produce counts, outputs and READER_STATE transitions,
 * same rules for what is undecided, rfid_lookahead_flush at the end of the input).  There is no restriction on where the
 * gate's input comes from; rfid_mf_work is not to be called on such a context.  max_items: decimated samples the device
 * takes per call at most (a larger call is taken in parts).  Call before the first sample.  The end of the input needs
 * no announcement (see above: the second fruitless call decides everything); rfid_lookahead_flush saves that one call. */
RFID_API int rfid_lookahead_enable_gate(rfid_ctx *ctx, int64_t max_items);
/* How many decimated samples gather before a whole-chain pass is submitted (default 65 536; clamped to [1 024, half the
 * staging]).  An adaptor that knows its scheduler's buffers tells the library here: with input buffers of C items the
 * gate can never be shown more than C, so it asks for C / 4 (a gate call shown 2 x this many items decides at once). */
RFID_API int rfid_lookahead_set_coalesce(rfid_ctx *ctx, int64_t items);
/* Late filter outputs (look-ahead keyed on rfid_mf_work only; off by default).  A rfid_mf_work call that returns its own
 * outputs waits for its samples' way through the device: ~17-28 us per call, a third of a block-by-block run at GNU Radio's
 * default buffers.  With late outputs on, a call stages and filters its samples as before but RETURNS OUTPUTS OF THE CALLS
 * BEFORE IT -- whatever the device has finished meanwhile, oldest first, as far as out_cap goes -- and holds its own back
 * (unless the device is through with them before the call returns):
 * *n_produced is what earlier calls made, not n_in / 5 of this one (it may be 0: the call has consumed its input all the
 * same).  A gr::block may do that (general_work consumes and produces what it says): the adaptor's forecast() asks for no
 * input while outputs are held back, so a scheduler calls the block again at the end of the input -- with n_in = 0: such a
 * call hands out what is held back (waiting for the device if need be: it always hands out something; also after
 * rfid_lookahead_flush) and does nothing else.  At most three sets of outputs are held back: a call that brings new
 * samples while three are held needs room for the rest of the oldest (RFID_ERR_CAPACITY otherwise, nothing consumed) -- an
 * adaptor whose output room is smaller than rfid_mf_pending() simply calls with n_in = 0 first.  A call takes at most the
 * max_chunk_raw given to rfid_lookahead_enable.  The gate / decoder calls see no difference: the gate is shown the
 * filter's outputs a call or two later, the passes run over what was uploaded. */
RFID_API int rfid_lookahead_set_late_outputs(rfid_ctx *ctx, int on);
/* filter outputs a late-outputs context holds back (0 otherwise) */
RFID_API int rfid_mf_pending(const rfid_ctx *ctx, int *n_outputs);
/* ... and how many of them the next call must have room for if it brings new samples (0 unless three sets are held back: then
 * what is left of the oldest) */
RFID_API int rfid_mf_must_fetch(const rfid_ctx *ctx, int *n_outputs);
/* What the adaptor knows about its scheduler: the buffer on the gate's input side holds gate_buffer_items items and no more
 * (GNU Radio: detail()->input(0)->max_possible_items_available(); 65 536-byte buffers = 8 192 items by default), or 0: the
 * queues between the blocks grow as needed (the single-threaded scheduler of rfid/mi355x.h).  Bounded: a quarter of the
 * buffer gathers before a pass, and a gate call that can decide nothing never answers (0, 0) -- it makes the device
 * decide at once (a block that moves nothing is, depending on the runtime, polled again at once or left alone for good:
 * neither helps anything gather).  Unbounded (the default): (0, 0) once per arrival of new samples, see above. */
RFID_API int rfid_lookahead_set_scheduler(rfid_ctx *ctx, int64_t gate_buffer_items);
/* Consume ahead (either keying; off by default; before the first gate call).  As described above, a gate call consumes up to
 * the point its windows are known and no further -- under a scheduler with small bounded buffers the buffer in front of
 * the gate is then full of samples the device already has, and nothing gathers.  With consume-ahead on, rfid_gate_work
 * CONSUMES EVERYTHING IT IS SHOWN (keyed on the gate: uploads it) and hands out the windows when the passes have found
 * them: the same windows, the same samples, in the same order, one window per call at most, the next one only after the
 * decoder / reader calls have armed the gate for it (gate_impl.cc:112-123) -- only *n_consumed no longer says where the
 * windows lie.  A call may bring no input (n_in = 0; out_cap >= 1): it hands out what has become known.  Nothing is forced in
 * this mode, so the adaptor must do two things a gr::block can do: (1) forecast() through rfid_gate_forecast -- the gate
 * needs no input while a window lies ready for it, or when its upstream neighbour is done and the device still holds
 * undecided samples; (2) when general_work is called with its upstream done and no input left, call rfid_lookahead_flush
 * (which then decides everything, whatever the keying) before rfid_gate_work.  rfid_lookahead_set_scheduler's bounded mode
 * is switched off by it (the gathering threshold goes back to 65 536). */
RFID_API int rfid_lookahead_set_consume_ahead(rfid_ctx *ctx, int on);
/* forecast() of a consume-ahead gate: *needs_input = 0 when a rfid_gate_work call can do something without input (see above),
 * 1 otherwise (always 1 without consume-ahead: the reference's forecast, gate_impl.cc:79-83).  upstream_done: the block that
 * feeds the gate has finished (GNU Radio: detail()->input(0)->done()). */
RFID_API int rfid_gate_forecast(const rfid_ctx *ctx, int upstream_done, int *needs_input);
/* windows the look-ahead holds: found by the passes and not yet (completely) handed out by rfid_gate_work /
 * handed out and waiting for their rfid_decoder_work call (a decoder call retires its window whether or not it asks for
 * scores).  Both stay small in a running flowgraph. */
RFID_API int rfid_lookahead_pending(const rfid_ctx *ctx, int *gate_windows, int *decoder_windows);
/* End of the input (a file source has run dry): everything still held back is decided now; the gate / decoder / reader
 * calls that follow hand it out.  rfid_mf_work fails with RFID_ERR_STATE afterwards.  No-op without look-ahead.
 * Optional since round 5: a flowgraph that never calls it loses nothing (the gate's second fruitless call decides what
 * is held back), it only pays that one extra call. */
RFID_API int rfid_lookahead_flush(rfid_ctx *ctx);
/* The flowgraph has stopped (gr::block::stop()) and no gate / decoder call will come any more: whatever the device still
 * holds is decided as at the end of a stream, and the windows nobody fetched are accounted in READER_STATE as the decoder /
 * reader calls would have accounted them, so that rfid_print_results counts them.  Under a scheduler that calls the blocks
 * until none can move there is nothing left to do here; it is the safety net for one that gives up earlier. */
RFID_API int rfid_lookahead_drain(rfid_ctx *ctx);
/* Page-locked host memory (nullptr on failure): samples handed to rfid_mf_work (look-ahead) / rfid_stream_work from such
 * memory -- or from any memory the caller page-locked himself -- go to the device without the staging copy. */
RFID_API void *rfid_host_alloc(size_t bytes);
RFID_API void rfid_host_free(void *p);
/* |out[i]|^2 of the samples the last rfid_gate_work wrote (READER_STATE::magn_squared_samples, lib/gate_impl.cc:171,175,186),
 * computed on the device with the reference's expression re*re + im*im.  Look-ahead mode only (else *n = 0). */
RFID_API int rfid_gate_magn_squared(rfid_ctx *ctx, float *out, int cap, int *n);
/* reader_impl::general_work, state transitions only (gate_status / decoder_status /
 * n_queries_sent) without the transmit waveform (see rfid_reader_work_tx).  n_in = float items
 * available on the reader's input (16 after an RN16). */
RFID_API int rfid_reader_work(rfid_ctx *ctx, int n_in, int *n_consumed);
/* reader_impl::general_work complete: the same state transitions AND the transmit waveform the block writes
 * to its output for the state it was in (lib/reader_impl.cc:43-129 tables, :200-380; float samples 0/1 at
 * dac_rate, e.g. preamble + 22 PIE-coded Query bits + 1295 us of carrier).  in_bits: the reader's float input
 * (the 16 RN16 bits when the state is SEND_ACK), n_in its item count.  *n_written = floats written to out
 * (what general_work returns); RFID_ERR_CAPACITY (state untouched) when out_cap is too small --
 * rfid_reader_tx_max(dac_rate) floats always suffice. */
RFID_API int rfid_reader_work_tx(rfid_ctx *ctx, int dac_rate, const float *in_bits, int n_in, float *out, int out_cap,
                                 int *n_consumed, int *n_written);
RFID_API int rfid_reader_tx_max(int dac_rate);
RFID_API int rfid_get_state(const rfid_ctx *ctx, rfid_reader_state *out);
/* reader_impl::print_results text (lib/reader_impl.cc:173-192) */
RFID_API int rfid_print_results(const rfid_ctx *ctx, char *buf, int cap, int *len);


/* ---- (1b) streaming, whole chain per call: raw chunk in -> decoded windows out ------------------------------------ */
/* The drop-in calls above cross the host / device boundary three times per buffer.  This family runs
 * matched filter -> gate -> tag_decoder for one RX stream in ONE submission per chunk, with all block state carried
 * on the device (filter history, gate state incl. both rings, window alternation, READER_STATE), and overlaps the
 * host -> HBM copy of chunk k+1 with the processing of chunk k (two pinned staging buffers, a copy stream).
 * The gate scan of a chunk uses the long-stream front end (units scanned concurrently, accepted only when bit-identical
 * to the sequential scan), so a single stream is not limited to one SIMD.  Results equal rfid_batch_process over the
 * concatenated stream, window for window. */
typedef struct rfid_stream_window {
  int64_t start;          /* index (400 ksps domain, from the start of the stream) of the first gated sample */
  int32_t type;           /* RFID_DECODE_RN16 / RFID_DECODE_EPC */
  int32_t reserved_;
  float dc_re, dc_im;     /* gate_impl::dc_est at the opening */
} rfid_stream_window;

/* Allocates the staging (2 pinned host buffers + 2 device buffers of max_chunk_raw samples, plus room for the samples a
 * call leaves unprocessed) and resets the stream (fresh blocks).  Replaces any batch plan of the context. */
RFID_API int rfid_stream_begin(rfid_ctx *ctx, int64_t max_chunk_raw);
/* the two pinned staging buffers (idx 0 / 1): filling them directly makes the upload a true asynchronous DMA; any other
 * host pointer passed to rfid_stream_work is first copied into one of them */
RFID_API int rfid_stream_staging(rfid_ctx *ctx, int idx, rfid_cf32 **host, int64_t *cap);
/* Hands over n_raw NEW samples (their upload starts at once) and processes the chunk handed over by the PREVIOUS call
 * while that upload runs; flush != 0 also processes the new samples and everything held back (end of stream).
 * A call holds back what follows the last idle point of the gate's state machine (the reference's blocks do the same
 * through consume_each(): lib/gate_impl.cc:189-199, lib/tag_decoder_impl.cc:223,291); held-back samples are processed
 * with a later call.  windows / results (cap entries each, in stream order) receive the windows completed by this call,
 * *n_out their number (RFID_ERR_CAPACITY if cap is too small: nothing is lost, call again with larger arrays and
 * n_raw = 0).  READER_STATE (rfid_get_state, rfid_print_results) advances as in the per-block calls.
 * raw may be page-locked host memory -- one of the staging buffers or the caller's own (hipHostMalloc, hipHostRegister,
 * a pinned torch tensor): it is then uploaded by DMA straight from there and must stay untouched until the NEXT call
 * has returned -- or ordinary host memory, which is first copied into the staging buffer of the call (free on return). */
RFID_API int rfid_stream_work(rfid_ctx *ctx, const rfid_cf32 *raw, int64_t n_raw, int flush, rfid_stream_window *windows,
                              rfid_decode_result *results, int64_t cap, int64_t *n_out);
RFID_API int rfid_stream_end(rfid_ctx *ctx);

/* ---- (2) batched offline, device buffers ---------------------------------------------- */
/* Plans workspace for n_streams traces of up to max_raw samples each (2 Msps domain).
 * Allocates, in HBM: matched-filter output [n_streams][max_raw/5], window tables, results.
 * On failure (e.g. RFID_ERR_HIP: out of memory) the context is left WITHOUT a plan: every later
 * rfid_batch_* call returns RFID_ERR_STATE until a plan succeeds. */
RFID_API int rfid_batch_plan(rfid_ctx *ctx, int n_streams, int64_t max_raw);
/* Number of traces (rows of d_raw, entries of d_lens) the following rfid_batch_* calls process:
 * 1 <= n_streams <= the planned count (rfid_batch_plan sets it to the planned count).  Lets one plan
 * serve batches of different sizes; results and statistics cover exactly these rows. */
RFID_API int rfid_batch_set_streams(rfid_ctx *ctx, int n_streams);
/* d_raw: device pointer to [n_streams][raw_stride] rfid_cf32; d_lens: device int64[n_streams]
 * valid sample counts per trace, or NULL when every trace has n_raw samples.  All launches
 * go to the ctx stream (a non-blocking stream of its own, see rfid_ctx_stream) and return without
 * synchronising: work the caller queued on OTHER streams that produces d_raw / d_lens must be
 * complete (or ordered before the ctx stream with an event) when these functions are called. */
RFID_API int rfid_batch_mf(rfid_ctx *ctx, const void *d_raw, int64_t raw_stride, int64_t n_raw,
                           const void *d_lens);
RFID_API int rfid_batch_gate(rfid_ctx *ctx);
RFID_API int rfid_batch_decode(rfid_ctx *ctx, int want_scores);
RFID_API int rfid_batch_stats(rfid_ctx *ctx);
/* mf -> gate -> decode -> stats on the ctx stream (asynchronous).  Matched filter and gate run as ONE launch
 * (fused front end: the raw samples are read from HBM once); results are identical to calling the four stage
 * functions above one after the other.  The matched-filter output stays available (rfid_batch_get_mf). */
RFID_API int rfid_batch_process(rfid_ctx *ctx, const void *d_raw, int64_t raw_stride, int64_t n_raw,
                                const void *d_lens, int want_scores);
/* Long-stream front end of rfid_batch_process: with few, long traces the gate scan (a sequential recurrence per
 * trace) leaves the chip idle, so each trace is cut along time at idle points of the gate's state machine and all
 * pieces are processed at once from guessed start values; a pass is accepted only when every piece's run is exact or
 * provably covers its true start value, i.e. the result IS the sequential scan (otherwise the sequential scan runs:
 * it is enqueued behind the front end and skips itself when that succeeded -- a pass has no host synchronisation).
 * mode 0: never, 1 (default): when it is expected to be faster than the fused front end -- few traces, long enough
 * (a cost estimate from the batch size and the trace length, calibrated on the device when the context is created),
 * 2: whenever a trace can be cut.  The environment variable RFID_LONG_STREAM overrides the default.
 * rfid_batch_ls_report synchronises with the pass. */
RFID_API int rfid_batch_set_long_stream(rfid_ctx *ctx, int mode);
RFID_API int rfid_batch_ls_report(const rfid_ctx *ctx, rfid_ls_report *out);
/* The switches the environment can set (INTEGRATION.md section 13 lists them: RFID_LONG_STREAM, RFID_OVERLAP,
 * RFID_LS_CALIBRATE, RFID_LS_DEBUG, RFID_LA_PROFILE, RFID_LA_UPLOAD_KERNEL, RFID_LS_FRONT_LDS_KB and the test hooks
 * RFID_FRONT_UNFUSED / RFID_FRONT_SINGLE_STEP / RFID_FRONT_CHUNKS / RFID_LS2_FSM_LANES_MIN / RFID_LS2_DC_ROUNDS / RFID_INVENTORY_SLOTS / RFID_COMMANDS_ROWS).  The environment is read ONCE,
 * by rfid_ctx_create; these two change / read a value of a living context by its lower-case name without the RFID_
 * prefix ("overlap", "front_chunks", ...; LS2_FSM_LANES_MIN is "fsm_lanes_min", LS2_DC_ROUNDS "dc_rounds").  RFID_ERR_INVALID: unknown name or a
 * value outside the knob's range.  A change that concerns buffers (overlap) takes effect with the next rfid_batch_plan. */
RFID_API int rfid_ctx_set_knob(rfid_ctx *ctx, const char *name, int value);
RFID_API int rfid_ctx_get_knob(const rfid_ctx *ctx, const char *name, int *value);
RFID_API int rfid_batch_sync(rfid_ctx *ctx);
/* synchronises, then reports per-kernel times of the last pass */
RFID_API int rfid_batch_timing_get(rfid_ctx *ctx, rfid_batch_timing *out);
/* host copies of the results of the last pass (synchronising).
 * windows/results/scores: up to cap entries, ordered by (stream, seq); *n = total count. */
RFID_API int rfid_batch_get_stats(rfid_ctx *ctx, rfid_stream_stats *out, int n_streams);
RFID_API int rfid_batch_get_windows(rfid_ctx *ctx, rfid_window *windows, rfid_decode_result *results,
                                    rfid_scores *scores, int64_t cap, int64_t *n);
/* device-side views for callers that keep everything in HBM */
RFID_API int rfid_batch_device_ptrs(rfid_ctx *ctx, void **d_mf_out, int64_t *mf_stride,
                                    void **d_stats, void **d_flat_count);
/* copies the matched-filter output of trace `stream` to host (debug tap, the
 * file_sink_matched_filter of apps/reader.py:69) */
RFID_API int rfid_batch_get_mf(rfid_ctx *ctx, int stream, rfid_cf32 *out, int64_t cap, int64_t *n);
/* copies the gated, DC-removed samples of window `seq` of trace `stream` to host -- in[i] - dc_est over the window,
 * exactly what the gate block writes to its output (lib/gate_impl.cc:176,187; debug tap = the file_sink_gate of
 * apps/reader.py:70).  *n = window length (250 / 1370). */
RFID_API int rfid_batch_get_gated(rfid_ctx *ctx, int stream, int seq, rfid_cf32 *out, int64_t cap, int64_t *n);
/* ---- (2b) batch inventory: the tags that were read, per trace, built on the device -------------------------------- */
/* The statistics of a pass count reads per ONE byte of the EPC (tag_reads[256], the reference's std::map); these calls
 * list every distinct 128-bit frame of every trace (rfid_tag_entry) without the results leaving HBM: a pass hands the
 * host 48 bytes per tag instead of 48 bytes per window.  Results are independent of the order in which the device gets
 * to the windows (integer atomics only): the same pass gives the same bytes.
 * rfid_batch_plan_inventory reserves the workspace of the current plan for up to max_tags_per_trace distinct frames per
 * trace (1..512; RFID_ERR_UNSUPPORTED above); a new rfid_batch_plan drops it. */
RFID_API int rfid_batch_plan_inventory(rfid_ctx *ctx, int max_tags_per_trace);
/* enqueues the inventory of the LAST pass behind its statistics (asynchronous, no host synchronisation): the traces of
 * rfid_batch_set_streams, the result set and statistics of that pass also when two result sets alternate.
 * RFID_ERR_STATE: no plan / no inventory workspace / no pass with statistics yet */
RFID_API int rfid_batch_inventory(rfid_ctx *ctx);
/* synchronises; entries ordered by (stream, first_seq); *n = total; counts (nullable): entries per trace, n_streams ints.
 * RFID_ERR_CAPACITY: cap too small (nothing lost: *n says how many there are, call again; entries may be NULL with
 * cap = 0), or a trace overflowed max_tags_per_trace (rfid_last_error names the first such trace; such traces list
 * nothing, plan a larger inventory and run it again) */
RFID_API int rfid_batch_get_inventory(rfid_ctx *ctx, rfid_tag_entry *entries, int64_t cap, int64_t *n, int32_t *counts);
/* synchronises; device time of the last rfid_batch_inventory (HIP events), from its first launch to the end of its last */
RFID_API int rfid_batch_inventory_ms(rfid_ctx *ctx, float *ms);
/* ---- (2c) batch tracks: every tag's reads in time order, built on the device -------------------------------------- */
/* Behind the inventory of a pass: one rfid_tag_read per read the inventory counts (EPC window, crc_ok == 1, window
 * index < n_windows_used), ONE array ordered by (stream, entry, seq) -- grouped by tag, each tag's reads in time order.
 * The order is total and every place is computed, not raced for: the bytes of a pass are a function of its input.
 * A trace whose inventory overflowed lists no reads, as it lists no entries.
 * rfid_batch_plan_tracks reserves the workspace of the current plan (ceil(wmax / 2) reads per trace: EPC windows are
 * every other window).  RFID_ERR_STATE without an inventory workspace; RFID_ERR_HIP when the allocation fails (the
 * plan and the inventory workspace stay usable).  A new rfid_batch_plan and a new rfid_batch_plan_inventory drop it. */
RFID_API int rfid_batch_plan_tracks(rfid_ctx *ctx);
/* enqueues the tracks of the LAST pass behind its inventory (asynchronous, no host synchronisation).
 * RFID_ERR_STATE: no tracks workspace, or no rfid_batch_inventory was enqueued since the last pass */
RFID_API int rfid_batch_tracks(rfid_ctx *ctx);
/* synchronises; *n = reads in all; offsets (nullable): n_entries + 1 values aligned with the packed entries of
 * rfid_batch_get_inventory -- reads offsets[i] .. offsets[i + 1] belong to entry i, offsets[i + 1] - offsets[i] ==
 * entries[i].reads.  RFID_ERR_CAPACITY: cap too small (nothing lost: *n says how many there are, call again; reads may
 * be NULL with cap = 0), or a trace overflowed the inventory (rfid_last_error names the first such trace) */
RFID_API int rfid_batch_get_tracks(rfid_ctx *ctx, rfid_tag_read *reads, int64_t cap, int64_t *n, int64_t *offsets);
/* synchronises; device time of the last rfid_batch_tracks (HIP events), from its first launch to the end of its last */
RFID_API int rfid_batch_tracks_ms(rfid_ctx *ctx, float *ms);
/* ---- (2d) batch read quality: per-read SNR and decision margin, built on the device -------------------------------- */
/* Behind the tracks of a pass: one rfid_read_quality (see its definition above) per EPC window with seq < n_windows_used,
 * CRC-verified or not, in a device table [n_streams][ceil(wmax / 2)] (row = seq >> 1; the rows of a trace behind its
 * cut-off are zeroed: the table's bytes repeat from pass to pass), and the records of the CRC-verified reads once more as
 * ONE array aligned with the tracks: quality[i] belongs to reads[i] of rfid_batch_get_tracks.
 * rfid_batch_plan_quality reserves both (2 x 32 bytes per possible EPC window).  RFID_ERR_STATE without a tracks
 * workspace; RFID_ERR_HIP when the allocation fails (the plan, the inventory and the tracks workspace stay usable).  A
 * new rfid_batch_plan, rfid_batch_plan_inventory or rfid_batch_plan_tracks drops it. */
RFID_API int rfid_batch_plan_quality(rfid_ctx *ctx);
/* enqueues the quality of the LAST pass behind its tracks (asynchronous, no host synchronisation).  RFID_ERR_STATE: no
 * quality workspace, or no rfid_batch_tracks was enqueued since the last pass.
 * It reads that pass's matched-filter output, window table, results and statistics on the context's main stream.  With two
 * result sets alternating (RFID_OVERLAP=2) all four belong to the set and the next pass's front end, on the same stream,
 * runs behind it.  The long-stream front end alternates the matched-filter output alone and starts a pass's first launch on
 * the second stream as soon as its buffer is free: this call records that buffer's "free" event again behind its own
 * launches, so the pass after next, which gets the buffer, waits for them. */
RFID_API int rfid_batch_quality(rfid_ctx *ctx);
/* synchronises; *n = reads in all, the number rfid_batch_get_tracks reports; q[i] belongs to its reads[i].
 * RFID_ERR_CAPACITY as there: cap too small (nothing lost: *n says how many there are, call again; q may be NULL with
 * cap = 0), or a trace overflowed the inventory (rfid_last_error names the first such trace) */
RFID_API int rfid_batch_get_quality(rfid_ctx *ctx, rfid_read_quality *q, int64_t cap, int64_t *n);
/* synchronises; debug tap (as rfid_batch_get_mf) and the way to look at failed slots: one trace's row of the table, every
 * EPC window before the cut-off in seq order, failed ones included: *n = n_windows_used / 2 as the statistics count it.
 * RFID_ERR_CAPACITY when cap < *n (nothing is copied; q may be NULL with cap = 0).  With cap > *n the table's rows behind
 * *n are copied too, up to min(cap, ceil(wmax / 2)) records in all: they are zero. */
RFID_API int rfid_batch_get_window_quality(rfid_ctx *ctx, int stream, rfid_read_quality *q, int64_t cap, int64_t *n);
/* synchronises; device time of the last rfid_batch_quality (HIP events), from its first launch to the end of its last */
RFID_API int rfid_batch_quality_ms(rfid_ctx *ctx, float *ms);
/* ---- (2e) batch repair: CRC-failed EPC frames recovered from their weakest decisions, built on the device ------------- */
/* Behind the inventory of a pass: one rfid_repair (see its definition above) per EPC window with seq < n_windows_used in a
 * device table [n_streams][ceil(wmax / 2)] (row = seq >> 1; the rows of a trace behind its cut-off are zeroed: the table's
 * bytes repeat from pass to pass), and the records with n_flips > 0 once more as ONE array ordered by (stream, seq).  Nothing
 * else a pass reports changes: results, statistics, inventory, tracks and quality know nothing of a repair.
 * rfid_batch_plan_repair reserves both (2 x 48 bytes per possible EPC window) and the counts and offsets between them.
 * RFID_ERR_STATE without an inventory workspace; RFID_ERR_HIP when the allocation fails (the plan and every other workspace
 * stay usable).  A new rfid_batch_plan or rfid_batch_plan_inventory drops it; it neither needs nor drops the tracks and
 * quality workspaces, and rfid_batch_plan_tracks / rfid_batch_plan_quality do not drop it. */
RFID_API int rfid_batch_plan_repair(rfid_ctx *ctx);
/* enqueues the repair of the LAST pass behind its inventory (asynchronous, no host synchronisation).  RFID_ERR_STATE: no
 * repair workspace, or no rfid_batch_inventory was enqueued since the last pass.  A side branch: rfid_batch_tracks and
 * rfid_batch_quality may be enqueued before or behind it.  It reads that pass's matched-filter output, window table, results,
 * statistics and inventory on the context's main stream and has rfid_batch_quality's duties there: with two result sets
 * alternating it reads the set of that pass, and it records the long-stream front end's "free" event of the matched-filter
 * buffer again behind its own launches. */
RFID_API int rfid_batch_repair(rfid_ctx *ctx);
/* synchronises; the records with n_flips > 0 of the last rfid_batch_repair, ordered by (stream, seq): every place is
 * computed, the same pass gives the same bytes.  RFID_ERR_CAPACITY: cap too small (nothing lost: *n says how many there
 * are, call again; out may be NULL with cap = 0).  An overflowed inventory is NOT an error here: the records of such a trace
 * carry flag bit 1 and entry = -1. */
RFID_API int rfid_batch_get_repairs(rfid_ctx *ctx, rfid_repair *out, int64_t cap, int64_t *n);
/* synchronises; one trace's row of the table: every EPC window before the cut-off in seq order, verified, repaired or not:
 * *n = n_windows_used / 2.  cap as rfid_batch_get_window_quality: RFID_ERR_CAPACITY when cap < *n (nothing is copied; out may
 * be NULL with cap = 0); with cap > *n the zeroed rows behind *n are copied too, up to min(cap, ceil(wmax / 2)) in all. */
RFID_API int rfid_batch_get_window_repairs(rfid_ctx *ctx, int stream, rfid_repair *out, int64_t cap, int64_t *n);
/* synchronises; device time of the last rfid_batch_repair (HIP events), from its first launch to the end of its last */
RFID_API int rfid_batch_repair_ms(rfid_ctx *ctx, float *ms);
/* the same search for ONE window in host memory: the per-call form (as rfid_decoder_work) for callers that work block by
 * block.  gated: the window's 1 370 gated, DC-free samples (what rfid_gate_work wrote / rfid_decoder_work read); res: the
 * result rfid_decoder_work gave for it (type RFID_DECODE_EPC, else RFID_ERR_INVALID).  One launch of the batch kernel's
 * device function, synchronising.  out: stream = seq = start = 0, entry = -1; flags bit 0 = res->crc_ok (then nothing is
 * searched). */
RFID_API int rfid_repair_window(rfid_ctx *ctx, const rfid_cf32 *gated, const rfid_decode_result *res, rfid_repair *out);
/* ---- (2f) batch slots: the second-order moments of every window, built on the device ---------------------------------- */
/* Behind a pass: one rfid_window_moments (see its definition above) per window with seq < n_windows_used, RN16 and EPC
 * alike, in a device table [n_streams][wmax] (row = seq; the rows of a trace behind its cut-off are zeroed: the table's
 * bytes repeat from pass to pass).  Nothing else a pass reports changes.  rfid_batch_plan_slots reserves the table (32 bytes
 * per possible window).  RFID_ERR_STATE without a plan; RFID_ERR_HIP when the allocation fails (the plan and every other
 * workspace stay usable).  A new rfid_batch_plan drops it; it neither needs nor drops the inventory, tracks, quality and
 * repair workspaces, and their plan calls do not drop it. */
RFID_API int rfid_batch_plan_slots(rfid_ctx *ctx);
/* enqueues the moments of the LAST pass behind its statistics (asynchronous, no host synchronisation).  RFID_ERR_STATE: no
 * slots workspace, or no pass with statistics yet.  It needs no inventory and may be enqueued before or behind the other
 * stages.  It reads that pass's matched-filter output, window table, results and statistics on the context's main stream
 * and has rfid_batch_quality's duties there: with two result sets alternating it reads the set of that pass, and it records
 * the long-stream front end's "free" event of the matched-filter buffer again behind its own launch. */
RFID_API int rfid_batch_slots(rfid_ctx *ctx);
/* synchronises; one trace's row of the table: every window before the cut-off in seq order: *n = n_windows_used.  cap as
 * rfid_batch_get_window_quality: RFID_ERR_CAPACITY when cap < *n (nothing is copied; out may be NULL with cap = 0); with
 * cap > *n the zeroed rows behind *n are copied too, up to min(cap, wmax) in all.  RFID_ERR_STATE before the first
 * rfid_batch_slots of this plan. */
RFID_API int rfid_batch_get_window_moments(rfid_ctx *ctx, int stream, rfid_window_moments *out, int64_t cap, int64_t *n);
/* synchronises; device time of the last rfid_batch_slots (HIP events) */
RFID_API int rfid_batch_slots_ms(rfid_ctx *ctx, float *ms);
/* the same sums for windows in host memory: the per-call form for callers that hold gated samples themselves.  gated:
 * n_windows x RFID_MOMENTS_SAMPLES samples that are already DC-free -- the first 240 of what rfid_gate_work /
 * rfid_stream_work hand out per window (dc = 0 in the definition).  One launch of the batch kernel's device function,
 * synchronising.  out[k]: stream = 0, seq = k, flags = 0. */
RFID_API int rfid_window_moments_of(rfid_ctx *ctx, const rfid_cf32 *gated, int n_windows, rfid_window_moments *out);
/* ---- (2g) batch commands: the reader's PIE command in front of every window, decoded on the device --------------------- */
/* Behind a pass: one rfid_command (see its definition above) per window with seq < n_windows_used, in a device table
 * [n_streams][wmax] (row = seq; the rows of a trace behind its cut-off are zeroed: the table's bytes repeat from pass to
 * pass).  Nothing else a pass reports changes.  rfid_batch_plan_commands reserves the table (48 bytes per possible window).
 * RFID_ERR_STATE without a plan; RFID_ERR_HIP when the allocation fails (the plan and every other workspace stay usable).  A
 * new rfid_batch_plan drops it; it neither needs nor drops any other stage's workspace, and their plan calls do not drop it. */
RFID_API int rfid_batch_plan_commands(rfid_ctx *ctx);
/* enqueues the commands of the LAST pass behind its statistics (asynchronous, no host synchronisation).  RFID_ERR_STATE: no
 * commands workspace, or no pass with statistics yet.  It needs no inventory and may be enqueued before or behind the other
 * stages: it neither needs nor changes their level.  It reads that pass's matched-filter output, window table, results and
 * statistics on the context's main stream and has rfid_batch_slots' duties there.  There is ONE table per plan, also when two
 * result sets alternate (RFID_OVERLAP=2): a later pass leaves it alone, but the next rfid_batch_commands overwrites it -- fetch a
 * pass's rows before enqueueing the stage behind the next pass, or they are lost. */
RFID_API int rfid_batch_commands(rfid_ctx *ctx);
/* synchronises; one trace's row of the table: every window before the cut-off in seq order: *n = n_windows_used.  cap as
 * rfid_batch_get_window_moments.  RFID_ERR_STATE before the first rfid_batch_commands of this plan. */
RFID_API int rfid_batch_get_window_commands(rfid_ctx *ctx, int stream, rfid_command *out, int64_t cap, int64_t *n);
/* synchronises; device time of the last rfid_batch_commands (HIP events) */
RFID_API int rfid_batch_commands_ms(rfid_ctx *ctx, float *ms);
/* the same decode for spans in host memory: the per-call form.  spans: n x RFID_CMD_SPAN samples, the span of row k in front
 * of a window whose dc is levels[k] (re, im).  One launch of the batch kernel's device function, synchronising.  out[k]:
 * stream = 0, seq = k, flag bits 0, 2 and 4 are 0. */
RFID_API int rfid_commands_of(rfid_ctx *ctx, const rfid_cf32 *spans, const rfid_cf32 *levels, int n, rfid_command *out);
/* ---- (2h) batch fine channel: the data-aided channel estimate of every EPC window, built on the device ------------------- */
/* Behind the tracks of a pass: one rfid_read_fine (see its definition above) per EPC window with seq < n_windows_used,
 * CRC-verified or not, in a device table [n_streams][ceil(wmax / 2)] (row = seq >> 1; the rows of a trace behind its cut-off
 * are zeroed: the table's bytes repeat from pass to pass), and the records of the CRC-verified reads once more as ONE array
 * aligned with the tracks: fine[i] belongs to reads[i] of rfid_batch_get_tracks.  Nothing else a pass reports changes.
 * rfid_batch_plan_fine reserves both (2 x 128 bytes per possible EPC window).  RFID_ERR_STATE without a tracks workspace;
 * RFID_ERR_HIP when the allocation fails (the plan and every other workspace stay usable).  A new rfid_batch_plan,
 * rfid_batch_plan_inventory or rfid_batch_plan_tracks drops it; it neither needs nor drops the quality and repair workspaces,
 * and their plan calls do not drop it. */
RFID_API int rfid_batch_plan_fine(rfid_ctx *ctx);
/* enqueues the fine stage of the LAST pass behind its tracks (asynchronous, no host synchronisation).  RFID_ERR_STATE: no fine
 * workspace, or no rfid_batch_tracks was enqueued since the last pass.  It may be enqueued before or behind rfid_batch_quality
 * and rfid_batch_repair and does not change the level of any stage.  It reads that pass's matched-filter output, window table,
 * results and statistics on the context's main stream and has rfid_batch_quality's duties there: with two result sets
 * alternating it reads the set of that pass, and it records the long-stream front end's "free" event of the matched-filter
 * buffer again behind its own launches. */
RFID_API int rfid_batch_fine(rfid_ctx *ctx);
/* synchronises; *n = reads in all, the number rfid_batch_get_tracks reports; out[i] belongs to its reads[i].
 * RFID_ERR_CAPACITY as there: cap too small (nothing lost: *n says how many there are, call again; out may be NULL with
 * cap = 0), or a trace overflowed the inventory (rfid_last_error names the first such trace) */
RFID_API int rfid_batch_get_fine(rfid_ctx *ctx, rfid_read_fine *out, int64_t cap, int64_t *n);
/* synchronises; one trace's row of the table: every EPC window before the cut-off in seq order, failed ones included:
 * *n = n_windows_used / 2.  cap as rfid_batch_get_window_quality: RFID_ERR_CAPACITY when cap < *n (nothing is copied; out may
 * be NULL with cap = 0); with cap > *n the zeroed rows behind *n are copied too, up to min(cap, ceil(wmax / 2)) in all. */
RFID_API int rfid_batch_get_window_fine(rfid_ctx *ctx, int stream, rfid_read_fine *out, int64_t cap, int64_t *n);
/* synchronises; device time of the last rfid_batch_fine (HIP events), from its first launch to the end of its last */
RFID_API int rfid_batch_fine_ms(rfid_ctx *ctx, float *ms);
/* the same sums for ONE window in host memory: the per-call form (as rfid_repair_window).  gated: the window's 1 370 gated,
 * DC-free samples (dc = 0 in the definition); res: the result rfid_decoder_work gave for it (type RFID_DECODE_EPC, else
 * RFID_ERR_INVALID) -- or that result with bits a caller has corrected, from rfid_repair::frame for instance.  One launch of
 * the batch kernel's device functions, synchronising.  out: stream = seq = start = 0, flags bit 0 = res->crc_ok. */
RFID_API int rfid_fine_window(rfid_ctx *ctx, const rfid_cf32 *gated, const rfid_decode_result *res, rfid_read_fine *out);
/* ---- (2i) batch retune: CRC-failed EPC frames decoded again over the Gen2 BLF tolerance, built on the device ----------------- */
/* Behind a pass: one rfid_retune (see its definition above) per EPC window with seq < n_windows_used in a device table
 * [n_streams][ceil(wmax / 2)] (row = seq >> 1; the rows of a trace behind its cut-off are zeroed: the table's bytes repeat from
 * pass to pass).  Nothing else a pass reports changes: a retuned frame is not a read.  rfid_batch_plan_retune reserves the table
 * (64 bytes per possible EPC window).  RFID_ERR_STATE without a plan; RFID_ERR_HIP when the allocation fails (the plan and every
 * other workspace stay usable).  A new rfid_batch_plan drops it; it neither needs nor drops any other stage's workspace, and their
 * plan calls do not drop it. */
RFID_API int rfid_batch_plan_retune(rfid_ctx *ctx);
/* enqueues the retune stage of the LAST pass behind its statistics (asynchronous, no host synchronisation).  RFID_ERR_STATE: no
 * retune workspace, or no pass with statistics yet.  It needs no inventory and may be enqueued before or behind the other stages:
 * it neither needs nor changes their level.  It reads that pass's matched-filter output -- up to 38 samples behind a window, never
 * behind the trace's own length: the lengths are the pass's (d_lens, which must still be valid, or n_raw) -- window table, results
 * and statistics on the context's main stream and has rfid_batch_slots' duties there.  ONE table per plan, as rfid_batch_commands. */
RFID_API int rfid_batch_retune(rfid_ctx *ctx);
/* synchronises; one trace's row of the table: every EPC window before the cut-off in seq order, verified, retuned or not:
 * *n = n_windows_used / 2.  cap as rfid_batch_get_window_quality.  RFID_ERR_STATE before the first rfid_batch_retune of this plan. */
RFID_API int rfid_batch_get_window_retunes(rfid_ctx *ctx, int stream, rfid_retune *out, int64_t cap, int64_t *n);
/* synchronises; device time of the last rfid_batch_retune (HIP events) */
RFID_API int rfid_batch_retune_ms(rfid_ctx *ctx, float *ms);
/* the same search for ONE span in host memory: the per-call form.  span: n samples from the window's first on, DC-free already
 * (dc = 0 in the definition), 1370 <= n <= RFID_RETUNE_SPAN (else RFID_ERR_INVALID): indices are held at n - 1 (flags bit 2); res:
 * the result rfid_decoder_work gave for the window (type RFID_DECODE_EPC with index 65 .. 79, else RFID_ERR_INVALID).  One launch
 * of the batch kernel's device functions, synchronising.  out: stream = seq = start = 0; flags bit 0 = res->crc_ok (then nothing
 * is searched). */
RFID_API int rfid_retune_window(rfid_ctx *ctx, const rfid_cf32 *span, int n, const rfid_decode_result *res, rfid_retune *out);
/* ---- (2j) batch collisions: both RN16s and both channels of a two-tag collided slot, built on the device ---------------------- */
/* Behind a pass: one rfid_collision (see its definition above) per RN16 window with seq < n_windows_used in a device table
 * [n_streams][ceil(wmax / 2)] (row = seq >> 1; the rows of a trace behind its cut-off are zeroed: the table's bytes repeat from
 * pass to pass).  Nothing else a pass reports changes: what the reader ACKed stays what it ACKed.  rfid_batch_plan_collisions
 * reserves the table (64 bytes per possible RN16 window).  RFID_ERR_STATE without a plan; RFID_ERR_HIP when the allocation fails
 * (the plan and every other workspace stay usable).  A new rfid_batch_plan drops it; it neither needs nor drops any other stage's
 * workspace, and their plan calls do not drop it. */
RFID_API int rfid_batch_plan_collisions(rfid_ctx *ctx);
/* enqueues the collisions stage of the LAST pass behind its statistics (asynchronous, no host synchronisation).  RFID_ERR_STATE:
 * no collisions workspace, or no pass with statistics yet.  It needs no inventory and may be enqueued before or behind the other
 * stages: it neither needs nor changes their level.  It reads that pass's matched-filter output, window table, results and
 * statistics on the context's main stream and has rfid_batch_slots' duties there.  ONE table per plan, as rfid_batch_commands. */
RFID_API int rfid_batch_collisions(rfid_ctx *ctx);
/* synchronises; one trace's row of the table: every RN16 window before the cut-off in seq order:
 * *n = (n_windows_used + 1) / 2.  cap as rfid_batch_get_window_quality.  RFID_ERR_STATE before the first rfid_batch_collisions of
 * this plan. */
RFID_API int rfid_batch_get_window_collisions(rfid_ctx *ctx, int stream, rfid_collision *out, int64_t cap, int64_t *n);
/* synchronises; device time of the last rfid_batch_collisions (HIP events) */
RFID_API int rfid_batch_collisions_ms(rfid_ctx *ctx, float *ms);
/* the same records for windows in host memory: the per-call form (as rfid_window_moments_of).  gated: n_windows x 250 gated,
 * DC-free samples (dc = 0 in the definition); results[k]: the result rfid_decoder_work gave for window k (type RFID_DECODE_RN16
 * with index 65 .. 79, else RFID_ERR_INVALID and nothing is launched).  One launch of the batch kernel's device functions,
 * synchronising.  out[k]: stream = 0, seq = k. */
RFID_API int rfid_collisions_of(rfid_ctx *ctx, const rfid_cf32 *gated, const rfid_decode_result *results, int n_windows,
                                rfid_collision *out);
/* ---- (2k) batch lengths: CRC-failed EPC frames read at the length their PC word announces, built on the device ---------------- */
/* Behind a pass: one rfid_sized_frame (see its definition above) per EPC window with seq < n_windows_used in a device table
 * [n_streams][ceil(wmax / 2)] (row = seq >> 1; the rows of a trace behind its cut-off are zeroed: the table's bytes repeat from
 * pass to pass).  Nothing else a pass reports changes: a frame found here is not a read.  rfid_batch_plan_lengths reserves the
 * table (64 bytes per possible EPC window).  RFID_ERR_STATE without a plan; RFID_ERR_HIP when the allocation fails (the plan and
 * every other workspace stay usable).  A new rfid_batch_plan drops it; it neither needs nor drops any other stage's workspace, and
 * their plan calls do not drop it. */
RFID_API int rfid_batch_plan_lengths(rfid_ctx *ctx);
/* enqueues the lengths stage of the LAST pass behind its statistics (asynchronous, no host synchronisation).  RFID_ERR_STATE: no
 * lengths workspace, or no pass with statistics yet.  It needs no inventory and may be enqueued before or behind the other stages:
 * it neither needs nor changes their level.  It reads that pass's matched-filter output -- up to 358 samples behind a window, never
 * behind the trace's own length: the lengths are the pass's (d_lens, which must still be valid, or n_raw) -- window table, results
 * and statistics on the context's main stream and has rfid_batch_slots' duties there.  ONE table per plan, as rfid_batch_commands. */
RFID_API int rfid_batch_lengths(rfid_ctx *ctx);
/* synchronises; one trace's row of the table: every EPC window before the cut-off in seq order, verified, recovered or not:
 * *n = n_windows_used / 2.  cap as rfid_batch_get_window_quality.  RFID_ERR_STATE before the first rfid_batch_lengths of this plan. */
RFID_API int rfid_batch_get_window_lengths(rfid_ctx *ctx, int stream, rfid_sized_frame *out, int64_t cap, int64_t *n);
/* synchronises; device time of the last rfid_batch_lengths (HIP events) */
RFID_API int rfid_batch_lengths_ms(rfid_ctx *ctx, float *ms);
/* the same for ONE span in host memory: the per-call form.  span: n samples from the window's first on, DC-free already (dc = 0
 * in the definition), 1370 <= n <= RFID_LENGTHS_SPAN (else RFID_ERR_INVALID): indices are held at n - 1 (flags bit 2); res: the
 * result rfid_decoder_work gave for the window -- type RFID_DECODE_EPC, index 65 .. 79 and T inside the decoder's own
 * 4.94999981 .. 5.05000019, else RFID_ERR_INVALID.  One launch of the batch kernel's device functions, synchronising.  out:
 * stream = seq = start = 0; flags bit 0 = res->crc_ok (then nothing is done). */
RFID_API int rfid_length_window(rfid_ctx *ctx, const rfid_cf32 *span, int n, const rfid_decode_result *res, rfid_sized_frame *out);
/* ---- (2l) batch diversity: the EPC windows of traces recorded together combined before the sign is taken, built on the device -- */
/* Behind a pass: one rfid_diversity (see its definition above) per EPC window of every group's anchor with seq < n_windows_used in a
 * device table [n_streams / members][ceil(wmax / 2)] (row = seq >> 1; the rows of a group behind its anchor's cut-off are zeroed:
 * the table's bytes repeat from pass to pass).  The first stage that looks across traces.  Nothing else a pass reports changes: a
 * combined frame is not a read.  rfid_batch_plan_diversity reserves the table (64 bytes per possible EPC window of a group) for
 * groups of `members` traces.  RFID_ERR_INVALID: members outside 2 .. RFID_DIVERSITY_MAX_MEMBERS; RFID_ERR_STATE without a plan;
 * RFID_ERR_HIP when the allocation fails (the plan and every other workspace stay usable).  A new rfid_batch_plan drops it; it neither
 * needs nor drops any other stage's workspace, and their plan calls do not drop it. */
RFID_API int rfid_batch_plan_diversity(rfid_ctx *ctx, int members);
/* enqueues the diversity stage of the LAST pass behind its statistics (asynchronous, no host synchronisation).  RFID_ERR_STATE: no
 * diversity workspace, or no pass with statistics yet; RFID_ERR_INVALID, with a message, when the pass's stream count is not a multiple
 * of `members`.  It needs no inventory and may be enqueued before or behind the other stages: it neither needs nor changes their level.
 * It reads that pass's matched-filter output -- never behind a trace's own length: the lengths are the pass's (d_lens, which must still
 * be valid, or n_raw) -- window table, results and statistics on the context's main stream and has rfid_batch_slots' duties there.
 * ONE table per plan, as rfid_batch_commands. */
RFID_API int rfid_batch_diversity(rfid_ctx *ctx);
/* synchronises; one GROUP's row of the table: every EPC window of its anchor before the cut-off in seq order: *n = n_windows_used / 2
 * of the anchor.  cap as rfid_batch_get_window_quality.  RFID_ERR_STATE before the first rfid_batch_diversity of this plan;
 * RFID_ERR_INVALID for a group the last rfid_batch_diversity did not cover. */
RFID_API int rfid_batch_get_window_diversity(rfid_ctx *ctx, int group, rfid_diversity *out, int64_t cap, int64_t *n);
/* synchronises; device time of the last rfid_batch_diversity (HIP events) */
RFID_API int rfid_batch_diversity_ms(rfid_ctx *ctx, float *ms);
/* the same for the windows of ONE row in host memory: the per-call form.  spans: [members][1370] samples, member after member, DC-free
 * already (dc_est = 0 in the definition); res: [members], the result rfid_decoder_work gave for each member's window.  All members are
 * present.  RFID_ERR_INVALID: members outside 2 .. RFID_DIVERSITY_MAX_MEMBERS, or a member's result that rfid_length_window would
 * refuse (type, index 65 .. 79, T inside 4.94999981 .. 5.05000019).  One launch of the batch kernel's device functions,
 * synchronising.  out: stream = seq = start = 0, present = 2^members - 1. */
RFID_API int rfid_diversity_window(rfid_ctx *ctx, const rfid_cf32 *spans, int members, const rfid_decode_result *res, rfid_diversity *out);
/* ---- (2m) batch match: known tags' frames found in CRC-failed EPC windows, built on the device ----------------------------------- */
/* Behind a pass: one rfid_match (see its definition above) per EPC window with seq < n_windows_used in a device table
 * [n_streams][ceil(wmax / 2)] (row = seq >> 1; rows behind a trace's cut-off are zeroed: the table's bytes repeat from pass to pass).
 * The first stage that detects where the others decode.  Nothing else a pass reports changes: an attribution is not a read.
 * rfid_batch_plan_match reserves the table (64 bytes per possible EPC window) and room for a list of RFID_MATCH_MAX_LIST frames.
 * RFID_ERR_STATE without a plan; RFID_ERR_HIP when the allocation fails (the plan and every other workspace stay usable).  A new
 * rfid_batch_plan drops it, and the list with it; it drops no other stage's workspace, and their plan calls do not drop it. */
RFID_API int rfid_batch_plan_match(rfid_ctx *ctx);
/* synchronises; the candidates of every trace from now on: n frames of four words each, packed as rfid_decode_result::bits, copied to
 * the device.  n = 0 or frames = NULL: every trace's own inventory again.  The list is kept until the workspace is dropped.
 * RFID_ERR_INVALID: n < 0 or n > RFID_MATCH_MAX_LIST; RFID_ERR_STATE without a match workspace. */
RFID_API int rfid_batch_match_set_list(rfid_ctx *ctx, const uint32_t *frames, int n);
/* enqueues the match stage of the LAST pass (asynchronous, no host synchronisation).  Without a list it reads that pass's inventory
 * and is enqueued behind it exactly as rfid_batch_repair is: RFID_ERR_STATE without an inventory workspace or without an
 * rfid_batch_inventory behind the last pass.  With a list it needs the pass's statistics only, as rfid_batch_lengths does.  Either
 * way it may be enqueued before or behind the other stages and neither raises nor lowers their level.  It reads that pass's
 * matched-filter output, window table, results and statistics on the context's main stream and has rfid_batch_slots' duties there.
 * ONE table per plan, as rfid_batch_commands. */
RFID_API int rfid_batch_match(rfid_ctx *ctx);
/* synchronises; one trace's row of the table: every EPC window before the cut-off in seq order: *n = n_windows_used / 2.  cap as
 * rfid_batch_get_window_quality.  RFID_ERR_STATE before the first rfid_batch_match of this plan; RFID_ERR_INVALID for a trace the
 * last rfid_batch_match did not cover. */
RFID_API int rfid_batch_get_window_matches(rfid_ctx *ctx, int stream, rfid_match *out, int64_t cap, int64_t *n);
/* synchronises; device time of the last rfid_batch_match (HIP events) */
RFID_API int rfid_batch_match_ms(rfid_ctx *ctx, float *ms);
/* the same for ONE window in host memory against n_frames candidate frames: the per-call form.  gated: 1370 samples, DC-free already
 * (dc = 0 in the definition); res: the result rfid_decoder_work gave for the window; frames: [n_frames][4] words.  RFID_ERR_INVALID:
 * n_frames outside 1 .. RFID_MATCH_MAX_LIST, or a result that rfid_diversity_window would refuse (type, index 65 .. 79, T inside
 * 4.94999981 .. 5.05000019).  One launch of the batch kernel's device functions, synchronising.  out: stream = seq = start = 0,
 * flags bit 3 set; bit 0 = res->crc_ok (then nothing is searched). */
RFID_API int rfid_match_window(rfid_ctx *ctx, const rfid_cf32 *gated, const rfid_decode_result *res, const uint32_t *frames, int n_frames,
                               rfid_match *out);
/* ---- (2n) batch stack: an unknown tag's repeated EPC frames combined over rounds, built on the device ----------------------------- */
/* Behind a pass: one rfid_stack (see its definition above) per EPC window with seq < n_windows_used in a device table
 * [n_streams][ceil(wmax / 2)] (row = seq >> 1; rows behind a trace's cut-off are zeroed: the table's bytes repeat from pass to pass).
 * Needs no antenna beside the trace's own and no list of known tags.  Nothing else a pass reports changes: a stacked frame is not a
 * read.  rfid_batch_plan_stack reserves the table (64 bytes per possible EPC window) and the list of failed rows (4 bytes each).
 * RFID_ERR_STATE without a plan; RFID_ERR_HIP when the allocation fails (the plan and every other workspace stay usable).  A new
 * rfid_batch_plan drops it; it drops no other stage's workspace, and their plan calls do not drop it. */
RFID_API int rfid_batch_plan_stack(rfid_ctx *ctx);
/* enqueues the stack stage of the LAST pass (asynchronous, no host synchronisation) with the partner threshold rho_min.
 * RFID_ERR_INVALID unless rho_min is finite and 0 < rho_min <= 1 (nothing is enqueued).  It needs the pass's statistics only, as
 * rfid_batch_match with a list does, and has its state rules and stream duties: it may be enqueued before or behind the other
 * stages and neither raises nor lowers their level.  ONE table per plan, as rfid_batch_commands. */
RFID_API int rfid_batch_stack(rfid_ctx *ctx, float rho_min);
/* synchronises; one trace's row of the table: every EPC window before the cut-off in seq order: *n = n_windows_used / 2.  cap as
 * rfid_batch_get_window_quality.  RFID_ERR_STATE before the first rfid_batch_stack of this plan; RFID_ERR_INVALID for a trace the
 * last rfid_batch_stack did not cover. */
RFID_API int rfid_batch_get_window_stacks(rfid_ctx *ctx, int stream, rfid_stack *out, int64_t cap, int64_t *n);
/* synchronises; device time of the last rfid_batch_stack (HIP events) */
RFID_API int rfid_batch_stack_ms(rfid_ctx *ctx, float *ms);
/* the same for n = 1 .. RFID_STACK_MAX_WINDOWS windows in host memory, one block: the per-call form.  gated: [n][1370] samples,
 * DC-free already (dc = 0 in the definition); res: [n] the results rfid_decoder_work gave for them; out: [n] records, out[i] for
 * window i, stream = seq = start = 0.  A window whose res has crc_ok = 1 is a read (bit 0) and takes no ordinal; the others get
 * their ordinals in the order given.  RFID_ERR_INVALID: n outside 1 .. 64, rho_min as for rfid_batch_stack, or a result that
 * rfid_match_window would refuse (type, index 65 .. 79, T inside 4.94999981 .. 5.05000019).  One launch of the batch kernel's device
 * functions, synchronising. */
RFID_API int rfid_stack_windows(rfid_ctx *ctx, const rfid_cf32 *gated, const rfid_decode_result *res, int n, float rho_min, rfid_stack *out);
/* the HIP stream the ctx launches on (hipStream_t as void*) */
RFID_API void *rfid_ctx_stream(rfid_ctx *ctx);

/* ---- (3) synthetic workloads (SURVEY.md section 8 d: noise replicas made on the device) ---------- */
/* d_out[s][i] = d_base[i] + sigma * (N(0,1) + j N(0,1)) for s in [0, n_streams), i in [0, n_raw): replica
 * first_replica + s of the base trace.  The noise is a pure function of (seed, replica index, i)
 * (Philox4x32-10 + Box-Muller), so a batch may be generated in pieces and on any number of GPUs.
 * Asynchronous on the ctx stream.  Not part of the receive path: the workload generator of bench.py
 * and of the HBM-capacity configurations. */
RFID_API int rfid_synth_replicas(rfid_ctx *ctx, const void *d_base, int64_t n_raw, void *d_out, int64_t out_stride,
                                 int n_streams, float sigma, uint64_t seed, int64_t first_replica);


/* ---- (3b) Gen2 trace synthesiser ------------------------------------------ */
/* One inventory slot of a synthetic receive trace: what the reader sends (reader_impl.cc:84-162: Query with
 * CRC-5 for the first slot of a round, QueryRep otherwise, then the ACK) and what the tags answer. */
#define RFID_SYNTH_MAX_RESP 8
#define RFID_SYNTH_MAX_TAGS 16
typedef struct rfid_synth_slot {
  uint8_t cmd;            /* 0 Query, 1 QueryRep */
  uint8_t q;              /* Q field of the Query (FIXED_Q) */
  uint8_t n_tags;         /* tags answering in this slot: 0 empty, 1 single, >1 collision (<= 8) */
  uint8_t has_epc;        /* the (single) responder backscatters its EPC frame after the ACK */
  uint8_t tag[RFID_SYNTH_MAX_RESP];   /* index of each responder's backscatter coefficient */
  uint16_t rn16[RFID_SYNTH_MAX_RESP]; /* the RN16 each responder backscatters, bit 15 sent first */
  uint16_t ack;           /* RN16 the reader's ACK carries, bit 15 first (the reference ACKs every slot) */
  int16_t reserved_;
  int32_t rn16_off_raw;   /* start of the RN16 replies, raw samples (2 Msps) after the end of the command: 500 = 250 us */
  int32_t epc_off_raw;    /* start of the EPC reply after the end of the ACK */
  uint32_t epc[4];        /* 128 EPC frame bits (PC + EPC + CRC-16), frame bit j at epc[j >> 5] bit (j & 31) */
} rfid_synth_slot;        /* 56 bytes */

typedef struct rfid_synth_gen2_params {
  float leak_re, leak_im;                 /* carrier leakage L */
  float h_re[RFID_SYNTH_MAX_TAGS];        /* backscatter coefficient of tag k */
  float h_im[RFID_SYNTH_MAX_TAGS];
  int32_t n_tags;
  int32_t tail_us;                        /* carrier after the last slot */
} rfid_synth_gen2_params;

/* Samples (2 Msps) of the trace these slots make: 4575 us carrier, then per slot command + 1295 us carrier +
 * ACK + 4575 us carrier (reader_impl.cc:69-70,218-224), then tail_us of carrier. */
RFID_API int rfid_synth_gen2_size(const rfid_synth_gen2_params *p, const rfid_synth_slot *slots, int64_t n_slots,
                                  int64_t *n_raw);
/* Writes the trace  x = L tx + sum_k h_k level_k tx + sigma (N(0,1) + j N(0,1))  into d_out (device, 16-byte
 * aligned, room for out_cap samples), generated on the device from the slot table (host pointer; copied).
 * The noise is that of rfid_synth_replicas for replica index `replica` (so sigma = 0 here followed by
 * rfid_synth_replicas gives the same bytes).  Asynchronous on the ctx stream; *n_raw = samples written. */
RFID_API int rfid_synth_gen2(rfid_ctx *ctx, const rfid_synth_gen2_params *p, const rfid_synth_slot *slots,
                             int64_t n_slots, void *d_out, int64_t out_cap, float sigma, uint64_t seed,
                             int64_t replica, int64_t *n_raw);

#ifdef __cplusplus
}
#endif
#endif /* RFID_MI355X_H */
