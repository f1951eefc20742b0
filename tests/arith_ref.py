"""The reference of the arithmetic primitives (TEST INFRASTRUCTURE; tests/arith_cases.py builds the operands, tests/arith_suite.py
compares rfid_selftest_arith with what stands here).  No kernel logic: every operation is written as the reference project's
scalar C++ performs it -- binary32 additions one after the other, a correctly rounded quotient, glibc's hypotf formula -- and
each is tied to exact rational arithmetic (fractions.Fraction, math.isqrt) before it is believed:

 * sums: numpy.float32 additions in order; pin_additions() re-derives a sample of them from exact rationals with rn32();
 * scan flags: the conditions written above chain_add_scan in csrc/rfid_kernels.hpp (and chain_add_scan2 in rfid_ls2.hpp),
   evaluated on the sequential sum -- not on an integer image of it;
 * divisions: numpy's binary32 division, which quotient_exact() (Fraction, subnormal grid included) pins on every operand
   of the division families;
 * hypot_f: RN32(RN64(sqrt(RN64(x^2 + y^2)))) in exact integers (hypot_exact) against numpy's double formula (hypot_np);
 * lds_sum25_in_order: (((0 + x_0) + x_1) + ...) + x_24 per component;
 * scan_add and the DPP building blocks: Python integers mod 2^32 and the lane maps of the ISA's row_shr:N, row_bcast:15,
   row_bcast:31 and wave_shr:1 with bound_ctrl off (a lane without a source keeps `fill`)."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
TWO22 = 4194304.0


def bits(a):
    return np.asarray(a, dtype=F32).view(np.uint32)


def from_bits(u):
    return np.asarray(u, dtype=np.uint32).view(F32)


def same(a, b):
    """bit for bit, or both NaN (payloads are not compared)"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


# ---- exact rationals -> binary formats -----------------------------------------------------------------------------------
def _round_fraction(fr, prec, emin, emax):
    """fr (a Fraction) to nearest-even in a binary format of `prec` significant bits whose least normal exponent is emin and
    greatest emax (value = m * 2^(e - prec + 1), 2^(prec-1) <= m < 2^prec; below 2^emin the grid of 2^(emin - prec + 1)) ->
    (sign, m, e) with value = m * 2^(e - prec + 1), or (sign, None, None) for an overflow to infinity"""
    sign = fr < 0
    fr = abs(fr)
    if fr == 0:
        return sign, 0, emin
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    assert Fraction(2) ** e <= fr < Fraction(2) ** (e + 1)
    e = max(e, emin)
    q = fr / Fraction(2) ** (e - prec + 1)
    m, rest = divmod(q.numerator, q.denominator)
    twice = 2 * rest
    if twice > q.denominator or (twice == q.denominator and (m & 1)):
        m += 1
    if m == 1 << prec:
        m >>= 1
        e += 1
    if e > emax:
        return sign, None, None
    return sign, m, e


def rn32(fr, negative_zero=False):
    """the binary32 number nearest to the Fraction fr, ties to even, subnormals and overflow included"""
    sign, m, e = _round_fraction(Fraction(fr), 24, -126, 127)
    if m is None:
        return F32(-np.inf) if sign else F32(np.inf)
    if m == 0:
        return F32(-0.0) if negative_zero else F32(0.0)
    v = math.ldexp(m, e - 23)          # exact: m has 24 bits
    return F32(-v if sign else v)


def rn64(fr):
    sign, m, e = _round_fraction(Fraction(fr), 53, -1022, 1023)
    if m is None:
        return -math.inf if sign else math.inf
    v = math.ldexp(m, e - 52)
    return -v if sign else v


def frac(x):
    return Fraction(float(x))


# ---- in-order sums --------------------------------------------------------------------------------------------------------
def seq_sum(carry, x):
    """carry [N], x [N, 64] -> [N, 64]: lane L = (((carry + x_0) + x_1) + ...) + x_L, binary32 additions in order"""
    carry, x = np.asarray(carry, dtype=F32), np.asarray(x, dtype=F32)
    out = np.empty_like(x)
    s = carry.copy()
    with np.errstate(all="ignore"):
        for lane in range(x.shape[1]):
            s = (s + x[:, lane]).astype(F32)
            out[:, lane] = s
    return out


def chain_sum(carry, x):
    """seq_sum as the DPP chains (chain_add, chain_add2) return it.  Their shift brings +0 in front of lane 0 at every one of the
    63 steps, and +0 + x is x for every x but -0: a partial sum that is -0 -- which takes a carry of -0 and nothing but -0 addends
    so far -- comes back as +0 in the lanes 0 .. 62, reached by that +0 one lane per step; lane 63, the next carry, is not reached
    and keeps the -0.  Everything else is the sequential sum bit for bit.  (No kernel passes a carry of -0: the sums start from
    +0, and a binary32 sum is -0 only when both operands are.)"""
    s = seq_sum(carry, x)
    u = bits(s).copy()
    u[:, :63][u[:, :63] == 0x80000000] = 0
    return u.view(F32)


def add_exact(a, b):
    """one binary32 addition from exact rationals (finite operands)"""
    a, b = F32(a), F32(b)
    s = frac(a) + frac(b)
    if s == 0:   # IEEE: x + (-x) = +0, (-0) + (-0) = -0
        return F32(-0.0) if (np.signbit(a) and np.signbit(b)) else F32(0.0)
    return rn32(s)


def pin_additions(carry, x, rng, count):
    """`count` additions of seq_sum(carry, x), drawn by rng among those with finite operands, re-derived exactly"""
    sums = seq_sum(carry, x)
    prev = np.concatenate([np.asarray(carry, dtype=F32)[:, None], sums[:, :-1]], axis=1)
    ok = np.argwhere(np.isfinite(prev) & np.isfinite(np.asarray(x, dtype=F32)))
    pick = ok[rng.choice(len(ok), size=min(count, len(ok)), replace=False)]
    for k, lane in pick:
        want = add_exact(prev[k, lane], x[k, lane])
        assert bits(want) == bits(sums[k, lane]), (k, lane, prev[k, lane], x[k, lane])
    return len(pick)


def scan_predicate(carry, xs):
    """The conditions above chain_add_scan, for one carry and any number of addends in order (64: one step, 128: a pair): the
    carry's biased exponent lies in [23, 254]; every |x * 2^(23 - e)| < 2^22; every partial sum of the sequential sum keeps the
    carry's exponent and sign and has a non-zero mantissa."""
    cb = int(bits(F32(carry)))
    e_b = (cb >> 23) & 0xff
    if e_b < 23 or e_b > 254:
        return False
    xs = np.asarray(xs, dtype=F32)
    t = xs.astype(np.float64) * math.ldexp(1.0, 23 - (e_b - 127))      # exact in binary64
    if not np.all(np.abs(t) < TWO22):                                  # (a NaN fails the comparison)
        return False
    part = bits(seq_sum(np.array([carry], dtype=F32), xs[None, :])[0])
    return bool(np.all(((part ^ np.uint32(cb)) & np.uint32(0xff800000)) == 0) and np.all((part & np.uint32(0x007fffff)) != 0))


def scaled(carry, xs):
    """x * 2^(23 - e) in the units of the carry's binade, sign folded as the kernels fold it (binary64, exact)"""
    cb = int(bits(F32(carry)))
    e_b = (cb >> 23) & 0xff
    t = np.asarray(xs, dtype=F32).astype(np.float64) * math.ldexp(1.0, 23 - (e_b - 127))
    return -t if cb >> 31 else t


def scan2_predicate(ca, cb, xs):
    """chain_add_scan2's comment adds: both carries in one binade with one sign, and B's partial sums in the binade with a
    non-zero mantissa too -- which, where both take the same integers, reads m + dm in [1, 2^23 - 1] on every lane (m: the
    mantissa of A's partial sum, dm = B - A in the integer image)."""
    ba, bb = int(bits(F32(ca))), int(bits(F32(cb)))
    if (ba ^ bb) & 0xff800000:
        return False
    return scan_predicate(ca, xs) and scan_predicate(cb, xs)


def scan2_shared_form(ca, cb, xs):
    """the same written as the comment writes it; equal to scan2_predicate wherever both carries take the same integers (dm even,
    or no tie in the step) -- arith_cases asserts that on its records"""
    ba, bb = int(bits(F32(ca))), int(bits(F32(cb)))
    if (ba ^ bb) & 0xff800000 or not scan_predicate(ca, xs):
        return False
    dm = (bb & 0x7fffffff) - (ba & 0x7fffffff)
    m = (bits(seq_sum(np.array([ca], dtype=F32), np.asarray(xs, dtype=F32)[None, :])[0]) & np.uint32(0x007fffff)).astype(np.int64)
    return bool(np.all((m + dm >= 1) & (m + dm <= (1 << 23) - 1)))


# ---- divisions ------------------------------------------------------------------------------------------------------------
def quotient_exact(x, d):
    """RN32(x / d) from exact rationals; IEEE's special cases spelt out (d finite and non-zero, or any: see below)"""
    x, d = F32(x), F32(d)
    if np.isnan(x) or np.isnan(d):
        return F32(np.nan)
    neg = bool(np.signbit(x)) != bool(np.signbit(d))
    if np.isinf(x):
        return F32(np.nan) if np.isinf(d) else F32(-np.inf if neg else np.inf)
    if np.isinf(d):
        return F32(-0.0 if neg else 0.0)
    if d == 0:
        return F32(np.nan) if x == 0 else F32(-np.inf if neg else np.inf)
    if x == 0:
        return F32(-0.0 if neg else 0.0)
    return rn32(frac(x) / frac(d), negative_zero=neg)


def quotient_np(x, d):
    with np.errstate(all="ignore"):
        return (np.asarray(x, dtype=F32) / np.asarray(d, dtype=F32)).astype(F32)


def div_admitted(x):
    """what div_const_ok's comment admits: |x| in [2^-100, inf), and +0"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        return (np.isfinite(x) & (np.abs(x) >= F32(2.0 ** -100))) | (bits(x) == 0)


def mask_of(flags):
    """[N, 64] booleans -> [N] 64-bit vote masks (bit L = lane L)"""
    w = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (np.asarray(flags, dtype=bool) * w).sum(axis=1, dtype=np.uint64)


# ---- hypot ------------------------------------------------------------------------------------------------------------------
def hypot_exact(x, y):
    """RN32(RN64(sqrt(RN64(x^2 + y^2)))) for finite x, y, in exact integers"""
    s = rn64(frac(x) ** 2 + frac(y) ** 2)
    if s == 0.0:
        return F32(0.0)
    if math.isinf(s):
        return F32(np.inf)
    # sqrt(s) to 53 bits: s = n / 2^k with k even and n wide enough that isqrt(n) has more than 54 bits; sticky bit from the remainder
    fs = Fraction(s)
    n, den = fs.numerator, fs.denominator
    k = den.bit_length() - 1
    if k & 1:
        n, k = n * 2, k + 1
    shift = max(0, 112 - n.bit_length())
    shift += shift & 1
    n <<= shift
    k += shift
    r = math.isqrt(n)
    sticky = 1 if r * r != n else 0
    root = Fraction(2 * r + sticky, 2) / Fraction(2) ** (k // 2)     # (r + sticky/2): never on a rounding boundary of 53 bits unless exact
    g = rn64(root)
    return rn32(Fraction(g))


def hypot_np(x, y):
    """numpy's double formula: products exact, one rounding in the sum, a correctly rounded square root, one cast"""
    xd, yd = np.asarray(x, dtype=F32).astype(np.float64), np.asarray(y, dtype=F32).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.sqrt(xd * xd + yd * yd).astype(F32)


def hypot_single_rounding(x, y):
    """a correctly rounded hypotf (one rounding of the exact value), to count where the reference's double rounding differs"""
    v = frac(x) ** 2 + frac(y) ** 2
    if v == 0:
        return F32(0.0)
    n, den = v.numerator, v.denominator
    k = den.bit_length() - 1
    assert den == 1 << k
    if k & 1:
        n, k = n * 2, k + 1
    shift = max(0, 112 - n.bit_length())
    shift += shift & 1
    n <<= shift
    k += shift
    r = math.isqrt(n)
    sticky = 1 if r * r != n else 0
    return rn32(Fraction(2 * r + sticky, 2) / Fraction(2) ** (k // 2))


# ---- filter sum -----------------------------------------------------------------------------------------------------------
def sum25(tile):
    """tile [N, 680] (340 complex, interleaved) -> [N, 128]: lane L's (re, im) = (((0 + x_0) + x_1) + ...) + x_24 over the samples 5 L .. 5 L + 24"""
    t = np.asarray(tile, dtype=F32).reshape(len(tile), 340, 2)
    lanes = 5 * np.arange(64)
    acc = np.zeros((len(t), 64, 2), dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(25):
            acc = (acc + t[:, lanes + k, :]).astype(F32)
    return acc.reshape(len(t), 128)


# ---- integer scan and DPP ---------------------------------------------------------------------------------------------------
def _i32(v):
    v = np.asarray(v, dtype=np.int64) & 0xffffffff
    return np.where(v >= 1 << 31, v - (1 << 32), v).astype(np.int32)


def scan_add(iv):
    return _i32(np.cumsum(np.asarray(iv, dtype=np.int64), axis=1))


def _lanes(iv, fill, src):
    """src[L]: the lane whose value lane L receives, or -1: lane L keeps fill"""
    iv = np.asarray(iv, dtype=np.int32)
    out = np.repeat(np.asarray(fill, dtype=np.int32)[:, None], 64, axis=1)
    for lane, s in enumerate(src):
        if s >= 0:
            out[:, lane] = iv[:, s]
    return out


def row_shr(iv, fill, n):
    """row_shr:n -- within each row of 16 lanes, lane L takes lane L - n; the first n lanes of a row have no source"""
    return _lanes(iv, fill, [lane - n if (lane % 16) >= n else -1 for lane in range(64)])


def row_bcast15(iv, fill):
    """row_bcast:15 under row mask 0xa -- every lane of rows 1 and 3 takes lane 15 of the row before; rows 0 and 2 are not written"""
    return _lanes(iv, fill, [16 * (lane // 16) - 1 if (lane // 16) in (1, 3) else -1 for lane in range(64)])


def row_bcast31(iv, fill):
    """row_bcast:31 under row mask 0xc -- every lane of rows 2 and 3 takes lane 31; rows 0 and 1 are not written"""
    return _lanes(iv, fill, [31 if lane >= 32 else -1 for lane in range(64)])


def wave_shr1(iv, fill):
    """wave_shr:1 -- lane L takes lane L - 1; lane 0 has no source"""
    return _lanes(iv, fill, [lane - 1 for lane in range(64)])


def shr1(x):
    """wv::shr1: wave_shr:1 with bound_ctrl on -- lane 0 receives +0.0"""
    u = bits(x)
    out = np.zeros_like(u)
    out[:, 1:] = u[:, :-1]
    return out.view(F32)


def rint(x):
    with np.errstate(all="ignore"):
        return np.rint(np.asarray(x, dtype=F32)).astype(F32)


def rint_exact(v):
    """to nearest, ties to even, from the exact value (finite v)"""
    fr = frac(v)
    lo = fr.numerator // fr.denominator
    rest = fr - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and (lo & 1)):
        lo += 1
    return lo
