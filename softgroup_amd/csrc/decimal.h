// decimal.h -- one decimal token -> IEEE double, correctly rounded (ties to even), for host and device code.
// What Python's float() returns, bit for bit, over the range below; everything outside it is DECLINED (the
// caller converts it elsewhere), never converted wrong.  Integer arithmetic only behind an optional one-operation
// fast path: no long double, no pow, no strtod.  Build with -ffp-contract=off.
//
//   number     [+-]? (D+ ('.' D*)? | '.' D+) ([eE] [+-]? D+)?
//   declined   [+-]? (inf | infinity | nan), any letter case
//   malformed  everything else: '_', hex, 'd' exponents, an empty token, a token above 64 bytes
//
// The digit string without its leading zeros is the integer m (trailing zeros stay), e = written exponent - number
// of fraction digits.  Converted here: m of at most 19 digits (< 2^64) with -27 <= e <= 27, and m == 0 (a signed
// zero) with any written exponent of at most 4 digits.  Declined: 20 digits and more, |e| > 27, 5 exponent digits.
// Inside the range the result is zero or a normal double, so there is neither subnormal nor overflow handling.
//
//   e >= 0   p = m * 5^e < 2^127 exactly (64 x 64 -> 128 bits), rounded to 53 bits, scaled by 2^e
//   e <  0   m shifted up to bit 63, (m' * 2^64) / 5^-e by long division (5^27 < 2^63: a quotient of at least 65
//            bits), the remainder is the sticky bit, rounded to 53 bits
//   Clinger  m < 2^53 and |e| <= 22: one IEEE multiplication or division by the exact double 10^|e|
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SG_DECIMAL_HD __host__ __device__
#else
#define SG_DECIMAL_HD
#endif

namespace sg {

constexpr int kDecimalOk = 0, kDecimalDeclined = 1, kDecimalMalformed = 2;
constexpr int kDecimalMaxToken = 64;

SG_DECIMAL_HD inline uint64_t decimal_pow5(int k) {      // k <= 27: 5^27 < 2^63
  uint64_t r = 1;
  for (int i = 0; i < 27; ++i)
    if (i < k) r *= 5;
  return r;
}

SG_DECIMAL_HD inline int decimal_clz64(uint64_t v) {      // v != 0
  return __builtin_clzll(v);
}

SG_DECIMAL_HD inline void decimal_mul64(uint64_t a, uint64_t b, uint64_t *hi, uint64_t *lo) {
  const uint64_t a0 = a & 0xFFFFFFFFu, a1 = a >> 32, b0 = b & 0xFFFFFFFFu, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFu) + (p10 & 0xFFFFFFFFu);      // < 3 * 2^32
  *lo = (p00 & 0xFFFFFFFFu) | (mid << 32);
  *hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

SG_DECIMAL_HD inline double decimal_from_bits(uint64_t bits) {
  union {
    uint64_t u;
    double d;
  } x;
  x.u = bits;
  return x.d;
}

// (hi:lo + a sticky fraction) * 2^b, hi:lo != 0, rounded half to even; the result must be a normal double
SG_DECIMAL_HD inline double decimal_round128(uint64_t hi, uint64_t lo, bool sticky, int b) {
  int lz;
  if (hi != 0) {
    lz = decimal_clz64(hi);
    if (lz) {
      hi = (hi << lz) | (lo >> (64 - lz));
      lo <<= lz;
    }
  } else {
    lz = 64 + decimal_clz64(lo);
    hi = lo << (lz - 64);
    lo = 0;
  }
  // hi:lo = N * 2^lz with bit 127 set: 53 bits of mantissa, then the half bit, then what is below it
  uint64_t mant = hi >> 11;
  const bool half = (hi & 0x400u) != 0;
  const bool below = (hi & 0x3FFu) != 0 || lo != 0 || sticky;
  if (half && (below || (mant & 1u))) ++mant;            // (2^53 carries into the exponent below)
  const int x = b - lz + 75;                               // value = mant * 2^x, 2^52 <= mant <= 2^53
  return decimal_from_bits((static_cast<uint64_t>(x + 1074) << 52) + mant);
}

SG_DECIMAL_HD inline bool decimal_word(const uint8_t *s, int len, const char *word, int wlen) {
  if (len != wlen) return false;
  for (int i = 0; i < wlen; ++i)
    if ((s[i] | 0x20) != static_cast<uint8_t>(word[i])) return false;
  return true;
}

// token s[0 .. len) -> *out; *out is written for kDecimalOk alone
SG_DECIMAL_HD inline int decimal_to_double(const uint8_t *s, int len, double *out) {
  if (len <= 0 || len > kDecimalMaxToken) return kDecimalMalformed;
  int i = 0;
  const bool neg = s[0] == '-';
  if (s[0] == '-' || s[0] == '+') ++i;
  if (decimal_word(s + i, len - i, "inf", 3) || decimal_word(s + i, len - i, "infinity", 8) ||
      decimal_word(s + i, len - i, "nan", 3))
    return kDecimalDeclined;
  uint64_t m = 0;
  int nd = 0;            // digits of m: those from the first non-zero one on
  int ndigits = 0;       // digits written
  int nfrac = 0;
  for (; i < len && s[i] >= '0' && s[i] <= '9'; ++i, ++ndigits) {
    if (nd || s[i] != '0') {
      if (nd < 19) m = m * 10 + (s[i] - '0');
      ++nd;
    }
  }
  if (i < len && s[i] == '.') {
    ++i;
    for (; i < len && s[i] >= '0' && s[i] <= '9'; ++i, ++ndigits, ++nfrac) {
      if (nd || s[i] != '0') {
        if (nd < 19) m = m * 10 + (s[i] - '0');
        ++nd;
      }
    }
  }
  if (ndigits == 0) return kDecimalMalformed;
  int ex = 0, exdigits = 0;
  if (i < len && (s[i] == 'e' || s[i] == 'E')) {
    ++i;
    bool eneg = false;
    if (i < len && (s[i] == '-' || s[i] == '+')) eneg = s[i++] == '-';
    for (; i < len && s[i] >= '0' && s[i] <= '9'; ++i, ++exdigits)
      if (exdigits < 4) ex = ex * 10 + (s[i] - '0');
    if (exdigits == 0) return kDecimalMalformed;
    if (eneg) ex = -ex;
  }
  if (i != len) return kDecimalMalformed;
  if (exdigits > 4 || nd > 19) return kDecimalDeclined;
  const uint64_t sign = neg ? 0x8000000000000000ULL : 0ULL;
  if (m == 0) {
    *out = decimal_from_bits(sign);
    return kDecimalOk;
  }
  const int e = ex - nfrac;
  if (e < -27 || e > 27) return kDecimalDeclined;
  double v;
  if (m < (1ULL << 53) && e >= -22 && e <= 22) {
    // 5^22 < 2^52 and the power of two are exact, so is their product: the exact double 10^|e|
    const int k = e < 0 ? -e : e;
    const double p10 = static_cast<double>(decimal_pow5(k)) * static_cast<double>(1ULL << k);
    v = e < 0 ? static_cast<double>(m) / p10 : static_cast<double>(m) * p10;
  } else if (e >= 0) {
    uint64_t hi, lo;
    decimal_mul64(m, decimal_pow5(e), &hi, &lo);
    v = decimal_round128(hi, lo, false, e);
  } else {
    const int k = -e;
    const uint64_t d = decimal_pow5(k);
    const int s0 = decimal_clz64(m);
    const uint64_t mm = m << s0;
    // (mm * 2^64) / d: the high word by one division, the low word bit by bit (r < d < 2^63: r * 2 fits)
    const uint64_t qhi = mm / d;
    uint64_t r = mm % d, qlo = 0;
    for (int b = 0; b < 64; ++b) {
      r <<= 1;
      qlo <<= 1;
      if (r >= d) {
        r -= d;
        qlo |= 1;
      }
    }
    v = decimal_round128(qhi, qlo, r != 0, -64 - s0 - k);
  }
  *out = neg ? -v : v;
  return kDecimalOk;
}

}  // namespace sg
