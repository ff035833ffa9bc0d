// swb_pow.hip.inc -- x ** 0.5 exactly as the reference computes it.
//
// spriteworld/tasks.py:127-128 evaluates `np.sum(...) ** 0.5` on a np.float64 scalar, which
// numpy lowers to libm pow(x, 0.5) -- not sqrt.  glibc's pow (>= 2.28, here 2.35) is accurate to
// ~0.52 ULP and differs from the correctly rounded sqrt in ~0.09 % of inputs, so bit-exact
// rewards need the same algorithm: sysdeps/ieee754/dbl-64/e_pow.c (from ARM optimized-routines),
// in the FMA build glibc selects on x86-64 CPUs with FMA (the ifunc'ed __pow_fma): log_inline
// with a 128-entry table and a degree-7 polynomial in double-double, then exp_inline with a
// 128-entry 2^(i/128) table.  The operation order below is that of the compiled function; it is
// specialised to y = 0.5 and to finite x >= 0.  Constants: swb_pow_tables.inc (generated from
// the system libm by tools/extract_glibc_pow_tables.py).  tests/test_pow_half.py compiles this
// file for the host and checks it bit-for-bit against libm pow over 10^7 inputs; on the device
// the function is exercised through the FindGoalPosition parity tests (rewards bit-exact against the oracle's libm pow).
//
// The file is plain C++ apart from three macros so that the host test can include it.
#ifndef SWB_POW_FN
#define SWB_POW_FN __device__
#define SWB_POW_CONST __device__ __constant__ const
#define SWB_FMA(a, b, c) __fma_rn((a), (b), (c))
#define SWB_BITS(x) ((unsigned long long)__double_as_longlong(x))
#define SWB_FROM_BITS(u) __longlong_as_double((long long)(u))
#endif

#include "swb_pow_tables.inc"

SWB_POW_FN double swb_pow_half(double x) {
  unsigned long long ix = SWB_BITS(x);
  if (x == 0.0) return 0.0;                           // pow(+-0, 0.5) = +0
  const unsigned top = (unsigned)(ix >> 52);
  if (top - 1u > 0x7fdu) {                            // subnormal, inf, nan or negative
    if (x != x || (ix >> 63)) return SWB_FROM_BITS(0x7ff8000000000000ull);   // pow(x<0, .5) = nan
    if (top == 0x7ffu) return x;                      // +inf
    ix = SWB_BITS(x * 4503599627370496.0);            // normalise a subnormal: * 2^52
    ix &= 0x7fffffffffffffffull;
    ix -= 52ull << 52;
  }
  // ---- log_inline(ix, &llo)
  const unsigned long long tmp = ix - 0x3fe6955500000000ull;
  const int i = (int)((tmp >> 45) & 127u);
  const int k = (int)((long long)tmp >> 52);
  const unsigned long long iz = ix - (tmp & (0xfffull << 52));
  const double z = SWB_FROM_BITS(iz);
  const double kd = (double)k;
  const double invc = swb_pow_T[i][0], logc = swb_pow_T[i][1], logctail = swb_pow_T[i][2];
  const double t1 = SWB_FMA(kd, swb_pow_ln2hi, logc);
  const double r = SWB_FMA(z, invc, -1.0);
  const double ar = r * swb_pow_A[0];
  const double lo1 = SWB_FMA(kd, swb_pow_ln2lo, logctail);
  const double q12 = SWB_FMA(r, swb_pow_A[2], swb_pow_A[1]);
  const double q34 = SWB_FMA(r, swb_pow_A[4], swb_pow_A[3]);
  const double t2 = t1 + r;
  const double ar2 = r * ar;
  const double ar3 = r * ar2;
  const double lo3 = SWB_FMA(ar, r, -ar2);
  const double lo2 = (t1 - t2) + r;
  const double q56 = SWB_FMA(r, swb_pow_A[6], swb_pow_A[5]);
  const double hi = t2 + ar2;
  const double lo4 = (t2 - hi) + ar2;
  const double q = SWB_FMA(q56, ar2, q34);
  const double P = SWB_FMA(ar2, q, q12);
  const double lo = SWB_FMA(ar3, P, ((lo1 + lo2) + lo3) + lo4);
  const double lhi = hi + lo;
  const double llo = (hi - lhi) + lo;
  // ---- ehi + elo = y * log(x), y = 0.5
  const double ehi = 0.5 * lhi;
  const double elo = SWB_FMA(0.5, llo, SWB_FMA(lhi, 0.5, -ehi));
  // ---- exp_inline(ehi, elo, 0)
  const unsigned abstop = (unsigned)(SWB_BITS(ehi) >> 52) & 0x7ffu;
  if (abstop - 0x3c9u > 0x3eu) {
    if ((int)(abstop - 0x3c9u) < 0) return 1.0 + ehi; // |y log x| < 2^-54
    // |y log x| >= 512 cannot happen for y = 0.5 and finite double x
  }
  const double zz = SWB_FMA(ehi, swb_exp_invln2N, swb_exp_shift);
  const unsigned long long ki = SWB_BITS(zz);
  const double kd2 = zz - swb_exp_shift;
  double rr = SWB_FMA(kd2, swb_exp_negln2hiN, ehi);
  rr = SWB_FMA(kd2, swb_exp_negln2loN, rr);
  rr = elo + rr;
  const int idx = 2 * (int)(ki & 127u);
  const unsigned long long topb = ki << 45;
  const double tail = SWB_FROM_BITS(swb_exp_T[idx]);
  const unsigned long long sbits = swb_exp_T[idx + 1] + topb;
  const double c23 = SWB_FMA(rr, swb_exp_C3, swb_exp_C2);
  const double tr = rr + tail;
  const double r2 = rr * rr;
  const double c45 = SWB_FMA(rr, swb_exp_C5, swb_exp_C4);
  const double t = SWB_FMA(c23, r2, tr);
  const double r4 = r2 * r2;
  const double tmpv = SWB_FMA(c45, r4, t);
  const double scale = SWB_FROM_BITS(sbits);
  return SWB_FMA(tmpv, scale, scale);
}
