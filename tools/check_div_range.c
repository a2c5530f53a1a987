/* Range check of the FAST-region packed divisions (csrc/gen_jit.py
 * manual_div_fast, manual_div_lc_fast, manual_div_rk_fast): with a lower
 * bound only, min(|numerator|, |rcp(divisor)|) >= 2^k, does a division that
 * passes the check ever return a finite value other than the IEEE quotient?
 *
 *   b_div     a / b    r = rcp(b); e = fma(-b, r, 1); r = fma(e, r, r); q = a*r;
 *                      e = fma(-b, q, a); q = fma(e, r, q); e = fma(-b, q, a); q = fma(e, r, q)
 *                      kept when min(|a|, |rcp(b)|) >= 2^k
 *   b_div_lc  c / a    the same sequence with the constant as the numerator,
 *                      kept when min(|c|, |rcp(a)|) >= 2^k
 *   b_div_rk  a / c    y = RN(1/c) from the host, |c| in [2^-60, 2^60];
 *                      q = a*y; r = fma(-c, q, a); q = fma(r, y, q)
 *                      kept when |a| >= 2^k
 *
 * Sweeps every pair of exponents -149 .. 127 (denormals included) with edge
 * and random significands and both signs, the special values (0, Inf, NaN),
 * and random pairs over the whole range. For the bound 2^k it reports, per
 * sequence,
 *   - the kept pairs whose result is finite and differs from RN(a/b), or is
 *     finite where RN(a/b) is not: these must be 0 (exit 1 otherwise);
 *   - the kept pairs whose result is not finite where RN(a/b) is: the
 *     quotients at the overflow edge and the denormal divisors. They are why
 *     the PRECISE region keeps its two-sided check: the FAST region answers a
 *     non-finite value by redoing the tile there.
 *
 * The limit of this model: rcp() below is RN(1/b) with v_rcp_f32's flush of
 * denormal inputs and results, nothing more. The hardware's reciprocal is
 * accurate to 1 ulp, not correctly rounded, and with r off by an ulp the
 * sequence can misround at any exponent; that the hardware's r gives the IEEE
 * quotient is pinned on the GPU (tests/test_div_lower_bound_gpu.py, and
 * tests/test_jit_gpu.py for the PRECISE bodies, which run the same sequence).
 * What this program shows is where the exponent range stops mattering.
 *
 * Build: cc -O2 -ffp-contract=off -mfma -o check_div_range check_div_range.c -lm
 * Usage: check_div_range K [NRANDOM]     (the bound is 2^K, e.g. K = -50) */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static float fb(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bf(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int denormal(float x) { return x != 0.0f && fabsf(x) < 0x1p-126f; }

/* v_rcp_f32 as far as the range goes: denormal in -> 0, denormal out -> 0 */
static float rcp(float b) {
  if (denormal(b)) b = copysignf(0.0f, b);
  float r = 1.0f / b;
  if (denormal(r)) r = copysignf(0.0f, r);
  return r;
}

typedef struct { const char* name; long kept, bad, nonfinite; int shown; } Stat;
static Stat st_div = {"b_div", 0, 0, 0, 0}, st_lc = {"b_div_lc", 0, 0, 0, 0}, st_rk = {"b_div_rk", 0, 0, 0, 0};
static float bound;

static void judge(Stat* s, float a, float b, float q) {
  const float ref = a / b;
  s->kept++;
  if (isfinite(q)) {
    if (bf(q) != bf(ref)) {
      if (s->shown++ < 5) printf("MISMATCH %s a=%a b=%a packed=%a ieee=%a\n", s->name, a, b, q, ref);
      s->bad++;
    }
  } else if (isfinite(ref)) {
    s->nonfinite++;
  }
}

/* the hardware's v_min3 / v_min skip a NaN operand: fminf does the same */
static int keep(float x, float y) { return bound <= fminf(fabsf(x), fabsf(y)); }

static void div_seq(Stat* s, float a, float b) {
  float r = rcp(b);
  if (!keep(a, r)) return;
  float e = fmaf(-b, r, 1.0f);
  r = fmaf(e, r, r);
  float q = a * r;
  e = fmaf(-b, q, a);
  q = fmaf(e, r, q);
  e = fmaf(-b, q, a);
  q = fmaf(e, r, q);
  judge(s, a, b, q);
}

static void rk_seq(float a, float c) {
  if (!(fabsf(c) >= 0x1p-60f && fabsf(c) <= 0x1p60f)) return;  /* the host's condition */
  if (!(bound <= fabsf(a))) return;                             /* NaN a: not kept */
  const float y = 1.0f / c;
  float q = a * y;
  const float r = fmaf(-c, q, a);
  q = fmaf(r, y, q);
  judge(&st_rk, a, c, q);
}

static void all(float a, float b) {
  div_seq(&st_div, a, b);
  div_seq(&st_lc, a, b);  /* c / a: the constant is the numerator here */
  rk_seq(a, b);
}

static uint64_t s = 88172645463325252ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }

/* significand m (23 bits) at exponent e; e < -126 gives a denormal */
static float mk(uint32_t m, int e) { return ldexpf(fb(0x3f800000u | m), e); }

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s K [NRANDOM]   (bound 2^K)\n", argv[0]); return 2; }
  const int k = atoi(argv[1]);
  const long nrand = argc > 2 ? atol(argv[2]) : 20000000L;
  bound = ldexpf(1.0f, k);
  enum { NE = 9, NR = 3, NM = NE + NR };
  uint32_t ma[NM] = {0x000000, 0x000001, 0x7fffff, 0x7ffffe, 0x400000, 0x3fffff, 0x400001, 0x555555, 0x2aaaab};
  uint32_t mb[NM];
  memcpy(mb, ma, sizeof ma);
  long n = 0;
  for (int ea = -149; ea <= 127; ++ea)
    for (int eb = -149; eb <= 127; ++eb) {
      for (int j = NE; j < NM; ++j) { ma[j] = (uint32_t)(rnd() & 0x7fffff); mb[j] = (uint32_t)(rnd() & 0x7fffff); }
      for (int i = 0; i < NM; ++i)
        for (int j = 0; j < NM; ++j) {
          const float a = mk(ma[i], ea), b = mk(mb[j], eb);
          all(a, b);
          all(-a, b);
          n += 2;
        }
    }
  /* the special values against every exponent */
  const float sp[] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, 0x1p-149f, 0x1.fffffep127f};
  for (size_t i = 0; i < sizeof sp / sizeof sp[0]; ++i) {
    for (size_t j = 0; j < sizeof sp / sizeof sp[0]; ++j) { all(sp[i], sp[j]); ++n; }
    for (int e = -149; e <= 127; ++e) {
      const float x = mk((uint32_t)(rnd() & 0x7fffff), e);
      all(sp[i], x);
      all(x, sp[i]);
      n += 2;
    }
  }
  /* random pairs over the whole range */
  for (long i = 0; i < nrand; ++i) {
    const uint64_t r = rnd();
    const int ea = (int)(r % 277) - 149, eb = (int)((r >> 9) % 277) - 149;
    const float a = mk((uint32_t)((r >> 18) & 0x7fffff), ea) * ((r >> 62) & 1 ? -1.0f : 1.0f);
    const float b = mk((uint32_t)(rnd() & 0x7fffff), eb) * ((r >> 63) & 1 ? -1.0f : 1.0f);
    all(a, b);
    ++n;
  }
  printf("bound 2^%d, %ld pairs\n", k, n);
  long bad = 0;
  Stat* const sts[] = {&st_div, &st_lc, &st_rk};
  for (int i = 0; i < 3; ++i) {
    printf("%-9s kept %ld, finite results that differ from IEEE %ld, non-finite where IEEE is finite %ld (%.2f %%)\n",
           sts[i]->name, sts[i]->kept, sts[i]->bad, sts[i]->nonfinite,
           sts[i]->kept ? 100.0 * (double)sts[i]->nonfinite / (double)sts[i]->kept : 0.0);
    bad += sts[i]->bad;
  }
  return bad != 0;
}
