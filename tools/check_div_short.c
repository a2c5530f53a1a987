/* CPU model of the shortened packed division (csrc/gen_jit.py manual_div,
 * manual_div_lc and their FAST forms), beside
 * tools/check_div_range.c, which models the sequence it replaces.
 *
 *   A  r = rcp(b); e = fma(-b, r, 1); y = fma(e, r, r);
 *      q = a*y; s = fma(-b, q, a); q' = fma(s, y, q)            (the bodies')
 *   B  r = rcp(b); q = a*r; s = fma(-b, q, a); q = fma(s, r, q);
 *      s = fma(-b, q, a); q' = fma(s, r, q)                     (the fallback)
 *
 * Markstein: with y = RN(1/b) and q = RN(a*y), RN(q + (a - b*q)*y) is RN(a/b).
 * So sequence A can only go wrong at a divisor whose refined reciprocal y is
 * not RN(1/b). The hardware's v_rcp_f32 is accurate to 1 ulp and no more, so
 * the model takes r as each of RN(1/b) and its two neighbours.
 *
 *   sig [NRANDOM] [MAXEXC]
 *       over all 2^23 divisor significands b in [1, 2) and the three r:
 *       where is y != RN(1/b)? Each such (b, r) is then run against all 2^23
 *       numerator significands (at most MAXEXC of them per r, default all),
 *       and NRANDOM (default 1e9) random significand pairs against the three
 *       r. Mismatches with a / b are counted per choice of r; the exit status
 *       is 1 if r = RN(1/b) has any. A mismatch under a neighbour shows a
 *       reciprocal the sequence does not tolerate: whether the hardware ever
 *       returns it is what tools/div_short_sweep.hip settles on the device
 *       (profiles/div_short_exhaustive.json).
 *   range K [NRANDOM]
 *       check_div_range.c's exponent-pair model (-149 .. 127, denormals,
 *       special values, random pairs) for the shorter sequence, r = RN(1/b)
 *       with v_rcp_f32's flushes: the FAST bodies' lower bound
 *       min(|a|, |rcp(b)|) >= 2^K and the PRECISE bodies' two-sided check
 *       2^-45 < |a|, |b| < 2^45. A kept pair must give the IEEE quotient or a
 *       non-finite value (exit 1 otherwise).
 *
 * Build: cc -O2 -ffp-contract=off -mfma -o check_div_short check_div_short.c -lm
 * Usage: check_div_short [A|B] sig [NRANDOM] [MAXEXC] | check_div_short [A|B] range K [NRANDOM] */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static float fb(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bf(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int seq_b = 0;

/* the sequence after the reciprocal */
static float div_seq(float a, float b, float r) {
  float y = r;
  if (!seq_b) {
    const float e = fmaf(-b, r, 1.0f);
    y = fmaf(e, r, r);
  }
  float q = a * y;
  float s = fmaf(-b, q, a);
  q = fmaf(s, y, q);
  if (seq_b) {
    s = fmaf(-b, q, a);
    q = fmaf(s, y, q);
  }
  return q;
}

static float refined(float b, float r) { return seq_b ? r : fmaf(fmaf(-b, r, 1.0f), r, r); }

static uint64_t s = 88172645463325252ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }

static const char* const rname[3] = {"RN(1/b) - 1 ulp", "RN(1/b)", "RN(1/b) + 1 ulp"};

static int run_sig(long nrand, long maxexc) {
  long nexc[3] = {0, 0, 0}, bad_exc[3] = {0, 0, 0}, bad_rnd[3] = {0, 0, 0}, shown = 0;
  for (int k = 0; k < 3; ++k) {
    long done = 0;
    for (uint32_t mb = 0; mb < (1u << 23); ++mb) {
      const float b = fb(0x3f800000u | mb);
      const float rn = 1.0f / b;
      const float r = fb(bf(rn) + (uint32_t)(k - 1));
      if (bf(refined(b, r)) == bf(rn)) continue;
      nexc[k]++;
      if (nexc[k] <= 8) printf("y != RN(1/b): r = %s, b = %a (0x%08x)\n", rname[k], b, bf(b));
      if (done++ >= maxexc) continue;
      for (uint32_t ma = 0; ma < (1u << 23); ++ma) {
        const float a = fb(0x3f800000u | ma);
        const float q = div_seq(a, b, r);
        if (bf(q) != bf(a / b)) {
          if (shown++ < 8) printf("MISMATCH r = %s a=%a b=%a sequence=%a ieee=%a\n", rname[k], a, b, q, a / b);
          bad_exc[k]++;
        }
      }
    }
  }
  for (long i = 0; i < nrand; ++i) {
    const uint64_t x = rnd();
    const float a = fb(0x3f800000u | (uint32_t)(x & 0x7fffff)), b = fb(0x3f800000u | (uint32_t)((x >> 23) & 0x7fffff));
    const float rn = 1.0f / b, ref = a / b;
    for (int k = 0; k < 3; ++k)
      if (bf(div_seq(a, b, fb(bf(rn) + (uint32_t)(k - 1)))) != bf(ref)) {
        if (shown++ < 8) printf("MISMATCH (random) r = %s a=%a b=%a ieee=%a\n", rname[k], a, b, ref);
        bad_rnd[k]++;
      }
  }
  printf("sequence %c, 2^23 divisor significands, %ld random pairs\n", seq_b ? 'B' : 'A', nrand);
  for (int k = 0; k < 3; ++k)
    printf("r = %-15s refined y != RN(1/b) at %ld divisors; those (first %ld) x 2^23 numerators: %ld mismatches; "
           "random pairs: %ld mismatches\n", rname[k], nexc[k], nexc[k] < maxexc ? nexc[k] : maxexc, bad_exc[k], bad_rnd[k]);
  return bad_exc[1] + bad_rnd[1] != 0;
}

/* ---- the exponent-pair model of check_div_range.c for this sequence ---- */
static int denormal(float x) { return x != 0.0f && fabsf(x) < 0x1p-126f; }

/* v_rcp_f32 as far as the range goes: denormal in -> 0, denormal out -> 0 */
static float rcp(float b) {
  if (denormal(b)) b = copysignf(0.0f, b);
  float r = 1.0f / b;
  if (denormal(r)) r = copysignf(0.0f, r);
  return r;
}

typedef struct { const char* name; long kept, bad, nonfinite; int shown; } Stat;
static Stat st_fast = {"FAST (lower bound)", 0, 0, 0, 0}, st_prec = {"PRECISE (two-sided)", 0, 0, 0, 0};
static float bound;

static void judge(Stat* st, float a, float b, float q) {
  const float ref = a / b;
  st->kept++;
  if (isfinite(q)) {
    if (bf(q) != bf(ref)) {
      if (st->shown++ < 5) printf("MISMATCH %s a=%a b=%a packed=%a ieee=%a\n", st->name, a, b, q, ref);
      st->bad++;
    }
  } else if (isfinite(ref)) {
    st->nonfinite++;
  }
}

static void both(float a, float b) {
  const float r = rcp(b);
  /* the hardware's v_min3 / v_min skip a NaN operand: fminf does the same */
  if (bound <= fminf(fabsf(a), fabsf(r))) judge(&st_fast, a, b, div_seq(a, b, r));
  /* v_cmp_gt / v_cmp_lt on v_max3 / v_min3 of |a|, |b|: false for a NaN */
  if (0x1p45f > fmaxf(fabsf(a), fabsf(b)) && 0x1p-45f < fminf(fabsf(a), fabsf(b)) && a == a && b == b)
    judge(&st_prec, a, b, div_seq(a, b, r));
}

static float mk(uint32_t m, int e) { return ldexpf(fb(0x3f800000u | m), e); }

static int run_range(int k, long nrand) {
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
          both(a, b);
          both(-a, b);
          n += 2;
        }
    }
  const float sp[] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, 0x1p-149f, 0x1.fffffep127f};
  for (size_t i = 0; i < sizeof sp / sizeof sp[0]; ++i) {
    for (size_t j = 0; j < sizeof sp / sizeof sp[0]; ++j) { both(sp[i], sp[j]); ++n; }
    for (int e = -149; e <= 127; ++e) {
      const float x = mk((uint32_t)(rnd() & 0x7fffff), e);
      both(sp[i], x);
      both(x, sp[i]);
      n += 2;
    }
  }
  for (long i = 0; i < nrand; ++i) {
    const uint64_t r = rnd();
    const int ea = (int)(r % 277) - 149, eb = (int)((r >> 9) % 277) - 149;
    const float a = mk((uint32_t)((r >> 18) & 0x7fffff), ea) * ((r >> 62) & 1 ? -1.0f : 1.0f);
    const float b = mk((uint32_t)(rnd() & 0x7fffff), eb) * ((r >> 63) & 1 ? -1.0f : 1.0f);
    both(a, b);
    ++n;
  }
  printf("sequence %c, FAST bound 2^%d, PRECISE bounds 2^-45 .. 2^45, %ld pairs\n", seq_b ? 'B' : 'A', k, n);
  long bad = 0;
  Stat* const sts[] = {&st_fast, &st_prec};
  for (int i = 0; i < 2; ++i) {
    printf("%-20s kept %ld, finite results that differ from IEEE %ld, non-finite where IEEE is finite %ld (%.2f %%)\n",
           sts[i]->name, sts[i]->kept, sts[i]->bad, sts[i]->nonfinite,
           sts[i]->kept ? 100.0 * (double)sts[i]->nonfinite / (double)sts[i]->kept : 0.0);
    bad += sts[i]->bad;
  }
  return bad != 0;
}

int main(int argc, char** argv) {
  int i = 1;
  if (i < argc && (!strcmp(argv[i], "A") || !strcmp(argv[i], "B"))) seq_b = argv[i++][0] == 'B';
  if (i < argc && !strcmp(argv[i], "sig"))
    return run_sig(i + 1 < argc ? atol(argv[i + 1]) : 1000000000L, i + 2 < argc ? atol(argv[i + 2]) : (1L << 23));
  if (i + 1 < argc && !strcmp(argv[i], "range"))
    return run_range(atoi(argv[i + 1]), i + 2 < argc ? atol(argv[i + 2]) : 20000000L);
  fprintf(stderr, "usage: %s [A|B] sig [NRANDOM] [MAXEXC] | %s [A|B] range K [NRANDOM]\n", argv[0], argv[0]);
  return 2;
}
