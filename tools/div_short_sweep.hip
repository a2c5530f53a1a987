// div_short_sweep.hip — exhaustive device check of a shortened Float32 division
// sequence (tools/, not part of the library).
//
// The tree code's packed division (csrc/gen_jit.py manual_div) is hipcc's IEEE
// sequence without its scaling steps. Whether a shorter sequence still gives
// the IEEE quotient depends on the hardware's v_rcp_f32, which no CPU model
// pins (tools/check_div_short.c takes RN(1/b) and its neighbours). This
// program runs a candidate on the device over EVERY pair of significands,
// a, b in [1, 2): 2^23 x 2^23 = 2^46 pairs, quotients in both binades. Inside
// the bodies' range checks exponents only scale every intermediate by a
// power of two (§3.1), so the significand pairs are the whole question.
//
//   A   r = rcp(b); e = fma(-b, r, 1); y = fma(e, r, r);
//       q = a*y; s = fma(-b, q, a); q' = fma(s, y, q)
//       (the present sequence without its second residual step)
//   B   r = rcp(b); q = a*r; s = fma(-b, q, a); q = fma(s, r, q);
//       s = fma(-b, q, a); q' = fma(s, r, q)
//       (both residual steps, no Newton step on r)
//   C   A without any residual step, q' = a*y: a control that must misround
//       (about a quarter of the pairs), to show that the comparison bites
//
// written with the body's operations: v_rcp_f32 (__builtin_amdgcn_rcpf),
// v_fma_f32 (__builtin_fmaf) and one v_mul_f32, contraction off. v_pk_fma_f32
// and v_pk_mul_f32 round as their scalar forms; that the packed bodies agree
// is pinned by tests/test_div_short_gpu.py. The reference is the compiler's
// correctly rounded a / b (hipcc's default Float32 division: v_div_scale,
// v_div_fmas, v_div_fixup).
//
// Float mode: the tree-code template (csrc/jit_template.hip) is compiled by
// the same compiler with no mode option and no s_setreg, so its kernels and
// this one run in hipcc's default mode for gfx950: round to nearest even for
// f32 and f64, f32 denormals kept (.amdhsa_float_denorm_mode_32 3), f64 / f16
// denormals kept (.amdhsa_float_denorm_mode_16_64 3), IEEE mode on
// (.amdhsa_ieee_mode 1), DX10 clamp on. Build with -ffp-contract=off as the
// template is. (v_rcp_f32 flushes denormals in any mode; no operand here is
// one.)
//
// Each thread owns one divisor significand and walks a slice of the numerator
// significands; one launch covers all 2^23 divisors x 2^SLICE_LOG2 numerators
// (default 2^16: 2^39 pairs, a fraction of a second), the HIP error is read
// after every launch and the first error ends the run. Also recorded: the
// divisor significands whose refined reciprocal y (sequence A) differs from
// RN(1/b) — the only divisors for which Markstein's argument does not already
// give the IEEE quotient — and how many raw v_rcp_f32 results do.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o tools/div_short_sweep tools/div_short_sweep.hip
// Usage: timeout 600 tools/div_short_sweep A|B|C [--out FILE.json] [--lib-hash HEX] [--slice-log2 16]
//            [--a-log2 23]   (--a-log2 N < 23: only the first 2^N numerators, a rehearsal)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(x)                                                                           \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__);          \
      std::exit(1);                                                                        \
    }                                                                                      \
  } while (0)

constexpr unsigned kSig = 1u << 23;  // significands of [1, 2)
constexpr unsigned kOne = 0x3f800000u;
constexpr int kMaxRec = 64;

struct Rec { unsigned a, b, got, ref; };
struct Result {
  unsigned long long mismatches;
  unsigned nrec;  // records claimed (may exceed kMaxRec; only the first kMaxRec are written)
  Rec rec[kMaxRec];
};

template <int SEQ>
__device__ __forceinline__ float refined(float b) {
  const float r = __builtin_amdgcn_rcpf(b);
  if constexpr (SEQ == 1) return r;
  const float e = __builtin_fmaf(-b, r, 1.0f);
  return __builtin_fmaf(e, r, r);
}

template <int SEQ>
__device__ __forceinline__ float quotient(float a, float b, float y) {
  float q = a * y;
  if constexpr (SEQ == 2) return q;
  float s = __builtin_fmaf(-b, q, a);
  q = __builtin_fmaf(s, y, q);
  if constexpr (SEQ == 1) {
    s = __builtin_fmaf(-b, q, a);
    q = __builtin_fmaf(s, y, q);
  }
  return q;
}

// grid: kSig / 256 blocks of 256 threads, thread <-> divisor significand
template <int SEQ>
__global__ void __launch_bounds__(256) sweep(unsigned a0, unsigned na, Result* res) {
  const unsigned mb = blockIdx.x * 256u + threadIdx.x;
  if (mb >= kSig) return;
  const float b = __uint_as_float(kOne | mb);
  const float y = refined<SEQ>(b);
  unsigned bad = 0;
  for (unsigned ma = a0; ma < a0 + na; ++ma) {
    const float a = __uint_as_float(kOne | ma);
    const float got = quotient<SEQ>(a, b, y);
    const float ref = a / b;
    if (__float_as_uint(got) != __float_as_uint(ref)) {
      ++bad;
      const unsigned k = atomicAdd(&res->nrec, 1u);
      if (k < (unsigned)kMaxRec) res->rec[k] = Rec{kOne | ma, kOne | mb, __float_as_uint(got), __float_as_uint(ref)};
    }
  }
  if (bad) atomicAdd(&res->mismatches, (unsigned long long)bad);
}

// flags[mb]: bit 0 the raw v_rcp_f32 differs from RN(1/b), bit 1 sequence A's refined y does
__global__ void __launch_bounds__(256) reciprocals(unsigned char* flags) {
  const unsigned mb = blockIdx.x * 256u + threadIdx.x;
  if (mb >= kSig) return;
  const float b = __uint_as_float(kOne | mb);
  const float rn = 1.0f / b;
  const float r = refined<1>(b), y = refined<0>(b);
  flags[mb] = (unsigned char)((__float_as_uint(r) != __float_as_uint(rn) ? 1 : 0) |
                              (__float_as_uint(y) != __float_as_uint(rn) ? 2 : 0));
}

int main(int argc, char** argv) {
  if (argc < 2 || std::strlen(argv[1]) != 1 || !std::strchr("ABC", argv[1][0])) {
    std::fprintf(stderr, "usage: %s A|B|C [--out FILE.json] [--lib-hash HEX] [--slice-log2 16] [--a-log2 23]\n", argv[0]);
    return 2;
  }
  const int seq = argv[1][0] - 'A';
  std::string out, libhash;
  int slice_log2 = 16, a_log2 = 23;
  for (int i = 2; i + 1 < argc; i += 2) {
    if (!std::strcmp(argv[i], "--out")) out = argv[i + 1];
    else if (!std::strcmp(argv[i], "--lib-hash")) libhash = argv[i + 1];
    else if (!std::strcmp(argv[i], "--slice-log2")) slice_log2 = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--a-log2")) a_log2 = std::atoi(argv[i + 1]);
    else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
  }
  if (a_log2 < 0 || a_log2 > 23 || slice_log2 < 0 || slice_log2 > a_log2) {
    std::fprintf(stderr, "need 0 <= slice-log2 <= a-log2 <= 23\n");
    return 2;
  }
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  std::printf("# %s (%s), sequence %c, 2^23 divisors x 2^%d numerators in slices of 2^%d\n", prop.name,
              prop.gcnArchName, "ABC"[seq], a_log2, slice_log2);

  unsigned char* d_flags;
  CHECK(hipMalloc(&d_flags, kSig));
  hipLaunchKernelGGL(reciprocals, dim3(kSig / 256), dim3(256), 0, 0, d_flags);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<unsigned char> flags(kSig);
  CHECK(hipMemcpy(flags.data(), d_flags, kSig, hipMemcpyDeviceToHost));
  unsigned long long raw_off = 0;
  std::vector<unsigned> exc;
  for (unsigned m = 0; m < kSig; ++m) {
    raw_off += flags[m] & 1;
    if (flags[m] & 2) exc.push_back(kOne | m);
  }
  std::printf("# v_rcp_f32 != RN(1/b) for %llu of 2^23 divisors; refined y != RN(1/b) for %zu\n", raw_off, exc.size());

  Result* d_res;
  CHECK(hipMalloc(&d_res, sizeof(Result)));
  Result h{};  // zeroed by a copy: no memset node
  CHECK(hipMemcpy(d_res, &h, sizeof h, hipMemcpyHostToDevice));
  const unsigned na_all = 1u << a_log2, na = 1u << slice_log2;
  unsigned long long pairs = 0;
  double worst = 0, total = 0;
  for (unsigned a0 = 0; a0 < na_all; a0 += na) {
    const auto t0 = std::chrono::steady_clock::now();
    if (seq == 0) hipLaunchKernelGGL(sweep<0>, dim3(kSig / 256), dim3(256), 0, 0, a0, na, d_res);
    else if (seq == 1) hipLaunchKernelGGL(sweep<1>, dim3(kSig / 256), dim3(256), 0, 0, a0, na, d_res);
    else hipLaunchKernelGGL(sweep<2>, dim3(kSig / 256), dim3(256), 0, 0, a0, na, d_res);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    worst = dt > worst ? dt : worst;
    total += dt;
    pairs += (unsigned long long)kSig * na;
    if ((a0 / na) % 8 == 7 || a0 + na >= na_all) {
      CHECK(hipMemcpy(&h, d_res, sizeof h, hipMemcpyDeviceToHost));
      std::printf("numerators < 0x%06x: %llu pairs, %llu mismatches, %.1f s (slowest slice %.2f s)\n", a0 + na, pairs,
                  h.mismatches, total, worst);
      std::fflush(stdout);
    }
  }
  CHECK(hipMemcpy(&h, d_res, sizeof h, hipMemcpyDeviceToHost));
  const unsigned nrec = h.nrec < (unsigned)kMaxRec ? h.nrec : (unsigned)kMaxRec;
  for (unsigned k = 0; k < nrec && k < 8; ++k)
    std::printf("MISMATCH a=0x%08x b=0x%08x sequence=0x%08x ieee=0x%08x\n", h.rec[k].a, h.rec[k].b, h.rec[k].got,
                h.rec[k].ref);
  std::printf("sequence %c: %llu pairs, %llu mismatches\n", "ABC"[seq], pairs, h.mismatches);

  if (!out.empty()) {
    FILE* f = std::fopen(out.c_str(), "w");
    if (!f) { std::perror(out.c_str()); return 1; }
    std::fprintf(f, "{\n \"tool\": \"tools/div_short_sweep.hip\",\n \"sequence\": \"%c\",\n", "ABC"[seq]);
    std::fprintf(f, " \"sequence_text\": \"%s\",\n",
                 seq == 1 ? "r = rcp(b); q = a*r; s = fma(-b,q,a); q = fma(s,r,q); s = fma(-b,q,a); q = fma(s,r,q)"
                 : seq == 2 ? "control: r = rcp(b); e = fma(-b,r,1); y = fma(e,r,r); q = a*y"
                            : "r = rcp(b); e = fma(-b,r,1); y = fma(e,r,r); q = a*y; s = fma(-b,q,a); q = fma(s,y,q)");
    std::fprintf(f, " \"reference\": \"hipcc's default Float32 a / b\",\n");
    std::fprintf(f, " \"float_mode\": \"round to nearest even, f32 denormals kept, IEEE mode on (hipcc's default, as the tree-code template)\",\n");
    std::fprintf(f, " \"device\": \"%s\",\n \"arch\": \"%s\",\n \"lib_sha256\": \"%s\",\n", prop.name, prop.gcnArchName,
                 libhash.c_str());
    std::fprintf(f, " \"divisor_significands\": %u,\n \"numerator_significands\": %u,\n \"pairs_checked\": %llu,\n", kSig,
                 na_all, pairs);
    std::fprintf(f, " \"exhaustive\": %s,\n", a_log2 == 23 ? "true" : "false");
    std::fprintf(f, " \"mismatches\": %llu,\n \"first_mismatches\": [", h.mismatches);
    for (unsigned k = 0; k < nrec; ++k)
      std::fprintf(f, "%s\n  {\"a\": \"0x%08x\", \"b\": \"0x%08x\", \"sequence\": \"0x%08x\", \"ieee\": \"0x%08x\"}", k ? "," : "",
                   h.rec[k].a, h.rec[k].b, h.rec[k].got, h.rec[k].ref);
    std::fprintf(f, "],\n \"raw_rcp_differs_from_rn\": %llu,\n", raw_off);
    std::fprintf(f, " \"refined_reciprocal_exceptions\": %zu,\n \"refined_reciprocal_exception_set\": [", exc.size());
    for (size_t k = 0; k < exc.size() && k < 4096; ++k)  // a longer set is cut at 4096 entries (the count above is whole)
      std::fprintf(f, "%s\"0x%08x\"", k ? ", " : "", exc[k]);
    std::fprintf(f, "],\n \"slices\": %u,\n \"slowest_slice_s\": %.3f,\n \"sweep_s\": %.1f\n}\n", na_all / na, worst, total);
    std::fclose(f);
  }
  return h.mismatches != 0;
}
