// grad2_interp.h — second-order forward mode over the gradient programs, for the
// constant gradients of a derivative objective (grad_deriv2.h): ∂²ŷ/∂c∂x.
//
// Every register carries the value v, one feature tangent dx = ∂v/∂x_f (f = the
// item's direction), GC constant tangents dc[j] = ∂v/∂c_{g0+j}, and the mixed
// partials dxc[j] = ∂²v/∂x_f∂c_{g0+j}. With the operator's partials from
// dev::uop_d2 / dev::bop_d2 (device_ops.h):
//   unary   dxc' = f2·dx·dc + f1·dxc
//   binary  dxc' = fxx·lx·lc + fxy·(lx·rc + lc·rx) + fyy·rx·rc + fx·lxc + fy·rxc
// and dx, dc propagate as in grad_interp.h. A leaf has dxc = 0; a feature leaf has
// dx = [its feature is f] and dc = 0, a constant leaf dx = 0 and dc[j] = [j == jc].
// Leaf operands of a binary instruction are applied with selects on those
// wave-uniform conditions, so an unseeded slot never multiplies a partial. The
// programs are the ordinary gradient programs (no folding; compile.cpp).
#pragma once
#include "grad_interp.h"

namespace srhip {
namespace interp {

template <typename T, int R, int GC>
struct Dual2 {
  T v[R];
  T dx[R];
  T dc[GC][R];
  T dxc[GC][R];
};

template <int U, typename T, int R, int GC>
__device__ __forceinline__ void un_grad2(Dual2<T, R, GC>& a, T& chk) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if constexpr (uop_lossy(U)) chk = mark(a.v[r], chk);
    T f, f1, f2;
    dev::uop_d2<U>(a.v[r], f, f1, f2);
    const T s = f2 * a.dx[r];
#pragma unroll
    for (int j = 0; j < GC; ++j) {
      a.dxc[j][r] = s * a.dc[j][r] + f1 * a.dxc[j][r];
      a.dc[j][r] = f1 * a.dc[j][r];
    }
    a.dx[r] = f1 * a.dx[r];
    a.v[r] = f;
  }
}

// fd: the item's feature (wave-uniform); jc: the tangent a constant operand seeds
template <int V, int B, typename T, int R, int GC>
__device__ __forceinline__ void bin_grad2(Dual2<T, R, GC>& a, const Dual2<T, R, GC>& t,
                                          const T* __restrict__ sXt, int rs, int lane, int f, T imm,
                                          int jc, int fd, T& chk) {
  constexpr int SL = src_l(V), SR = src_r(V);
  constexpr bool LL = bop_lossy_lhs(B), LR = bop_lossy_rhs(B);
  constexpr bool CL = computed(SL), CR = computed(SR);
  T xa[R], xb[R];
  if constexpr (SL == S_X || SR == S_X) lds_rows<T, R>(sXt + f * rs, lane, xa);
  if constexpr (SR == S_X2) lds_rows<T, R>(sXt + imm_int(imm) * rs, lane, xb);
  // a leaf operand's seeds: wave-uniform
  const bool lsx = SL == S_X && f == fd;
  const bool rsx = (SR == S_X && f == fd) || (SR == S_X2 && imm_int(imm) == fd);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    T lv, rv;
    if constexpr (SL == S_ACC) lv = a.v[r];
    else if constexpr (SL == S_TMP) lv = t.v[r];
    else if constexpr (SL == S_X) lv = xa[r];
    else lv = imm;
    if constexpr (SR == S_ACC) rv = a.v[r];
    else if constexpr (SR == S_TMP) rv = t.v[r];
    else if constexpr (SR == S_X) rv = xa[r];
    else if constexpr (SR == S_X2) rv = xb[r];
    else rv = imm;
    if constexpr (LL && CL) chk = mark(lv, chk);
    if constexpr (LR && CR) chk = mark(rv, chk);
    T fv, fx, fy, fxx, fxy, fyy;
    dev::bop_d2<B>(lv, rv, fv, fx, fy, fxx, fxy, fyy);
    // the operands' feature tangents (a computed operand carries its own)
    T lx = T(0), rx = T(0);
    if constexpr (SL == S_ACC) lx = a.dx[r];
    else if constexpr (SL == S_TMP) lx = t.dx[r];
    if constexpr (SR == S_ACC) rx = a.dx[r];
    else if constexpr (SR == S_TMP) rx = t.dx[r];
#pragma unroll
    for (int j = 0; j < GC; ++j) {
      const bool lsc = SL == S_C && j == jc, rsc = SR == S_C && j == jc;
      T lc = T(0), rc = T(0), lxc = T(0), rxc = T(0);
      if constexpr (SL == S_ACC) { lc = a.dc[j][r]; lxc = a.dxc[j][r]; }
      else if constexpr (SL == S_TMP) { lc = t.dc[j][r]; lxc = t.dxc[j][r]; }
      if constexpr (SR == S_ACC) { rc = a.dc[j][r]; rxc = a.dxc[j][r]; }
      else if constexpr (SR == S_TMP) { rc = t.dc[j][r]; rxc = t.dxc[j][r]; }
      // dxc' = fxx·lx·lc + fxy·(lx·rc + lc·rx) + fyy·rx·rc + fx·lxc + fy·rxc: a
      // leaf's factors are 0 or 1, taken with selects
      T m = T(0);
      if constexpr (CL) {
        m = fxx * lx * lc;  // both from the computed left operand
        if constexpr (CR) m = m + fxy * (lx * rc + lc * rx);
        else if constexpr (SR == S_C) m = rsc ? m + fxy * lx : m;
        else m = rsx ? m + fxy * lc : m;
        if constexpr (CR) m = m + fyy * rx * rc;
        m = m + fx * lxc;
        if constexpr (CR) m = m + fy * rxc;
      } else if constexpr (CR) {
        // left leaf: lx·lc = 0 (a leaf seeds one kind), lxc = 0
        if constexpr (SL == S_C) m = lsc ? fxy * rx : T(0);
        else m = lsx ? fxy * rc : T(0);
        m = m + fyy * rx * rc;
        m = m + fy * rxc;
      } else {
        // two leaves: only a feature against a constant has a mixed term
        if constexpr (SL == S_X && SR == S_C) m = (lsx && rsc) ? fxy : T(0);
        else if constexpr (SL == S_C && SR == S_X) m = (lsc && rsx) ? fxy : T(0);
      }
      T nc = T(0);
      if constexpr (CL) nc = fx * lc;
      else if constexpr (SL == S_C) nc = lsc ? fx : T(0);
      if constexpr (CR) nc = nc + fy * rc;
      else if constexpr (SR == S_C) nc = rsc ? nc + fy : nc;
      a.dxc[j][r] = m;
      a.dc[j][r] = nc;
    }
    T nx = T(0);
    if constexpr (CL) nx = fx * lx;
    else if constexpr (SL == S_X) nx = lsx ? fx : T(0);
    if constexpr (CR) nx = nx + fy * rx;
    else if constexpr (SR == S_X || SR == S_X2) nx = rsx ? nx + fy : nx;
    a.dx[r] = nx;
    a.v[r] = fv;
  }
}

#define SRG2_PUSH(K)                                                     \
  case OP_PUSH0 + K:                                                     \
    if constexpr (K < D) slot[K] = a;                                    \
    break;
#define SRG2_POP(K)                                                      \
  case OP_POP0 + K:                                                      \
    if constexpr (K < D) t = slot[K];                                    \
    break;
#define SRG2_UN(U) \
  case OP_UN0 + U: un_grad2<U, T, R, GC>(a, chk); break;
#define SRG2_BV(V, B) \
  case bin_opcode(V, B): bin_grad2<V, B, T, R, GC>(a, t, sXt, rs, lane, f, imm, jc, fd, chk); break;
#define SRG2_BIN(B) SRG2_BV(V_AX, B) SRG2_BV(V_XA, B) SRG2_BV(V_AC, B) SRG2_BV(V_CA, B) \
  SRG2_BV(V_AT, B) SRG2_BV(V_TA, B) SRG2_BV(V_XX, B) SRG2_BV(V_XC, B) SRG2_BV(V_CX, B)

// Run one tree's gradient program over one row tile with the feature tangent of
// fd and the tangents of constants g0 .. g0+GC-1; the result is left in a. The
// full operator set (no expression operators: refused by the caller).
template <typename T, int R, int D, int GC>
__device__ __forceinline__ void run_program_grad2(CIns<T>* __restrict__ p, const T* __restrict__ sXt, int rs,
                                                  int lane, int g0, int fd, Dual2<T, R, GC>& a, T& chk) {
  Dual2<T, R, GC> t;
  Dual2<T, R, GC> slot[D];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    a.v[r] = T(0); a.dx[r] = T(0);
    t.v[r] = T(0); t.dx[r] = T(0);
#pragma unroll
    for (int j = 0; j < GC; ++j) { a.dc[j][r] = T(0); a.dxc[j][r] = T(0); t.dc[j][r] = T(0); t.dxc[j][r] = T(0); }
  }
  Ins<T> cur = fetch<T>(p);
  for (;;) {
    const Ins<T> nxt = fetch<T>(p + 1);
    const uint32_t code = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur.code);
    const T imm = uni(cur.imm);
    const int f = (int)(code >> 16);
    const int jc = (int)((code >> 8) & 0xffu) - g0;
    switch (code & 0xffu) {
      case OP_END: return;
      case OP_LDX:
        lds_rows<T, R>(sXt + f * rs, lane, a.v);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          a.dx[r] = (f == fd) ? T(1) : T(0);
#pragma unroll
          for (int j = 0; j < GC; ++j) { a.dc[j][r] = T(0); a.dxc[j][r] = T(0); }
        }
        break;
      case OP_LDC:
#pragma unroll
        for (int r = 0; r < R; ++r) {
          a.v[r] = imm;
          a.dx[r] = T(0);
#pragma unroll
          for (int j = 0; j < GC; ++j) { a.dc[j][r] = (j == jc) ? T(1) : T(0); a.dxc[j][r] = T(0); }
        }
        break;
      SRG2_PUSH(0) SRG2_PUSH(1) SRG2_PUSH(2) SRG2_PUSH(3) SRG2_PUSH(4) SRG2_PUSH(5) SRG2_PUSH(6) SRG2_PUSH(7)
      SRG2_PUSH(8) SRG2_PUSH(9) SRG2_PUSH(10) SRG2_PUSH(11) SRG2_PUSH(12) SRG2_PUSH(13) SRG2_PUSH(14) SRG2_PUSH(15)
      SRG2_POP(0) SRG2_POP(1) SRG2_POP(2) SRG2_POP(3) SRG2_POP(4) SRG2_POP(5) SRG2_POP(6) SRG2_POP(7)
      SRG2_POP(8) SRG2_POP(9) SRG2_POP(10) SRG2_POP(11) SRG2_POP(12) SRG2_POP(13) SRG2_POP(14) SRG2_POP(15)
      SRG2_UN(0) SRG2_UN(1) SRG2_UN(2) SRG2_UN(3) SRG2_UN(4) SRG2_UN(5) SRG2_UN(6) SRG2_UN(7) SRG2_UN(8)
      SRG2_UN(9) SRG2_UN(10) SRG2_UN(11) SRG2_UN(12) SRG2_UN(13) SRG2_UN(14) SRG2_UN(15) SRG2_UN(16)
      SRG2_UN(17) SRG2_UN(18) SRG2_UN(19) SRG2_UN(20) SRG2_UN(21) SRG2_UN(22) SRG2_UN(23) SRG2_UN(24)
      SRG2_UN(25) SRG2_UN(26) SRG2_UN(27) SRG2_UN(28)
      SRG2_BIN(0) SRG2_BIN(1) SRG2_BIN(2) SRG2_BIN(3) SRG2_BIN(4) SRG2_BIN(5) SRG2_BIN(6) SRG2_BIN(7)
      SRG2_BIN(8) SRG2_BIN(9) SRG2_BIN(10)
      default: break;
    }
    cur = nxt;
    ++p;
  }
}

}  // namespace interp
}  // namespace srhip
