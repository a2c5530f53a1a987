// tail_map.h — block → (row group, tree group, sub-workgroup) of the loss tree
// code's launch when the tree groups of its last row groups are split.
//
// Row groups [0, tbig) (the head) run one workgroup per tree group in the block
// order every launch had before: plain, block b = rg·ntg + g, or dealt over
// the XCDs (xcd; jit_template.hip block_of, a.rotate == 2: the hardware runs
// block b on XCD b mod 8, so rg = (b/8 / ntg)·8 + b mod 8 and g = (b/8) mod ntg
// keep a row group on one XCD; the head is padded to whole octets of row
// groups). Each tree group of the row groups [tbig, nrg) (the tail) is run by
// S workgroups instead; their blocks come after all the others, so the
// dispatcher hands them out last and the launch drains on work units a S-th
// the size. Sub-workgroup `sub` of group g owns the group's list positions
// i ≡ sub (mod S): its claim k is position i = k·S + sub, and its walk ends
// at the first i >= tpb. A position's slot, flag, code offset and partial are
// the ones of the unsplit launch, so the results do not change.
//
// Tail blocks are always dealt over the XCDs: tail block t = b − (head blocks)
// belongs to tail row group (t/8 / (ntg·S))·8 + t mod 8, so all workgroups of
// a tail row group have one residue b mod 8, run on one XCD and share its X
// tile and columns in that XCD's L2. The tail is padded to whole octets of
// row groups; padding blocks own nothing.
//
// tail_map / tail_grid / tail_block are shared by jit_template.hip (the
// drivers), jit.cpp (the grid) and tests/tail_map_test.cpp.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SR_TAIL_HD __host__ __device__ inline
#else
#define SR_TAIL_HD inline
#endif

namespace srhip {

struct TailMap {
  int nrg, ntg;  // row groups, tree groups
  int tbig;      // first tail row group (nrg: no tail)
  int S;         // workgroups per tree group of a tail row group (1: no tail)
  int xcd;       // head blocks dealt over the XCDs (else in plain order)
};

// S < 2 or no tail row group: the plain launch.
SR_TAIL_HD TailMap tail_map(int nrg, int ntg, int tbig, int S, int xcd) {
  TailMap m{nrg, ntg, tbig, S, xcd};
  if (S < 2 || tbig < 0 || tbig >= nrg) {
    m.tbig = nrg;
    m.S = 1;
  }
  return m;
}

SR_TAIL_HD unsigned tail_head(const TailMap& m) {  // blocks of the head, padding included
  return (m.xcd ? (unsigned)(m.tbig + 7) / 8u * 8u : (unsigned)m.tbig) * (unsigned)m.ntg;
}

SR_TAIL_HD unsigned tail_grid(const TailMap& m) {
  const unsigned head = tail_head(m);
  if (m.tbig >= m.nrg) return head;
  const unsigned oct = (unsigned)(m.nrg - m.tbig + 7) / 8u;
  return head + oct * 8u * (unsigned)m.ntg * (unsigned)m.S;
}

// False: a padding block. S_blk is the block's S (1 outside the tail).
SR_TAIL_HD bool tail_block(const TailMap& m, unsigned b, int& rg, int& g, int& sub, int& S_blk) {
  const unsigned head = tail_head(m);
  if (b < head) {
    sub = 0;
    S_blk = 1;
    if (m.xcd) {
      const unsigned k = b >> 3;
      const unsigned oct = k / (unsigned)m.ntg;
      rg = (int)(oct * 8u + (b & 7u));
      g = (int)(k - oct * (unsigned)m.ntg);
      return rg < m.tbig;
    }
    rg = (int)(b / (unsigned)m.ntg);
    g = (int)(b - (unsigned)rg * (unsigned)m.ntg);
    return true;
  }
  const unsigned t = b - head;
  const unsigned k = t >> 3;
  const unsigned per = (unsigned)m.ntg * (unsigned)m.S;  // workgroups of a tail row group
  const unsigned oct = k / per;
  const unsigned w = k - oct * per;
  rg = m.tbig + (int)(oct * 8u + (t & 7u));
  g = (int)(w / (unsigned)m.S);
  sub = (int)(w - (unsigned)g * (unsigned)m.S);
  S_blk = m.S;
  return rg < m.nrg;
}

// The walk itself (claim k of sub-workgroup sub is list position k·S + sub, its
// slot i·ntg + snake(g)) is not in this header: the hand-written loops make it
// (jit_template.hip: the LDS counter started at sub, stepped by S; the slot
// from s41 - s43) and tests/test_jit_tail_trees_gpu.py checks them on the GPU.

}  // namespace srhip
