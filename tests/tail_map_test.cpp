// The block map of the tree-wise tail split (csrc/tail_map.h), checked on the
// CPU: a stand-alone program, no GPU.
//
// For nrg ∈ {1, 3, 4, 977}, ntg ∈ {1, 3, 17, 64}, tpb ∈ {4, 61, 64, 241},
// S ∈ {1, 2, 4, 8}, every forced tail count 0 … nrg and full and ragged nlist:
//   1. every (row group, list position) whose slot is below nlist is owned by
//      exactly one (block, claim);
//   2. no block owns a position >= tpb;
//   3. S = 1 reproduces the unsplit block -> (rg, g), in the plain block order
//      and in the XCD-dealt one (every check runs in both);
//   4. the blocks of a tail row group share one XCD residue (block mod 8).
// The block map (tail_map, tail_grid, tail_block) is the code the kernels and
// the host run. The walk over a group's list positions is made by the
// hand-written loops (jit_template.hip), not by C++: walk_position and
// walk_slot below are a model of it (the LDS counter started at sub and stepped
// by S, the snake-dealt slot), so (1) and (2) check the design of the walk
// against the block map; the loops themselves are checked on the GPU
// (tests/test_jit_tail_trees_gpu.py).
// Ownership factors: a block owns the positions of its (g, sub) in its row
// group, whichever row group that is. So (1) holds when (a) block ->
// (rg, g, sub) is one-to-one onto {head rg} × g × {0} ∪ {tail rg} × g × sub,
// checked for every tail count (it does not depend on tpb or nlist), and (b)
// for every g the walks of sub = 0 … S−1 (and of the single head workgroup)
// cover each position with a slot below nlist once, checked for every tpb and
// nlist. The small grids (nrg <= 4) are also enumerated directly, block by
// block and claim by claim, with no such reasoning.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tail_map.h"

using namespace srhip;

// the loops' walk, as a model: claim k of sub-workgroup sub, and a position's list slot
static int walk_position(int k, int S, int sub) { return k * S + sub; }
static int walk_slot(int i, int ntg, int g) { return i * ntg + ((i & 1) ? ntg - 1 - g : g); }

static long long checks = 0;
#define REQUIRE(c, ...)                           \
  do {                                            \
    ++checks;                                     \
    if (!(c)) {                                   \
      std::printf("FAILED %s: ", #c);             \
      std::printf(__VA_ARGS__);                   \
      std::printf("\n");                          \
      std::exit(1);                               \
    }                                             \
  } while (0)

// (a), (3), (4) for one launch
static void check_blocks(int nrg, int ntg, int ntail, int S, int dealt, std::vector<unsigned char>& seen,
                         std::vector<int>& xcd) {
  const TailMap m = tail_map(nrg, ntg, nrg - ntail, S, dealt);
  const bool split = S > 1 && ntail > 0;
  REQUIRE(m.S == (split ? S : 1) && m.tbig == (split ? nrg - ntail : nrg), "normalised map nrg %d ntail %d S %d", nrg, ntail, S);
  const unsigned grid = tail_grid(m);
  // the unsplit launch's grid (jit.cpp launch): the XCD deal pads to whole octets of row groups
  if (!split) REQUIRE(grid == (unsigned)(dealt ? (nrg + 7) / 8 * 8 : nrg) * (unsigned)ntg, "unsplit grid");
  seen.assign((size_t)nrg * ntg * m.S, 0);
  xcd.assign((size_t)nrg, -1);
  size_t owned = 0;
  for (unsigned b = 0; b < grid; ++b) {
    int rg = -1, g = -1, sub = -1, Sb = -1;
    // the unsplit launch's map (jit_template.hip block_of), which the head keeps
    const int prg = dealt ? (int)((b >> 3) / (unsigned)ntg) * 8 + (int)(b & 7u) : (int)(b / (unsigned)ntg);
    const int pg = dealt ? (int)((b >> 3) % (unsigned)ntg) : (int)(b % (unsigned)ntg);
    if (!tail_block(m, b, rg, g, sub, Sb)) {
      REQUIRE(rg >= (b < tail_head(m) ? m.tbig : nrg), "a padding block inside the grid's row groups");
      if (!split) REQUIRE(prg >= nrg, "block %u is padding in the split map only", b);
      continue;
    }
    REQUIRE(rg >= 0 && rg < nrg && g >= 0 && g < ntg, "block %u -> rg %d g %d", b, rg, g);
    const bool tail = rg >= m.tbig;
    REQUIRE(Sb == (tail ? m.S : 1) && sub >= 0 && sub < Sb, "block %u sub %d of %d", b, sub, Sb);
    if (!tail) REQUIRE(rg == prg && g == pg, "head block %u moved", b);
    if (tail) {
      REQUIRE(b >= tail_head(m), "a tail block before a head block");
      if (xcd[rg] < 0) xcd[rg] = (int)(b & 7u);
      REQUIRE(xcd[rg] == (int)(b & 7u), "tail row group %d on XCD residues %d and %u", rg, xcd[rg], b & 7u);
    }
    unsigned char& s = seen[((size_t)rg * ntg + g) * m.S + (tail ? sub : 0)];
    REQUIRE(s == 0, "(rg %d, g %d, sub %d) twice", rg, g, sub);
    s = 1;
    ++owned;
  }
  REQUIRE(owned == (size_t)m.tbig * ntg + (size_t)(nrg - m.tbig) * ntg * m.S, "blocks owned %zu", owned);
}

// (b), (2) for one tree group layout
static void check_walks(int ntg, int tpb, int S, int nlist, std::vector<int>& cnt) {
  std::vector<unsigned char> slot((size_t)ntg * tpb, 0);
  int below = 0;  // positions whose slot is below nlist, over all groups
  for (int g = 0; g < ntg; ++g) {
    cnt.assign((size_t)tpb, 0);
    for (int sub = 0; sub < S; ++sub)
      for (int k = 0;; ++k) {
        const int i = walk_position(k, S, sub);
        if (i >= tpb) break;  // the walk ends here: nothing at or past tpb is owned
        ++cnt[i];
      }
    for (int i = 0; i < tpb; ++i) {
      REQUIRE(cnt[i] == 1, "ntg %d tpb %d S %d g %d: position %d owned %d times", ntg, tpb, S, g, i, cnt[i]);
      const int s = walk_slot(i, ntg, g);
      REQUIRE(s >= 0 && s < ntg * tpb, "slot %d", s);
      REQUIRE(slot[s] == 0, "slot of (g %d, i %d) twice", g, i);
      slot[s] = 1;
      below += s < nlist;
    }
  }
  // every slot below nlist is some group's position, once
  REQUIRE(below == nlist, "ntg %d tpb %d nlist %d: %d positions with a slot below nlist", ntg, tpb, nlist, below);
}

// (1), (2) block by block and claim by claim
static void check_direct(int nrg, int ntg, int tpb, int ntail, int S, int dealt, int nlist, std::vector<int>& own) {
  const TailMap m = tail_map(nrg, ntg, nrg - ntail, S, dealt);
  own.assign((size_t)nrg * nlist, 0);
  const unsigned grid = tail_grid(m);
  for (unsigned b = 0; b < grid; ++b) {
    int rg, g, sub, Sb;
    if (!tail_block(m, b, rg, g, sub, Sb)) continue;
    for (int k = 0;; ++k) {
      const int i = walk_position(k, Sb, sub);
      if (i >= tpb) break;
      const int s = walk_slot(i, ntg, g);
      if (s < nlist) ++own[(size_t)rg * nlist + s];  // a slot past nlist is passed over
    }
  }
  for (size_t j = 0; j < own.size(); ++j)
    REQUIRE(own[j] == 1, "nrg %d ntg %d tpb %d ntail %d S %d nlist %d: (rg %zu, slot %zu) owned %d times", nrg, ntg, tpb,
            ntail, S, nlist, j / nlist, j % nlist, own[j]);
}

int main() {
  const int NRG[] = {1, 3, 4, 977}, NTG[] = {1, 3, 17, 64}, TPB[] = {4, 61, 64, 241}, SS[] = {1, 2, 4, 8};
  std::vector<unsigned char> seen;
  std::vector<int> xcd, cnt, own;
  for (int nrg : NRG)
    for (int ntg : NTG)
      for (int S : SS)
        for (int dealt = 0; dealt < 2; ++dealt)
          for (int ntail = 0; ntail <= nrg; ++ntail) check_blocks(nrg, ntg, ntail, S, dealt, seen, xcd);
  for (int ntg : NTG)
    for (int tpb : TPB)
      for (int S : SS) {
        const int full = ntg * tpb;
        // ragged: the last positions of some groups have no slot
        const int ragged = full > 1 ? full - (ntg > 1 ? ntg / 2 + 1 : 1) : 1;
        for (int nlist : {full, ragged}) {
          check_walks(ntg, tpb, S, nlist, cnt);
          for (int nrg : {1, 3, 4})
            for (int dealt = 0; dealt < 2; ++dealt)
              for (int ntail = 0; ntail <= nrg; ++ntail) check_direct(nrg, ntg, tpb, ntail, S, dealt, nlist, own);
        }
      }
  std::printf("tail map ok (%lld checks)\n", checks);
  return 0;
}
