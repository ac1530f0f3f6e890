// rank_list.h -- the order-dependent rank update of searchPart (search.cpp:464-474) with
// checkOverlap (:327-356).  Plain C++ with no HIP dependency: replay_kernel and
// replay_frames_kernel (search.hip) use these functions as they are, and
// tests/test_rank_list_cpu.py drives them in a host program against a transcription of the
// reference loop.
//
// A list entry E is anything with { double score; int x, y, z, mode; } (c3h_det).
//
// Two forms of one update.  rank_update is the reference's loop over a list in memory.
// rank_slot_update is the same update for a list spread over lanes, slot j on lane j: with
//   i   = the first slot whose score the candidate exceeds (rank_first_greater), and
//   num = the first slot < rank - 1 the candidate overlaps, else rank - 1 (rank_stop_slot),
// both taken on the list before the update, slot j becomes the candidate if j == i <= num,
// the old slot j - 1 if i < j <= num, and stays otherwise -- the reference shifts slots
// i .. num - 1 down by one, dropping slot num, and writes the candidate into slot i, and does
// nothing of either when i > num.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define C3H_RANK_HD __host__ __device__ inline
#else
#define C3H_RANK_HD inline
#endif

namespace c3h {

// the box of a search mode: a permutation of the model's ranges (search.cpp:218-251)
C3H_RANK_HD void get_range(int mode, int r1, int r2, int r3, int& xr, int& yr, int& zr) {
  switch (mode) {
    case 0: xr = r1; yr = r2; zr = r3; break;
    case 1: xr = r1; yr = r3; zr = r2; break;
    case 2: xr = r2; yr = r1; zr = r3; break;
    case 3: xr = r2; yr = r3; zr = r1; break;
    case 4: xr = r3; yr = r1; zr = r2; break;
    default: xr = r3; yr = r2; zr = r1; break;
  }
}

// checkOverlap's test of one entry against a candidate box at (x, y, z) with the candidate
// mode's range (xr, yr, zr): the entry's box is taken with the entry's own mode
template <class E>
C3H_RANK_HD bool rank_overlaps(const E& e, int x, int y, int z, int xr, int yr, int zr, int r1,
                               int r2, int r3) {
  int oxr, oyr, ozr;
  get_range(e.mode, r1, r2, r3, oxr, oyr, ozr);
  int v1 = e.x - x;
  v1 = v1 < 0 ? -v1 - oxr : v1 - xr;
  int v2 = e.y - y;
  v2 = v2 < 0 ? -v2 - oyr : v2 - yr;
  int v3 = e.z - z;
  v3 = v3 < 0 ? -v3 - ozr : v3 - zr;
  return v1 <= 0 && v2 <= 0 && v3 <= 0;
}

// rank update of searchPart (search.cpp:464-474) incl. checkOverlap (:327-356)
template <class E>
C3H_RANK_HD void rank_update(E* L, int rank, double cs, int x, int y, int z, int mode, int xr,
                             int yr, int zr, int r1, int r2, int r3) {
  for (int i = 0; i < rank; i++) {
    if (cs > L[i].score) {
      int num;
      for (num = 0; num < rank - 1; num++)
        if (rank_overlaps(L[num], x, y, z, xr, yr, zr, r1, r2, r3)) break;
      for (int q = 0; q < num - i; q++) L[num - q] = L[num - 1 - q];
      if (i <= num) {
        L[i].score = cs;
        L[i].x = x;
        L[i].y = y;
        L[i].z = z;
        L[i].mode = mode;
      }
      break;
    }
  }
}

// ---- the per-slot form (rank <= 64: one 64-bit mask bit per slot) ----------------------
// index of the lowest set bit (mask != 0)
C3H_RANK_HD int rank_low_bit(uint64_t mask) { return __builtin_ctzll(mask); }

// the slots that take part: bits 0 .. rank - 1
C3H_RANK_HD uint64_t rank_slots(int rank) { return rank >= 64 ? ~0ull : (1ull << rank) - 1; }

// i: greater has bit j set where the candidate's score exceeds slot j's.  -1: no slot, the
// candidate is dropped
C3H_RANK_HD int rank_first_greater(uint64_t greater, int rank) {
  greater &= rank_slots(rank);
  return greater ? rank_low_bit(greater) : -1;
}

// num: overlap has bit j set where the candidate overlaps slot j.  The last slot is never
// tested (checkOverlap's loop ends at rank - 1)
C3H_RANK_HD int rank_stop_slot(uint64_t overlap, int rank) {
  overlap &= rank_slots(rank - 1);
  return overlap ? rank_low_bit(overlap) : rank - 1;
}

// slot j after the update: self and below are slots j and j - 1 before it (below is unused
// for j == 0), i >= 0
template <class E>
C3H_RANK_HD E rank_slot_update(int j, const E& self, const E& below, int i, int num, double cs,
                               int x, int y, int z, int mode) {
  E e = self;
  if (i < j && j <= num) e = below;
  if (j == i && i <= num) {
    e.score = cs;
    e.x = x;
    e.y = y;
    e.z = z;
    e.mode = mode;
  }
  return e;
}

}  // namespace c3h
