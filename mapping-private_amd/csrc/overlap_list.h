// overlap_list.h -- SearchObjMulti::removeOverlap (search.cpp:972-992) for lists spread over
// lanes.  Plain C++ with no HIP dependency, in the style of rank_list.h (whose overlap test
// and mask helpers it uses): remove_overlap_frames_kernel (search.hip) uses these functions
// as they are, and tests/test_remove_overlap_cpu.py drives them in a host program against a
// transcription of the reference loop.
//
// The reference walks the model pairs (m, m2), m2 != m, in order.  One step:
//   ov = the first slot < rank - 1 of model m2 whose box the box of model m's slot 0
//        overlaps (checkOverlap with slot 0's own mode), else rank - 1;
//   if Lm[0].score > Lm2[ov].score, m2's slots ov .. rank - 2 take the slot above them,
//   otherwise m's slots 0 .. rank - 2 do.  The last slot keeps its entry either way.
// The loop is order-dependent: when m loses, its slot 0 changes and the next m2 sees the new
// one.  Rank 1 has no slot below rank - 1, so nothing moves there.
//
// The per-slot form, slot j on lane j: with `overlap` the ballot of rank_overlaps over m2's
// slots against m's slot 0, ov = rank_stop_slot(overlap, rank); the loser's slot j becomes
// the slot above it for from <= j < rank - 1 (overlap_slot_shift), from = ov for m2 and 0
// for m.  Lane j only ever holds, reads and writes slot j of a list.
#pragma once
#include "rank_list.h"

namespace c3h {

// the step's decision: model m keeps its list and m2's shifts (true), or m's shifts (false)
C3H_RANK_HD bool overlap_m_wins(double score_m0, double score_m2_ov) { return score_m0 > score_m2_ov; }

// slot j of the shifting list after the step: self and above are slots j and j + 1 before it
// (above is unused for j >= rank - 1)
template <class E>
C3H_RANK_HD E overlap_slot_shift(int j, const E& self, const E& above, int from, int rank) {
  return (j >= from && j < rank - 1) ? above : self;
}

}  // namespace c3h
