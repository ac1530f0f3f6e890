// occ_sched.h -- the chunk schedule of the bitmap occupancy stream (occupancy_bits_body,
// c3hlac_dev.h).  Plain C++ with no HIP dependency: the kernel uses these helpers as they
// are, the host sizes its launches with them (build_c3_args, launch_tick), and
// tests/test_occ_sched_cpu.py walks them in a host program.
//
// A frame of n4 16-byte words (4 voxels each) is cut into chunks of kOccSchedBlock * depth
// words; lane tid's load j of chunk c reads word c * chunk4 + j * kOccSchedBlock + tid.  The
// last chunk may be partial.  Chunks [0, nstat) are the frame's own: workgroup bx of gdx
// takes one per round, rotated (or one contiguous range).  Chunks [nstat, nch) are the
// pooled tail of the tick: cut into units of steal_unit chunks, unit u of the launch belongs
// to frame u % nframes.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define C3H_SCHED_HD __host__ __device__ inline
#else
#define C3H_SCHED_HD inline
#endif

namespace c3h {

constexpr int kOccSchedBlock = 256;  // threads of a streaming workgroup (kBlock)

// 16-B non-temporal loads per lane per chunk.  The general path holds two more arrays per
// load and spills above 16.  The row-wave path's whole chunks take one lane offset for all
// loads, so up to 24 (96 KiB in flight per CU) fit the tick kernel's 128 VGPRs without a
// spill -- but the tick is fastest at 16: against the clamped loads at 16, the whole tick
// ran +4.0 % at 16, +3.2 % at 12, +1.1 % at 18, -2 % at 20, -4.7 % at 24, -6 % at 8, although
// the stream alone is faster at every depth from 16 to 24 (profiles/r7/occ_depth/).
#ifndef C3H_OCC_UNROLL
#define C3H_OCC_UNROLL 16
#endif
#ifndef C3H_OCC_ROW_UNROLL
#define C3H_OCC_ROW_UNROLL 16
#endif
constexpr int kOccBitsUnroll = C3H_OCC_UNROLL;
constexpr int kOccRowUnroll = C3H_OCC_ROW_UNROLL;

// row-wave path: gx = 256, 512 or 1024 with the axis maps in LDS (a wave's load is one grid row)
C3H_SCHED_HD bool occ_rowwave(int gx, bool ax) { return ax && (gx & 255) == 0 && 1024 % gx == 0; }
C3H_SCHED_HD int occ_depth(bool rowwave) { return rowwave ? kOccRowUnroll : kOccBitsUnroll; }
C3H_SCHED_HD int64_t occ_nchunks(int64_t n4, int depth) {
  const int64_t chunk4 = (int64_t)kOccSchedBlock * depth;
  return (n4 + chunk4 - 1) / chunk4;
}

struct OccSched {
  int64_t n4;      // 16-B words of a frame
  int64_t nch;     // chunks of a frame (the last may be partial)
  int64_t nstat;   // the frame's own chunks are [0, nstat), the pooled tail is [nstat, nch)
  int64_t per;     // rounds: own chunks per workgroup, ceil(nch / gdx)
  int chunk4;      // words per chunk
  int gdx;         // streaming workgroups per frame
  int contiguous;  // 1: workgroup bx streams chunks [bx * per, (bx + 1) * per)
  int steal_unit, steal_units, nframes;  // the pooled tail (steal_unit = 0: none)
};

C3H_SCHED_HD OccSched occ_sched(int64_t n4, int depth, int gdx, int contiguous, int steal_from, int steal_unit,
                                int steal_units, int nframes) {
  OccSched s;
  s.n4 = n4;
  s.chunk4 = kOccSchedBlock * depth;
  s.nch = occ_nchunks(n4, depth);
  s.gdx = gdx;
  s.contiguous = contiguous;
  s.per = (s.nch + gdx - 1) / gdx;
  s.steal_unit = steal_unit > 0 ? steal_unit : 0;
  s.steal_units = steal_unit > 0 ? steal_units : 0;
  s.nframes = nframes;
  s.nstat = steal_unit > 0 ? steal_from : s.nch;
  return s;
}

// Round i in [0, s.per) of workgroup bx: the chunk it streams; a value >= s.nstat means none
// this round (the last, partial round, or a chunk of the pooled tail).  Rotated: chunk
// i * gdx + (bx + i) % gdx, so every workgroup visits every y band of the grid (a fixed
// stride would give workgroup bx the same rows of every plane, and frames' occupancy varies
// with y: the workgroups of one frame ended up to 70 us apart, profiles/r1/tq3_occ_spread.txt).
C3H_SCHED_HD int64_t occ_chunk_of(const OccSched& s, int bx, int64_t i) {
  if (s.contiguous) return i < s.per ? bx * s.per + i : s.nch;
  return i * s.gdx + (int64_t)(((uint32_t)bx + (uint32_t)i) % (uint32_t)s.gdx);
}

// whole chunk: every word of it lies inside the frame (the fast path's unclamped loads)
C3H_SCHED_HD bool occ_chunk_whole(const OccSched& s, int64_t c) { return (c + 1) * s.chunk4 <= s.n4; }

// the word lane tid's load j of chunk c reads
C3H_SCHED_HD int64_t occ_word(const OccSched& s, int64_t c, int j, int tid) {
  return c * s.chunk4 + (int64_t)j * kOccSchedBlock + tid;
}

// A partial chunk on the row-wave path: n4 is a multiple of 64 there (gx of 256), so the 64
// words wave `wave` reads with load j of chunk c lie all inside the frame or all past its end
C3H_SCHED_HD bool occ_wave_load_inside(const OccSched& s, int64_t c, int j, int wave) {
  return occ_word(s, c, j, wave * 64) < s.n4;
}

// unit u in [0, s.steal_units) of the pooled tail: chunks [cb, ce) of frame `frame`
struct OccUnit {
  int frame;
  int64_t cb, ce;
};
C3H_SCHED_HD OccUnit occ_unit(const OccSched& s, int u) {
  OccUnit r;
  r.frame = u % s.nframes;
  r.cb = s.nstat + (int64_t)(u / s.nframes) * s.steal_unit;
  r.ce = r.cb + s.steal_unit < s.nch ? r.cb + s.steal_unit : s.nch;
  return r;
}

// ---- the segment-occupancy map (row-wave path of the tick only)
// One entry (occ_seg_t, below) per span of 256 consecutive voxels (one wave-wide load: 64 lanes x 16 B):
// entry = voxel index >> 8, (folded) bit s set iff any of the 16 words of the span's s-th aligned
// 64-byte segment is non-zero.  gx is a multiple of 256 on this path, so a grid row is
// gx / 256 whole spans and a voxel's bit depends on its x alone.  The stream writes every
// span of every chunk in every frame (the map is allocated in whole chunks, so a partial
// last chunk writes zeros past the grid end); the tile role of the next tick skips the halo
// words whose bit is clear.
constexpr int kOccSpanVox = 256;
C3H_SCHED_HD int64_t occ_seg_entry(int64_t voxel) { return voxel >> 8; }
C3H_SCHED_HD int occ_seg_bit(int64_t voxel) { return (int)((voxel >> 4) & 15); }
// spans of a chunk of `depth` loads (4 waves x depth), and the map entries of a frame
C3H_SCHED_HD int occ_chunk_spans(int depth) { return kOccSchedBlock / 64 * depth; }
C3H_SCHED_HD int64_t occ_seg_entries(int64_t n4, int depth) { return occ_nchunks(n4, depth) * occ_chunk_spans(depth); }
// the span wave `wave` reads with load j of chunk c (= occ_word(s, c, j, wave * 64) * 4 >> 8)
C3H_SCHED_HD int64_t occ_span_of(const OccSched& s, int64_t c, int j, int wave) {
  return c * (s.chunk4 >> 6) + (int64_t)j * (kOccSchedBlock / 64) + wave;
}
// a span's entry from the wave's ballot of non-zero 16-byte quads (lane l = quad l)
C3H_SCHED_HD uint32_t occ_seg_fold32(uint32_t b) {
  uint32_t y = (b | (b >> 1) | (b >> 2) | (b >> 3)) & 0x11111111u;  // bit 4s: nibble s non-zero
  y = (y | (y >> 3)) & 0x03030303u;
  y = (y | (y >> 6)) & 0x000F000Fu;
  return (y | (y >> 12)) & 0xFFu;
}
C3H_SCHED_HD uint16_t occ_seg_fold(uint64_t ballot) {
  return (uint16_t)(occ_seg_fold32((uint32_t)ballot) | (occ_seg_fold32((uint32_t)(ballot >> 32)) << 8));
}
// What the stream stores per span: the folded 16 bits (128 KB per 256^3 frame; the stream
// folds, ~25 VALU per chunk in its row loop).  Measured and removed: the ballot stored as it
// is (8 bytes, 512 KB per frame, the reader folds) -- without the fold the stream alone still
// ended 55-65 us later than with it, the whole tick 4 % later.
typedef uint16_t occ_seg_t;
C3H_SCHED_HD occ_seg_t occ_seg_make(uint64_t ballot) { return occ_seg_fold(ballot); }
C3H_SCHED_HD bool occ_seg_test(occ_seg_t e, int64_t voxel) { return ((e >> occ_seg_bit(voxel)) & 1u) != 0; }

// host: the last 1/div of every frame's chunks go to the pool in units of `unit` chunks
struct OccSteal {
  int from, unit, units;  // unit = 0: no pooled tail
};
inline OccSteal occ_steal_plan(int64_t nch, int nframes, int div, int unit) {
  OccSteal p{0, 0, 0};
  if (div <= 0 || unit <= 0 || nch < 2 * (int64_t)div) return p;
  const int64_t tail = nch / div;
  p.from = (int)(nch - tail);
  p.unit = unit;
  p.units = (int)(nframes * ((tail + unit - 1) / unit));
  return p;
}

}  // namespace c3h
