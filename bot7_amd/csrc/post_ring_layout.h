// LDS image of one stage of the tall posterior kernel (post_kernel_w4t, posterior.hip) and who fills which part of it.
//
// A stage image is ROWS rows (the 256 L^-1 rows of the n-tile, then the workgroup's 128 candidates) of 16 doubles at a
// 128-byte pitch, no padding.  A row is eight 16-byte chunks; chunk c of row r lives at physical chunk c ^ swz(r),
// swz(r) = (r >> 1) & 7.  The image is filled by LDS-DMA: one wave instruction writes one PIECE, 1 KiB = eight whole rows,
// lane l its bytes [16 l, 16 l + 16) -- the destination is linear in the lane, so the permutation sits in the SOURCE
// address: lane l of piece p fetches dma_src(p, l).  Fragment reads apply the same involution (frag_byte).
//
// Bank model (ds_read_b64: 64 banks of 4 bytes, 256 bytes per pass, so a wave is served as two groups of 32 lanes,
// 0..31 and 32..63): lane (r = l & 15, q = l >> 4) of a fragment read takes row 16 I + r, k = 4 s + q.  A group holds
// sixteen rows and two values of q in ONE chunk 2 s + (q >> 1); its bank pair is 16 (r & 1) + 2 ((2 s + (q >> 1)) ^ (r >> 1))
// + (q & 1): the sixteen (r & 1, r >> 1) are distinct and the XOR permutes them, so the 32 lanes hit 32 distinct pairs.
// swz(16 I + r) = swz(r): the strip offset stays an immediate, a lane needs one address per k-step.
//
// Plain constexpr C++: the kernel and the host test (tests/test_post_ring_layout.py) compile this same file.
#pragma once

namespace post_ring {
constexpr int CHUNK_BYTES = 16, ROW_BYTES = 128, PIECE_BYTES = 1024, PIECE_ROWS = PIECE_BYTES / ROW_BYTES, WAVES = 4;

struct Chunk {
  int row, chunk;
};

constexpr int swz(int row) { return (row >> 1) & 7; }

// byte offset of (row, chunk) in the stage image
constexpr int slot_byte(int row, int chunk) { return row * ROW_BYTES + (chunk ^ swz(row)) * CHUNK_BYTES; }

// what lane `lane` of the DMA instruction that writes piece `piece` must fetch: its slot is piece * 1024 + 16 * lane
constexpr Chunk dma_src(int piece, int lane) {
  const int row = piece * PIECE_ROWS + (lane >> 3);
  return Chunk{row, (lane & 7) ^ swz(row)};
}

// the pieces of a stage are dealt round-robin: instruction i of wave w writes piece 4 i + w.  8 (4 i + w) + (lane >> 3)
// has the same bits 1..3 for every i, so a lane's source chunk -- its whole per-lane address offset -- does not depend on i.
constexpr int piece_of(int wave, int i) { return WAVES * i + wave; }

// byte offset of element (row, k) as a fragment read sees it
constexpr int frag_byte(int row, int k) { return slot_byte(row, k >> 1) + (k & 1) * 8; }
}  // namespace post_ring
