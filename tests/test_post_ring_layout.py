"""The LDS image of the tall posterior kernel's stages (bot7_amd/csrc/post_ring_layout.h), checked on the host: the
kernel fills the image by LDS-DMA, whose destination is linear in the lane, so the one constexpr map decides both which
16 bytes every lane fetches and where a fragment read finds them.  No GPU needed: a small C++ program includes the
header the kernel includes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "post_ring_layout.h"
#include <cstdio>
#include <set>
#include <vector>
using namespace post_ring;
int main() {
  const int ROWS = 256 + 128, PIECES = ROWS / PIECE_ROWS, SLOTS = ROWS * ROW_BYTES / CHUNK_BYTES, ND = PIECES / WAVES;
  int bad = 0;
  // (1) every 16-byte slot of the image is written by exactly one (wave, instruction, lane);
  // (2) every (row, chunk) is fetched exactly once, and lands where slot_byte() says a reader finds it
  std::vector<int> written(SLOTS, 0), fetched(ROWS * 8, 0);
  for (int w = 0; w < WAVES; ++w)
    for (int i = 0; i < ND; ++i)
      for (int l = 0; l < 64; ++l) {
        const int piece = piece_of(w, i), byte = piece * PIECE_BYTES + CHUNK_BYTES * l;
        if (piece < 0 || piece >= PIECES) { ++bad; continue; }
        ++written[byte / CHUNK_BYTES];
        const Chunk c = dma_src(piece, l);
        if (c.row < 0 || c.row >= ROWS || c.chunk < 0 || c.chunk >= 8) { ++bad; continue; }
        ++fetched[c.row * 8 + c.chunk];
        bad += slot_byte(c.row, c.chunk) != byte;
        // the per-lane source offset (row within the piece, chunk) is the same for every instruction of the wave,
        // and the pieces below 32 are L^-1 rows, the others candidates, for every wave alike
        const Chunk c0 = dma_src(piece_of(w, 0), l);
        bad += c.chunk != c0.chunk || c.row - PIECE_ROWS * piece != (l >> 3) || c.row - c0.row != 32 * i;
      }
  for (int s = 0; s < SLOTS; ++s) bad += written[s] != 1;
  for (int s = 0; s < ROWS * 8; ++s) bad += fetched[s] != 1;
  std::printf("slots %d rows*chunks %d bad %d\n", SLOTS, ROWS * 8, bad);
  // (3) fragment reads: lane (r = l & 15, q = l >> 4) of strip I, k-step s reads 8 bytes at frag_byte(16 I + r, 4 s + q).
  // ds_read_b64 is served in two groups of 32 lanes (0..31, 32..63: 32 x 8 bytes = one pass over the 64 four-byte banks);
  // within a group no bank may be used twice.  The strip offset is an immediate: frag_byte is linear in 16 I.
  int conflicts = 0, nonimm = 0;
  for (int s = 0; s < 4; ++s)
    for (int I = 0; I < ROWS / 16; ++I)
      for (int g = 0; g < 2; ++g) {
        std::set<int> banks;
        for (int l = 32 * g; l < 32 * g + 32; ++l) {
          const int a = frag_byte(16 * I + (l & 15), 4 * s + (l >> 4));
          nonimm += a - frag_byte(l & 15, 4 * s + (l >> 4)) != 16 * I * ROW_BYTES;
          banks.insert((a / 4) % 64);
          banks.insert((a / 4 + 1) % 64);
        }
        conflicts += banks.size() != 64;
      }
  std::printf("conflicts %d nonimm %d\n", conflicts, nonimm);
  return bad || conflicts || nonimm;
}
"""


def test_stage_image_is_filled_once_and_read_without_bank_conflicts(tmp_path):
    src, exe = tmp_path / "ring_layout_check.cpp", tmp_path / "ring_layout_check"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "bot7_amd", "csrc"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "slots 3072 rows*chunks 3072 bad 0" in out.stdout and "conflicts 0 nonimm 0" in out.stdout, out.stdout
