"""Where the checkpointed traceback of 257..512-column calls keeps its extension bits and checkpoints (dp_device.h, the lite_group_*
functions with eight waves, which the sweep k_lite_w8, the walk k_walk_w8 and the planner's pool sizing all call): a stand-alone C++
program, built with the host compiler and run under AddressSanitizer / UBSan, enumerates every cell and every checkpoint slot of a
group of one or two calls and checks that writer and reader can never collide and never leave what the allocator reserves -- and that
the four-wave instance of the same functions is the lite_wide_* layout of the 129..256-column class, value for value."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "dp_device.h"
using namespace mpa;
static int fail(const char *what, int n_calls, int max_nl, int a, int b, int c)
{
	printf("FAIL %s: calls %d max_nl %d at (%d, %d, %d)\n", what, n_calls, max_nl, a, b, c);
	return 1;
}
int main()
{
	const int NW = MPA_LITE_W8_WAVES, NC = 64 * NW;
	if (NW != 8 || NC != 512) return fail("eight waves, 512 columns", 0, 0, NW, NC, 0);
	const int nls[] = { 3, 4, 5, 23, 24, 25, 97, 98, 99, 194, 300 };
	long cells = 0, slots = 0, same = 0;
	for (int n_calls = 1; n_calls <= 2; ++n_calls)
		for (int max_nl : nls) {
			// ---- extension bits: every (row, column, call) owns four bits of its own inside the reserved dwords
			const int64_t n_bits = lite_group_bits_dwords(NW, max_nl);
			if (n_bits <= 0) return fail("bits reserved", n_calls, max_nl, 0, 0, 0);
			std::vector<uint32_t> used((size_t)n_bits, 0u);            // bit mask of the nibbles taken, per dword
			std::vector<uint32_t> owner((size_t)n_bits, 0u);           // ... and which call took each bit
			for (int slot = 0; slot < n_calls; ++slot)
				for (int i = 2; i < max_nl; ++i)
					for (int j = 0; j < NC; ++j) {
						int32_t sh = -1;
						const int64_t at = lite_group_bit_at(NW, i, j, slot, &sh);
						if (at < 0 || at >= n_bits) return fail("bit word outside the reserved size", n_calls, max_nl, i, j, slot);
						if (sh < 0 || sh > 28 || sh % 4) return fail("nibble position", n_calls, max_nl, i, j, slot);
						if (sh / 16 != slot) return fail("nibble outside the call's half", n_calls, max_nl, i, j, slot);
						const uint32_t m = 0xfu << sh;
						if (used[(size_t)at] & m) return fail("two cells share a nibble", n_calls, max_nl, i, j, slot);
						used[(size_t)at] |= m;
						if (slot) owner[(size_t)at] |= m;
						++cells;
					}
			for (int64_t k = 0; k < n_bits; ++k)                         // the two calls of a pair never share a bit
				if ((used[(size_t)k] & ~owner[(size_t)k] & 0xffff0000u) || (owner[(size_t)k] & 0x0000ffffu)) return fail("calls share bits", n_calls, max_nl, (int)k, 0, 0);
			// the sweep's own addressing: a lane's pointer starts at the word of row 2 and moves by the distance between rows 2 and 5 every three rows;
			// a sweep that ends inside a word still writes that word
			for (int j = 0; j < NC; ++j) {
				int32_t sh;
				const int64_t p0 = lite_group_bit_at(NW, 2, j, 0, &sh), step = lite_group_bit_at(NW, 5, j, 0, &sh) - p0;
				for (int i = 2; i < max_nl; ++i)
					if (lite_group_bit_at(NW, i, j, 0, &sh) != p0 + (int64_t)((i - 2) / 3) * step) return fail("the lane's running pointer", n_calls, max_nl, i, j, 0);
				const int64_t last = p0 + (int64_t)((max_nl - 1 - 2) / 3) * step;
				if (last < 0 || last >= n_bits) return fail("last word of the sweep", n_calls, max_nl, j, 0, 0);
			}
			// ---- checkpoints: nine dwords per (block >= 1, column), 64 apart; the calls differ by their half
			const int64_t n_ck = lite_group_ckpt_dwords(NW, max_nl);
			int n_blk = 0;                                               // blocks k >= 1, counted from the rows: a checkpoint is written (and may be read) at
			for (int i = 3; i < max_nl; ++i)                             // every row 2 < i < max_nl that is the first of a block of 96, and those blocks are 1, 2, ...
				if ((i - 2) % MPA_TB_BLOCK == 0) { if ((i - 2) / MPA_TB_BLOCK != ++n_blk) return fail("block numbering", n_calls, max_nl, i, n_blk, 0); }
			if (n_ck < (int64_t)n_blk * 9 * NC) return fail("checkpoints reserved: fewer than nine dwords per block and column", n_calls, max_nl, n_blk, (int)n_ck, 0);
			if (n_ck < 0 || (n_blk > 0 && n_ck == 0)) return fail("checkpoints reserved", n_calls, max_nl, n_blk, 0, 0);
			std::vector<uint8_t> taken((size_t)n_ck, 0);
			for (int k = 1; k <= n_blk; ++k)
				for (int j = 0; j < NC; ++j) {
					int32_t sh0 = -1, sh1 = -1;
					const int64_t at = lite_group_ckpt_at(NW, k, j, 0, &sh0);
					if (lite_group_ckpt_at(NW, k, j, 1, &sh1) != at || sh0 != 0 || sh1 != 16) return fail("checkpoint halves", n_calls, max_nl, k, j, 0);
					// the walk finds column block cb's checkpoint MPA_LITE_CKPT_WAVE_STEP dwords behind block cb - 1's
					if (at != lite_group_ckpt_at(NW, k, j & 63, 0, &sh0) + (int64_t)(j >> 6) * MPA_LITE_CKPT_WAVE_STEP) return fail("checkpoint wave step", n_calls, max_nl, k, j, 0);
					for (int q = 0; q < 9; ++q) {
						const int64_t d = at + 64 * q;
						if (d < 0 || d >= n_ck) return fail("checkpoint outside the reserved size", n_calls, max_nl, k, j, q);
						if (taken[(size_t)d]) return fail("two checkpoint values share a dword", n_calls, max_nl, k, j, q);
						taken[(size_t)d] = 1;
						++slots;
					}
				}
			// ---- the four-wave instance is the layout of the 129..256-column class: the lite_wide_* functions, and the closed forms they had
			// before the layout took the wave count
			const int W4 = MPA_LITE_WIDE_WAVES;
			if (W4 != 4) return fail("four waves", n_calls, max_nl, W4, 0, 0);
			if (lite_group_bits_dwords(W4, max_nl) != lite_wide_bits_dwords(max_nl) || lite_wide_bits_dwords(max_nl) != ((int64_t)max_nl / 3 + 2) * 256)
				return fail("four-wave bits reserved", n_calls, max_nl, 0, 0, 0);
			if (lite_group_ckpt_dwords(W4, max_nl) != lite_wide_ckpt_dwords(max_nl) || lite_wide_ckpt_dwords(max_nl) != (int64_t)(max_nl > 3 ? (max_nl - 3) / 96 : 0) * 9 * 256)
				return fail("four-wave checkpoints reserved", n_calls, max_nl, 0, 0, 0);
			for (int slot = 0; slot < n_calls; ++slot) {
				for (int i = 2; i < max_nl; ++i)
					for (int j = 0; j < 256; ++j) {
						int32_t a = -1, b = -1;
						const int64_t x = lite_group_bit_at(W4, i, j, slot, &a), y = lite_wide_bit_at(i, j, slot, &b);
						if (x != y || a != b || y != (int64_t)((i - 2) / 3) * 256 + j || b != 16 * slot + 4 * (2 - (i - 2) % 3)) return fail("four-wave bit", n_calls, max_nl, i, j, slot);
						++same;
					}
				for (int k = 1; k <= n_blk; ++k)
					for (int j = 0; j < 256; ++j) {
						int32_t a = -1, b = -1;
						const int64_t x = lite_group_ckpt_at(W4, k, j, slot, &a), y = lite_wide_ckpt_at(k, j, slot, &b);
						if (x != y || a != b || y != ((int64_t)(k - 1) * 4 + (j >> 6)) * (9 * 64) + (j & 63) || b != 16 * slot) return fail("four-wave checkpoint", n_calls, max_nl, k, j, slot);
						++same;
					}
			}
		}
	printf("OK %ld cells %ld checkpoint dwords %ld four-wave values\n", cells, slots, same);
	return 0;
}
"""


def test_class13_bits_and_checkpoints_never_collide(tmp_path):
    """both halves, groups of one and of two calls, max_nl in {3, 4, 5, 23, 24, 25, 97, 98, 99, 194, 300} (no block; the rows at which the
    last of the eight waves starts; one block exactly, one row into the second and third block, a partial last word): every cell (row
    2..nl-1, column 0..511) maps to a nibble of its own inside lite_group_bits_dwords(8, .), every (block >= 1, column) to nine dwords of
    its own inside lite_group_ckpt_dwords(8, .), the two calls of a pair never share a bit, and lite_group_*(4, ...) equals lite_wide_*"""
    src = tmp_path / "ckpt_w8_layout.cpp"
    src.write_text(PROG)
    exe = str(tmp_path / "ckpt_w8_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "miniprot_amd", "csrc"), str(src), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout + r.stderr
