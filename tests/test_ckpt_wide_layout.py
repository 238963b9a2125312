"""Where the checkpointed traceback of 129..256-column calls keeps its extension bits and checkpoints (dp_device.h, the lite_wide_*
functions that the sweep, the walk and the executor's pool sizing all call): a stand-alone C++ program, built with the host compiler
and run under AddressSanitizer / UBSan, enumerates every cell and every checkpoint slot of a group of one or two calls and checks
that writer and reader can never collide and never leave what the allocator reserves."""
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
	const int nls[] = { 3, 4, 5, 97, 98, 99, 194, 300 };
	long cells = 0, slots = 0;
	for (int n_calls = 1; n_calls <= 2; ++n_calls)
		for (int max_nl : nls) {
			// ---- extension bits: every (row, column, call) owns four bits of its own inside the reserved dwords
			const int64_t n_bits = lite_wide_bits_dwords(max_nl);
			if (n_bits <= 0) return fail("bits reserved", n_calls, max_nl, 0, 0, 0);
			std::vector<uint32_t> used((size_t)n_bits, 0u);            // bit mask of the nibbles taken, per dword
			std::vector<uint32_t> owner((size_t)n_bits, 0u);           // ... and which call took each bit
			for (int slot = 0; slot < n_calls; ++slot)
				for (int i = 2; i < max_nl; ++i)
					for (int j = 0; j < 256; ++j) {
						int32_t sh = -1;
						const int64_t at = lite_wide_bit_at(i, j, slot, &sh);
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
			// ---- checkpoints: nine dwords per (block >= 1, column), 64 apart; the calls differ by their half
			const int64_t n_ck = lite_wide_ckpt_dwords(max_nl);
			int n_blk = 0;                                               // blocks k >= 1, counted from the rows: a checkpoint is written (and may be read) at
			for (int i = 3; i < max_nl; ++i)                             // every row 2 < i < max_nl that is the first of a block of 96, and those blocks are 1, 2, ...
				if ((i - 2) % 96 == 0) { if ((i - 2) / 96 != ++n_blk) return fail("block numbering", n_calls, max_nl, i, n_blk, 0); }
			if (n_ck < (int64_t)n_blk * 9 * 256) return fail("checkpoints reserved: fewer than nine dwords per block and column", n_calls, max_nl, n_blk, (int)n_ck, 0);
			if (n_ck < 0 || (n_blk > 0 && n_ck == 0)) return fail("checkpoints reserved", n_calls, max_nl, n_blk, 0, 0);
			std::vector<uint8_t> taken((size_t)n_ck, 0);
			for (int k = 1; k <= n_blk; ++k)
				for (int j = 0; j < 256; ++j) {
					int32_t sh0 = -1, sh1 = -1;
					const int64_t at = lite_wide_ckpt_at(k, j, 0, &sh0);
					if (lite_wide_ckpt_at(k, j, 1, &sh1) != at || sh0 != 0 || sh1 != 16) return fail("checkpoint halves", n_calls, max_nl, k, j, 0);
					for (int q = 0; q < 9; ++q) {
						const int64_t d = at + 64 * q;
						if (d < 0 || d >= n_ck) return fail("checkpoint outside the reserved size", n_calls, max_nl, k, j, q);
						if (taken[(size_t)d]) return fail("two checkpoint values share a dword", n_calls, max_nl, k, j, q);
						taken[(size_t)d] = 1;
						++slots;
					}
				}
		}
	printf("OK %ld cells %ld checkpoint dwords\n", cells, slots);
	return 0;
}
"""


def test_class12_bits_and_checkpoints_never_collide(tmp_path):
    """both halves, groups of one and of two calls, max_nl in {3, 4, 5, 97, 98, 99, 194, 300} (no block, one block exactly, one row
    into the second and third block, a partial last word): every cell (row 2..nl-1, column 0..255) maps to a nibble of its own inside
    lite_wide_bits_dwords(), every (block >= 1, column) to nine dwords of its own inside lite_wide_ckpt_dwords(), and the two calls of
    a pair never share a bit"""
    src = tmp_path / "ckpt_wide_layout.cpp"
    src.write_text(PROG)
    exe = str(tmp_path / "ckpt_wide_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "miniprot_amd", "csrc"), str(src), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout + r.stderr
