// hugewg_check.cpp -- the schedule of k_ext_huge_wg (miniprot_amd/csrc/ext_huge_wg_core.h) walked step by step without a device, under
// AddressSanitizer and UBSan (tests/test_ext_huge_wg_cpu.py compiles and runs it).  The workgroup's LDS is a heap block of exactly
// hwg::LDS_BYTES and a call's bnd[] rows one of exactly nl records, so an offset past either faults.  A boundary record is modelled
// as a tag (block, row, pass, step that wrote it).  Within a step the waves run in no particular order: every shape is walked with the
// waves ascending and descending, and a read must find the same record both times.  Checked for every shape:
//   every (block, row) is swept exactly once;
//   an LDS read finds the record of (block - 1, same row) written in the step before (so: not yet overwritten);
//   an HBM read at a pass's left edge finds the record of (block - 1, same row) written in the pass before;
//   every wave passes the same number of barriers;
//   the areas of the waves and the rings do not overlap.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>
#include "ext_huge_wg_core.h"

using namespace mpa;
using namespace mpa::hwg;

struct Tag { int32_t blk, row, pass, step; };
static_assert(sizeof(Tag) == BND_BYTES, "a tag stands for one boundary record");

static long n_bad = 0;
static void fail(const char *what, int32_t nblk, int32_t nl, int32_t p, int32_t s, int w, int32_t i)
{
	if (++n_bad <= 20) fprintf(stderr, "MISMATCH %s: nblk %d nl %d pass %d step %d wave %d row %d\n", what, nblk, nl, p, s, w, i);
}

static void walk(const int32_t nblk, const int32_t nl, const bool descending)
{
	char *lds = (char*)malloc(LDS_BYTES);
	Tag *bnd = (Tag*)malloc(sizeof(Tag) * (size_t)(nl > 0 ? nl : 1));
	memset(lds, 0xff, LDS_BYTES);
	memset(bnd, 0xff, sizeof(Tag) * (size_t)(nl > 0 ? nl : 1));
	std::vector<int32_t> swept((size_t)nblk * nl, 0);
	long barriers[W] = { 0 };
	const int32_t np = n_pass(nblk), ns = n_step(nl);
	if (ns != (n_chunk(nl) ? n_chunk(nl) + W - 1 : 0)) fail("steps of a pass", nblk, nl, 0, 0, 0, 0);
	for (int32_t p = 0; p < np; ++p) {
		if (p > 0) for (int w = 0; w < W; ++w) ++barriers[w];              // drain, barrier, fence between passes
		for (int w = 0; w < W; ++w) {                                       // a wave's own area: profile columns and record ring
			if (block_of(p, w) >= nblk) continue;
			if (wave_area(w) < 0 || wave_area(w) + WAVE_LDS > ring_slot(0, 0, 0)) fail("wave area reaches the rings", nblk, nl, p, 0, w, 0);
			memset(lds + wave_area(w), w, WAVE_LDS);
		}
		for (int32_t s = 0; s < ns; ++s) {
			for (int k = 0; k < W; ++k) {
				const int w = descending ? W - 1 - k : k;
				const int32_t blk = block_of(p, w);
				const int32_t c = blk < nblk ? chunk_at(s, w, nl) : -1;
				if (c >= 0) {
					const int le = left_edge(blk, w), re = right_edge(blk, w, nblk);
					const int32_t i0 = chunk_first_row(c), i1 = chunk_end_row(c, nl);
					if (i0 < FIRST_ROW || i1 > nl || i1 <= i0 || i1 - i0 > R || (i0 - FIRST_ROW) % 3 != 0) fail("chunk bounds", nblk, nl, p, s, w, i0);
					for (int32_t i = i0; i < i1; ++i) {
						if (le == EDGE_LDS) {
							Tag t;
							memcpy(&t, lds + ring_read(w, s, i), sizeof t);
							if (t.blk != blk - 1 || t.row != i || t.pass != p || t.step != s - 1) fail("LDS read", nblk, nl, p, s, w, i);
						} else if (le == EDGE_HBM) {
							const Tag t = bnd[i];
							if (t.blk != blk - 1 || t.row != i || t.pass != p - 1) fail("HBM read", nblk, nl, p, s, w, i);
						} else if (blk != 0) fail("a later block without a left edge", nblk, nl, p, s, w, i);
						++swept[(size_t)blk * nl + i];
						const Tag out{ blk, i, p, s };
						if (re == EDGE_LDS) {
							if (ring_write(w, s, i) != ring_read(w + 1, s + 1, i)) fail("ring slot of writer and reader", nblk, nl, p, s, w, i);
							if (ring_write(w, s, i) < W * WAVE_LDS) fail("ring slot inside a wave area", nblk, nl, p, s, w, i);
							memcpy(lds + ring_write(w, s, i), &out, sizeof out);
						} else if (re == EDGE_HBM) bnd[i] = out;
						else if (blk != nblk - 1) fail("an inner block without a right edge", nblk, nl, p, s, w, i);
					}
				}
			}
			for (int w = 0; w < W; ++w) ++barriers[w];                          // one workgroup barrier per step
		}
	}
	for (int w = 1; w < W; ++w) if (barriers[w] != barriers[0]) fail("barriers", nblk, nl, 0, 0, w, 0);
	if (barriers[0] != (long)np * ns + (np - 1)) fail("barrier count", nblk, nl, 0, 0, 0, 0);
	for (int32_t b = 0; b < nblk; ++b)
		for (int32_t i = 0; i < nl; ++i)
			if (swept[(size_t)b * nl + i] != (i >= FIRST_ROW ? 1 : 0)) fail("swept", nblk, nl, 0, 0, b % W, i);
	for (int w = 0; w < W && w < nblk; ++w)                                 // the rings never reached into a wave's area
		for (int k = 0; k < WAVE_LDS; ++k) if (lds[wave_area(w) + k] != (char)w) { fail("wave area overwritten", nblk, nl, 0, 0, w, k); break; }
	free(bnd);
	free(lds);
}

int main()
{
	static_assert(W >= 2 && R >= 3 && R % 3 == 0 && MIN_BLOCKS >= 1, "constants");
	static_assert(LDS_BYTES == W * (WAVE_LDS + 2 * R * BND_BYTES) && LDS_BYTES <= 65536, "LDS size");
	const int32_t nblks[] = { MIN_BLOCKS, W - 1, W, W + 1, 2 * W, 2 * W + 1, 107 };
	const int32_t nls[] = { 2, 3, 4, R + 1, R + 2, R + 3, 2 * R + 2, (W - 1) * R + 1, W * R + 3, 5000 };
	long shapes = 0;
	for (int32_t nblk : nblks)
		for (int32_t nl : nls) {
			if (nblk < 1) continue;
			walk(nblk, nl, false), walk(nblk, nl, true), ++shapes;
		}
	uint64_t x = 0x9e3779b97f4a7c15ull;
	auto rnd = [&x](uint32_t n) { x ^= x << 13, x ^= x >> 7, x ^= x << 17; return (int32_t)((x >> 11) % n); };
	for (int k = 0; k < 200; ++k) {
		const int32_t nblk = 1 + rnd(k % 4 == 0 ? 120 : 3 * W), nl = 2 + rnd(k % 5 == 0 ? 6000 : (W + 3) * R);
		walk(nblk, nl, false), walk(nblk, nl, true), ++shapes;
	}
	// which calls take the kernel, and what the executor counts for them
	for (int32_t ncol = 8; ncol <= 8192; ncol += 8)
		if (takes_wg(ncol) != ((ncol + 63) / 64 >= MIN_BLOCKS) || n_pass(n_blocks(ncol)) * W < n_blocks(ncol) || (n_pass(n_blocks(ncol)) - 1) * W >= n_blocks(ncol))
			fail("takes_wg / n_pass", n_blocks(ncol), 0, 0, 0, 0, ncol);
	printf("W %d R %d MIN_BLOCKS %d LDS %d bytes: %ld shapes, %ld mismatches\n", W, R, MIN_BLOCKS, LDS_BYTES, shapes, n_bad);
	return n_bad ? 1 : 0;
}
