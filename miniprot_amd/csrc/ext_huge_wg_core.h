// ext_huge_wg_core.h -- the schedule of k_ext_huge_wg (dp_huge_kernels.hip): the block-major int32 sweep of an X_HUGE
// extension call with one wave per 64-column block, W waves in one workgroup, boundary records handed from a block to its right
// neighbour through LDS.  Host and device compile the same text: the kernel takes every loop bound, ring slot and LDS offset from
// here, and tests/hugewg_check.cpp walks the same functions step by step without a device.  No HIP, no std::, no globals.
#pragma once
#include <cstdint>
#include "dp_device.h"

#define MPA_HWG_HD __host__ __device__ static inline

namespace mpa {
namespace hwg {

// W waves per workgroup, R rows per chunk (a multiple of 3: the row loop is unrolled over the three-row ring, and a chunk starts at
// slot 2 like the sweep itself), MIN_BLOCKS: the fewest column blocks at which a call takes the workgroup kernel (below that the
// pipeline is mostly fill and drain, and the one-wave kernel leaves the CU's LDS to the round).
static const int W = 16;
static const int R = 24;
static const int MIN_BLOCKS = 4;
static const int FIRST_ROW = 2;                 // rows 0 and 1 are the start state; the sweep runs rows 2 .. nl - 1

// LDS: W wave areas as the one-wave kernel has one (profile columns of the wave's block, record ring), then W boundary rings of two
// parities x R records of 16 bytes.  16 x 3328 + 16 x 768 = 65536 bytes: what a launch may ask for without an attribute.
static const int WAVE_LDS = 22 * 64 * 2 + 4 * 32 * 4;           // GLOB_NARROW_LDS of dp_kernels.hip (dp_huge_kernels.hip asserts the two equal)
static const int BND_BYTES = 16;
static const int RING_BYTES = 2 * R * BND_BYTES;
static const int LDS_BYTES = W * (WAVE_LDS + RING_BYTES);
static_assert(R % 3 == 0, "a chunk is a whole number of turns of the three-row ring");
static_assert(LDS_BYTES <= 64 * 1024, "the workgroup's LDS stays within 64 KB");

MPA_HWG_HD int32_t n_blocks(int32_t ncol) { return (ncol + 63) / 64; }
MPA_HWG_HD bool takes_wg(int32_t ncol) { return n_blocks(ncol) >= MIN_BLOCKS; }
MPA_HWG_HD int32_t n_pass(int32_t nblk) { return (nblk + W - 1) / W; }
MPA_HWG_HD int32_t n_chunk(int32_t nl) { return nl > FIRST_ROW ? (nl - FIRST_ROW + R - 1) / R : 0; }
// steps of a pass, one workgroup barrier each: the last wave starts W - 1 steps behind the first.  Uniform over the workgroup.
MPA_HWG_HD int32_t n_step(int32_t nl) { const int32_t nc = n_chunk(nl); return nc > 0 ? nc + W - 1 : 0; }
// the block wave w owns in pass p; it exists when it is below nblk (a wave without a block is idle but passes every barrier)
MPA_HWG_HD int32_t block_of(int32_t p, int w) { return p * W + w; }
// the chunk wave w sweeps at step s of a pass, or -1
MPA_HWG_HD int32_t chunk_at(int32_t s, int w, int32_t nl) { const int32_t c = s - w; return c >= 0 && c < n_chunk(nl) ? c : -1; }
MPA_HWG_HD int32_t chunk_first_row(int32_t c) { return FIRST_ROW + c * R; }
MPA_HWG_HD int32_t chunk_end_row(int32_t c, int32_t nl) { const int32_t e = FIRST_ROW + (c + 1) * R; return e < nl ? e : nl; }
// where the left boundary of a block comes from and where its right boundary goes: nowhere (the call's first / last block), the
// call's bnd[] rows in HBM (the two ends of a pass, like the one-wave kernel between consecutive blocks) or an LDS ring
enum Edge : int { EDGE_NONE = 0, EDGE_HBM = 1, EDGE_LDS = 2 };
MPA_HWG_HD int left_edge(int32_t blk, int w) { return blk == 0 ? EDGE_NONE : w == 0 ? EDGE_HBM : EDGE_LDS; }
MPA_HWG_HD int right_edge(int32_t blk, int w, int32_t nblk) { return blk == nblk - 1 ? EDGE_NONE : w == W - 1 ? EDGE_HBM : EDGE_LDS; }
// byte offsets in the workgroup's LDS: wave w's own area, and the record of row i (of the chunk swept at step s) in wave w's ring.
// Wave w writes at the parity of its step; wave w + 1 reads the same chunk one step later, so at the other parity of ITS step.
MPA_HWG_HD int32_t wave_area(int w) { return w * WAVE_LDS; }
MPA_HWG_HD int32_t ring_slot(int w, int32_t s, int32_t row_in_chunk) { return W * WAVE_LDS + w * RING_BYTES + (((s & 1) * R + row_in_chunk) * BND_BYTES); }
MPA_HWG_HD int32_t ring_write(int w, int32_t s, int32_t i) { return ring_slot(w, s, (i - FIRST_ROW) % R); }
MPA_HWG_HD int32_t ring_read(int w, int32_t s, int32_t i) { return ring_slot(w - 1, s - 1, (i - FIRST_ROW) % R); }

} // namespace hwg
} // namespace mpa
