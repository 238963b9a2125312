// dp_traceback_kernels.hip -- the traceback launches outside the round kernel: k_glob_narrow / k_glob_wide (the int32 traceback sweeps
// glob_narrow / glob_wide_body of dp_kernels.hip as launches of their own: the traceback chunks after a round's first, the 512/1024-
// thread classes, and every traceback of a run whose penalties do not fit a record's byte), k_backtrack (the walk over traceback
// words), k_walk / k_walk_w8 / walk_call (the walk of the checkpointed traceback, which sweeps a block of rows again where the path is
// not in a run) and k_cigar_gather (the dense copy of the CIGARs).  Launched by dp_exec.hip behind the round's sweeps (phase 4); none of this
// code runs inside k_dp_round or k_dp_worker.
// Included by dp_exec.hip behind dp_kernels.hip.  Relies on dp_kernels.hip for: WavePos / whole_block, wave_sync, GlobArgs, GlobResume,
// glob_narrow, glob_wide_body and GLOB_NARROW_LDS; on dp_device.h for the layout of the extension-bit words and checkpoints.
#pragma once
#include "dp_kernels.hip"

namespace mpa {

// One launch for the three narrow shapes (16 / 32 / 64 lanes per call): wave b of the launch belongs to the class whose
// range of wave descriptors contains it.  Fewer, larger launches matter because every concurrently running kernel
// occupies a hardware queue and a stream of batches keeps several rounds in flight (dp_exec.hip).
struct NarrowMap { int32_t first[4], cnt[4]; };

// one launch for the narrow traceback shapes (classes 16 / 32 / 64 lanes and the block-major one), see k_ext_narrow
template<bool WIDE>
__global__ __launch_bounds__(64) void k_glob_narrow(GlobArgs a, NarrowMap m)
{
	int b = blockIdx.x;
	extern __shared__ __attribute__((aligned(16))) uint32_t lds_raw[];
	const WavePos wp = whole_block((char*)lds_raw);
	if (b < m.cnt[0]) { glob_narrow<16, false, false, WIDE>(a, a.waves[m.first[0] + b], wp); return; }
	b -= m.cnt[0];
	if (b < m.cnt[1]) { glob_narrow<32, false, false, WIDE>(a, a.waves[m.first[1] + b], wp); return; }
	b -= m.cnt[1];
	if (b < m.cnt[2]) { glob_narrow<64, false, false, WIDE>(a, a.waves[m.first[2] + b], wp); return; }
	b -= m.cnt[2];
	glob_narrow<64, true, false, WIDE>(a, a.waves[m.first[3] + b], wp);
}

template<int NW, bool WIDE>
__global__ __launch_bounds__(NW * 64) void k_glob_wide(GlobArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds_raw[];
	glob_wide_body<NW, WIDE>(a, a.waves[blockIdx.x], whole_block((char*)lds_raw));
}

// ------------------------------------------------------------------------------------------------
// traceback walk (ns_backtrack nasw-sse.c:40-89), one WAVE per call.
//
// The reference follows one cell per step.  The path is made of runs that move in a fixed direction while
// a bit of the traceback word stays set (match runs on the diagonal, gap/intron extensions along a column
// or a row), so the 64 lanes fetch the next 64 cells of the current direction at once, a ballot finds where
// the run ends, and the whole run is emitted as one CIGAR operation.  A 50 kb intron costs ~800 dependent
// memory round trips instead of 50 000.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_backtrack(const DTask *tasks, const int32_t *list, int32_t n_list, const uint16_t *tbpool, uint32_t *cigpool, int32_t *n_cigar)
{
	MPA_SHORT_KERNEL();
	if ((int32_t)blockIdx.x >= n_list) return;
	const int32_t tid = list[blockIdx.x];
	const DTask t = tasks[tid];
	const uint16_t *tb = tbpool + t.tb_off;
	uint32_t *cig = cigpool + t.cig_off;
	const int32_t ncol = t.ncol, cap = t.cig_cap, lane = threadIdx.x;
	int32_t i = t.nl - 1, j = t.al - 1, carry = 0, n = 0;
	// the CIGAR operation being accumulated (ns_push_cigar merges equal neighbours except F/G, nasw.h:141-152)
	int32_t cur_op = -1, cur_len = 0;
	auto push = [&](int32_t op, int32_t len) {
		if (cur_op == op && op != 10 && op != 11) { cur_len += len; return; }
		if (cur_op >= 0) { if (lane == 0 && n < cap) cig[n] = (uint32_t)cur_len << 4 | (uint32_t)cur_op; ++n; }
		cur_op = op, cur_len = len;
	};
	auto state_of = [](int32_t w) { return (w >> 9 & 1) ? 1 : (w & 0xf); };   // a cell raised by the cross-lane I counts as I
	while (i >= 2 && j >= 0) {
		int32_t st = carry;
		if (st == 0) {                                           // fresh cell: its own state decides the direction
			const int32_t w0 = tb[(int64_t)i * ncol + j];
			st = state_of(w0);
		}
		if (st == 0) {                                           // run of matches on the diagonal (i-3l, j-l)
			const int32_t ii = i - 3 * lane, jj = j - lane;
			const bool ok = ii >= 2 && jj >= 0;
			const int32_t w = ok ? tb[(int64_t)ii * ncol + jj] : 0xf;
			const uint64_t stop = __ballot(!ok || state_of(w) != 0);
			const int32_t run = stop ? __ffsll((unsigned long long)stop) - 1 : 64;
			push(0, run), i -= 3 * run, j -= run, carry = 0;
		} else if (st <= 5) {                                    // extension runs: I along the row, D/N/U/V along the column
			const int32_t di = st == 1 ? 0 : st == 2 ? 3 : 1, dj = st == 1 ? 1 : 0;
			const int32_t ii = i - di * lane, jj = j - dj * lane;
			const bool ok = ii >= 2 && jj >= 0;
			const int32_t w = ok ? tb[(int64_t)ii * ncol + jj] : 0;
			const bool ext = ok && (w >> (st + 3) & 1);
			const uint64_t inval = __ballot(!ok), noext = __ballot(!ext);
			// cells are consumed up to and including the first one whose extension bit is clear; a cell outside
			// the matrix ends the walk before it is consumed
			const int32_t first_noext = noext ? __ffsll((unsigned long long)noext) - 1 : 64;
			const int32_t first_inval = inval ? __ffsll((unsigned long long)inval) - 1 : 64;
			int32_t run;
			bool closed;                                          // did the run meet a cell with the extension bit clear?
			if (first_noext < first_inval) run = first_noext + 1, closed = true;
			else run = first_inval, closed = false;
			static const int32_t op_of[6] = { 0, 1, 2, 3, 12, 13 };
			push(op_of[st], run);
			i -= di * run, j -= dj * run;
			if (closed && (st == 4 || st == 5)) --j;               // the intron of phase 1/2 ends inside a codon
			carry = closed ? 0 : st;
			if (run == 0) break;                                  // cannot happen (the loop condition holds for lane 0)
		} else {                                                 // frameshifts: one cell
			if (st == 6) push(10, 1), i -= 1;
			else if (st == 7) push(10, 2), i -= 2;
			else if (st == 8) push(11, 1), i -= 1, j -= 1;
			else push(11, 2), i -= 2, j -= 1;
			carry = 0;
		}
	}
	if (j > 0) push(1, j);
	if (i >= 0) {
		const int32_t l = (i + 1) / 3 * 3, r = (i + 1) % 3;
		if (l > 0) push(2, l);
		if (r != 0) push(10, r);
	}
	push(-2, 0);                                                 // flush
	if (n > cap) n = cap;
	__syncthreads();
	for (int32_t x = lane; x < n >> 1; x += 64) { uint32_t tmp = cig[x]; cig[x] = cig[n - 1 - x], cig[n - 1 - x] = tmp; }
	__syncthreads();
	for (int32_t x = lane; x < n; x += 64) {                      // ns_fix_tiny_UV
		const uint32_t op = cig[x] & 0xf;
		if ((op == 12 || op == 13) && cig[x] >> 4 < 3) cig[x] = cig[x] >> 4 << 4 | 11;
	}
	if (lane == 0) n_cigar[tid] = n;
}

// ------------------------------------------------------------------------------------------------
// The walk of the checkpointed traceback (dp_device.h): ns_backtrack (nasw-sse.c:40-89) over a call whose sweep kept only the four
// extension bits per cell and a checkpoint per block of MPA_TB_BLOCK rows.  One wave per call.  Deletion and intron runs (states 2..5)
// are followed on the bits, 64 cells at a time; in any other state the wave first recomputes the traceback words of the block it
// stands in (glob_narrow restarted from the block's checkpoint, words into LDS) and walks those, exactly like k_backtrack -- a run
// that leaves the block is simply continued in the next iteration.  A call is swept twice only where its path is not in a run.
// ------------------------------------------------------------------------------------------------
struct WalkArgs {
	GlobArgs ga;                 // tasks, records, profiles, scoring
	const int32_t *list;         // the calls
	int32_t n_list;
	const uint32_t *lite, *ckpt; // extension-bit words and checkpoints of the packed sweeps
	uint32_t *cig;
	int32_t *n_cigar;
	unsigned long long *n_blocks; // (statistics) blocks recomputed
};
// (per class of the packed sweep -- 16 / 32 / 64 / 128 / 256 / 512 columns at most: 8 / 11 / 17 / 29 / 53 / 101 KB; one launch per class, so that the
// narrow calls' walks, most of them, take LDS for their own block of direction words and not for a 256- or 512-column one)
#define WALK_LDS(NC) (GLOB_NARROW_LDS + (size_t)MPA_TB_BLOCK * (NC) * 2 + (size_t)(MPA_TB_BLOCK + 2) * 16)
// DUAL: a call of 65..128 columns, swept with column c + 64 in the high half of lane c (ext_narrow<64, true, true>) and recomputed
// by the block-major traceback sweep (two blocks of 64 columns, boundary records in LDS)
// WIDE4: a call of 129..256 columns, swept by a four-wave group (lite_wide_body; the call is int16 half `slot` of every lane) and
// recomputed by the same block-major sweep over up to four blocks of 64 columns, each from the checkpoint of the wave that swept it
// DUAL and WIDE4 together: a call of 257..512 columns, swept by an EIGHT-wave group (k_walk_w8; the same template parameters, so that the
// instances k_walk is made of keep their names and k_walk its code object): everything of WIDE4 with GW = 8 waves, up to eight blocks of
// 64 columns whose (checkpoint, shift) pairs are worked out per column block from the first (glob_narrow's CKSTEP), not held for all eight
template<int G, bool DUAL = false, bool WIDE4 = false>
__device__ __forceinline__ void walk_call(const WalkArgs &wa, const DTask &t, const int32_t tid, char *lds, const int lane)
{
	constexpr int GW = WIDE4 ? (DUAL ? MPA_LITE_W8_WAVES : MPA_LITE_WIDE_WAVES) : 0;   // the waves of the group that swept the call (its int16 half is its slot)
	constexpr bool DUAL2 = DUAL && !WIDE4;                         // the 65..128-column class proper
	static_assert(!(DUAL || WIDE4) || G == 64, "the block-major classes are swept in blocks of 64 columns");
	constexpr int NG = 64 / G;
	const int slot = DUAL2 ? 0 : (t.flag >> MPA_LITE_SLOT_SHIFT) & 15, half = WIDE4 ? slot : slot / NG, lane0 = WIDE4 ? 0 : (slot % NG) * G;
	const uint32_t *lite = wa.lite + t.tb_off + lane0;
	uint16_t *tbs = (uint16_t*)(lds + GLOB_NARROW_LDS);            // [MPA_TB_BLOCK][ncol] words of the block that is materialised
	int4 *bnds = (int4*)(lds + GLOB_NARROW_LDS + (size_t)MPA_TB_BLOCK * (WIDE4 ? GW * 64 : DUAL ? 128 : G) * 2);
	uint32_t *cig = wa.cig + t.cig_off;
	const int32_t ncol = t.ncol, cap = t.cig_cap;
	int32_t blk = -1, blk_lo = 0, blk_hi = 0;                      // the materialised block and its rows [blk_lo, blk_hi)
	auto ensure = [&](const int32_t row) {
		if (blk >= 0 && row >= blk_lo && row < blk_hi) return;
		const int32_t b = (row - 2) / MPA_TB_BLOCK;
		constexpr int NCB = GW == 4 ? 4 : DUAL2 ? 2 : 1, CKSTEP = GW == 8 ? MPA_LITE_CKPT_WAVE_STEP : 0;
		GlobResume<NCB> rz;
		rz.row_off = b * MPA_TB_BLOCK, rz.n_rows = t.nl - 2 - rz.row_off < MPA_TB_BLOCK ? t.nl - 2 - rz.row_off : MPA_TB_BLOCK;
#pragma unroll
		for (int cb = 0; cb < NCB; ++cb) {
			rz.ck[cb] = nullptr, rz.sh[cb] = 0;
			if (b == 0) continue;
			if (WIDE4) rz.ck[cb] = wa.ckpt + t.bnd_off + lite_group_ckpt_at(GW, b, 64 * cb, half, &rz.sh[cb]);
			else rz.ck[cb] = wa.ckpt + t.bnd_off + (int64_t)(b - 1) * 9 * 64 + lane0, rz.sh[cb] = 16 * (DUAL ? cb : half);
		}
		rz.tb = tbs, rz.bnd = bnds;
		GlobWave gw;
		gw.task[0] = tid, gw.task[1] = gw.task[2] = gw.task[3] = -1, gw.max_nl = rz.n_rows + 2;
		wave_sync();
		glob_narrow<G, DUAL || WIDE4, false, false, NCB, CKSTEP>(wa.ga, gw, WavePos{ lds, lane, 0, lane }, &rz);
		wave_sync();
		blk = b, blk_lo = 2 + rz.row_off, blk_hi = blk_lo + rz.n_rows;
		if (lane == 0) atomicAdd(wa.n_blocks, 1ULL);
	};
	auto full = [&](const int32_t ii, const int32_t jj) -> int32_t { return tbs[(ii - blk_lo) * ncol + jj]; };
	auto nibble = [&](const int32_t ii, const int32_t jj) -> int32_t {
		if (WIDE4) {
			int32_t sh;
			const int64_t at = lite_group_bit_at(GW, ii, jj, half, &sh);
			return (int32_t)(lite[at] >> sh) & 0xf;
		}
		const uint32_t r = (uint32_t)(ii - 2);
		return (int32_t)(lite[(int64_t)(r / 3) * 64 + (DUAL ? jj & 63 : jj)] >> (16 * (DUAL ? jj >> 6 : half) + 4 * (2 - r % 3))) & 0xf;
	};
	int32_t i = t.nl - 1, j = t.al - 1, carry = 0, n = 0;
	int32_t cur_op = -1, cur_len = 0;                              // (ns_push_cigar merges equal neighbours except F/G, nasw.h:141-152)
	auto push = [&](int32_t op, int32_t len) {
		if (cur_op == op && op != 10 && op != 11) { cur_len += len; return; }
		if (cur_op >= 0) { if (lane == 0 && n < cap) cig[n] = (uint32_t)cur_len << 4 | (uint32_t)cur_op; ++n; }
		cur_op = op, cur_len = len;
	};
	auto state_of = [](int32_t w) { return (w >> 9 & 1) ? 1 : (w & 0xf); };
	while (i >= 2 && j >= 0) {
		int32_t st = carry;
		if (st == 0) { ensure(i); st = state_of(full(i, j)); }          // fresh cell: its own state decides the direction
		if (st == 0) {                                               // run of matches on the diagonal (i-3l, j-l), inside the block
			const int32_t ii = i - 3 * lane, jj = j - lane;
			const bool ok = ii >= blk_lo && jj >= 0;
			const int32_t w = ok ? full(ii, jj) : 0xf;
			const uint64_t stop = __ballot(!ok || state_of(w) != 0);
			const int32_t run = stop ? __ffsll((unsigned long long)stop) - 1 : 64;
			push(0, run), i -= 3 * run, j -= run, carry = 0;
		} else if (st <= 5) {                                        // extension runs: I along the row (words), D/N/U/V along the column (bits)
			const int32_t di = st == 1 ? 0 : st == 2 ? 3 : 1, dj = st == 1 ? 1 : 0;
			if (st == 1) ensure(i);
			const int32_t ii = i - di * lane, jj = j - dj * lane;
			const bool ok = ii >= 2 && jj >= 0;
			bool ext = false;
			if (ok) ext = st == 1 ? (full(ii, jj) >> 4 & 1) != 0 : (nibble(ii, jj) >> (st - 2) & 1) != 0;
			const uint64_t inval = __ballot(!ok), noext = __ballot(!ext);
			const int32_t first_noext = noext ? __ffsll((unsigned long long)noext) - 1 : 64;
			const int32_t first_inval = inval ? __ffsll((unsigned long long)inval) - 1 : 64;
			int32_t run;
			bool closed;
			if (first_noext < first_inval) run = first_noext + 1, closed = true;
			else run = first_inval, closed = false;
			static const int32_t op_of[6] = { 0, 1, 2, 3, 12, 13 };
			push(op_of[st], run);
			i -= di * run, j -= dj * run;
			if (closed && (st == 4 || st == 5)) --j;
			carry = closed ? 0 : st;
			if (run == 0) break;
		} else {                                                     // frameshifts: one cell
			if (st == 6) push(10, 1), i -= 1;
			else if (st == 7) push(10, 2), i -= 2;
			else if (st == 8) push(11, 1), i -= 1, j -= 1;
			else push(11, 2), i -= 2, j -= 1;
			carry = 0;
		}
	}
	if (j > 0) push(1, j);
	if (i >= 0) {
		const int32_t l = (i + 1) / 3 * 3, r = (i + 1) % 3;
		if (l > 0) push(2, l);
		if (r != 0) push(10, r);
	}
	push(-2, 0);                                                 // flush
	if (n > cap) n = cap;
	__syncthreads();
	for (int32_t x = lane; x < n >> 1; x += 64) { uint32_t tmp = cig[x]; cig[x] = cig[n - 1 - x], cig[n - 1 - x] = tmp; }
	__syncthreads();
	for (int32_t x = lane; x < n; x += 64) {                      // ns_fix_tiny_UV
		const uint32_t op = cig[x] & 0xf;
		if ((op == 12 || op == 13) && cig[x] >> 4 < 3) cig[x] = cig[x] >> 4 << 4 | 11;
	}
	if (lane == 0) wa.n_cigar[tid] = n;
}
__global__ __launch_bounds__(64) void k_walk(WalkArgs wa)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds_raw[];
	if ((int32_t)blockIdx.x >= wa.n_list) return;
	const int32_t tid = wa.list[blockIdx.x];
	const DTask t = wa.ga.tasks[tid];
	const int lane = (int)threadIdx.x;
	switch (t.cls) {                                             // (class of the call's packed sweep)
	case T_LITE16: walk_call<16>(wa, t, tid, (char*)lds_raw, lane); break;
	case T_LITE32: walk_call<32>(wa, t, tid, (char*)lds_raw, lane); break;
	case T_LITE64: walk_call<64>(wa, t, tid, (char*)lds_raw, lane); break;
	case T_LITE128: walk_call<64, true>(wa, t, tid, (char*)lds_raw, lane); break;   // 65..128 columns, one call per wave
	case T_LITE_W4: walk_call<64, false, true>(wa, t, tid, (char*)lds_raw, lane); break;   // 129..256 columns, a four-wave group per pair of calls
	default: break;
	}
}
// the walk of the 257..512-column class (T_LITE_W8), a kernel of its own: its block of direction words takes WALK_LDS(512) and its
// recomputation goes over up to eight column blocks -- inside k_walk it would set that kernel's registers and LDS for every class
__global__ __launch_bounds__(64) void k_walk_w8(WalkArgs wa)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds_raw[];
	if ((int32_t)blockIdx.x >= wa.n_list) return;
	const int32_t tid = wa.list[blockIdx.x];
	const DTask t = wa.ga.tasks[tid];
	if (t.cls == T_LITE_W8) walk_call<64, true, true>(wa, t, tid, (char*)lds_raw, (int)threadIdx.x);   // (DUAL and WIDE4: the eight-wave class)
}

// dense copy of the CIGARs: every call's slot was sized for the worst case, only n_cigar words are real
__global__ __launch_bounds__(64) void k_cigar_gather(const DTask *tasks, const int32_t *list, const int64_t *dst_off, int32_t n_list,
                                                     const int32_t *n_cigar, const uint32_t *src, uint32_t *dst)
{
	MPA_SHORT_KERNEL();
	if ((int32_t)blockIdx.x >= n_list) return;
	const int32_t tid = list[blockIdx.x], n = n_cigar[tid];
	const uint32_t *from = src + tasks[tid].cig_off;
	uint32_t *to = dst + dst_off[blockIdx.x];
	for (int32_t k = threadIdx.x; k < n; k += 64) to[k] = from[k];
}

} // namespace mpa
