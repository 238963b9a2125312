// dp_huge_kernels.hip -- the X_HUGE extension calls (wider than 1024 columns, and whatever the int16 sweeps may not take), swept in
// int32 in 64-column blocks: k_ext_huge (one wave per call, the blocks one after the other), k_ext_huge_wg / ext_huge_wg_body (one
// wave per column block, MPA_DP_HUGE_WG=1; schedule and LDS layout in ext_huge_wg_core.h) and k_ext_replay (best row and x-drop
// replayed over the per-row keys either sweep leaves); and k_glob_mb_wg, the workgroup schedule under the row of a traceback call of class T_MB
// (MPA_DP_MB_WG=1).  Launched by dp_exec.hip on a side stream of the round; none of this code runs inside k_dp_round or k_dp_worker.
// Included by dp_exec.hip behind dp_kernels.hip.  Relies on dp_kernels.hip for: WavePos / whole_block, wave_sync, lds_barrier, GlobArgs,
// GlobState / glob_state_init / glob_cands, glob_narrow<64, true, true, WIDE> (k_ext_huge IS that body as a launch; ext_huge_wg_body
// repeats its row operation for operation), GLOB_NARROW_LDS, SEG_BIG, the int32 scans and imax.
#pragma once
#include "dp_kernels.hip"
#include "ext_huge_wg_core.h"

namespace mpa {

// Extension calls wider than 1024 columns: one wave per call, 64-column blocks swept one after the other (each all rows),
// boundary records through HBM, per-row keys combined across blocks with 64-bit atomic maxima.
// wg_min_blocks > 0 (MPA_DP_HUGE_WG): calls of that many column blocks or more are k_ext_huge_wg's, launched over the same list.
template<bool WIDE>
__global__ __launch_bounds__(64) void k_ext_huge(GlobArgs a, int32_t wg_min_blocks)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds_raw[];
	if (wg_min_blocks > 0) {
		const int32_t tid = a.waves[blockIdx.x].task[0];
		if (tid >= 0 && hwg::n_blocks(a.tasks[tid].ncol) >= wg_min_blocks) return;
	}
	glob_narrow<64, true, true, WIDE>(a, a.waves[blockIdx.x], whole_block((char*)lds_raw));
}

// The same sweep with one wave per column block (MPA_DP_HUGE_WG; schedule and LDS layout: ext_huge_wg_core.h).  W waves of one
// workgroup own W neighbouring blocks of a pass; wave w runs one chunk of R rows behind wave w - 1, takes the boundary records of
// that chunk from its neighbour's LDS ring and leaves its own in its ring, at the parity of the step; one workgroup barrier per
// step, the same number for every wave, and nothing that polls or spins.  Only the two ends of a pass go through the call's
// bnd[] rows in HBM, as every block of the one-wave kernel does.  Per row the arithmetic is glob_narrow<64, true, true, WIDE>'s,
// operation for operation: the per-row keys, and so k_ext_replay's results, are the same bits.
static_assert(hwg::WAVE_LDS == GLOB_NARROW_LDS, "ext_huge_wg_core.h: a wave's LDS area is the one-wave kernel's");
typedef int v4i __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i *lds_v4p;
// EXT = false (MPA_DP_MB_WG, k_glob_mb_wg below): the same schedule under the row of a traceback call of class T_MB, which is
// glob_narrow<64, true, false, WIDE>'s: no per-row key; one direction word per live cell at tb[i * ncol + column], where k_backtrack
// reads it, and H of the last row at column al - 1 as the call's score (tid: the call, for that store).
template<bool WIDE, bool EXT = true>
__device__ __forceinline__ void ext_huge_wg_body(const GlobArgs &a, const DTask &t, char *lds, const int lane, const int w, const int32_t tid = -1)
{
	constexpr int G = 64;
	int16_t *lds_prof = (int16_t*)(lds + hwg::wave_area(w));    // [22][64] for the wave's column block
	const int col = lane;
	const DpConst c = a.c;
	const int32_t nl = t.nl, ncol = t.ncol, slen = ncol >> 3;
	const int32_t nblk = hwg::n_blocks(ncol), npass = hwg::n_pass(nblk), nstep = hwg::n_step(nl);
	const int32_t go = c.go, ge = c.ge, goe = (int16_t)(c.go + c.ge), io = t.io, fs = c.fs;
	const uint32_t *rec = a.rec + t.rec_off;
	unsigned long long *rowkey = EXT ? a.rowkey64 + t.tb_off : nullptr;
	uint16_t *tb = EXT ? nullptr : a.tb + t.tb_off;
	int4 *bnd = a.bnd + t.bnd_off;
	const uint32_t go_s = splat16(go), io_s = splat16(io), fs_s = splat16(fs), ge_s = splat16(ge);
	const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;

	for (int32_t p = 0; p < npass; ++p) {
		// bnd[] rows of this pass's right end overwrite the ones its left end read: the stores of the pass before are drained, every
		// wave has passed, and the CU's L1 (which may still hold lines of the earlier reads) is dropped before the first read
		if (p > 0) {
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			lds_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
		}
		const int32_t blk = hwg::block_of(p, w);
		const bool have = blk < nblk;                               // (uniform over the wave; a wave without a block only passes the barriers)
		const int32_t gc = blk * G + col;                           // global column of this lane
		const bool live = have && gc < ncol;
		const int ledge = hwg::left_edge(blk, w), redge = have ? hwg::right_edge(blk, w, nblk) : (int)hwg::EDGE_NONE;
		const bool first_blk = blk == 0;
		uint32_t *ring = (uint32_t*)(lds_prof + 22 * G);
		const bool loader = col < 16;
		uint32_t pf = 0;
		if (have) {
			// stage this block's profile columns
			wave_sync();
			const int16_t *src = a.prof + t.prof_off;
			for (int k = lane; k < 22 * G; k += 64) {
				int aidx = k / G, cc = k - aidx * G, gcc = blk * G + cc;
				lds_prof[k] = gcc < t.pw ? src[aidx * t.pw + gcc] : (int16_t)NEG16;
			}
			wave_sync();
			// record ring (see k_ext): rows [0,16) now, rows [16,32) wait in pf, then 16 rows per refill
			if (loader) ring[col] = rec[col], pf = rec[16 + col];
			wave_sync();
		}
		const int32_t seg = slen > 0 ? gc / slen : 0;
		const bool seg_start = slen > 0 && gc % slen == 0;
		const int32_t cge = gc * ge, yoff = seg * SEG_BIG + cge;
		GlobState gs;
		glob_state_init(gs, have ? ring[0] : 0u, have ? ring[1] : 0u, first_blk && col == 0, fs);
		const char *profb = (const char*)(lds_prof + col);      // + byte0(record) * G = this lane's score for the row's amino acid
		uint32_t r[3];                                          // records of rows i, i+1 (and, once fetched, i+2) at slot row mod 3
		r[2] = have ? ring[2] : 0u, r[0] = have ? ring[3] : 0u, r[1] = 0;
		const bool carry_src = seg_start && gc >= slen;         // lanes that feed the carry scan
		int32_t hfin = NEG16;                                   // (!EXT) H of the last row

		// LDS addresses (explicit address space: ds_read_b128 / ds_write_b128, never a flat access that would have to pick its path
		// at run time) of the chunk's records in the left neighbour's ring, for the chunk's first row, and of this wave's own
		uint32_t rd = lds0, wr = lds0;
		int32_t i0 = 0;
		auto row = [&](auto kc, const int32_t i) {
			constexpr int K = decltype(kc)::value;
			if ((i & 15) == 12) { if (loader) ring[((i + 4) & 31) + col] = pf, pf = rec[i + 20 + col]; }   // rows [i+4, i+20) published, the next 16 requested
			r[(K + 2) % 3] = ring[(i + 2) & 31];                           // two rows ahead: LDS latency is off the critical path
			const uint32_t rcur = r[K];
			const char *sp = profb + (rcur & 0xff) * G;
			const uint32_t S = prof2(sp, sp);
			// boundary record of the block to the left
			int4 bin = make_int4(NEG32, NEG32, (int)NEGP, NEG16);
			if (ledge == hwg::EDGE_LDS) { const v4i b = *(lds_v4p)(uintptr_t)(rd + (uint32_t)(i - i0) * hwg::BND_BYTES); bin = make_int4(b.x, b.y, b.z, b.w); }
			else if (ledge == hwg::EDGE_HBM) bin = bnd[i];
			const int32_t Hb = lo16((uint32_t)bin.z), h1b = hi16((uint32_t)bin.z), I1b = bin.w;

			uint32_t dD, dA, dB, dC;
			const int32_t knon = glob_cands<K, WIDE>(gs, rcur, S, go_s, io_s, fs_s, dD, dA, dB, dC, ge_s);
			const int32_t nonI = knon >> 16;
			const int32_t py = scan_max_i32<G>(nonI + yoff);
			int32_t pex = shift1_i32<G>(py, NEG32, lane);
			pex = imax(pex, bin.x);
			const int32_t py_tot = imax(bin.x, __shfl(py, G - 1));
			const int32_t I1 = imax(pex - yoff - go, NEG16);
			const int32_t kbest = imax(knon, st_key((uint32_t)I1, 1));
			const int32_t h1 = kbest >> 16;
			const int32_t hl_raw = shift1_i32<G>(h1, first_blk ? NEG16 : h1b, lane);
			const int32_t il_raw = shift1_i32<G>(I1, first_blk ? NEG16 : I1b, lane);
			const int32_t dI = seg_start ? 0 : s_sub(hl_raw, go) - il_raw;
			const int32_t E = imax(s_sub(hl_raw, goe), s_sub(il_raw, ge));
			const int32_t z = carry_src ? E + cge : NEG32;
			int32_t pz = scan_max_i32<G>(z);
			pz = imax(pz, bin.y);
			const int32_t Gc = imax(pz - cge, NEG16);
			const int32_t h = imax(h1, Gc);
			if (!EXT) {
				// bits 9..4 of the direction word: Gc > h1 | C | B | A | D | il > hl - go; bits 3..0: the state
				if (live) {
					const uint32_t dw = push_neg(push_neg(push_neg(push_neg(push_neg((uint32_t)(h1 - Gc) >> 31, dC), dB), dA), dD), (uint32_t)dI);
					tb[(int64_t)i * ncol + gc] = (uint16_t)((dw << 4) | (uint32_t)(15 - (kbest & 15)));
				}
				hfin = h;
			} else {
				(void)dI;
				// key of this block's row: best (H + end bonus) among the live columns, ties to the smallest column
				const int32_t hb = h + (gc == t.al - 1 ? c.end_bonus : 0);
				const uint32_t kk = reduce_max_u32(live ? ((uint32_t)(imax(hb, NEG16) + 32768) << 6) | (63u - (uint32_t)lane) : 0u);
				if (lane == 63 && kk != 0)
					atomicMax(&rowkey[i], (unsigned long long)(kk >> 6) << 32 | (0xffffffffu - (uint32_t)(blk * 64 + 63 - (int32_t)(kk & 63))));
			}
			// boundary record for the block to the right
			if (col == G - 1) {
				const int4 out = make_int4(py_tot, pz, (int)pack16(h, h1), I1);
				if (redge == hwg::EDGE_LDS) *(lds_v4p)(uintptr_t)(wr + (uint32_t)(i - i0) * hwg::BND_BYTES) = v4i{ out.x, out.y, out.z, out.w };
				else if (redge == hwg::EDGE_HBM) bnd[i] = out;
			}
			const uint32_t hsp = spl(h);
			gs.H[K] = hsp;
			gs.Hs[K] = shift1<G>(hsp, first_blk ? NEGP : splat16(Hb), lane);
			if (K == 2) { if (i == 2 && first_blk && col == 0) gs.Hs[0] = NEGP, gs.Hs[1] = NEGP; }
		};
		for (int32_t s = 0; s < nstep; ++s) {
			const int32_t ch = have ? hwg::chunk_at(s, w, nl) : -1;
			if (ch >= 0) {
				i0 = hwg::chunk_first_row(ch);
				const int32_t i1 = hwg::chunk_end_row(ch, nl);
				if (ledge == hwg::EDGE_LDS) rd = lds0 + (uint32_t)hwg::ring_read(w, s, i0);
				wr = lds0 + (uint32_t)hwg::ring_write(w, s, i0);
				for (int32_t i = i0; i < i1; i += 3) {
					row(std::integral_constant<int, 2>(), i);
					if (i + 1 < i1) row(std::integral_constant<int, 0>(), i + 1);
					if (i + 2 < i1) row(std::integral_constant<int, 1>(), i + 2);
				}
			}
			lds_barrier();
		}
		if (!EXT && have && nl >= 3 && gc == t.al - 1) a.score[tid] = hfin;
	}
}
template<bool WIDE>
__global__ __launch_bounds__(hwg::W * 64) void k_ext_huge_wg(GlobArgs a)
{
	__shared__ __attribute__((aligned(16))) char lds[hwg::LDS_BYTES];
	const int32_t tid = a.waves[blockIdx.x].task[0];
	if (tid < 0) return;
	const DTask t = a.tasks[tid];
	if (!hwg::takes_wg(t.ncol)) return;                             // (uniform over the workgroup, before its first barrier)
	ext_huge_wg_body<WIDE>(a, t, lds, (int)(threadIdx.x & 63), __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)));
}

// MPA_DP_MB_WG: the traceback calls of class T_MB (more than 1024 columns, so 17 column blocks or more: hwg::takes_wg holds for every
// one) swept like that instead of by glob_narrow<64, true> on one wave: one workgroup per call of list[0, gridDim.x), the T_MB calls of
// a traceback chunk (the tail of the chunk's call list, which k_backtrack walks).  Launched by dp_exec.hip next to the round or, for
// later chunks, next to k_glob_narrow.
template<bool WIDE>
__global__ __launch_bounds__(hwg::W * 64) void k_glob_mb_wg(GlobArgs a, const int32_t *list)
{
	__shared__ __attribute__((aligned(16))) char lds[hwg::LDS_BYTES];
	const int32_t tid = list[blockIdx.x];
	const DTask t = a.tasks[tid];
	if (t.nl < 3) { if (threadIdx.x == 0) a.score[tid] = NEG16; return; }   // no row to sweep: no step, no barrier (uniform over the workgroup); as glob_narrow writes it
	ext_huge_wg_body<WIDE, false>(a, t, lds, (int)(threadIdx.x & 63), __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), tid);
}

// nasw-sse.c:423-443 replayed over per-row keys ((row max + 32768) << 32 | ~column): best row under the length penalty,
// x-drop stop.  One wave per call.
__global__ __launch_bounds__(64) void k_ext_replay(const DTask *tasks, const int32_t *list, int32_t n_list, const unsigned long long *rowkey64,
                                                   ExtOut *out, DpConst c, PenTable pen)
{
	MPA_SHORT_KERNEL();
	if ((int32_t)blockIdx.x >= n_list) return;
	const int32_t tid = list[blockIdx.x];
	const DTask t = tasks[tid];
	const int lane = threadIdx.x;
	const unsigned long long *key = rowkey64 + t.tb_off;
	const int64_t pen_len = 3 * (int64_t)t.al;
	int32_t G = INT32_MIN, best_i = -1, best_sc = INT32_MIN, best_col = -1;
	bool stopped = false;
	for (int32_t base = 2; base < t.nl && !stopped; base += 64) {
		const int32_t i = base + lane;
		const bool ok = i < t.nl;
		const unsigned long long kv = ok ? key[i] : 0ULL;
		int32_t pv = 0;
		{
			const int64_t x = (int64_t)i - pen_len;
			int k = 0;
			while (k + 1 < MPA_PEN_MAX && x >= (int64_t)pen.x[k + 1]) ++k;
			pv = pen.val[k];
		}
		const int32_t sc = (int32_t)(kv >> 32) - 32768;
		const int32_t v = ok ? sc - pv : INT32_MIN;
		int32_t m = v;
#pragma unroll
		for (int off = 1; off < 64; off <<= 1) { const int32_t o = __shfl_up(m, off); if (lane >= off) m = imax(m, o); }
		m = imax(m, G);
		const int32_t up = __shfl_up(m, 1);
		const bool imp = ok && v > (lane == 0 ? G : up);
		const bool brk = ok && (int64_t)m - (int64_t)v > c.xdrop;
		const uint64_t bm = __ballot(brk);
		const int first_brk = bm ? __ffsll((unsigned long long)bm) - 1 : 64;
		const uint64_t im = __ballot(imp) & (first_brk >= 63 ? ~0ULL : ((2ULL << first_brk) - 1));
		if (im) {
			const int last = 63 - __clzll((long long)im);
			best_i = base + last;
			G = __shfl(v, last);
			best_sc = __shfl(sc, last);
			best_col = (int32_t)(0xffffffffu - (uint32_t)__shfl((int)(uint32_t)kv, last));
		}
		if (bm) stopped = true;
	}
	if (lane == 0) {
		ExtOut o;
		o.nt_len = best_i + 1;
		o.aa_len = best_i < 0 ? 0 : best_col + 1;
		o.score = best_sc;
		o.flags = (best_i >= 0 && best_col >= t.al) ? 1 : 0;
		out[tid] = o;
	}
}

} // namespace mpa
