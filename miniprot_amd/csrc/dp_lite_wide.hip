// dp_lite_wide.hip -- k_lite_wide, k_lite_w8 and their body lite_wide_body<NW>: the packed int16 sweep of the checkpointed traceback for
// calls of 129..256 columns (class 12, dp_device.h; four waves) and of 257..512 columns (class 13; eight waves).  Launches of their own
// on side streams of the round (dp_exec.hip, next to k_dp_round, like the 512/1024-thread traceback classes); none of this code runs
// inside k_dp_round or k_dp_worker.
// Included by dp_exec.hip behind dp_kernels.hip.  Relies on dp_kernels.hip for: WavePos / whole_block, lds_barrier, the packed int16
// helpers, ExtArgs, the profile and record-ring layout (PROF_*, EXT_WIDE_RING, ring_entry, prof2s, lds_s16p, v2u / lds_u2p) and the
// row macros MPA_ROW_HEAD_L, MPA_ROW_TAIL_WL and MPA_NIBBLE -- the rows are defined there, next to the ones they are variants of.
#pragma once
#include "dp_kernels.hip"

namespace mpa {

// ------------------------------------------------------------------------------------------------
// The packed sweep of the checkpointed traceback for calls of 129..256 columns (class 12, dp_device.h): one workgroup of four
// waves per PAIR of calls (the two int16 halves), one column per lane, wave w three rows behind wave w - 1 and the hand-over of
// {scan carry, H of the wave's last column} through lane 0 and the LDS exchange slots, one barrier per step of three rows --
// ext_wide_body<4, false> without the per-row keys and the x-drop replay (a global alignment sweeps every row), with the rows
// of ext_narrow<G, true>: the four differences whose signs are the extension bits, the three-row nibble word and the checkpoints.
// The two calls may differ in rows: the group iterates max_nl, a call past its end only produces bits and checkpoints nobody
// reads; its score H(nl - 1, al - 1) is taken from the wave and lane that own column al - 1 behind the step that holds row nl - 1.
// NW waves (4: class 12, k_lite_wide; 8: class 13, 257..512 columns, k_lite_w8): what depends on the count is the profile area, the
// exchange slots (3 NW per step parity, in a stride of 16 or 32), where the bits and checkpoints lie (lite_group_*, dp_device.h) and
// how far the last wave runs behind the first -- 3 (NW - 1) rows, which the record ring must still hold (below).
// Barriers: a wave passes w of them before its first step, one per step, and NW - 1 - w behind its last; the steps are counted by the
// one loop nest below from max_nl alone (the group's longer call: a scalar every wave reads from the same descriptor), never from the
// wave index, a call's own rows or an empty half -- so every wave of a group passes NW - 1 + steps(max_nl) barriers, whatever max_nl.
// ------------------------------------------------------------------------------------------------
#define LITE_GROUP_XSLOTS(NW) ((NW) <= 4 ? 16 : 32)        /* exchange slots per step parity: 3 NW of them are used */
#define LITE_GROUP_LDS(NW) ((size_t)(NW) * 2 * 64 * PROF_COL_STRIDE + (EXT_WIDE_RING + 1) * 16 + 2 * LITE_GROUP_XSLOTS(NW) * 8 + 32 + (64 * 8 + 32))   /* bytes per group; a multiple of 16 */
#define LITE_WIDE_LDS LITE_GROUP_LDS(MPA_LITE_WIDE_WAVES)
template<int NW>
__device__ __forceinline__ void lite_wide_body(const ExtArgs &a, const int group_idx, const WavePos wp)
{
	constexpr int RING = EXT_WIDE_RING, XS = LITE_GROUP_XSLOTS(NW);
	static_assert(3 * NW <= XS, "a step's exchange slots: three per wave");
	// the leading wave's refill at row i overwrites the ring slots of rows i - 34 .. i - 23; the last wave is then at row i - 3 (NW - 1) and reads rows from there on
	static_assert(RING == 48 && 3 * (NW - 1) < 23, "the record ring must still hold the last wave's rows");
	// per wave: profile of its 64 columns for both halves [2][64 columns][23] int16; then the record ring, the exchange slots
	// [2 step parities][NW waves][3 rows] of {scan, H of the wave's last column}, 32 bytes of -inf and the dump area
	char *lds_prof = wp.lds;
	uint4 *ring = (uint4*)(lds_prof + NW * 2 * 64 * PROF_COL_STRIDE);  // [RING + 1] decoded records of both halves
	uint2 *xch = (uint2*)(ring + RING + 1);                          // [2][XS] slots: parity * XS + 3 w + k
	uint2 *xneg = xch + 2 * XS;                                      // [4] {-inf, -inf}
	uint2 *xdump = xneg + 4;                                         // [64 + 4]
	const int lane = wp.lane, w = wp.w;                              // w: wave index inside the group, scalar
	const ExtWave *wvp = &a.waves[group_idx];
	const DpConst c = a.c;
	const uint32_t *recbase = a.rec + wvp->rec_base;

	int32_t tid[2], end_row[2], al[2];
	uint32_t roff[2];
#pragma unroll
	for (int h = 0; h < 2; ++h) {
		tid[h] = __builtin_amdgcn_readfirstlane(wvp->task[h]);
		if (tid[h] >= 0) {
			const DTask *t = &a.tasks[tid[h]];
			end_row[h] = __builtin_amdgcn_readfirstlane(t->nl) - 1, al[h] = t->al, roff[h] = (uint32_t)(t->rec_off - wvp->rec_base);
		} else end_row[h] = -1, al[h] = 1, roff[h] = 0;
	}
	// profile columns of this wave: global [22][pw] int16 -> LDS [column][amino acid]
	// (Same text in ext_wide_body, dp_kernels.hip, as is the ring prefill below; a shared inline function changes the code of
	// k_dp_round, k_dp_worker and k_lite_wide -- tried: DESIGN.md section 5, file layout of the DP kernels.)
	for (int h = 0; h < 2; ++h) {
		char *dst = lds_prof + (size_t)(w * 2 + h) * 64 * PROF_COL_STRIDE;
		if (tid[h] < 0) {   // (an empty half scores zero everywhere; nobody reads what it produces)
			for (int k = lane; k < 64 * PROF_COL_STRIDE / 2; k += 64) ((uint16_t*)dst)[k] = 0;
			continue;
		}
		const DTask *t = &a.tasks[tid[h]];
		const int16_t *src = a.prof + t->prof_off;
		for (int k = lane; k < 22 * 64; k += 64) {
			const int aidx = k >> 6, cc = k & 63, gcc = w * 64 + cc;
			*(int16_t*)(dst + cc * PROF_COL_STRIDE + aidx * PROF_AA_STRIDE) = gcc < t->pw ? src[aidx * t->pw + gcc] : (int16_t)NEG16;
		}
	}
	if (wp.tg < 2 * XS + 4) xch[wp.tg] = make_uint2(NEGP, NEGP);   // the exchange slots and, behind them, the slots of -inf
	// record ring, filled by the leading wave (ext_wide_body's scheme): row r in slot (r + 44) % 48
	const bool loader = w == 0 && lane < 12;
	uint2 pf = make_uint2(0, 0);
	if (w == 0 && lane < 16) {
		const uint4 e = ring_entry(recbase[roff[0] + lane], recbase[roff[1] + lane]);
		ring[lane < 4 ? lane + 44 : lane - 4] = e;
		if (lane == 4) ring[RING] = e;
	}
	if (loader) pf = make_uint2(recbase[roff[0] + 16 + lane], recbase[roff[1] + 16 + lane]);
	__syncthreads();

	const int gc = w * 64 + lane;
	const uint32_t jge = splat16(gc * c.ge), gojge = splat16(c.go + gc * c.ge);
	const uint32_t goP = __builtin_amdgcn_readfirstlane(splat16(c.go)), fsP = __builtin_amdgcn_readfirstlane(splat16(c.fs));
	const uint32_t ioP = pack16(tid[0] >= 0 ? a.tasks[tid[0]].io : 0, tid[1] >= 0 ? a.tasks[tid[1]].io : 0);
	const uint32_t sel_lo = __builtin_amdgcn_readfirstlane(0x05040100u);
	const uint32_t nb1 = __builtin_amdgcn_readfirstlane(0x00010001u), nb2 = __builtin_amdgcn_readfirstlane(0x00020002u),
	               nb4 = __builtin_amdgcn_readfirstlane(0x00040004u), nb8 = __builtin_amdgcn_readfirstlane(0x00080008u);
	// absolute LDS addresses: this lane's two profile columns; the exchange slot it reads / writes in a step of parity 0
	const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)wp.lds;
	const uint32_t pb0 = lds0 + (uint32_t)(((w * 2 + 0) * 64 + lane) * PROF_COL_STRIDE), pb1 = pb0 + 64 * PROF_COL_STRIDE;
	const uint32_t xch0 = lds0 + (uint32_t)((char*)xch - wp.lds), xneg0 = lds0 + (uint32_t)((char*)xneg - wp.lds), xdump0 = lds0 + (uint32_t)((char*)xdump - wp.lds);
	const uint32_t xwr_even = lane == 63 ? xch0 + (uint32_t)(3 * w) * 8 : xdump0 + (uint32_t)lane * 8;
	const uint32_t xwr_flip = lane == 63 ? (uint32_t)(XS * 8) : 0u; // (the other parity's slots: + XS slots)
	const bool takes_left = lane == 0 && w > 0;

	uint32_t Hr[3], Hs[3], Dr[3], dn[3], ac[3], M[3], A = NEGP, B = NEGP, C = NEGP;
#pragma unroll
	for (int k = 0; k < 3; ++k) Hr[k] = Hs[k] = Dr[k] = M[k] = NEGP;
	uint32_t k0 = NEGP, k1 = NEGP, k2 = NEGP, k3 = NEGP, ke = NEGP;    // fill registers of the asm rows' scan: only ever written by DPP moves
	if (gc == 0) Hs[2] = 0u, Hs[1] = splat16(-c.fs), Hs[0] = splat16(-c.fs);
	{
		const uint4 q0 = ring[44], q1 = ring[45];
		dn[1] = q0.x, dn[0] = q1.x, ac[1] = q0.y, ac[0] = q1.y, dn[2] = ac[2] = 0;
	}
	const int32_t max_nl = __builtin_amdgcn_readfirstlane(wvp->max_nl);
	uint4 rcur = ring[46], rnext = ring[47];                           // records of rows i and i + 1
	uint32_t S = prof2s(pb0 + (rcur.w & 0xffff), pb1 + (rcur.w >> 16));   // profile scores of row i (generic rows)
	bool have_hD = false;                                              // hD already holds row i's max(diagonal, D) (behind the asm rows)
	uint32_t hD = NEGP;
	// the three-row accumulator of nibbles, the difference that holds row i's D bit, the D state the precomputation for row i replaced
	// (what a checkpoint wants), this wave's slice of the group's bit words and checkpoints (dp_device.h)
	uint32_t acc = 0, dDc = 0, Dold = NEGP;
	int32_t sh_;
	uint32_t *lite_p = a.lite + wvp->lite_off + lite_group_bit_at(NW, 2, gc, 0, &sh_);
	const int64_t lite_step = lite_group_bit_at(NW, 5, gc, 0, &sh_) - lite_group_bit_at(NW, 2, gc, 0, &sh_);
	auto checkpoint = [&](const int32_t i, const uint32_t d3) {        // top of row i = 2 + k * MPA_TB_BLOCK: slots 0, 1, 2 hold rows i-1, i-2, i-3
		uint32_t *p = a.ckpt + wvp->ck_off + lite_group_ckpt_at(NW, (i - 2) / MPA_TB_BLOCK, gc, 0, &sh_);
		p[0] = Hr[0], p[64] = Hr[1], p[128] = Hr[2], p[192] = Dr[0], p[256] = Dr[1], p[320] = d3, p[384] = A, p[448] = B, p[512] = C;
	};
	// the score of a call whose last row is among the rows [i, i + 3) just swept: h0, h1, h2 = their H rows (slots 2, 1, 0; passed by
	// value: a choice among the elements of Hr[] by a run-time index would move the array out of the registers)
	auto scores = [&](const int32_t i, const uint32_t h0, const uint32_t h1, const uint32_t h2) {
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			const int32_t k = end_row[h] - i;
			uint32_t v = h2;
			v = k == 1 ? h1 : v, v = k == 0 ? h0 : v;
			if (tid[h] >= 0 && (uint32_t)k < 3u && gc == al[h] - 1) a.score[tid[h]] = half16(v, h);
		}
	};
	auto refill = [&](const int32_t i, const int rs) {                 // the leading wave, every twelfth row
		if (loader) {
			const uint4 e = ring_entry(pf.x, pf.y);
			const int at = (rs + 12) % RING + lane;
			ring[at] = e;
			if (at == 0) ring[RING] = e;                                       // slot 0 again behind slot 47
			pf = make_uint2(recbase[roff[0] + (uint32_t)i + 26 + lane], recbase[roff[1] + (uint32_t)i + 26 + lane]);
		}
	};
	v2u cv[3];
	uint32_t xwr = 0;
	auto step_begin = [&](const int par) {                             // what the wave to the left produced for the step's three rows, in the previous step
		uint32_t at = xneg0;
		if (takes_left) at = xch0 + (uint32_t)(((par ^ 1) * XS + 3 * (w - 1)) * 8);
#pragma unroll
		for (int k = 0; k < 3; ++k) cv[k] = *(lds_u2p)(uintptr_t)(at + 8 * k);
		xwr = xwr_even + (par ? xwr_flip : 0u);
	};
	// the generic row (plain C++): the first twelve rows and what the blocks of asm rows leave over
	auto row = [&](auto kc, const int32_t i, const int rs) {
		constexpr int K = decltype(kc)::value;
		constexpr int R1 = (3 - K) % 3, R2 = (4 - K) % 3, R3 = (5 - K) % 3;
		if (K == 0 && i > 2 && (uint32_t)(i - 2) % MPA_TB_BLOCK == 0) checkpoint(i, have_hD ? Dold : Dr[R3]);
		const uint32_t Snext = prof2s(pb0 + (rnext.w & 0xffff), pb1 + (rnext.w >> 16));
		const uint4 rnn = ring[rs + K];                                    // record of row i + 2
		dn[R3] = rcur.x, ac[R3] = rcur.y;                                  // donor[i+1], acceptor[i]
		uint32_t h, t, u, dA, dB, dC;
		if (have_hD) h = hD;
		else {
			h = p_adds(Hs[R3], S);
			u = p_subs(Hr[R3], goP); dDc = p_subs(u, Dr[R3]); t = p_max(u, Dr[R3]);
			t = p_subs(t, rcur.z); Dr[R3] = t; h = p_max(h, t);
		}
		u = p_subs(Hr[R1], ioP); t = p_subs(u, dn[R2]); dA = p_subs(t, A);
		t = p_max(t, A); A = t; h = p_max(h, p_subs(t, ac[R3]));
		u = p_subs(Hs[R1], ioP); t = p_subs(u, dn[R1]); dB = p_subs(t, B);
		t = p_max(t, B); B = t; h = p_max(h, p_subs(t, ac[R2]));
		t = p_subs(u, dn[R3]); dC = p_subs(t, C);
		t = p_max(t, C); C = t; h = p_max(h, p_subs(t, ac[R1]));
		{
			const uint32_t nib = (dDc >> 15 & 0x00010001u) | (dA >> 14 & 0x00020002u) | (dB >> 13 & 0x00040004u) | (dC >> 12 & 0x00080008u);
			acc = K == 0 ? nib : (acc << 4 | nib);
			if (K == 2) *lite_p = acc, lite_p += lite_step;
		}
		t = p_max(p_max(Hr[R1], Hr[R2]), p_max(Hs[R1], Hs[R2]));
		h = p_max(h, p_subs(t, fsP));
		const uint32_t y = scan_max_pk<64>(p_max(p_adds(h, jge), cv[K].x));   // (the incoming carry through lane 0)
		const uint32_t ex = shift1<64>(y, cv[K].x, lane);
		h = p_max(h, p_subs(ex, gojge));
		Hr[R3] = h, Hs[R3] = shift1<64>(h, cv[K].y, lane);
		*(lds_u2p)(uintptr_t)(xwr + 8 * K) = v2u{ y, h };
		if (i == 2 && gc == 0) Hs[R1] = NEGP, Hs[R2] = NEGP;
		S = Snext;
		rcur = rnext, rnext = rnn, have_hD = false;
	};

	// Wave w runs 3 w rows behind wave 0: one barrier per step of three rows, w barriers of delay first and NW-1-w at the end so
	// that every wave passes the same number.  Step parity = (step + w) & 1.
	for (int k = 0; k < w; ++k) lds_barrier();
	{
		int par = w & 1;
		int32_t i = 2;
		int rs = 0, rs12 = 0;                                              // (i - 2) % 48, % 12 at the top of a step
		auto generic_step = [&](const int n_rows) {
			if (w == 0 && rs12 == 0) refill(i, rs);
			step_begin(par);
			row(std::integral_constant<int, 0>(), i, rs);
			if (n_rows > 1) row(std::integral_constant<int, 1>(), i + 1, rs);
			if (n_rows > 2) row(std::integral_constant<int, 2>(), i + 2, rs);
			if (n_rows < 3) *lite_p = acc << (4 * (3 - n_rows));               // (the sweep ends inside a word)
			if ((uint32_t)(end_row[0] - i) < 3u || (uint32_t)(end_row[1] - i) < 3u) scores(i, Hr[2], Hr[1], Hr[0]);
			lds_barrier();
			i += 3, par ^= 1, rs = rs == RING - 3 ? 0 : rs + 3, rs12 = rs12 == 9 ? 0 : rs12 + 3;
		};
		while (i < 14 && i + 3 <= max_nl) generic_step(3);
		// ---- the asm rows, in blocks of four steps (i = 2 + 12 k: the record ring is refilled and checkpoints are written at block starts only)
		if (i + 12 <= max_nl) {
			uint32_t tA_, tB_, tC_, h, x, hDn, a0, a1, dA, dB, dC, drn, dDn;
			v2s sraw0, sraw1;                                              // (.x = a profile score; .y is never set: v_perm_b32 takes the low halves)
			M[0] = p_max(Hr[0], Hs[0]), M[1] = p_max(Hr[1], Hs[1]);
			{                                                              // row i's diagonal term and D state (slot R3 = 2)
				const uint32_t u = p_subs(Hr[2], goP), t = p_max(u, Dr[2]);
				dDc = p_subs(u, Dr[2]), Dold = Dr[2];
				Dr[2] = p_subs(t, rcur.z);
				hD = p_max(p_adds(Hs[2], S), Dr[2]);
			}
			sraw0.x = *(lds_s16p)(uintptr_t)(pb0 + (rnext.w & 0xffff)), sraw1.x = *(lds_s16p)(uintptr_t)(pb1 + (rnext.w >> 16));
			uint4 rnn = ring[rs];                                          // record of row i + 2; from here on fetched a row before it is needed
			do {
				if (w == 0) refill(i, rs);
				if ((uint32_t)(i - 2) % MPA_TB_BLOCK == 0) checkpoint(i, Dold);
				const uint4 *rb = ring + rs;
#pragma unroll 1
				for (int st = 0; st < 4; ++st, rb += 3) {
					step_begin(par);
#define MPA_LW_ROW(K, R1, R2, R3, NIB) { \
					MPA_ROW_HEAD_L(Hr[R1], Hs[R1], dn[R1], dn[R2], rcur.x, ac[R1], ac[R2], rcur.y, M[R1], M[R2]); \
					dn[R3] = rcur.x, ac[R3] = rcur.y; \
					MPA_ROW_TAIL_WL(Hr[R2], Hs[R2], Dr[R2], Hs[R3], M[R3], cv[K].x, cv[K].y); \
					MPA_NIBBLE(NIB); \
					Dold = Dr[R2], Dr[R2] = drn, dDc = dDn; \
					if (K == 2) *lite_p = acc, lite_p += lite_step; \
					{ v2s f0, f1; f0.x = *(lds_s16p)(uintptr_t)a0, f1.x = *(lds_s16p)(uintptr_t)a1; sraw0 = f0, sraw1 = f1; } \
					rcur = rnext, rnext = rnn, rnn = rb[K + 1]; \
					Hr[R3] = h, hD = hDn; \
					*(lds_u2p)(uintptr_t)(xwr + 8 * K) = v2u{ x, h }; }
					MPA_LW_ROW(0, 0, 1, 2, MPA_NIB_FIRST)
					MPA_LW_ROW(1, 2, 0, 1, MPA_NIB_NEXT)
					MPA_LW_ROW(2, 1, 2, 0, MPA_NIB_NEXT)
#undef MPA_LW_ROW
					if ((uint32_t)(end_row[0] - i) < 3u || (uint32_t)(end_row[1] - i) < 3u) scores(i, Hr[2], Hr[1], Hr[0]);
					lds_barrier();
					i += 3, par ^= 1;
				}
				rs = rs == RING - 12 ? 0 : rs + 12;
			} while (i + 12 <= max_nl);
			have_hD = true;
		}
		while (i + 3 <= max_nl) generic_step(3);
		if (i < max_nl) generic_step(max_nl - i);
	}
	for (int k = w; k < NW - 1; ++k) lds_barrier();
}
// (a launch of its own on a side stream of the round, like the 512/1024-thread traceback classes: k_dp_round stays what it is)
__global__ __launch_bounds__(MPA_LITE_WIDE_WAVES * 64) void k_lite_wide(ExtArgs a, int first_group)
{
	__shared__ __attribute__((aligned(16))) char lds[LITE_WIDE_LDS];
	lite_wide_body<MPA_LITE_WIDE_WAVES>(a, first_group + (int)blockIdx.x, whole_block(lds));
}
// (257..512 columns, class 13: the same body on eight waves, on a side stream of its own; about 51 KB of LDS)
__global__ __launch_bounds__(MPA_LITE_W8_WAVES * 64) void k_lite_w8(ExtArgs a, int first_group)
{
	__shared__ __attribute__((aligned(16))) char lds[LITE_GROUP_LDS(MPA_LITE_W8_WAVES)];
	lite_wide_body<MPA_LITE_W8_WAVES>(a, first_group + (int)blockIdx.x, whole_block(lds));
}

} // namespace mpa
