// dp_prep_kernels.hip -- the two kernels that write a DP round's inputs once to HBM: k_prep_rows (the 4-byte record per window row:
// codon amino acid, donor / acceptor penalties, the row's gap extension) and k_prep_prof (the 22 x pw query profile per call), with
// DevTables, the scoring tables both take by value.  Launched by dp_exec.hip behind the round's upload (phase 1), in front of
// k_dp_round; none of this code runs inside k_dp_round or k_dp_worker, which read the records and profiles it leaves.
// Included by dp_exec.hip behind dp_kernels.hip.  Relies on: dp_device.h (DTask, PrepChunk, DpConst, DevGenome, make_rec,
// MPA_PREP_CHUNK_ROWS, MPA_SHORT_KERNEL), dev_common.h (packed_window16) and NEG16 of dp_kernels.hip.
#pragma once
#include "dp_kernels.hip"

namespace mpa {

struct DevTables { uint8_t aa20[256]; uint8_t codon[64]; int8_t mat[484]; };

// ------------------------------------------------------------------------------------------------
// K3: per-row records and query profiles
// ------------------------------------------------------------------------------------------------
#define PROF_AA_STRIDE_REC 2   /* byte0 of a record = amino acid * 2 = byte offset into an int16 profile column (k_ext) */

// donor/acceptor/nas of window row i (the window fetch, ntseq.c:89-114 -- 4-bit unpack, reverse complement -- is folded into the
// addressing).  Forward: ns_prep_seq (nasw-sse.c:106-155); left extension:
// ns_prep_seq_left (nasw-sse.c:157-210).  int8 wrap-around of the reference's arrays is preserved.
// Four rows per thread (rows i, i + 256, i + 512, i + 768 of a 1 024-row chunk): the kernel is bound by the chain of dependent loads
// chunk -> task -> contig -> genome words and by how many waves the chip holds at once, not by bandwidth or arithmetic (round 4:
// 1.8 ms alone for 200 M rows = 0.5 TB/s, and 2-6 x that next to the other kernels of the stream, on every round's critical
// path) -- a thread that fetches the words of four rows together pays the chain once for four records.
#define MPA_PREP_ROWS (MPA_PREP_CHUNK_ROWS / 256)
__global__ __launch_bounds__(256) void k_prep_rows(DevGenome g, const DTask *tasks, const PrepChunk *chunks, uint32_t *rec, DpConst c, DevTables tb)
{
	MPA_SHORT_KERNEL();
	const PrepChunk ch = chunks[blockIdx.x];
	const DTask t = tasks[ch.task];
	const int32_t nl = t.nl;
	const int cid = t.vid >> 1, rev = t.vid & 1, left = (t.flag & 2) != 0;
	const int64_t off = g.ctg_off[cid], len = g.ctg_len[cid];
	// w[j] = b[i-6+j], j=0..15, where b[] is the (possibly reversed) window; 15 = outside the window.
	// The sixteen bases are consecutive in the packed genome (ascending, or descending for a reversed window / the minus strand):
	// three aligned words cover them, and the sixteen nibbles are shifted out of those -- instead of sixteen dependent byte loads
	// with 64-bit address arithmetic each.  The genome buffer is padded by 16 bytes; what lies outside the
	// window is masked to 15 whatever was read for it.
	uint64_t nibs[MPA_PREP_ROWS];
	const int64_t x0 = t.nt_off + (left ? nl - 1 : 0);             // strand position of window position 0
	const int64_t p0 = rev ? off + len - 1 - x0 : off + x0;        // ... its position in the packed genome
	const int dir = (left != (rev != 0)) ? -1 : 1;
#pragma unroll
	for (int r = 0; r < MPA_PREP_ROWS; ++r) {
		const int32_t i = ch.row0 + (int32_t)threadIdx.x + 256 * r;
		nibs[r] = i < nl ? packed_window16(g.seq, g.l_seq, p0 + (int64_t)dir * (i - 6), dir, rev) : 0;
	}
#pragma unroll
	for (int r = 0; r < MPA_PREP_ROWS; ++r) {
	const int32_t i = ch.row0 + (int32_t)threadIdx.x + 256 * r;
	if (i >= nl) continue;
	uint64_t nib = nibs[r];
	{
		const int32_t jlo = 6 - i > 0 ? (6 - i > 16 ? 16 : 6 - i) : 0;                        // w[j], j < jlo: before the window
		const int32_t jhi = nl - i + 6 < 16 ? (nl - i + 6 < 0 ? 0 : nl - i + 6) : 16;       // w[j], j >= jhi: behind it
		uint64_t valid = jhi >= 16 ? ~0ULL : ((1ULL << (4 * jhi)) - 1);
		valid &= jlo >= 16 ? 0ULL : ~((1ULL << (4 * jlo)) - 1);
		nib = (nib & valid) | ~valid;
	}
	uint32_t w[16];
#pragma unroll
	for (int j = 0; j < 16; ++j) w[j] = (uint32_t)(nib >> (4 * j)) & 15u;
#define B_(d) w[6 + (d)]   /* b[i+d] */
	uint32_t nas = 21;
	int32_t don, acc;
	const int32_t sp3 = (int8_t)c.sp[3];
	if (!left) {
		if (i >= 2 && B_(0) < 4 && B_(-1) < 4 && B_(-2) < 4) nas = tb.codon[B_(-2) << 4 | B_(-1) << 2 | B_(0)];
		{ // donor[k], k = i+1
			const int32_t k = i + 1;
			don = sp3;
			if (k < nl - 3) {
				int tt = 3;
				if (B_(2) == 2 && B_(3) == 3) tt = (B_(4) == 0 || B_(4) == 2) ? (B_(1) == 2 ? -1 : 4) : 0;
				else if (B_(2) == 2 && B_(3) == 1 && B_(1) == 2) tt = 1;
				else if (B_(2) == 0 && B_(3) == 3) tt = 2;
				don = tt < 0 ? 0 : (int8_t)c.sp[tt];
			}
		}
		{ // acceptor[i]
			acc = sp3;
			if (i >= 1) {
				int tt = 3, pen_y = 0;
				if (B_(-1) == 0 && B_(0) == 2) {
					tt = (i >= 2 && (B_(-2) == 1 || B_(-2) == 3)) ? -1 : 0;
#pragma unroll
					for (int d = 4; d <= 6; ++d)
						if (i - d >= 0 && B_(-d) != 1 && B_(-d) != 3) pen_y += c.sp[5];
				} else if (B_(-1) == 0 && B_(0) == 1) tt = 2;
				acc = tt < 0 ? 0 : (int8_t)c.sp[tt];
				if (tt == -1 || tt == 0) acc = (int8_t)(acc + pen_y);
			}
		}
	} else {
		if (i >= 2 && B_(0) < 4 && B_(-1) < 4 && B_(-2) < 4) nas = tb.codon[B_(0) << 4 | B_(-1) << 2 | B_(-2)];
		{ // "donor"[k] of the reversed string, k = i+1 (really the acceptor signal read backwards)
			const int32_t k = i + 1;
			don = sp3;
			if (k < nl - 3) {
				int tt = 3, pen_y = 0;
				if (B_(2) == 2 && B_(3) == 0) {
					tt = (B_(4) == 1 || B_(4) == 3) ? -1 : 0;
#pragma unroll
					for (int d = 6; d <= 8; ++d)       // j = k+5 .. k+7  ->  b[i+6 .. i+8]
						if (i + d < nl && B_(d) != 1 && B_(d) != 3) pen_y += c.sp[5];
				} else if (B_(2) == 1 && B_(3) == 0) tt = 2;
				don = tt < 0 ? 0 : (int8_t)c.sp[tt];
				if (tt == -1 || tt == 0) don = (int8_t)(don + pen_y);
			}
		}
		{ // "acceptor"[i] of the reversed string (really the donor signal read backwards)
			acc = sp3;
			if (i >= 1) {
				int tt = 3;
				if (B_(-1) == 3 && B_(0) == 2)
					tt = (i >= 2 && (B_(-2) == 0 || B_(-2) == 2)) ? ((i + 1 < nl && B_(1) == 2) ? -1 : 4) : 0;
				else if (B_(-1) == 1 && B_(0) == 2 && i + 1 < nl && B_(1) == 1) tt = 1;
				else if (B_(-1) == 3 && B_(0) == 0) tt = 2;
				acc = tt < 0 ? 0 : (int8_t)c.sp[tt];
			}
		}
	}
#undef B_
	if (g.spsc) {
		// --spsc: the score track adjusts the penalties (nasw-sse.c:138-152, left: 189-203).  ss[p] belongs to window position p
		// (forward); forward calls shift it onto donor/acceptor[p-1], the reversed left extension onto [nl-1-p] with the two
		// roles swapped.  int8 wrap-around as in the reference's arrays.
		const uint8_t *track = g.spsc + (rev ? g.l_seq : 0) + off;
		const int32_t max_spsc = (t.io + 1) / 2 - 1;
		auto ss_at = [&](int32_t p) -> int32_t {             // -1: outside what the reference reads
			if (p < (left ? 0 : 1) || p >= nl) return -1;
			if (p == 0 && (t.flag & 8)) return 0xff;           // MPA_F_SS_SKIP0
			return track[t.nt_off + p];
		};
		auto adjust = [&](int32_t v, int32_t ss, bool for_acceptor_entry) -> int32_t {
			if (ss < 0) return v;
			if (ss == 0xff) return (int8_t)(v - c.sp_null_bonus);
			if (((ss & 1) != 0) != for_acceptor_entry) return v;
			int32_t spsc = (int8_t)(ss >> 1) - 64;
			if (spsc > max_spsc) spsc = max_spsc;
			return (int8_t)(v - spsc);
		};
		if (!left) {
			don = adjust(don, ss_at(i + 2), false);          // donor[i+1] <- ss[i+2] (donor entries)
			acc = adjust(acc, ss_at(i + 1), true);           // acceptor[i] <- ss[i+1] (acceptor entries)
		} else {
			don = adjust(don, ss_at(nl - 2 - i), true);      // "donor"[i+1] of the reversed string <- acceptor entries at nl-1-(i+1)
			acc = adjust(acc, ss_at(nl - 1 - i), false);     // "acceptor"[i] <- donor entries at nl-1-i
		}
	}
	// (byte 2: the row's gap extension -- fs on a stop codon, nasw-sse.c:263,370 -- or, when the penalties do not fit a byte, just the stop flag)
	rec[t.rec_off + i] = make_rec(nas * PROF_AA_STRIDE_REC, don, c.wide_ge ? (uint32_t)(nas == 20) : nas == 20 ? (uint32_t)c.fs : (uint32_t)c.ge, acc);
	}
}

// query profile prof[a][col] = mat[a][aa(col)] (ns_gen_prof nasw-sse.c:212-224); columns >= al score -32768
__global__ __launch_bounds__(256) void k_prep_prof(const DTask *tasks, const char *qseq, int16_t *prof, DevTables tb)
{
	MPA_SHORT_KERNEL();
	const DTask t = tasks[blockIdx.x];
	const int left = (t.flag & 2) != 0;
	for (int idx = threadIdx.x; idx < 22 * t.pw; idx += blockDim.x) {
		int a = idx / t.pw, col = idx - a * t.pw;
		int16_t v = NEG16;
		if (col < t.al) {
			uint8_t ch = (uint8_t)qseq[t.q_off + (left ? t.al - 1 - col : col)];
			v = tb.mat[a * 22 + tb.aa20[ch]];
		}
		prof[t.prof_off + idx] = v;
	}
}

} // namespace mpa
