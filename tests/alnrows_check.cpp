// alnrows_check.cpp -- a stand-alone check of miniprot_amd/csrc/aln_rows_core.h (tests/test_aln_rows_cpu.py compiles it with
// -fsanitize=address,undefined and runs it).  Hand-written CIGARs over a small two-contig genome go through the shared core twice --
// with a team of one (StatsSerial, what MPA_GPU_ROWS=model runs) and with a team of 64 host threads that meet at a barrier for every
// sum and broadcast (the device's wavefront in slow motion) -- under each of the three flag combinations, and the slots are compared
// with a plain sequential walk over the unpacked strand, restated here from put_residues() of host_format.cpp (format.c:189-331).
// The two slots of a case sit back to back, sized by aln_rows_slot(), with guard bytes in front, between and behind: after every
// case every byte of the buffer that the plain walk does not account for is as it was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <functional>
#include <string>
#include <thread>
#include <vector>
#include <pthread.h>
#include "aln_rows_core.h"

using namespace mpa;

// ---- a team of 64 threads ---------------------------------------------------------------------------
static pthread_barrier_t g_bar;
static uint64_t g_slot[64];
static thread_local int tl_lane = 0;
struct RowThreads {
	static int lane() { return tl_lane; }
	static int width() { return 64; }
	static uint32_t bcast(uint32_t v, int k)
	{
		g_slot[tl_lane] = v;
		pthread_barrier_wait(&g_bar);
		const uint32_t r = (uint32_t)g_slot[k];
		pthread_barrier_wait(&g_bar);
		return r;
	}
	static int32_t sum(int32_t v)
	{
		g_slot[tl_lane] = (uint32_t)v;
		pthread_barrier_wait(&g_bar);
		int32_t all = 0;
		for (int i = 0; i < 64; ++i) all += (int32_t)g_slot[i];
		pthread_barrier_wait(&g_bar);
		return all;
	}
};

// ---- tables and genome ------------------------------------------------------------------------------
static const char *kAA20 = "ARNDCQEGHILKMFPSTWYV*X";
static const char *kCode = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF";   // codon = b0 << 4 | b1 << 2 | b2 over A0 C1 G2 T3
static const int kAsize = 22;
static uint8_t g_tab[ALN_TAB_BYTES];

static uint64_t g_rng = 88172645463325252ULL;
static uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 20) % n); }

static void make_tables()
{
	memset(g_tab, 0, sizeof(g_tab));
	for (int c = 0; c < 256; ++c) g_tab[ALN_TAB_AA20 + c] = 21;
	for (int i = 0; i < 22; ++i) g_tab[ALN_TAB_AA20 + (uint8_t)kAA20[i]] = (uint8_t)i, g_tab[ALN_TAB_AA20 + (uint8_t)(kAA20[i] | 0x20)] = (uint8_t)i;
	for (int c = 0; c < 64; ++c) g_tab[ALN_TAB_CODON + c] = g_tab[ALN_TAB_AA20 + (uint8_t)kCode[c]];
	// a symmetric matrix of small scores, positive on the diagonal and for about a third of the pairs: '|', '+' and ' ' all occur
	for (int a = 0; a < kAsize; ++a)
		for (int b = a; b < kAsize; ++b) {
			const int8_t v = a == b ? 5 : (int8_t)((int)rnd(9) - 5);
			g_tab[ALN_TAB_MAT + a * kAsize + b] = g_tab[ALN_TAB_MAT + b * kAsize + a] = (uint8_t)v;
		}
}

struct Genome {                                              // two contigs, packed four bits per base, low nibble = even offset
	std::vector<uint8_t> packed;
	int64_t off[2], len[2];
	std::vector<uint8_t> strand[4];                          // the same, unpacked per (contig, strand): what the plain walk reads
};
struct PackedReader {
	const uint8_t *seq; int64_t off, len; int rev;
	uint32_t base(int64_t x) const
	{
		if (x < 0 || x >= len) return 4;
		const int64_t p = rev ? off + len - 1 - x : off + x;
		const uint32_t c = (seq[p >> 1] >> ((p & 1) * 4)) & 0xf;
		return rev && c < 4 ? 3 - c : c;
	}
};

// ---- the plain walk: put_residues() of host_format.cpp (format.c:189-331) over an unpacked strand -------------------------------
struct Rows { std::string atn, ata, aas, aqa, sta; };
static uint8_t plain_aa(const uint8_t *nt) { return nt[0] > 3 || nt[1] > 3 || nt[2] > 3 ? 21 : g_tab[ALN_TAB_CODON + (nt[0] << 4 | nt[1] << 2 | nt[2])]; }
static char plain_up(char c) { return c >= 'a' && c <= 'z' ? (char)(c - 'a' + 'A') : c; }
static Rows plain(const std::vector<uint8_t> &strand, int64_t vs, int64_t ve, const char *aa, const std::vector<uint32_t> &cigar, int32_t flank)
{
	static const char UC[] = "ACGTN", LC[] = "acgtn";
	// the fetched span: [vs, ve + 3) cut at the strand's end, zeros behind it as in the host's buffer
	std::vector<uint8_t> ntv((size_t)(ve - vs + 3), 0);
	const int64_t en = ve + 3 > (int64_t)strand.size() ? (int64_t)strand.size() : ve + 3, l_nt = en - vs;
	memcpy(ntv.data(), strand.data() + vs, (size_t)l_nt);
	const uint8_t *nt = ntv.data();
	Rows r;
	char last = '\t';
	auto col = [&](char a, char b, char c, char d) { r.atn += a, r.ata += b, r.aas += c, r.aqa += d; };
	auto put_sta = [&](uint8_t t) { r.sta += kAA20[t], last = kAA20[t]; };
	auto match_char = [&](uint8_t t, char q) {
		const uint8_t qa = g_tab[ALN_TAB_AA20 + (uint8_t)q];
		return t == qa ? '|' : (int8_t)g_tab[ALN_TAB_MAT + t * kAsize + qa] > 0 ? '+' : ' ';
	};
	int64_t nl = 0;
	int32_t al = 0;
	for (uint32_t c : cigar) {
		const int32_t op = c & 0xf, len = (int32_t)(c >> 4);
		if (op == 0) {
			for (int32_t l = 0; l < len; ++l, nl += 3, ++al) {
				const uint8_t t = plain_aa(nt + nl);
				put_sta(t);
				col(UC[nt[nl]], kAA20[t], match_char(t, aa[al]), plain_up(aa[al])), col(UC[nt[nl + 1]], '.', ' ', ' '), col(UC[nt[nl + 2]], '.', ' ', ' ');
			}
		} else if (op == 1) {
			for (int32_t l = 0; l < len; ++l, ++al) col('-', '-', ' ', plain_up(aa[al])), col('-', '.', ' ', ' '), col('-', '.', ' ', ' ');
		} else if (op == 2) {
			for (int32_t l = 0; l < len; ++l, nl += 3) {
				const uint8_t t = plain_aa(nt + nl);
				put_sta(t);
				col(UC[nt[nl]], kAA20[t], ' ', '-'), col(UC[nt[nl + 1]], '.', ' ', ' '), col(UC[nt[nl + 2]], '.', ' ', ' ');
			}
		} else if (op == 10) {
			for (int32_t l = 0; l < len; ++l, ++nl) col(UC[nt[nl]], '!', ' ', ' ');
		} else if (op == 11) {
			for (int32_t l = 0; l < len; ++l, ++nl) col(UC[nt[nl]], '$', ' ', l == 0 ? plain_up(aa[al]) : ' ');
			++al;
		} else if (op == 3 || op == 12 || op == 13) {
			const int32_t intron = op == 3 ? len : len - 3;
			if (op != 3) {
				const uint8_t c3[3] = { nt[nl], op == 12 ? nt[nl + len - 2] : nt[nl + 1], nt[nl + len - 1] };
				const uint8_t t = plain_aa(c3);
				put_sta(t);
				col(UC[nt[nl]], kAA20[t], match_char(t, aa[al]), plain_up(aa[al]));
				++nl;
				if (op == 13) col(UC[nt[nl]], '.', ' ', ' '), ++nl;
				++al;
			}
			if (intron <= flank * 2) {
				for (int32_t l = 0; l < intron; ++l) col(LC[nt[nl + l]], ' ', ' ', ' ');
			} else {
				char num[16];
				snprintf(num, sizeof num, "%d", intron);
				for (int32_t l = 0; l < flank; ++l) col(LC[nt[nl + l]], ' ', ' ', ' ');
				col('~', ' ', ' ', ' ');
				for (const char *p = num; *p; ++p) col(*p, ' ', ' ', ' ');
				col('~', ' ', ' ', ' ');
				for (int32_t l = 0; l < flank; ++l) col(LC[nt[nl + intron - flank + l]], ' ', ' ', ' ');
			}
			nl += intron;
			if (op != 3) {
				col(UC[nt[nl]], '.', ' ', ' '), ++nl;
				if (op == 12) col(UC[nt[nl]], '.', ' ', ' '), ++nl;
			}
		}
	}
	if (l_nt == ve - vs + 3 && last != '*') {
		const uint8_t t = plain_aa(nt + nl);
		r.sta += kAA20[t];
		col(UC[nt[nl]], kAA20[t], ' ', ' '), col(UC[nt[nl + 1]], '.', ' ', ' '), col(UC[nt[nl + 2]], '.', ' ', ' ');
	}
	return r;
}

// ---- one case -----------------------------------------------------------------------------------------
static int g_fail = 0, g_cases = 0, g_trailing = 0, g_no_trailing = 0;
static const Genome *g_gen;
static bool g_wave = true;                                  // the team of 64 threads too
static const int kGuard = 16;
typedef std::function<bool(int, int32_t, int32_t)> Pattern;   // (M operation number, codon, codons of the operation) -> a mismatch there?

// vs < 0: place the alignment so that it ends -vs - 1 bases before its strand's end
static void run_case(const char *name, int vid, int64_t vs, int32_t qs, int32_t tail, const std::vector<uint32_t> &cigar, const Pattern &pat, int32_t flank, bool lower = false,
                     int want_trailing = -1)
{
	const std::vector<uint8_t> &strand = g_gen->strand[vid];
	int64_t nl = 0;
	int32_t al = 0;
	for (uint32_t c : cigar) {
		const int32_t op = c & 0xf, len = (int32_t)(c >> 4);
		if (op == 0) nl += 3 * (int64_t)len, al += len;
		else if (op == 1) al += len;
		else if (op == 2) nl += 3 * (int64_t)len;
		else if (op == 10) nl += len;
		else if (op == 11) nl += len, ++al;
		else nl += len, al += op != 3;
	}
	if (vs < 0) vs = (int64_t)strand.size() - nl - (-vs - 1);
	if (vs < 0 || vs + nl > (int64_t)strand.size()) { fprintf(stderr, "case %s does not fit its strand\n", name); ++g_fail; return; }
	AlnStatsJob J;
	memset(&J, 0, sizeof(J));
	J.vs = vs, J.ve = vs + nl, J.as = vs, J.ae = vs + nl, J.vid = vid, J.qs = qs, J.qe = qs + al, J.qlen = qs + al + tail, J.n_cigar = (int32_t)cigar.size();
	// the protein: noise, and under every M codon the residue the pattern asks for -- the codon's own, or one that differs
	std::string prot((size_t)J.qlen, 'A');
	for (auto &ch : prot) ch = kAA20[rnd(20)];
	{
		int64_t x = vs;
		int32_t a = qs, m = 0;
		for (uint32_t c : cigar) {
			const int32_t op = c & 0xf, len = (int32_t)(c >> 4);
			if (op == 0) {
				for (int32_t l = 0; l < len; ++l) {
					const uint8_t t = plain_aa(&strand[(size_t)(x + 3 * (int64_t)l)]);
					prot[(size_t)(a + l)] = pat(m, l, len) ? kAA20[(t + 1 + rnd(19)) % 20] : kAA20[t];
				}
				x += 3 * (int64_t)len, a += len, ++m;
			} else if (op == 1) a += len;
			else if (op == 2) x += 3 * (int64_t)len;
			else if (op == 10) x += len;
			else if (op == 11) x += len, ++a;
			else x += len, a += op != 3;
		}
	}
	if (lower) for (auto &ch : prot) ch = (char)(ch >= 'A' && ch <= 'Z' ? ch | 0x20 : ch);
	const Rows want = plain(strand, vs, J.ve, prot.c_str() + qs, cigar, flank);
	const int64_t cols = aln_rows_cols(cigar.data(), (int32_t)cigar.size(), flank), codons = aln_rows_codons(cigar.data(), (int32_t)cigar.size());
	const bool trailing = (int64_t)want.atn.size() == cols + 3;
	// the bound functions are exact but for the trailing codon
	if (((int64_t)want.atn.size() != cols && !trailing) || (int64_t)want.sta.size() != codons + trailing || want.atn.size() != want.ata.size() ||
	    want.atn.size() != want.aas.size() || want.atn.size() != want.aqa.size()) {
		fprintf(stderr, "BOUND %s: rows of %zu columns and %zu STA bytes; aln_rows_cols %lld, aln_rows_codons %lld\n", name, want.atn.size(), want.sta.size(), (long long)cols, (long long)codons);
		++g_fail;
	}
	if (want_trailing >= 0 && (int)trailing != want_trailing) {
		fprintf(stderr, "TRAILING %s: the plain walk %s a trailing codon\n", name, trailing ? "printed" : "did not print");
		++g_fail;
	}
	g_trailing += trailing, g_no_trailing += !trailing;
	const PackedReader g{ g_gen->packed.data(), g_gen->off[vid >> 1], g_gen->len[vid >> 1], vid & 1 };
	for (int combo = 1; combo <= 3; ++combo) {               // --aln, --trans, both
		const AlnRowsParams P{ kAsize, flank, combo & 1, combo >> 1 };
		const int64_t slot = aln_rows_slot(cigar.data(), (int32_t)cigar.size(), P), stride = P.show_aln ? cols + 3 : 0;
		if (slot != 4 * stride + (P.show_trans ? codons + 1 : 0)) { fprintf(stderr, "SLOT %s: %lld bytes\n", name, (long long)slot); ++g_fail; }
		// guard | slot of the team of one | guard | slot of the team of 64 | guard
		std::vector<char> buf((size_t)(3 * kGuard + 2 * slot));
		for (size_t i = 0; i < buf.size(); ++i) buf[i] = (char)(0xA5 ^ (i * 7));
		std::vector<char> expect = buf;
		char *slot_a = buf.data() + kGuard, *slot_b = slot_a + slot + kGuard;
		auto overlay = [&](size_t at) {                          // what a slot must hold, over the pattern; everything else stays
			char *d = expect.data() + at;
			if (P.show_aln) {
				memcpy(d, want.atn.data(), want.atn.size()), memcpy(d + stride, want.ata.data(), want.ata.size());
				memcpy(d + 2 * stride, want.aas.data(), want.aas.size()), memcpy(d + 3 * stride, want.aqa.data(), want.aqa.size());
			}
			if (P.show_trans) memcpy(d + 4 * stride, want.sta.data(), want.sta.size());
		};
		auto good = [&](const AlnRowsOut &o) { return !o.bad && o.width == (P.show_aln ? (int32_t)want.atn.size() : 0) && o.n_sta == (int32_t)want.sta.size(); };
		overlay((size_t)kGuard);
		bool ok = good(aln_rows_core<StatsSerial>(J, P, g_tab, (const uint8_t*)prot.c_str(), cigar.data(), g, slot_a));
		if (g_wave) {
			overlay((size_t)(2 * kGuard + slot));
			std::vector<AlnRowsOut> outs(64);
			std::vector<std::thread> th;
			for (int l = 0; l < 64; ++l)
				th.emplace_back([&, l] { tl_lane = l; outs[(size_t)l] = aln_rows_core<RowThreads>(J, P, g_tab, (const uint8_t*)prot.c_str(), cigar.data(), g, slot_b); });
			for (auto &t : th) t.join();
			for (int l = 0; l < 64; ++l) ok = ok && good(outs[(size_t)l]);
		}
		if (!ok || buf != expect) {
			size_t at = 0;
			while (at < buf.size() && buf[at] == expect[at]) ++at;
			++g_fail;
			fprintf(stderr, "MISMATCH %s (flags %d, flank %d): record %s, first differing byte %zu of %zu (slot %lld, stride %lld)\n  want ATN %.120s\n  want STA %.120s\n", name, combo, flank,
			        ok ? "good" : "wrong", at, buf.size(), (long long)slot, (long long)stride, want.atn.c_str(), want.sta.c_str());
		}
		++g_cases;
	}
}

static uint32_t op(char c, int32_t len)
{
	const char *ops = "MIDN......FGUV";
	return (uint32_t)len << 4 | (uint32_t)(strchr(ops, c) - ops);
}

int main()
{
	make_tables();
	pthread_barrier_init(&g_bar, nullptr, 64);
	// contig 0: 1 300 000 bases without N but for a few planted ones; contig 1: 30 001 bases (an odd length behind an odd offset: both
	// nibbles, both strands) with 3 % N
	Genome G;
	G.off[0] = 0, G.len[0] = 1300000, G.off[1] = 1300001, G.len[1] = 30001;
	const int64_t total = G.off[1] + G.len[1];
	std::vector<uint8_t> flat((size_t)total);
	for (int64_t i = 0; i < total; ++i) flat[(size_t)i] = i >= G.off[1] && rnd(100) < 3 ? 4 : (uint8_t)rnd(4);
	for (int64_t x : { 62, 63, 110, 402, 1299000 }) flat[(size_t)x] = 4;     // (contig 0: codons and introns with N under the walks that start at 50)
	// contig 0 forward: TAA at 5000 + 3 * 9 (the tenth codon of a walk from 5000), and no stop in the codons before or behind it
	for (int64_t x = 5000; x < 5060; ++x) flat[(size_t)x] = (uint8_t)(1 + rnd(2));   // (C and G only)
	flat[5027] = 3, flat[5028] = 0, flat[5029] = 0;
	G.packed.assign((size_t)(total + 1) / 2 + 16, 0);
	for (int64_t i = 0; i < total; ++i) G.packed[(size_t)(i >> 1)] |= (uint8_t)(flat[(size_t)i] << ((i & 1) * 4));
	for (int c = 0; c < 2; ++c) {
		G.strand[2 * c].assign(flat.begin() + G.off[c], flat.begin() + G.off[c] + G.len[c]);
		std::vector<uint8_t> &r = G.strand[2 * c + 1];
		r.resize((size_t)G.len[c]);
		for (int64_t i = 0; i < G.len[c]; ++i) { const uint8_t b = flat[(size_t)(G.off[c] + G.len[c] - 1 - i)]; r[(size_t)i] = b < 4 ? 3 - b : b; }
	}
	g_gen = &G;

	const Pattern all_match = [](int, int32_t, int32_t) { return false; };
	const Pattern all_mism = [](int, int32_t, int32_t) { return true; };
	const Pattern alternating = [](int, int32_t l, int32_t) { return (l & 1) != 0; };
	const Pattern noise = [](int, int32_t, int32_t) { return rnd(4) == 0; };
	char nm[128];
	for (int vid = 0; vid < 4; ++vid) {
		const int64_t vs = 50;
		g_wave = vid == 0 || vid == 3;                           // (the team of 64 on contig 0 forward and contig 1 reverse; the team of one everywhere)
		// M runs: 21 / 22 codons straddle 64 columns, 63 - 65 straddle 64 codons
		for (int32_t n : { 1, 21, 22, 63, 64, 65, 1000 }) {
			snprintf(nm, sizeof nm, "M%d all match, vid %d", n, vid), run_case(nm, vid, vs, 3, 2, { op('M', n) }, all_match, 200);
			snprintf(nm, sizeof nm, "M%d alternating, vid %d", n, vid), run_case(nm, vid, vs, 3, 2, { op('M', n) }, alternating, 200);
			snprintf(nm, sizeof nm, "M%d all mismatch, vid %d", n, vid), run_case(nm, vid, vs, 0, 0, { op('M', n) }, all_mism, 200);
		}
		run_case("M M M back to back", vid, vs, 1, 1, { op('M', 21), op('M', 22), op('M', 65) }, noise, 200);
		run_case("I1 I2 D1 D2 F1 F2 G1 G2", vid, vs, 0, 3,
		         { op('M', 7), op('I', 1), op('M', 5), op('I', 2), op('M', 3), op('D', 1), op('M', 2), op('D', 2), op('M', 4), op('F', 1), op('M', 5), op('F', 2), op('M', 66), op('G', 1), op('M', 3), op('G', 2), op('M', 4) }, noise, 200);
		run_case("long I and D", vid, vs, 0, 3, { op('M', 5), op('I', 70), op('M', 5), op('D', 66), op('M', 5), op('I', 130) }, noise, 200);
		run_case("I first, D last", vid, vs, 0, 0, { op('I', 3), op('M', 5), op('D', 3) }, noise, 200);
		for (int32_t flank : { 0, 1, 200 }) {
			// introns first, last and back to back
			run_case("N first and last", vid, vs, 2, 0, { op('N', 70), op('M', 9), op('N', 71) }, noise, flank);
			run_case("U first", vid, vs, 0, 1, { op('U', 80), op('M', 20) }, noise, flank);
			run_case("V first", vid, vs, 0, 1, { op('V', 80), op('M', 20) }, noise, flank);
			run_case("U last", vid, vs, 2, 0, { op('M', 20), op('U', 75) }, noise, flank);
			run_case("V last", vid, vs, 2, 0, { op('M', 20), op('V', 75) }, noise, flank);
			run_case("U V back to back", vid, vs, 1, 4, { op('M', 10), op('U', 70), op('V', 90), op('M', 12) }, noise, flank);
			run_case("V U N N back to back", vid, vs, 1, 4, { op('M', 10), op('V', 70), op('U', 90), op('N', 72), op('N', 5), op('M', 70) }, noise, flank);
			// intron lengths around twice the flank: the longest printed whole, the shortest abridged
			for (int32_t intron : { 2 * flank - 1, 2 * flank, 2 * flank + 1 }) {
				if (intron < 1) continue;
				snprintf(nm, sizeof nm, "N of %d at flank %d, vid %d", intron, flank, vid), run_case(nm, vid, vs, 0, 0, { op('M', 3), op('N', intron), op('M', 3) }, noise, flank);
				snprintf(nm, sizeof nm, "U of %d at flank %d, vid %d", intron, flank, vid), run_case(nm, vid, vs, 0, 0, { op('M', 3), op('U', intron + 3), op('M', 3) }, noise, flank);
				snprintf(nm, sizeof nm, "V of %d at flank %d, vid %d", intron, flank, vid), run_case(nm, vid, vs, 0, 0, { op('M', 3), op('V', intron + 3), op('M', 3) }, noise, flank);
			}
			// intron lengths of 1 to 7 digits (contig 1 holds up to five)
			for (int32_t digits = 1; digits <= (vid < 2 ? 7 : 5); ++digits) {
				int32_t lo = 1;
				for (int d = 1; d < digits; ++d) lo *= 10;
				const int32_t hi = lo * 10 - 1 > 1200000 ? 1200000 : lo * 10 - 1;
				for (int32_t printed : { lo, hi }) {
					if (printed > (vid < 2 ? 1200000 : 25000)) continue;
					snprintf(nm, sizeof nm, "N of %d, flank %d, vid %d", printed, flank, vid), run_case(nm, vid, vs, 0, 0, { op('M', 3), op('N', printed), op('M', 3) }, noise, flank);
					snprintf(nm, sizeof nm, "U of %d, flank %d, vid %d", printed, flank, vid), run_case(nm, vid, vs, 0, 0, { op('M', 3), op('U', printed + 3), op('M', 3) }, noise, flank);
					snprintf(nm, sizeof nm, "V of %d, flank %d, vid %d", printed, flank, vid), run_case(nm, vid, vs, 0, 0, { op('M', 3), op('V', printed + 3), op('M', 3) }, noise, flank);
				}
			}
			{
				std::vector<uint32_t> c;                             // 70 words: more than one round of 64
				for (int k = 0; k < 14; ++k) c.push_back(op('M', 2 + k % 3)), c.push_back(op('I', 1)), c.push_back(op('D', 1)), c.push_back(op("NUV"[k % 3], 6 + k)), c.push_back(op('M', 1));
				run_case("70 words", vid, vs, 5, 5, c, noise, flank);
				c.insert(c.end(), c.begin(), c.end());
				c.resize(100);
				run_case("100 words", vid, 21, 5, 5, c, noise, flank);
			}
			// introns with N (contig 0 forward: 62, 63, 110 and 402 are N; contig 1: 3 % N), whole at flank 200 and inside the flanks at 1
			run_case("N in a split codon and its intron", vid, vs, 0, 0, { op('M', 4), op('U', 30), op('M', 3), op('N', 340), op('M', 2) }, noise, flank);
		}
		// codons with N: under an M, among deleted and frameshift bases
		run_case("N codons under M", vid, vs, 0, 0, { op('M', 30) }, all_match, 200);
		run_case("N codons under M, mismatching", vid, vs, 0, 0, { op('M', 30) }, all_mism, 200);
		run_case("N among D, F and G bases", vid, 59, 0, 0, { op('D', 2), op('M', 1), op('F', 2), op('M', 14), op('G', 2), op('M', 2) }, noise, 200);
		// a lower-case query: residues print in upper case, matching is case-blind
		run_case("lower-case query", vid, vs, 2, 2, { op('M', 70), op('I', 3), op('M', 10), op('V', 50), op('G', 1), op('M', 5) }, alternating, 200, true);
		// the ends of the strand: an alignment that ends 0, 1, 2 and 3 bases before it -- the trailing codon at 3 only (unless the last
		// codon happens to be a stop there)
		run_case("from the first base", vid, 0, 0, 0, { op('N', 64), op('M', 64), op('U', 64) }, noise, 200);
		for (int k = 0; k <= 3; ++k) {
			snprintf(nm, sizeof nm, "ends %d before the end, vid %d", k, vid);
			run_case(nm, vid, -1 - k, 0, 0, { op('M', 20), op('V', 60), op('M', 20) }, noise, 200, false, k < 3 ? 0 : -1);
			snprintf(nm, sizeof nm, "no codon, ends %d before the end, vid %d", k, vid);
			run_case(nm, vid, -1 - k, 0, 0, { op('I', 2), op('N', 70), op('F', 2), op('G', 1) }, noise, 200, false, k == 3);
		}
		// no codon at all: nothing was written to STA, so the trailing codon is printed
		run_case("no codon at all", vid, vs, 0, 0, { op('I', 2), op('N', 70), op('F', 1), op('G', 2), op('I', 1) }, noise, 1, false, 1);
	}
	// the last codon is a stop (contig 0 forward, the TAA planted at 5027): no trailing codon; one codon less: printed, and it is the stop
	g_wave = true;
	run_case("last codon a stop", 0, 5000, 0, 0, { op('M', 10) }, all_match, 200, false, 0);
	run_case("last codon a stop, deleted", 0, 5000, 0, 0, { op('M', 9), op('D', 1) }, all_match, 200, false, 0);
	run_case("stop behind the last codon", 0, 5000, 0, 0, { op('M', 9) }, all_match, 200, false, 1);
	run_case("stop in the middle", 0, 5000, 0, 0, { op('M', 15) }, noise, 200, false, 1);
	run_case("a split last codon", 0, 4997, 0, 0, { op('M', 9), op('U', 33) }, noise, 200, false, -1);
	// random CIGARs
	for (int it = 0; it < 300; ++it) {
		std::vector<uint32_t> c;
		const int n = 1 + (int)rnd(it % 10 == 0 ? 90 : 12);
		for (int k = 0; k < n; ++k) {
			const char o = "MMMMIDNUVFG"[rnd(11)];
			const int32_t len = o == 'M' ? 1 + (int32_t)rnd(it % 7 == 0 ? 200 : 9) : o == 'I' || o == 'D' ? 1 + (int32_t)rnd(4) : o == 'F' || o == 'G' ? 1 + (int32_t)rnd(2) : 4 + (int32_t)rnd(400);
			c.push_back(op(o, len));
		}
		const int vid = (int)rnd(4);
		const int percent = (int)rnd(101);
		snprintf(nm, sizeof nm, "random %d", it);
		g_wave = it % 10 == 0;
		run_case(nm, vid, 20 + rnd(60), (int32_t)rnd(5), (int32_t)rnd(2), c, [percent](int, int32_t, int32_t) { return (int)rnd(100) < percent; }, (int32_t)rnd(3) == 0 ? 200 : (int32_t)rnd(40), it % 13 == 0);
	}
	if (!g_trailing || !g_no_trailing) { fprintf(stderr, "COVERAGE: %d cases with a trailing codon, %d without\n", g_trailing, g_no_trailing); ++g_fail; }
	printf("alnrows_check: %d cases, %d mismatches (%d walks with a trailing codon, %d without)\n", g_cases, g_fail, g_trailing, g_no_trailing);
	return g_fail ? 1 : 0;
}
