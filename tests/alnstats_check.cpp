// alnstats_check.cpp -- a stand-alone check of miniprot_amd/csrc/aln_stats_core.h (tests/test_aln_stats_cpu.py compiles it with
// -fsanitize=address,undefined and runs it).  Hand-written CIGARs over a 600-base window of a small two-strand genome go through
// the shared core twice -- with a team of one (StatsSerial, what MPA_GPU_STATS=model runs) and with a team of 64 host threads that
// meet at a barrier for every ballot, sum and broadcast (the device's wavefront in slow motion: same lane-strided loops, same lane-0
// work) -- and are compared, field by field, with a plain sequential walk over the unpacked strand written here after
// mp_extra_stop, mp_extra_start and mp_extra_cal (align.c:82-237).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>
#include <pthread.h>
#include "aln_stats_core.h"

using namespace mpa;

// ---- a team of 64 threads ---------------------------------------------------------------------------
static pthread_barrier_t g_bar;
static uint64_t g_slot[64];
static thread_local int tl_lane = 0;
struct StatsThreads {
	static int lane() { return tl_lane; }
	static int width() { return 64; }
	static void sync() { pthread_barrier_wait(&g_bar); }
	static uint64_t ballot(bool p)
	{
		g_slot[tl_lane] = p;
		pthread_barrier_wait(&g_bar);
		uint64_t m = 0;
		for (int i = 0; i < 64; ++i) m |= (uint64_t)(g_slot[i] & 1) << i;
		pthread_barrier_wait(&g_bar);
		return m;
	}
	static int lowest(uint64_t m) { return __builtin_ctzll(m); }
	static int32_t sum(int32_t v)
	{
		g_slot[tl_lane] = (uint32_t)v;
		pthread_barrier_wait(&g_bar);
		uint32_t s = 0;
		for (int i = 0; i < 64; ++i) s += (uint32_t)g_slot[i];
		pthread_barrier_wait(&g_bar);
		return (int32_t)s;
	}
	static uint32_t bcast(uint32_t v, int k)
	{
		g_slot[tl_lane] = v;
		pthread_barrier_wait(&g_bar);
		const uint32_t r = (uint32_t)g_slot[k];
		pthread_barrier_wait(&g_bar);
		return r;
	}
};

// ---- tables and genome ------------------------------------------------------------------------------
static const char *kAA20 = "ARNDCQEGHILKMFPSTWYV*X";
static const char *kCode = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF";   // codon = b0 << 4 | b1 << 2 | b2 over A0 C1 G2 T3
static uint8_t g_tab[ALN_TAB_BYTES];
static void make_tables()
{
	for (int c = 0; c < 256; ++c) g_tab[ALN_TAB_AA20 + c] = 21;
	for (int i = 0; i < 22; ++i) g_tab[ALN_TAB_AA20 + (uint8_t)kAA20[i]] = (uint8_t)i, g_tab[ALN_TAB_AA20 + (uint8_t)(kAA20[i] | 0x20)] = (uint8_t)i;
	for (int c = 0; c < 64; ++c) g_tab[ALN_TAB_CODON + c] = g_tab[ALN_TAB_AA20 + (uint8_t)kCode[c]];
	for (int a = 0; a < 22; ++a)
		for (int b = 0; b < 22; ++b) g_tab[ALN_TAB_MAT + a * 22 + b] = (uint8_t)(int8_t)(a == b ? 4 + a % 7 : (a * 7 + b * 3) % 9 - 5);
}

static uint64_t g_rng = 88172645463325252ULL;
static uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 20) % n); }

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

// ---- the plain walk ---------------------------------------------------------------------------------
struct Want { AlnStatsOut o; std::vector<AlnFeat> feat; };
static uint8_t plain_aa(const uint8_t *nt) { return nt[0] > 3 || nt[1] > 3 || nt[2] > 3 ? 21 : g_tab[ALN_TAB_CODON + (nt[0] << 4 | nt[1] << 2 | nt[2])]; }
static Want plain(const std::vector<uint8_t> &strand, const AlnStatsJob &J, const AlnStatsParams &p, const char *aa_full, const std::vector<uint32_t> &cigar)
{
	Want w;
	memset(&w.o, 0, sizeof(w.o));
	const uint8_t *nt = strand.data() + J.as;                // the window, as mp_align() fetches it
	w.o.dist_stop = -1;
	for (int64_t j = J.ve; j + 2 < J.ae; j += 3)
		if (plain_aa(nt + (j - J.as)) == 20) { w.o.dist_stop = (int32_t)(j - J.ve); break; }
	w.o.dist_start = -1;
	for (int64_t j = J.vs; j >= J.as && j + 2 < J.ae; j -= 3) {
		const uint8_t a = plain_aa(nt + (j - J.as));
		if (a == 20) break;
		if (a == 12) { w.o.dist_start = (int32_t)(J.vs - j); break; }
	}
	nt = strand.data() + J.vs;
	const int64_t l_nt = J.ae - J.vs;
	const char *aa = aa_full + J.qs;
	const char *i2c = "ACGTN";
	const bool has_stop = J.qe == J.qlen && w.o.dist_stop == 0;
	int32_t n_intron = 0;
	for (uint32_t c : cigar) n_intron += (c & 0xf) == 3 || (c & 0xf) == 12 || (c & 0xf) == 13;
	AlnFeat zero;
	memset(&zero, 0, sizeof(zero));
	w.feat.assign((size_t)n_intron + 1 + has_stop, zero);
	int32_t nl = 0, al = 0, ft = 0, blen = 0, n_iden = 0, n_plus = 0, n_fs = 0, n_stop = 0, dp_max = 0;
	int32_t blen0 = 0, iden0 = 0, score0 = 0, fs0 = 0, stop0 = 0, phase0 = 0, qs0 = J.qs;
	int64_t vs0 = J.vs;
	char acc0[2] = { 0, 0 };
	auto residue = [&](uint8_t nt_aa, int32_t j) {
		const uint8_t q = g_tab[ALN_TAB_AA20 + (uint8_t)aa[j]];
		const int32_t s = (int8_t)g_tab[ALN_TAB_MAT + nt_aa * p.asize + q];
		n_stop += nt_aa == 20, n_iden += nt_aa == q, n_plus += s > 0, dp_max += s;
	};
	auto exon = [&](AlnFeat &f, int64_t ve) {
		f.type = 0, f.vs = vs0, f.ve = ve, f.qs = qs0, f.qe = J.qs + al, f.phase = (int16_t)phase0;
		f.blen = blen - blen0, f.n_iden = n_iden - iden0, f.n_fs = n_fs - fs0, f.n_stop = n_stop - stop0, f.score = dp_max - score0;
		if (ft > 0) f.acceptor[0] = acc0[0], f.acceptor[1] = acc0[1];
	};
	for (uint32_t c : cigar) {
		const int32_t op = c & 0xf, len = (int32_t)(c >> 4);
		if (op == 0) {
			for (int32_t l = 0; l < len; ++l) residue(plain_aa(nt + nl + 3 * l), al + l);
			nl += 3 * len, al += len, blen += 3 * len;
		} else if (op == 1) dp_max -= p.go + p.ge * len, al += len, blen += 3 * len;
		else if (op == 2) {
			for (int32_t l = 0; l < len; ++l) n_stop += plain_aa(nt + nl + 3 * l) == 20;
			dp_max -= p.go + p.ge * len, nl += 3 * len, blen += 3 * len;
		} else if (op == 10) dp_max -= p.fs, nl += len, blen += len, ++n_fs;
		else if (op == 11) dp_max -= p.fs, nl += len, ++al, blen += 3, ++n_fs;
		else {
			if (op != 3) {
				uint8_t cod[3] = { nt[nl], op == 12 ? nt[nl + len - 2] : nt[nl + 1], nt[nl + len - 1] };
				residue(plain_aa(cod), al);
				blen += 3;
			}
			AlnFeat &f = w.feat[(size_t)ft];
			exon(f, J.vs + nl + (op == 3 ? 0 : op == 12 ? 1 : 2));
			++ft;
			vs0 = J.vs + nl + len - (op == 3 ? 0 : op == 12 ? 2 : 1), phase0 = op == 3 ? 0 : op == 12 ? 2 : 1;
			f.donor[0] = f.ve - J.vs < l_nt ? i2c[nt[f.ve - J.vs]] : '.';
			f.donor[1] = f.ve - J.vs + 1 < l_nt ? i2c[nt[f.ve - J.vs + 1]] : '.';
			qs0 = f.qe, fs0 = n_fs, stop0 = n_stop, score0 = dp_max, blen0 = blen, iden0 = n_iden;
			acc0[0] = vs0 - J.vs >= 2 ? i2c[nt[vs0 - J.vs - 2]] : '.';
			acc0[1] = vs0 - J.vs >= 1 ? i2c[nt[vs0 - J.vs - 1]] : '.';
			nl += len, al += op != 3;
		}
	}
	exon(w.feat[(size_t)ft], J.vs + nl);
	++ft;
	if (has_stop) {
		AlnFeat &f = w.feat[(size_t)ft++];
		f.type = 1, f.vs = J.ve, f.ve = J.ve + 3, f.qs = f.qe = J.qe + al, f.blen = 3;
	}
	w.o.dp_max = dp_max, w.o.blen = blen, w.o.n_iden = n_iden, w.o.n_plus = n_plus, w.o.n_fs = n_fs, w.o.n_stop = n_stop;
	w.o.bad = !(nl == J.ve - J.vs && al == J.qe - J.qs), w.o.n_feat = ft;
	return w;
}

// ---- comparison -------------------------------------------------------------------------------------
static int g_fail = 0, g_cases = 0;
static bool same_out(const AlnStatsOut &a, const AlnStatsOut &b)
{
	return a.dist_stop == b.dist_stop && a.dist_start == b.dist_start && a.dp_max == b.dp_max && a.blen == b.blen && a.n_iden == b.n_iden && a.n_plus == b.n_plus &&
	       a.n_fs == b.n_fs && a.n_stop == b.n_stop && a.bad == b.bad && a.n_feat == b.n_feat;
}
static bool same_feat(const AlnFeat &a, const AlnFeat &b)
{
	return a.vs == b.vs && a.ve == b.ve && a.qs == b.qs && a.qe == b.qe && a.type == b.type && a.phase == b.phase && a.n_fs == b.n_fs && a.n_stop == b.n_stop &&
	       a.score == b.score && a.n_iden == b.n_iden && a.blen == b.blen && !memcmp(a.donor, b.donor, 2) && !memcmp(a.acceptor, b.acceptor, 2);
}
static void compare(const char *name, const char *team, const Want &w, const AlnStatsOut &o, const std::vector<AlnFeat> &feat)
{
	bool ok = same_out(w.o, o);
	for (int32_t k = 0; ok && k < w.o.n_feat; ++k) ok = same_feat(w.feat[(size_t)k], feat[(size_t)k]);
	if (ok) return;
	++g_fail;
	fprintf(stderr, "MISMATCH %s (%s): want stop %d start %d max %d blen %d iden %d plus %d fs %d nstop %d bad %d feat %d; got %d %d %d %d %d %d %d %d %d %d\n", name, team,
	        w.o.dist_stop, w.o.dist_start, w.o.dp_max, w.o.blen, w.o.n_iden, w.o.n_plus, w.o.n_fs, w.o.n_stop, w.o.bad, w.o.n_feat, o.dist_stop, o.dist_start, o.dp_max, o.blen,
	        o.n_iden, o.n_plus, o.n_fs, o.n_stop, o.bad, o.n_feat);
}

static const Genome *g_gen;
static bool g_wave = true;                                  // the team of 64 threads too (64 threads per case: the cases that need it)
static void run_case(const char *name, int vid, int64_t as, int64_t ae, int64_t vs, int32_t qs, int32_t tail, const std::vector<uint32_t> &cigar, const std::string &prot_hint = "")
{
	int64_t nl = 0;
	int32_t al = 0, n_intron = 0;
	for (uint32_t c : cigar) {
		const int32_t op = c & 0xf, len = (int32_t)(c >> 4);
		if (op == 0) nl += 3 * len, al += len;
		else if (op == 1) al += len;
		else if (op == 2) nl += 3 * len;
		else if (op == 10) nl += len;
		else if (op == 11) nl += len, ++al;
		else nl += len, al += op != 3, ++n_intron;
	}
	AlnStatsJob J;
	memset(&J, 0, sizeof(J));
	J.vs = vs, J.ve = vs + nl, J.as = as, J.ae = ae, J.vid = vid, J.qs = qs, J.qe = qs + al, J.qlen = qs + al + tail, J.n_cigar = (int32_t)cigar.size();
	if (!(as <= vs && J.ve <= ae && ae <= g_gen->len[vid >> 1])) { fprintf(stderr, "case %s does not fit its window\n", name); ++g_fail; return; }
	// the protein: the translation of the strand under the walk where that is cheap to say (so that identities occur), noise elsewhere
	std::string prot((size_t)J.qlen, 'A');
	const std::vector<uint8_t> &strand = g_gen->strand[vid];
	for (int32_t i = 0; i < J.qlen; ++i) prot[(size_t)i] = kAA20[rnd(20)];
	for (int32_t i = 0; i < al; ++i) {
		const int64_t x = vs + 3 * (int64_t)i;
		if (x + 2 < ae && rnd(3)) { const uint8_t a = plain_aa(&strand[(size_t)x]); if (a < 20) prot[(size_t)(qs + i)] = kAA20[a]; }
	}
	if (!prot_hint.empty()) prot.replace((size_t)qs, prot_hint.size(), prot_hint);
	const AlnStatsParams p{ 11, 1, 23, 22 };
	const Want w = plain(strand, J, p, prot.c_str(), cigar);
	const PackedReader g{ g_gen->packed.data(), g_gen->off[vid >> 1], g_gen->len[vid >> 1], vid & 1 };
	AlnFeat zero;
	memset(&zero, 0, sizeof(zero));
	{
		std::vector<AlnFeat> feat((size_t)n_intron + 2, zero);
		const AlnStatsOut o = aln_stats_core<StatsSerial>(J, p, g_tab, (const uint8_t*)prot.c_str(), cigar.data(), g, feat.data());
		compare(name, "team of one", w, o, feat);
	}
	if (g_wave || strstr(name, "stop") || strstr(name, "N codon")) {
		std::vector<AlnFeat> feat((size_t)n_intron + 2, zero);
		std::vector<AlnStatsOut> outs(64);
		std::vector<std::thread> th;
		for (int l = 0; l < 64; ++l)
			th.emplace_back([&, l] { tl_lane = l; outs[(size_t)l] = aln_stats_core<StatsThreads>(J, p, g_tab, (const uint8_t*)prot.c_str(), cigar.data(), g, feat.data()); });
		for (auto &t : th) t.join();
		for (int l = 0; l < 64; ++l) compare(name, "team of 64", w, outs[(size_t)l], feat);
	}
	++g_cases;
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
	// contig 0: 700 bases, contig 1: 641 (an odd length and an odd offset: both nibbles, both strands); 3 % N
	Genome G;
	G.off[0] = 0, G.len[0] = 700, G.off[1] = 701, G.len[1] = 641;
	const int64_t total = G.off[1] + G.len[1];
	std::vector<uint8_t> flat((size_t)total);
	for (auto &b : flat) b = rnd(100) < 3 ? 4 : (uint8_t)rnd(4);
	// a stop codon (TAA) on the forward strand of contig 0 at 230..232, in frame with the walks that start at 50; an M codon (ATG) at 35
	flat[230] = 3, flat[231] = 0, flat[232] = 0;
	flat[35] = 0, flat[36] = 3, flat[37] = 2;
	// a codon with N under the walks that start at 50
	flat[62] = 4;
	G.packed.assign((size_t)(total + 1) / 2 + 16, 0);
	for (int64_t i = 0; i < total; ++i) G.packed[(size_t)(i >> 1)] |= (uint8_t)(flat[(size_t)i] << ((i & 1) * 4));
	for (int c = 0; c < 2; ++c) {
		G.strand[2 * c].assign(flat.begin() + G.off[c], flat.begin() + G.off[c] + G.len[c]);
		std::vector<uint8_t> &r = G.strand[2 * c + 1];
		r.resize((size_t)G.len[c]);
		for (int64_t i = 0; i < G.len[c]; ++i) { const uint8_t b = flat[(size_t)(G.off[c] + G.len[c] - 1 - i)]; r[(size_t)i] = b < 4 ? 3 - b : b; }
	}
	g_gen = &G;

	// every case on both strands of both contigs; the window is 600 bases: [20, 620)
	for (int vid = 0; vid < 4; ++vid) {
		const int64_t as = 20, ae = 620, vs = 50;
		g_wave = vid == 3;                                       // (contig 1, reverse strand; the cases that lean on what contig 0 holds run it there too)
		char nm[96];
		for (int32_t n : { 1, 63, 64, 65, 129 }) { snprintf(nm, sizeof nm, "M%d vid %d", n, vid); run_case(nm, vid, as, ae, vs, 3, 2, { op('M', n) }); }
		run_case("U first", vid, as, ae, vs, 0, 1, { op('U', 80), op('M', 20) });
		run_case("V first", vid, as, ae, vs, 0, 1, { op('V', 80), op('M', 20) });
		run_case("U last", vid, as, ae, vs, 2, 0, { op('M', 20), op('U', 75) });
		run_case("V last", vid, as, ae, vs, 2, 0, { op('M', 20), op('V', 75) });
		run_case("N first and last", vid, as, ae, vs, 2, 0, { op('N', 70), op('M', 9), op('N', 71) });
		run_case("U V back to back", vid, as, ae, vs, 1, 4, { op('M', 10), op('U', 70), op('V', 90), op('M', 12) });
		run_case("V U N back to back", vid, as, ae, vs, 1, 4, { op('M', 10), op('V', 70), op('U', 90), op('N', 72), op('M', 70) });
		run_case("F1 F2 G", vid, as, ae, vs, 0, 3, { op('M', 7), op('F', 1), op('M', 5), op('F', 2), op('M', 66), op('G', 1), op('M', 3), op('G', 2), op('M', 4) });
		run_case("D across a stop", vid, as, ae, vs, 0, 3, { op('M', 55), op('D', 9), op('M', 30) });   // (forward strand of contig 0: TAA at 230 = codon 60)
		run_case("I and D", vid, as, ae, vs, 0, 3, { op('M', 5), op('I', 70), op('M', 5), op('D', 66), op('M', 5) });
		{
			std::vector<uint32_t> c;                             // 70 operations: more than one round of 64 words
			for (int k = 0; k < 14; ++k) c.push_back(op('M', 2 + k % 3)), c.push_back(op('I', 1)), c.push_back(op('D', 1)), c.push_back(op("NUV"[k % 3], 6 + k)), c.push_back(op('M', 1));
			run_case("70 operations", vid, as, ae, vs, 5, 5, c);
			c.insert(c.end(), c.begin(), c.end());
			c.resize(100);
			run_case("100 operations", vid, 0, G.len[vid >> 1], 21, 5, 5, c);
		}
		run_case("N codon", vid, as, ae, vs, 0, 0, { op('M', 3), op('U', 30), op('M', 3) });   // (contig 0 forward: base 62 is N, inside codon 4 of the walk: the split codon)
		// windows that start at vs and end at ve + 1 (the donor of a last intron: one base, then '.'), at ve, and at the contig's end
		run_case("window = [vs, ve + 1)", vid, vs, vs + 3 * 20 + 75 + 1, vs, 0, 0, { op('M', 20), op('U', 75) });
		run_case("window = [vs, ve)", vid, vs, vs + 3 * 20 + 75, vs, 0, 0, { op('M', 20), op('V', 75) });
		run_case("window ends with the contig", vid, 300, G.len[vid >> 1], G.len[vid >> 1] - 3 * 40 - 1, 0, 0, { op('M', 40) });
		run_case("vs = as = 0", vid, 0, 600, 0, 0, 2, { op('N', 64), op('M', 64), op('U', 64) });
		// the scans: a start far from the window's start (more than 64 codons back), ends far from a stop
		run_case("late start", vid, as, ae, 590, 0, 0, { op('M', 4) });
		run_case("late start, frame 1", vid, as, ae, 588, 0, 0, { op('M', 4) });
		run_case("late start, frame 2", vid, 21, ae, 589, 0, 0, { op('M', 4) });
		// qe == qlen with a stop codon right behind ve (contig 0 forward: TAA at 230): the stop-codon feature
		run_case("stop feature", vid, as, ae, vs, 4, 0, { op('M', 60) }, "");
		run_case("stop feature behind an intron", vid, as, ae, 230 - 3 * 20 - 71, 4, 0, { op('M', 10), op('V', 71), op('M', 10) });
	}
	// random CIGARs
	for (int it = 0; it < 300; ++it) {
		std::vector<uint32_t> c;
		const int n = 1 + (int)rnd(it % 10 == 0 ? 90 : 12);
		int64_t nl = 0;
		for (int k = 0; k < n && nl < 420; ++k) {
			const char o = "MMMMIDNUVFG"[rnd(11)];
			int32_t len = o == 'M' ? 1 + (int32_t)rnd(it % 7 == 0 ? 70 : 9) : o == 'I' || o == 'D' ? 1 + (int32_t)rnd(4) : o == 'F' || o == 'G' ? 1 + (int32_t)rnd(2) : 4 + (int32_t)rnd(40);
			c.push_back(op(o, len));
			nl += o == 'M' || o == 'D' ? 3 * len : o == 'I' ? 0 : len;
		}
		const int vid = (int)rnd(4);
		const int64_t vs = 20 + rnd(60), ve = vs + nl;
		const int64_t as = rnd(2) ? vs : 20 - (int64_t)rnd(21), ae = rnd(3) == 0 ? ve + rnd(3) : 620;
		char nm[64];
		snprintf(nm, sizeof nm, "random %d", it);
		g_wave = it % 20 == 0;
		run_case(nm, vid, as, ae > G.len[vid >> 1] ? G.len[vid >> 1] : ae, vs, (int32_t)rnd(5), (int32_t)rnd(2), c);
	}
	printf("alnstats_check: %d cases, %d mismatches\n", g_cases, g_fail);
	return g_fail ? 1 : 0;
}
