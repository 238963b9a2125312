// alncs_check.cpp -- a stand-alone check of miniprot_amd/csrc/aln_cs_core.h (tests/test_aln_cs_cpu.py compiles it with
// -fsanitize=address,undefined and runs it).  Hand-written CIGARs over a small two-contig genome go through the shared core twice --
// with a team of one (StatsSerial, what MPA_GPU_CS=model runs) and with a team of 64 host threads that meet at a barrier for every
// ballot, scan and broadcast (the device's wavefront in slow motion) -- and both bodies are compared with a plain sequential walk
// over the unpacked strand written here after mp_write_cs (format.c:102-187).  The two slots of a case sit back to back, sized by
// aln_cs_bound(), with guard bytes in front, between and behind: after every case the guards are intact and length <= bound.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <functional>
#include <string>
#include <thread>
#include <vector>
#include <pthread.h>
#include "aln_cs_core.h"

using namespace mpa;

// ---- a team of 64 threads ---------------------------------------------------------------------------
static pthread_barrier_t g_bar;
static uint64_t g_slot[64];
static thread_local int tl_lane = 0;
struct CsThreads {
	static int lane() { return tl_lane; }
	static int width() { return 64; }
	static uint64_t ballot(bool p)
	{
		g_slot[tl_lane] = p;
		pthread_barrier_wait(&g_bar);
		uint64_t m = 0;
		for (int i = 0; i < 64; ++i) m |= (uint64_t)(g_slot[i] & 1) << i;
		pthread_barrier_wait(&g_bar);
		return m;
	}
	static uint32_t bcast(uint32_t v, int k)
	{
		g_slot[tl_lane] = v;
		pthread_barrier_wait(&g_bar);
		const uint32_t r = (uint32_t)g_slot[k];
		pthread_barrier_wait(&g_bar);
		return r;
	}
	static int32_t scan32(int32_t v, int32_t *total)
	{
		g_slot[tl_lane] = (uint32_t)v;
		pthread_barrier_wait(&g_bar);
		int32_t below = 0, all = 0;
		for (int i = 0; i < 64; ++i) { if (i < tl_lane) below += (int32_t)g_slot[i]; all += (int32_t)g_slot[i]; }
		pthread_barrier_wait(&g_bar);
		*total = all;
		return below;
	}
};

// ---- tables and genome ------------------------------------------------------------------------------
static const char *kAA20 = "ARNDCQEGHILKMFPSTWYV*X";
static const char *kCode = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF";   // codon = b0 << 4 | b1 << 2 | b2 over A0 C1 G2 T3
static uint8_t g_tab[ALN_TAB_BYTES];
static void make_tables()
{
	memset(g_tab, 0, sizeof(g_tab));
	for (int c = 0; c < 256; ++c) g_tab[ALN_TAB_AA20 + c] = 21;
	for (int i = 0; i < 22; ++i) g_tab[ALN_TAB_AA20 + (uint8_t)kAA20[i]] = (uint8_t)i, g_tab[ALN_TAB_AA20 + (uint8_t)(kAA20[i] | 0x20)] = (uint8_t)i;
	for (int c = 0; c < 64; ++c) g_tab[ALN_TAB_CODON + c] = g_tab[ALN_TAB_AA20 + (uint8_t)kCode[c]];
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

// ---- the plain walk (format.c:102-187) ----------------------------------------------------------------
static uint8_t plain_aa(const uint8_t *nt) { return nt[0] > 3 || nt[1] > 3 || nt[2] > 3 ? 21 : g_tab[ALN_TAB_CODON + (nt[0] << 4 | nt[1] << 2 | nt[2])]; }
static char plain_up(char c) { return c >= 'a' && c <= 'z' ? (char)(c - 'a' + 'A') : c; }
static std::string plain(const std::vector<uint8_t> &strand, int64_t vs, const char *aa, const std::vector<uint32_t> &cigar)
{
	const uint8_t *nt = strand.data() + vs;
	const char *lc = "acgtn";
	std::string s;
	char num[16];
	int64_t nl = 0;
	int32_t al = 0;
	for (uint32_t c : cigar) {
		const int32_t op = c & 0xf, len = (int32_t)(c >> 4);
		if (op == 0) {
			int32_t run = 0;
			for (int32_t l = 0; l < len; ++l, nl += 3, ++al) {
				if (plain_aa(nt + nl) == g_tab[ALN_TAB_AA20 + (uint8_t)aa[al]]) { ++run; continue; }
				if (run) snprintf(num, sizeof num, ":%d", run), s += num;
				run = 0;
				s += '*', s += lc[nt[nl]], s += lc[nt[nl + 1]], s += lc[nt[nl + 2]], s += plain_up(aa[al]);
			}
			if (run) snprintf(num, sizeof num, ":%d", run), s += num;
		} else if (op == 1) {
			s += '+';
			for (int32_t l = 0; l < len; ++l) s += plain_up(aa[al++]);
		} else if (op == 2 || op == 10) {
			s += '-';
			for (int32_t i = 0, n = op == 2 ? 3 * len : len; i < n; ++i) s += lc[nt[nl++]];
		} else if (op == 11) {
			s += '*';
			for (int32_t i = 0; i < len; ++i) s += lc[nt[nl++]];
			s += plain_up(aa[al++]);
		} else if (op == 3 || op == 12 || op == 13) {
			const int32_t head = op == 3 ? 0 : op == 12 ? 1 : 2, tail = head ? 3 - head : 0;
			const uint8_t *in = nt + nl + head, *end = nt + nl + len - tail;   // the intron proper: [in, end)
			if (head) {
				s += '*';
				for (int32_t i = 0; i < head; ++i) s += lc[nt[nl + i]];
				s += plain_up(aa[al++]);
			}
			snprintf(num, sizeof num, "%d", len - head - tail);
			s += '~', s += lc[in[0]], s += lc[in[1]], s += num, s += lc[end[-2]], s += lc[end[-1]];
			if (tail) {
				s += '-';
				for (int32_t i = 0; i < tail; ++i) s += lc[end[i]];
			}
			nl += len;
		}
	}
	return s;
}

// ---- one case -----------------------------------------------------------------------------------------
static int g_fail = 0, g_cases = 0;
static const Genome *g_gen;
static bool g_wave = true;                                  // the team of 64 threads too
static const int kGuard = 16;
typedef std::function<bool(int, int32_t, int32_t)> Pattern;   // (M operation number, codon, codons of the operation) -> a mismatch there?

static void fail(const char *name, const char *team, const std::string &want, const char *got, int32_t len)
{
	++g_fail;
	fprintf(stderr, "MISMATCH %s (%s): want %zu bytes, got %d\n  want %.200s\n  got  %.*s\n", name, team, want.size(), len, want.c_str(), len < 200 ? (len < 0 ? 0 : len) : 200, got);
}

static void run_case(const char *name, int vid, int64_t vs, int32_t qs, int32_t tail, const std::vector<uint32_t> &cigar, const Pattern &pat, bool lower = false,
                     bool expect_exact_bound = false)
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
					// (a mismatch: one of the 20 amino acids other than t -- any of them when the codon is a stop or holds an N)
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
	const std::string want = plain(strand, vs, prot.c_str() + qs, cigar);
	const int64_t bound = aln_cs_bound(cigar.data(), (int32_t)cigar.size());
	if ((int64_t)want.size() > bound || (expect_exact_bound && (int64_t)want.size() != bound)) {
		fprintf(stderr, "BOUND %s: the body has %zu bytes, the bound is %lld\n", name, want.size(), (long long)bound);
		++g_fail;
	}
	const PackedReader g{ g_gen->packed.data(), g_gen->off[vid >> 1], g_gen->len[vid >> 1], vid & 1 };
	// guard | slot of the team of one | guard | slot of the team of 64 | guard
	std::vector<char> buf((size_t)(3 * kGuard + 2 * bound));
	for (size_t i = 0; i < buf.size(); ++i) buf[i] = (char)(0xA5 ^ (i * 7));
	const std::vector<char> before = buf;
	char *slot_a = buf.data() + kGuard, *slot_b = slot_a + bound + kGuard;
	{
		const AlnCsOut o = aln_cs_core<StatsSerial>(J, g_tab, (const uint8_t*)prot.c_str(), cigar.data(), g, slot_a);
		if (o.bad || o.len > bound || o.len != (int32_t)want.size() || memcmp(slot_a, want.data(), want.size())) fail(name, "team of one", want, slot_a, o.len);
	}
	if (g_wave) {
		std::vector<AlnCsOut> outs(64);
		std::vector<std::thread> th;
		for (int l = 0; l < 64; ++l)
			th.emplace_back([&, l] { tl_lane = l; outs[(size_t)l] = aln_cs_core<CsThreads>(J, g_tab, (const uint8_t*)prot.c_str(), cigar.data(), g, slot_b); });
		for (auto &t : th) t.join();
		bool ok = true;
		for (int l = 0; l < 64; ++l) ok = ok && !outs[(size_t)l].bad && outs[(size_t)l].len == (int32_t)want.size();
		if (!ok || memcmp(slot_b, want.data(), want.size())) fail(name, "team of 64", want, slot_b, outs[0].len);
	}
	// the guards, and what lies behind each body inside its slot, are as they were
	auto untouched = [&](size_t from, size_t to) { return from >= to || !memcmp(buf.data() + from, before.data() + from, to - from); };
	const size_t a0 = (size_t)kGuard, b0 = (size_t)(2 * kGuard + bound);
	if (!untouched(0, a0) || !untouched(a0 + want.size(), b0) || !untouched(g_wave ? b0 + want.size() : b0, buf.size())) {
		fprintf(stderr, "GUARD %s: bytes outside the body were written\n", name);
		++g_fail;
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
	// contig 0: 1 300 000 bases without N but for a few planted ones; contig 1: 30 001 bases (an odd length behind an odd offset: both
	// nibbles, both strands) with 3 % N
	Genome G;
	G.off[0] = 0, G.len[0] = 1300000, G.off[1] = 1300001, G.len[1] = 30001;
	const int64_t total = G.off[1] + G.len[1];
	std::vector<uint8_t> flat((size_t)total);
	for (int64_t i = 0; i < total; ++i) flat[(size_t)i] = i >= G.off[1] && rnd(100) < 3 ? 4 : (uint8_t)rnd(4);
	for (int64_t x : { 62, 63, 110, 402, 1299000 }) flat[(size_t)x] = 4;     // (contig 0: codons with N under the walks that start at 50)
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
		for (int32_t n : { 1, 63, 64, 65, 129, 1000 }) {
			snprintf(nm, sizeof nm, "M%d all match, vid %d", n, vid), run_case(nm, vid, vs, 3, 2, { op('M', n) }, all_match);
			snprintf(nm, sizeof nm, "M%d all mismatch, vid %d", n, vid), run_case(nm, vid, vs, 3, 2, { op('M', n) }, all_mism, false, true);   // (length = the bound: the last byte of the slot is written)
			snprintf(nm, sizeof nm, "M%d alternating, vid %d", n, vid), run_case(nm, vid, vs, 3, 2, { op('M', n) }, alternating);
			for (int32_t at : { 0, 63, 64, n - 1 }) {
				if (at >= n) continue;
				snprintf(nm, sizeof nm, "M%d one mismatch at %d, vid %d", n, at, vid);
				run_case(nm, vid, vs, 3, 2, { op('M', n) }, [at](int, int32_t l, int32_t) { return l == at; });
			}
		}
		// match runs of 9, 10, 99, 100 and 1 000 (the digit count changes) in front of, between and behind mismatches
		for (int32_t r : { 9, 10, 99, 100, 1000 }) {
			snprintf(nm, sizeof nm, "run of %d between mismatches, vid %d", r, vid);
			run_case(nm, vid, vs, 0, 0, { op('M', r + 2) }, [r](int, int32_t l, int32_t) { return l == 0 || l == r + 1; });
			snprintf(nm, sizeof nm, "runs of %d, vid %d", r, vid);
			run_case(nm, vid, vs, 0, 0, { op('M', 2 * r + 1) }, [r](int, int32_t l, int32_t) { return l == r; });
		}
		// a match run that spans three steps: mismatches at 60 and 60 + 140 only
		run_case("run over three steps", vid, vs, 1, 1, { op('M', 260) }, [](int, int32_t l, int32_t) { return l == 60 || l == 200; });
		// two M operations back to back: the run must not carry over (":70:30", not ":100")
		run_case("M M back to back", vid, vs, 1, 1, { op('M', 70), op('M', 30) }, all_match);
		run_case("M M M back to back, mismatches at the seams", vid, vs, 1, 1, { op('M', 64), op('M', 64), op('M', 65) }, [](int, int32_t l, int32_t n) { return l == n - 1; });
		run_case("I1 I2 D1 D2 F1 F2 G1 G2", vid, vs, 0, 3,
		         { op('M', 7), op('I', 1), op('M', 5), op('I', 2), op('M', 3), op('D', 1), op('M', 2), op('D', 2), op('M', 4), op('F', 1), op('M', 5), op('F', 2), op('M', 66), op('G', 1), op('M', 3), op('G', 2), op('M', 4) }, noise);
		run_case("long I and D", vid, vs, 0, 3, { op('M', 5), op('I', 70), op('M', 5), op('D', 66), op('M', 5), op('I', 130) }, noise);
		run_case("I first, D last", vid, vs, 0, 0, { op('I', 3), op('M', 5), op('D', 3) }, noise);
		// introns first, last and back to back
		run_case("N first and last", vid, vs, 2, 0, { op('N', 70), op('M', 9), op('N', 71) }, noise);
		run_case("U first", vid, vs, 0, 1, { op('U', 80), op('M', 20) }, noise);
		run_case("V first", vid, vs, 0, 1, { op('V', 80), op('M', 20) }, noise);
		run_case("U last", vid, vs, 2, 0, { op('M', 20), op('U', 75) }, noise);
		run_case("V last", vid, vs, 2, 0, { op('M', 20), op('V', 75) }, noise);
		run_case("U V back to back", vid, vs, 1, 4, { op('M', 10), op('U', 70), op('V', 90), op('M', 12) }, noise);
		run_case("V U N N back to back", vid, vs, 1, 4, { op('M', 10), op('V', 70), op('U', 90), op('N', 72), op('N', 5), op('M', 70) }, noise);
		// intron lengths of 1 to 7 digits (the printed number is len for N, len - 3 for U and V); contig 1 holds up to five
		for (int32_t digits = 1; digits <= (vid < 2 ? 7 : 5); ++digits) {
			int32_t lo = 1;
			for (int d = 1; d < digits; ++d) lo *= 10;
			const int32_t hi = lo * 10 - 1 > 1200000 ? 1200000 : lo * 10 - 1;
			for (int32_t printed : { lo, hi }) {
				if (printed > (vid < 2 ? 1200000 : 25000)) continue;
				snprintf(nm, sizeof nm, "N of %d, vid %d", printed, vid), run_case(nm, vid, vs, 0, 0, { op('M', 3), op('N', printed), op('M', 3) }, noise);
				snprintf(nm, sizeof nm, "U of %d, vid %d", printed, vid), run_case(nm, vid, vs, 0, 0, { op('M', 3), op('U', printed + 3), op('M', 3) }, noise);
				snprintf(nm, sizeof nm, "V of %d, vid %d", printed, vid), run_case(nm, vid, vs, 0, 0, { op('M', 3), op('V', printed + 3), op('M', 3) }, noise);
			}
		}
		{
			std::vector<uint32_t> c;                             // 70 words: more than one round of 64
			for (int k = 0; k < 14; ++k) c.push_back(op('M', 2 + k % 3)), c.push_back(op('I', 1)), c.push_back(op('D', 1)), c.push_back(op("NUV"[k % 3], 6 + k)), c.push_back(op('M', 1));
			run_case("70 words", vid, vs, 5, 5, c, noise);
			c.insert(c.end(), c.begin(), c.end());
			c.resize(100);
			run_case("100 words", vid, 21, 5, 5, c, noise);
		}
		// codons with N: under an M (contig 0 forward: 62, 63 and 110 are N), inside a split codon, among deleted and frameshift bases
		run_case("N codons under M", vid, vs, 0, 0, { op('M', 30) }, all_match);
		run_case("N codons under M, mismatching", vid, vs, 0, 0, { op('M', 30) }, all_mism);
		run_case("N in a split codon", vid, vs, 0, 0, { op('M', 4), op('U', 30), op('M', 3) }, noise);
		run_case("N among D, F and G bases", vid, 59, 0, 0, { op('D', 2), op('M', 1), op('F', 2), op('M', 14), op('G', 2), op('M', 2) }, noise);
		// a lower-case query: residues print in upper case, matching is case-blind
		run_case("lower-case query", vid, vs, 2, 2, { op('M', 70), op('I', 3), op('M', 10), op('V', 50), op('G', 1), op('M', 5) }, alternating, true);
		// the ends of the strand
		run_case("from the first base", vid, 0, 0, 0, { op('N', 64), op('M', 64), op('U', 64) }, noise);
		run_case("to the last base", vid, (int64_t)G.strand[vid].size() - 3 * 40 - 60, 0, 0, { op('M', 20), op('V', 60), op('M', 20) }, noise);
	}
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
		run_case(nm, vid, 20 + rnd(60), (int32_t)rnd(5), (int32_t)rnd(2), c, [percent](int, int32_t, int32_t) { return (int)rnd(100) < percent; }, it % 13 == 0);
	}
	printf("alncs_check: %d cases, %d mismatches\n", g_cases, g_fail);
	return g_fail ? 1 : 0;
}
