// spans_check.cpp -- a stand-alone check of miniprot_amd/csrc/spans_core.h (tests/test_spans_cpu.py compiles it with
// -fsanitize=address,undefined and runs it).  Hand-written and random plans over a small genome go through the shared core twice --
// with a team of one (SpansSerial, what MPA_GPU_SPANS=model runs) and with a team of 64 host threads that meet at a barrier for every
// sync, sum, scan and broadcast (the device's wavefront in slow motion) -- and are compared, field by field and word by word, with
// plain restatements of the host functions on std::vector, written here after host_align.cpp and host_plan.cpp (take_round1_emit_round2,
// store_result; make_segment, ungapped_score; assemble_alignment, append_cigar, count_exons).  Every output slot is a heap block of exactly the
// plan's size, so a word written past it is AddressSanitizer's to report.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>
#include <pthread.h>
#include "spans_core.h"

using namespace mpa;

// ---- a team of 64 threads ---------------------------------------------------------------------------
static pthread_barrier_t g_bar;
static int64_t g_slot[64];
static thread_local int tl_lane = 0;
struct SpansThreads {
	static int lane() { return tl_lane; }
	static int width() { return 64; }
	static void sync() { pthread_barrier_wait(&g_bar); }
	template<class F> static auto all(int64_t v, F f) -> decltype(f())
	{
		g_slot[tl_lane] = v;
		pthread_barrier_wait(&g_bar);
		auto r = f();
		pthread_barrier_wait(&g_bar);
		return r;
	}
	static int32_t sum(int32_t v) { return all(v, [] { uint32_t s = 0; for (int i = 0; i < 64; ++i) s += (uint32_t)g_slot[i]; return (int32_t)s; }); }
	static uint32_t bcast(uint32_t v, int k) { return all(v, [k] { return (uint32_t)g_slot[k]; }); }
	static int64_t scan_excl(int64_t v, int64_t *total)
	{
		int64_t t = 0;
		const int64_t below = all(v, [&t] { int64_t s = 0, b = 0; for (int i = 0; i < 64; ++i) { if (i == tl_lane) b = s; s += g_slot[i]; } t = s; return b; });
		*total = t;
		return below;
	}
	static int64_t scan_max_excl(int64_t v, int64_t *total)
	{
		int64_t t = 0;
		const int64_t below = all(v, [&t] { int64_t m = INT64_MIN, b = INT64_MIN; for (int i = 0; i < 64; ++i) { if (i == tl_lane) b = m; m = std::max(m, g_slot[i]); } t = m; return b; });
		*total = t;
		return below;
	}
};

static uint64_t g_rng = 88172645463325252ULL;
static uint64_t rnd(uint64_t n) { g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17; return g_rng % n; }
static int g_fail = 0, g_cases = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "CASE DOES NOT SHOW WHAT IT IS FOR: %s (line %d)\n", #cond, __LINE__); ++g_fail; } } while (0)

// ---- the genome, the tables ---------------------------------------------------------------------------
static const int64_t kCtgLen[2] = { 9000, 5000 };
static int64_t g_ctg_off[2];
static std::vector<uint8_t> g_fwd;                        // nt4 codes of the forward strands, contig after contig
static uint8_t g_tab[ALN_TAB_BYTES];
struct StrandReader {                                     // what the core reads the genome through
	int64_t off, len;
	int rev;
	uint32_t base(int64_t x) const
	{
		if (x < 0 || x >= len) return 4;
		const uint8_t c = rev ? g_fwd[(size_t)(off + len - 1 - x)] : g_fwd[(size_t)(off + x)];
		return rev && c < 4 ? 3u - c : c;
	}
};
// the plain side's fetch (mp_ntseq_get_by_v, ntseq.c:108-114): the strand written out, then indexed
static std::vector<uint8_t> plain_strand(uint32_t vid)
{
	const int64_t off = g_ctg_off[vid >> 1], len = kCtgLen[vid >> 1];
	std::vector<uint8_t> s(g_fwd.begin() + off, g_fwd.begin() + off + len);
	if (vid & 1) {
		std::reverse(s.begin(), s.end());
		for (uint8_t &c : s) if (c < 4) c = (uint8_t)(3 - c);
	}
	return s;
}
static void make_world()
{
	int64_t o = 0;
	for (int c = 0; c < 2; ++c) g_ctg_off[c] = o, o += kCtgLen[c];
	g_fwd.resize((size_t)o);
	for (uint8_t &b : g_fwd) b = rnd(40) == 0 ? 4 : (uint8_t)rnd(4);
	const char *codon = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF", *aa = "ARNDCQEGHILKMFPSTWYV*X";
	memset(g_tab, 21, sizeof g_tab);
	for (int i = 0; i < 22; ++i) g_tab[ALN_TAB_AA20 + (uint8_t)aa[i]] = (uint8_t)i;
	for (int i = 0; i < 64; ++i) g_tab[ALN_TAB_CODON + i] = g_tab[ALN_TAB_AA20 + (uint8_t)codon[i]];
	for (int i = 0; i < 484; ++i) g_tab[ALN_TAB_MAT + i] = (uint8_t)(int8_t)((int)rnd(14) - 4);
}

// ---- a case: one plan, its round-1 results, and the words its DP segments come back with ---------------------------------------
typedef std::vector<uint32_t> Words;
static uint32_t W(uint32_t op, uint32_t len) { return len << 4 | op; }
struct Gap { int32_t nlen, alen; Words words; int32_t score; };          // words empty and the shortcut's shape: the shortcut
struct Case {
	uint32_t vid = 0;
	int32_t qlen = 400, as1 = 100, mid_qe = 0, has_right = 1, retry = 1, base1 = 3;
	int64_t vs0 = 3000, ae = 8000;
	int32_t l[2][2] = { { 0, 0 }, { 0, 0 } }, r[2][2] = { { 0, 0 }, { 0, 0 } };   // {nt_len, aa_len} of the first call and of the repeat
	std::vector<Gap> gaps;
	Words left_words = { W(0, 1) }, right_words = { W(0, 1) };               // what a span's DP call returns
	int32_t left_score = 11, right_score = 13;
	std::string prot;
};
static SpansParams params() { return SpansParams{ 5, 1000, 29, 22 }; }

struct Built {                                           // the case as both sides read it
	SpansPlan P;
	std::vector<SegRec> seg;
	std::vector<mpa_dp_rst_t> rst1;
	Words pool1;
};
static Built build(const SpansParams &p, const Case &c)
{
	Built b;
	PlanRec &pl = b.P.pl;
	memset(&b.P, 0, sizeof b.P);
	b.rst1.assign((size_t)c.base1, mpa_dp_rst_t{ 77, 77, 77, 0, 0 });                  // (another query's results before this one's)
	auto push = [&](int32_t nt, int32_t aa) { b.rst1.push_back(mpa_dp_rst_t{ nt, aa, 5, 0, 0 }); return (int32_t)b.rst1.size() - 1 - c.base1; };
	pl.reg = 0, pl.as = 0, pl.ae = c.ae, pl.vs0 = c.vs0, pl.as1 = c.as1, pl.vs1 = c.vs0 + 600, pl.has_right = c.has_right;
	pl.t_left2 = pl.t_right = pl.t_right2 = -1;
	pl.t_left = push(c.l[0][0], c.l[0][1]);
	if (c.retry) pl.t_left2 = push(c.l[1][0], c.l[1][1]);
	if (c.has_right) { pl.t_right = push(c.r[0][0], c.r[0][1]); if (c.retry) pl.t_right2 = push(c.r[1][0], c.r[1][1]); }
	pl.gap0 = 2, pl.n_gap = (int32_t)c.gaps.size();
	b.seg.assign(2, SegRec{ 9, 9, 9, 9, 9, 9 });                                         // (another plan's segments before this one's)
	int32_t ne = 600, ae = c.as1;
	b.pool1.assign(5, 0xdeadu);
	for (const Gap &g : c.gaps) {
		SegRec s{ ne, ne + g.nlen, ae, ae + g.alen, -1, 0 };
		if (g.nlen == g.alen * 3 && g.alen <= p.kmer2 && g.words.empty()) s.score = g.score;
		else {
			b.rst1.push_back(mpa_dp_rst_t{ g.nlen, g.alen, g.score, (int32_t)g.words.size(), (int64_t)b.pool1.size() });
			s.task = (int32_t)b.rst1.size() - 1 - c.base1;
			b.pool1.insert(b.pool1.end(), g.words.begin(), g.words.end());
		}
		b.seg.push_back(s);
		ne += g.nlen, ae += g.alen;
	}
	pl.mid_ve = c.vs0 + ne, pl.mid_qe = c.mid_qe ? c.mid_qe : ae;
	b.P.q_off = 17, b.P.qid = 4, b.P.qlen = c.qlen, b.P.vid = c.vid, b.P.base1 = c.base1;
	return b;
}

// ---- the plain side ---------------------------------------------------------------------------------------
struct PlainSeg { int32_t ne0, ne1, ae0, ae1, task = -1, score = 0; Words cigar; };
struct Plain {
	int32_t l_nt = 0, l_aa = 0, r_nt = 0, r_aa = 0, qs = 0, qe = 0, dp_score = 0, n_exon = 0;
	int64_t vs = 0, ve = 0;
	bool has_right_span = false, l_rep = false, r_rep = false;
	PlainSeg left, right;
	std::vector<mpa_dp_task_t> tasks;
	Words cigar;
};
static int32_t plain_ungapped(uint32_t vid, int64_t nt_off, int32_t alen, const char *aa)
{
	const std::vector<uint8_t> s = plain_strand(vid);
	int32_t sc = 0;
	for (int32_t i = 0, j = 0; i < alen; i += 3, ++j) {
		uint8_t nt[3];
		for (int k = 0; k < 3; ++k) { const int64_t x = nt_off + i + k; nt[k] = x >= 0 && x < (int64_t)s.size() ? s[(size_t)x] : 4; }
		const uint32_t a = nt[0] > 3 || nt[1] > 3 || nt[2] > 3 ? 21u : g_tab[ALN_TAB_CODON + (nt[0] << 4 | nt[1] << 2 | nt[2])];
		sc += (int8_t)g_tab[ALN_TAB_MAT + a * 22 + g_tab[ALN_TAB_AA20 + (uint8_t)aa[j]]];
	}
	return sc;
}
static void plain_segment(const SpansParams &p, const Built &b, const std::string &text, int32_t ne0, int32_t ne1, int32_t ae0, int32_t ae1, std::vector<mpa_dp_task_t> &tasks, PlainSeg &s)
{
	s.ne0 = ne0, s.ne1 = ne1, s.ae0 = ae0, s.ae1 = ae1;
	const int32_t nlen = ne1 - ne0, alen = ae1 - ae0;
	if (nlen == alen * 3 && alen <= p.kmer2) {
		s.task = -1, s.score = plain_ungapped(b.P.vid, b.P.pl.vs0 + ne0, alen, text.data() + b.P.q_off + ae0), s.cigar.assign(1, (uint32_t)alen << 4);
	} else {
		s.task = (int32_t)tasks.size();
		mpa_dp_task_t t;
		t.nt_off = b.P.pl.vs0 + ne0, t.vid = (int32_t)b.P.vid, t.nl = nlen, t.qid = b.P.qid, t.aa_off = ae0, t.al = alen, t.flag = MPA_F_CIGAR, t.io = p.io, t.tag = 0;
		tasks.push_back(t);
	}
}
static void plain_accept(const SpansParams &p, const Built &b, const std::string &text, int32_t task0, Plain &o)
{
	const PlanRec &pl = b.P.pl;
	const mpa_dp_rst_t *mine = b.rst1.data() + b.P.base1;
	o.tasks.assign((size_t)task0, mpa_dp_task_t());                              // (the tasks of the plans before this one)
	// (a call that consumed no row extended nothing, whatever its aa_len says: an extension call of fewer than three rows returns
	// (0, al + 1, INT32_MIN), include/mpamd.h)
	auto aa_of = [](const mpa_dp_rst_t &x) { return x.nt_len > 0 ? x.aa_len : 0; };
	o.l_nt = mine[pl.t_left].nt_len, o.l_aa = aa_of(mine[pl.t_left]);
	if (pl.t_left2 >= 0 && o.l_aa != pl.as1 && o.l_nt < p.max_ext && aa_of(mine[pl.t_left2]) == pl.as1) o.l_nt = mine[pl.t_left2].nt_len, o.l_aa = mine[pl.t_left2].aa_len, o.l_rep = true;
	if (pl.has_right) {
		o.r_nt = mine[pl.t_right].nt_len, o.r_aa = aa_of(mine[pl.t_right]);
		if (pl.t_right2 >= 0 && o.r_aa < b.P.qlen - pl.mid_qe && o.r_nt < p.max_ext && aa_of(mine[pl.t_right2]) == b.P.qlen - pl.mid_qe)
			o.r_nt = mine[pl.t_right2].nt_len, o.r_aa = mine[pl.t_right2].aa_len, o.r_rep = true;
	}
	o.vs = pl.vs1 - o.l_nt, o.qs = pl.as1 - o.l_aa;
	plain_segment(p, b, text, (int32_t)(o.vs - pl.vs0), (int32_t)(pl.vs1 - pl.vs0), o.qs, pl.as1, o.tasks, o.left);
	if (pl.has_right && o.r_nt > 0 && o.r_aa > 0) {
		const int32_t ne0 = (int32_t)(pl.mid_ve - pl.vs0);
		o.has_right_span = true;
		plain_segment(p, b, text, ne0, ne0 + o.r_nt, pl.mid_qe, pl.mid_qe + o.r_aa, o.tasks, o.right);
	}
}
static void plain_push(Words &cig, uint32_t op, int32_t len)
{
	if (!cig.empty() && (cig.back() & 0xf) == op && op != 10 && op != 11) cig.back() += (uint32_t)len << 4;
	else cig.push_back((uint32_t)len << 4 | op);
}
static void plain_assemble(const Built &b, const std::vector<mpa_dp_rst_t> &rst2, const Words &pool2, Plain &o)
{
	const PlanRec &pl = b.P.pl;
	auto store = [](PlainSeg &s, const mpa_dp_rst_t *rst, const Words &pool) {
		if (s.task < 0) return;
		s.score = rst[s.task].score, s.cigar.assign(pool.begin() + rst[s.task].cigar_off, pool.begin() + rst[s.task].cigar_off + rst[s.task].n_cigar);
	};
	store(o.left, rst2.data(), pool2);
	if (o.has_right_span) store(o.right, rst2.data(), pool2);
	int32_t score = 0;
	auto add = [&](const PlainSeg &s) { for (uint32_t c : s.cigar) plain_push(o.cigar, c & 0xf, (int32_t)(c >> 4)); score += s.score; };
	add(o.left);
	for (int32_t g = 0; g < pl.n_gap; ++g) {
		const SegRec &z = b.seg[(size_t)(pl.gap0 + g)];
		PlainSeg s;
		s.task = z.task, s.score = z.score;
		if (z.task < 0) s.cigar.assign(1, (uint32_t)(z.ae1 - z.ae0) << 4);
		store(s, b.rst1.data() + b.P.base1, b.pool1);
		add(s);
	}
	if (o.has_right_span) add(o.right);
	o.ve = pl.mid_ve, o.qe = pl.mid_qe;
	if (pl.has_right && o.r_nt > 0 && o.r_aa > 0) o.ve += o.r_nt, o.qe += o.r_aa;
	o.dp_score = score;
	int32_t n_intron = 0;
	for (uint32_t c : o.cigar) { const uint32_t op = c & 0xf; n_intron += (op == 3 || op == 12 || op == 13); }
	o.n_exon = n_intron + 1;
}

// ---- both sides of a case ---------------------------------------------------------------------------------
#define F(what, x, y) if ((int64_t)(x) != (int64_t)(y)) { fprintf(stderr, "MISMATCH %s (%s): " what " %lld, expected %lld\n", name, team, (long long)(x), (long long)(y)); ++g_fail; return w; }
static Plain run_case(const char *name, const SpansParams &p, const Case &c)
{
	const Built b = build(p, c);
	std::string text(17, 'W');
	text += c.prot.empty() ? std::string((size_t)c.qlen, 'A') : c.prot;
	const int32_t task0 = 6;
	Plain w;
	plain_accept(p, b, text, task0, w);
	// the round-2 results: the words the case gives its spans (behind other queries' words)
	std::vector<mpa_dp_rst_t> rst2((size_t)task0, mpa_dp_rst_t{ 1, 1, 1, 0, 0 });
	Words pool2(3, 0xbeefu);
	for (size_t k = (size_t)task0; k < w.tasks.size(); ++k) {
		const bool is_left = w.left.task == (int32_t)k;
		const Words &ww = is_left ? c.left_words : c.right_words;
		rst2.push_back(mpa_dp_rst_t{ w.tasks[k].nl, w.tasks[k].al, is_left ? c.left_score : c.right_score, (int32_t)ww.size(), (int64_t)pool2.size() });
		pool2.insert(pool2.end(), ww.begin(), ww.end());
	}
	plain_assemble(b, rst2, pool2, w);
	++g_cases;
	for (int pass = 0; pass < 2; ++pass) {
		const char *team = pass ? "team of 64" : "team of one";
		SpanRec R;
		mpa_dp_task_t t[2];
		const StrandReader g{ g_ctg_off[c.vid >> 1], kCtgLen[c.vid >> 1], (int)(c.vid & 1) };
		const int32_t n = spans_accept(p, b.P, b.rst1.data(), g, g_tab, (const uint8_t*)text.data(), R, t);
		if (R.left.task >= 0) R.left.task += task0;
		if (R.right.task >= 0) R.right.task += task0;
		F("tasks", n, (int64_t)w.tasks.size() - task0)
		F("l_nt", R.l_nt, w.l_nt) F("l_aa", R.l_aa, w.l_aa) F("r_nt", R.r_nt, w.r_nt) F("r_aa", R.r_aa, w.r_aa) F("vs", R.vs, w.vs) F("qs", R.qs, w.qs)
		F("flags", R.flags, SPANS_LEFT | (w.has_right_span ? SPANS_RIGHT : 0) | (w.l_rep ? SPANS_LREP : 0) | (w.r_rep ? SPANS_RREP : 0))
		for (int side = 0; side < 2; ++side) {
			if (side && !w.has_right_span) { F("right.task", R.right.task, -1) continue; }
			const SegRec &y = side ? R.right : R.left;
			const PlainSeg &x = side ? w.right : w.left;
			F("span ne0", y.ne0, x.ne0) F("span ne1", y.ne1, x.ne1) F("span ae0", y.ae0, x.ae0) F("span ae1", y.ae1, x.ae1) F("span task", y.task, x.task)
			if (x.task < 0) F("span score", y.score, x.score)
			if (x.task >= 0 && memcmp(&t[x.task - task0], &w.tasks[(size_t)x.task], sizeof(mpa_dp_task_t))) F("span task record", 0, 1)
		}
		int64_t slot = 0;
		for (int32_t s = 0; s < spans_n_seg(b.P, R); ++s) slot += spans_seg_words(b.P, R, b.seg.data(), b.rst1.data(), rst2.data(), s);
		uint32_t *out = (uint32_t*)malloc((size_t)(slot > 0 ? slot : 1) * 4);   // (exactly the slot: a word past it is the sanitizer's)
		AsmRec A;
		if (!pass) A = spans_assemble<SpansSerial>(b.P, R, b.seg.data(), b.rst1.data(), b.pool1.data(), rst2.data(), pool2.data(), out);
		else {
			std::vector<AsmRec> as(64);
			std::vector<std::thread> th;
			for (int l = 0; l < 64; ++l) th.emplace_back([&, l] { tl_lane = l; as[(size_t)l] = spans_assemble<SpansThreads>(b.P, R, b.seg.data(), b.rst1.data(), b.pool1.data(), rst2.data(), pool2.data(), out); });
			for (auto &x : th) x.join();
			A = as[0];
			for (int l = 1; l < 64; ++l) if (memcmp(&as[(size_t)l], &as[0], sizeof(AsmRec))) { fprintf(stderr, "MISMATCH %s: lane %d returns another record than lane 0\n", name, l); ++g_fail; }
		}
		Words got(out, out + (A.n_cigar >= 0 && A.n_cigar <= slot ? A.n_cigar : 0));
		free(out);
		F("bad", A.bad, 0) F("n_cigar", A.n_cigar, (int64_t)w.cigar.size()) F("ve", A.ve, w.ve) F("qe", A.qe, w.qe) F("dp_score", A.dp_score, w.dp_score) F("n_exon", A.n_exon, w.n_exon)
		F("n_merged", A.n_merged, slot - (int64_t)w.cigar.size())
		for (size_t i = 0; i < got.size(); ++i) if (got[i] != w.cigar[i]) { fprintf(stderr, "MISMATCH %s (%s): word %zu is %x, expected %x\n", name, team, i, got[i], w.cigar[i]); ++g_fail; return w; }
	}
	return w;
}
#undef F

// a DP segment's words as ns_push_cigar leaves them: no two mergeable neighbours
static Words random_words(int n)
{
	static const uint32_t ops[8] = { 0, 1, 2, 3, 10, 11, 12, 13 };
	Words w;
	while ((int)w.size() < n) {
		const uint32_t op = ops[rnd(8)];
		if (!w.empty() && (w.back() & 0xf) == op && op != 10 && op != 11) continue;
		w.push_back(W(op, 1 + (uint32_t)rnd(40)));
	}
	return w;
}
static Gap dp_gap(const Words &w, int32_t score = 7) { return Gap{ 40, 9, w, score }; }     // (9 residues: above kmer2)
static Gap short_gap(int32_t alen, int32_t score = 3) { return Gap{ 3 * alen, alen, Words(), score }; }

int main()
{
	pthread_barrier_init(&g_bar, nullptr, 64);
	make_world();
	const SpansParams P = params();
	{	// an empty left span (l_nt = l_aa = 0) followed by an M that merges into the zero-length word
		Case c;
		c.gaps.push_back(dp_gap({ W(0, 12), W(3, 80), W(0, 4) }));
		const Plain w = run_case("empty left span, then M", P, c);
		EXPECT(w.l_nt == 0 && w.left.task < 0 && w.left.score == 0 && w.cigar.size() == 3 && w.cigar[0] == W(0, 12) && !w.has_right_span);
	}
	{	// the repeat conditions at each threshold
		Case c;
		c.l[0][0] = P.max_ext - 1, c.l[0][1] = 60, c.l[1][0] = 500, c.l[1][1] = c.as1;
		Plain w = run_case("left repeat: l_nt == max_ext - 1", P, c);
		EXPECT(w.l_rep && w.l_nt == 500 && w.l_aa == c.as1);
		c.l[0][0] = P.max_ext;
		w = run_case("left repeat: l_nt == max_ext", P, c);
		EXPECT(!w.l_rep && w.l_nt == P.max_ext);
		c.l[0][0] = 300, c.l[0][1] = c.as1;
		w = run_case("left repeat: l_aa == as1", P, c);
		EXPECT(!w.l_rep && w.l_aa == c.as1);
		c.l[0][1] = 60, c.l[1][1] = c.as1 - 1;
		w = run_case("left repeat: one residue short", P, c);
		EXPECT(!w.l_rep && w.l_aa == 60);
		c.retry = 0;
		w = run_case("left repeat: none issued", P, c);
		EXPECT(!w.l_rep);
		Case d;
		d.gaps.push_back(dp_gap({ W(0, 9) }));
		const int32_t rest = d.qlen - (d.as1 + 9);
		d.r[0][0] = P.max_ext - 1, d.r[0][1] = 50, d.r[1][0] = 700, d.r[1][1] = rest;
		w = run_case("right repeat: r_nt == max_ext - 1", P, d);
		EXPECT(w.r_rep && w.r_aa == rest && w.has_right_span);
		d.r[0][0] = P.max_ext;
		w = run_case("right repeat: r_nt == max_ext", P, d);
		EXPECT(!w.r_rep && w.r_nt == P.max_ext);
		d.r[0][0] = 400, d.r[0][1] = rest;
		w = run_case("right repeat: r_aa reaches the end", P, d);
		EXPECT(!w.r_rep && w.r_aa == rest);
		d.r[0][1] = 50, d.r[1][1] = rest - 1;
		w = run_case("right repeat: one residue short", P, d);
		EXPECT(!w.r_rep && w.r_aa == 50);
	}
	{	// the right span with r_nt == 0, with r_aa == 0, and with has_right == 0
		Case c;
		c.gaps.push_back(dp_gap({ W(0, 9) }));
		c.retry = 0;
		c.r[0][0] = 0, c.r[0][1] = 4;
		Plain w = run_case("right span: r_nt == 0", P, c);
		EXPECT(!w.has_right_span && w.tasks.size() == 6);
		c.r[0][0] = 12, c.r[0][1] = 0;
		w = run_case("right span: r_aa == 0", P, c);
		EXPECT(!w.has_right_span && w.ve == 3000 + 600 + 40);
		c.has_right = 0;
		w = run_case("right span: has_right == 0", P, c);
		EXPECT(!w.has_right_span);
		// windows of fewer than three rows: mpa_dp_run() answers (0, al + 1, INT32_MIN); neither side moves, no repeat counts
		c.has_right = 1, c.retry = 1;
		const int32_t rest = c.qlen - (c.as1 + 9);
		c.r[0][0] = 0, c.r[0][1] = rest + 1, c.r[1][0] = 0, c.r[1][1] = rest + 1;
		c.l[0][0] = 0, c.l[0][1] = c.as1 + 1, c.l[1][0] = 0, c.l[1][1] = c.as1 + 1;
		w = run_case("both extensions on windows of fewer than three rows", P, c);
		EXPECT(!w.has_right_span && !w.r_rep && !w.l_rep && w.r_aa == 0 && w.l_aa == 0 && w.qs == c.as1 && w.l_nt == 0);
		c = Case();
		c.gaps.push_back(dp_gap({ W(0, 9) }));
		c.retry = 0;
		c.has_right = 1, c.r[0][0] = 12, c.r[0][1] = 4;
		w = run_case("right span: made", P, c);
		EXPECT(w.has_right_span && w.right.task < 0 && w.ve == 3000 + 600 + 40 + 12);
	}
	{	// the shortcut at alen == kmer2 and at kmer2 + 1, nlen != 3 * alen, and a codon with an N
		Case c;
		c.retry = 0, c.has_right = 0;
		c.prot = std::string(400, 'A');
		for (size_t i = 0; i < c.prot.size(); ++i) c.prot[i] = "ARNDCQEGHILKMFPSTWYV"[rnd(20)];
		c.l[0][0] = 3 * P.kmer2, c.l[0][1] = P.kmer2;
		Plain w = run_case("shortcut: alen == kmer2", P, c);
		EXPECT(w.left.task < 0 && w.tasks.size() == 6);
		c.l[0][0] = 3 * (P.kmer2 + 1), c.l[0][1] = P.kmer2 + 1;
		w = run_case("shortcut: alen == kmer2 + 1", P, c);
		EXPECT(w.left.task == 6);
		c.l[0][0] = 3 * P.kmer2 + 1, c.l[0][1] = P.kmer2;
		w = run_case("shortcut: nlen != 3 alen", P, c);
		EXPECT(w.left.task == 6);
		c.l[0][0] = 3 * P.kmer2, c.l[0][1] = P.kmer2;
		int found = 0;
		for (int64_t vs0 = 100; vs0 < 8000 && !found; ++vs0) {                 // a left span whose first codon holds an N, on either strand
			for (uint32_t vid = 0; vid < 2 && !found; ++vid) {
				const StrandReader g{ g_ctg_off[0], kCtgLen[0], (int)vid };
				if (g.base(vs0 + 600 - 15) != 4) continue;
				c.vs0 = vs0, c.vid = vid, found = 1;
			}
		}
		EXPECT(found);
		w = run_case("shortcut: a codon with an N", P, c);
		EXPECT(w.left.task < 0);
	}
	{	// boundaries M|M, M|I, 10|10 and 11|11 (these never merge), and N|N
		struct { const char *name; uint32_t a, b; bool merges; } bd[] = { { "M|M", 0, 0, true }, { "M|I", 0, 1, false }, { "10|10", 10, 10, false }, { "11|11", 11, 11, false },
		                                                                   { "N|N", 3, 3, true } };
		for (auto &x : bd) {
			Case c;
			c.gaps.push_back(dp_gap({ W(1, 2), W(x.a, 7) })), c.gaps.push_back(dp_gap({ W(x.b, 5), W(2, 3) }));
			const Plain w = run_case(x.name, P, c);
			EXPECT(w.cigar.size() == (x.merges ? 4u : 5u));
			if (x.merges) EXPECT(w.cigar[2] == W(x.a, 12));
			if (x.a == 3) EXPECT(w.n_exon == 2);
		}
	}
	{	// seven single-word M segments in a row collapse to one word
		Case c;
		for (int i = 0; i < 7; ++i) c.gaps.push_back(i % 2 ? short_gap(3) : dp_gap({ W(0, 9) }));
		c.l[0][0] = 9, c.l[0][1] = 3;
		const Plain w = run_case("seven single-word M segments", P, c);
		EXPECT(w.cigar.size() == 1 && w.cigar[0] == W(0, 3 + 4 * 9 + 3 * 3));
	}
	for (int n : { 0, 1, 63, 64, 65, 200 }) {                                  // plans with 0, 1, 63, 64, 65 and 200 gap segments
		Case c;
		c.qlen = 4000;
		c.l[0][0] = 90, c.l[0][1] = 31, c.left_words = { W(0, 20), W(3, 27), W(0, 1) };
		for (int i = 0; i < n; ++i) c.gaps.push_back(i % 3 == 0 ? short_gap(1 + i % 5) : dp_gap(random_words(1 + (int)rnd(4)), (int)rnd(50)));
		c.r[0][0] = 33, c.r[0][1] = 12, c.retry = 0, c.right_words = { W(0, 11), W(10, 1) };
		char name[64];
		snprintf(name, sizeof name, "%d gap segments", n);
		const Plain w = run_case(name, P, c);
		EXPECT(w.has_right_span && w.right.task == 7);
	}
	for (int n : { 1, 64, 65, 300 }) {                                         // a segment of 1, 64, 65 and 300 words
		Case c;
		c.gaps.push_back(dp_gap({ W(0, 5) })), c.gaps.push_back(dp_gap(random_words(n))), c.gaps.push_back(short_gap(2));
		c.l[0][0] = 200, c.l[0][1] = 40, c.left_words = random_words(n);
		char name[64];
		snprintf(name, sizeof name, "a segment of %d words", n);
		(void)run_case(name, P, c);
	}
	{	// a DP call that comes back without a word: the next first word looks past it
		Case c;
		c.gaps.push_back(dp_gap({ W(2, 3), W(0, 6) })), c.gaps.push_back(dp_gap(Words())), c.gaps.push_back(dp_gap({ W(0, 2) }));
		const Plain w = run_case("an empty segment between two M", P, c);
		EXPECT(w.cigar.size() == 3 && w.cigar[2] == W(0, 8));
	}
	for (int it = 0; it < 400; ++it) {                                         // random plans
		Case c;
		c.vid = (uint32_t)rnd(4), c.vs0 = 700 + (int64_t)rnd(2000), c.qlen = 3000, c.as1 = 50 + (int32_t)rnd(100), c.retry = (int32_t)rnd(2), c.has_right = rnd(5) != 0;
		c.base1 = (int32_t)rnd(4);
		const int n = rnd(8) == 0 ? 60 + (int)rnd(80) : (int)rnd(6);
		for (int i = 0; i < n; ++i) c.gaps.push_back(rnd(3) == 0 ? short_gap(1 + (int32_t)rnd(5), (int32_t)rnd(30)) : dp_gap(random_words((int)rnd(rnd(6) == 0 ? 90 : 5)), (int32_t)rnd(99) - 20));
		for (int k = 0; k < 2; ++k) {
			c.l[k][1] = rnd(3) == 0 ? c.as1 : (int32_t)rnd((uint64_t)c.as1 + 1), c.l[k][0] = rnd(4) == 0 ? 3 * c.l[k][1] : (int32_t)rnd(1200);
			if (rnd(6) == 0) c.l[k][1] = (int32_t)rnd(7), c.l[k][0] = 3 * c.l[k][1];
		}
		c.left_words = random_words(1 + (int)rnd(6)), c.right_words = random_words(1 + (int)rnd(6));
		int32_t used = c.as1;
		for (const Gap &g : c.gaps) used += g.alen;
		const int32_t rest = c.qlen - used;
		for (int k = 0; k < 2; ++k) {
			c.r[k][1] = rnd(3) == 0 ? rest : (int32_t)rnd((uint64_t)rest + 1), c.r[k][0] = (int32_t)rnd(1200);
			if (rnd(5) == 0) c.r[k][1] = (int32_t)rnd(7), c.r[k][0] = rnd(2) ? 3 * c.r[k][1] : 0;
		}
		char name[64];
		snprintf(name, sizeof name, "random plan %d", it);
		(void)run_case(name, P, c);
	}
	printf("%d cases, %d mismatches\n", g_cases, g_fail);
	return g_fail ? 1 : 0;
}
