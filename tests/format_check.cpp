// format_check.cpp -- a stand-alone check of miniprot_amd/csrc/format_core.h (tests/test_format_cpu.py compiles it with
// -fsanitize=address,undefined and runs it).
//  1. Random batches go through the three stages twice -- with a team of one (FormatSerial, what MPA_GPU_FORMAT=model runs) and with a
//     team of 64 host threads that meet at a barrier for every scan, sum and vote (the device's wavefront in slow motion) -- into a
//     text and an id table of exactly the sized bytes (the sanitizer guards their ends), and are compared with a plain restatement of
//     the host formatter written with printf formats after format.c:333-473 and map.c:298-311.
//  2. The same hits read as the finish step leaves them on the device (FinRec / FinOut / FinCounts, rows `stride` apart) give the same
//     text; the rows of a slot whose rows lie further apart than they are wide (what the walks leave on the device) are closed up.
//  3. fmt_ratio against snprintf("%.4f") for every n <= blen <= 3 000 and for random 31-bit pairs.
//  4. format_patch_ids at the width edge of "%.6ld".
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>
#include <pthread.h>
#include "format_core.h"

using namespace mpa;

// ---- a team of 64 threads ---------------------------------------------------------------------------
static pthread_barrier_t g_bar;
static int64_t g_slot[64];
static thread_local int tl_lane = 0;
struct FormatThreads {
	static int lane() { return tl_lane; }
	static int width() { return 64; }
	static void sync() { pthread_barrier_wait(&g_bar); }
	static void gather(int64_t v, int64_t *all)
	{
		g_slot[tl_lane] = v;
		pthread_barrier_wait(&g_bar);
		for (int i = 0; i < 64; ++i) all[i] = g_slot[i];
		pthread_barrier_wait(&g_bar);
	}
	static bool any(bool p) { int64_t a[64]; gather(p, a); for (int i = 0; i < 64; ++i) if (a[i]) return true; return false; }
	static int64_t scan_excl(int64_t v, int64_t *total) { int64_t a[64], s = 0, t = 0; gather(v, a); for (int i = 0; i < 64; ++i) { if (i < tl_lane) s += a[i]; t += a[i]; } *total = t; return s; }
	static int64_t sum64(int64_t v) { int64_t t; scan_excl(v, &t); return t; }
};

static uint64_t g_rng = 88172645463325252ULL;
static uint64_t rnd(uint64_t n) { g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17; return g_rng % n; }
static int64_t g_bad = 0;
static void fail(const char *what, int64_t a = 0, int64_t b = 0) { if (++g_bad <= 20) printf("MISMATCH %s (%lld, %lld)\n", what, (long long)a, (long long)b); }

// ---- a batch ------------------------------------------------------------------------------------------
struct Batch {
	FmtOpt o;
	std::vector<mpa_hit_t> hits;
	std::vector<int64_t> hit_off, q_off, qname_off, cname_off, clen;
	std::vector<uint32_t> cigars;
	std::vector<mpa_feat_t> feats;
	std::vector<FinCsRef> cs;
	std::vector<FinRowsRef> rows;
	std::string cs_text, rows_text, qname, cname;
	FmtSrc src() const
	{
		FmtSrc S;
		S.hits = hits.data(), S.hit_off = hit_off.data(), S.cigars = cigars.data(), S.feats = feats.data();
		S.cs = cs.empty() ? nullptr : cs.data(), S.cs_text = cs_text.data(), S.rows = rows.empty() ? nullptr : rows.data(), S.rows_text = rows_text.data();
		S.q_off = q_off.data(), S.qname = qname.data(), S.qname_off = qname_off.data(), S.cname = cname.data(), S.cname_off = cname_off.data(), S.clen = clen.data();
		return S;
	}
};

static std::string rand_text(size_t n, const char *alphabet)
{
	std::string s(n, ' ');
	const size_t m = strlen(alphabet);
	for (size_t i = 0; i < n; ++i) s[i] = alphabet[rnd(m)];
	return s;
}

static const uint32_t FLAGSETS[] = { 0, MPA_MF_SHOW_UNMAP, MPA_MF_SHOW_UNMAP | MPA_MF_GFF, MPA_MF_GTF, MPA_MF_GFF | MPA_MF_NO_PAF | MPA_MF_NO_CS, MPA_MF_SHOW_UNMAP | MPA_MF_SHOW_RESIDUE,
                                     MPA_MF_SHOW_TRANS | MPA_MF_GFF, MPA_MF_SHOW_RESIDUE | MPA_MF_SHOW_TRANS | MPA_MF_GTF, MPA_MF_GFF | MPA_MF_NO_CS, MPA_MF_GTF | MPA_MF_SHOW_UNMAP | MPA_MF_NO_CS };

static Batch random_batch(int n_query, int which)
{
	Batch b;
	memset(&b.o, 0, sizeof b.o);
	b.o.flag = FLAGSETS[which % 10];
	static const float sims[] = { 0.0f, 0.5f, 0.97f, 0.99f, 1.0f }, covs[] = { 0.0f, 0.1f, 1.0f };
	b.o.out_n = which % 7 == 3 ? 1 : which % 11 == 5 ? 0 : 1000, b.o.out_sim = sims[rnd(5)], b.o.out_cov = covs[rnd(3)];
	b.o.gff_delim = which % 4 == 1 ? '#' : -1;
	const std::string prefix = which % 3 == 0 ? "MP" : which % 3 == 1 ? "a_long_prefix." : std::string(64, 'p');
	memcpy(b.o.prefix, prefix.data(), prefix.size()), b.o.prefix_len = (int32_t)prefix.size();
	const uint32_t flag = b.o.flag;
	const bool residues = flag & (MPA_MF_SHOW_RESIDUE | MPA_MF_SHOW_TRANS), paf = flag & MPA_MF_GTF ? residues : !(flag & MPA_MF_NO_PAF), want_cs = paf && !(flag & MPA_MF_NO_CS);
	b.clen = { 5000000, 1234567, ((int64_t)1 << 31) + 123456789 };
	b.cname = "chr1ctg_twobig", b.cname_off = { 0, 4, 11, 14 };
	b.hit_off.push_back(0), b.q_off.push_back(0), b.qname_off.push_back(0);
	b.cigars.assign(3, 0x11), b.feats.resize(1), b.cs_text = "#####", b.rows_text = "%%%%%%%";
	memset(b.feats.data(), 0, sizeof(mpa_feat_t));
	for (int q = 0; q < n_query; ++q) {
		const int32_t qlen = 30 + (int32_t)rnd(3000);
		char nm[64];
		snprintf(nm, sizeof nm, q % 5 == 2 ? "sp|Q%05d|LONG_NAME" : "q%d", q);
		b.qname += nm, b.qname_off.push_back((int64_t)b.qname.size()), b.q_off.push_back(b.q_off.back() + qlen);
		const int n_hit = (int)rnd(5);
		int32_t best = 100 + (int32_t)rnd(3000);
		for (int j = 0; j < n_hit; ++j) {
			mpa_hit_t h;
			memset(&h, 0, sizeof h);
			h.qid = q, h.id = j, h.has_aln = rnd(8) != 0;
			h.qs = (int32_t)rnd((uint64_t)qlen - 20), h.qe = rnd(3) ? h.qs + 1 + (int32_t)rnd((uint64_t)(qlen - h.qs)) : qlen;
			const int c = (int)rnd(3);
			h.vid = (uint32_t)(2 * c + (int)rnd(2)), h.vs = (int64_t)rnd((uint64_t)b.clen[c] - 40000), h.ve = h.vs + 30 + (int64_t)rnd(30000);
			const int32_t sc = j == 0 ? best : rnd(4) == 0 ? (int32_t)((double)best * b.o.out_sim) + (int32_t)rnd(3) - 1 : (int32_t)rnd((uint64_t)best + 50) - 40;
			h.dp_max = h.has_aln ? sc : 1, h.chn_sc = h.has_aln ? (int32_t)rnd(900) : sc, h.chn_sc_ungap = (int32_t)rnd(900) - 5, h.cnt = (int32_t)rnd(100000);
			h.dp_score = (int32_t)rnd(5000) - 100, h.blen = 1 + (int32_t)rnd(9000), h.n_iden = (int32_t)rnd(3001), h.n_plus = (int32_t)rnd(3001), h.n_fs = (int32_t)rnd(3) * (rnd(3) == 0);
			h.n_stop = (int32_t)rnd(2), h.dist_stop = (int32_t)rnd(3) - 1, h.dist_start = (int32_t)rnd(100) - 1;
			if (h.has_aln) {
				static const int cig_n[] = { 1, 2, 3, 7, 63, 64, 65, 130 }, feat_n[] = { 0, 1, 2, 3, 5, 64, 65, 70 };
				h.n_cigar = cig_n[rnd(8)], h.cigar_off = (int64_t)b.cigars.size();
				for (int k = 0; k < h.n_cigar; ++k) { uint64_t lim = 10; for (int d = (int)rnd(9); d > 0; --d) lim *= 10; b.cigars.push_back((uint32_t)((1 + rnd(lim < 268435455 ? lim : 268435455)) << 4 | rnd(16))); }
				h.n_feat = feat_n[rnd(8)], h.feat_off = (int64_t)b.feats.size();
				for (int k = 0; k < h.n_feat; ++k) {
					mpa_feat_t f;
					memset(&f, 0, sizeof f);
					f.vs = h.vs + 100 * k, f.ve = k == h.n_feat - 1 || rnd(9) == 0 ? h.ve : f.vs + 99, f.qs = h.qs + k, f.qe = f.qs + 1 + (int32_t)rnd(50);
					f.type = k == h.n_feat - 1 && h.n_feat > 1 && rnd(2) ? 1 : 0, f.phase = (int16_t)rnd(3), f.n_fs = (int32_t)rnd(3) * (rnd(3) == 0), f.n_stop = (int32_t)rnd(3) * (rnd(3) == 0);
					f.score = (int32_t)rnd(5000) - 20, f.n_iden = (int32_t)rnd(400), f.blen = 1 + (int32_t)rnd(1300);
					static const char *const sp[] = { "GT", "AG", "GC", "AT", "\0\0", "G\0", "A\0" };
					memcpy(f.donor, sp[rnd(7)], 2), memcpy(f.acceptor, sp[rnd(7)], 2);
					b.feats.push_back(f);
				}
			}
			b.hits.push_back(h);
		}
		b.hit_off.push_back((int64_t)b.hits.size());
	}
	if (want_cs || residues)
		for (const mpa_hit_t &h : b.hits) {
			FinCsRef c{ 0, 0, 0 };
			FinRowsRef r{ 0, 0, 0, 0, 0 };
			if (h.has_aln && want_cs) {
				static const int cs_n[] = { 1, 2, 63, 64, 65, 300 };
				c = FinCsRef{ (int64_t)b.cs_text.size(), cs_n[rnd(6)], 1 };
				b.cs_text += rand_text((size_t)c.len, ":*+-~acgtnACDEFGHIKLMNPQRSTVWY0123456789");
			}
			if (h.has_aln && residues) {
				static const int row_w[] = { 1, 63, 64, 65, 200 };
				r = FinRowsRef{ (int64_t)b.rows_text.size(), row_w[rnd(5)], (int32_t)rnd(70), 1, 0 };
				b.rows_text += rand_text((size_t)(4 * r.width + r.n_sta), "ACGTacgt~-.|+ 0123456789*X");
			}
			if (want_cs) b.cs.push_back(c);
			if (residues) b.rows.push_back(r);
		}
	return b;
}

// ---- the plain side: the host formatter in printf formats ------------------------------------------------------------------------
static void P(std::string &s, const char *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	const int n = vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	s.append(buf, (size_t)n);
}

static std::string plain_format(const Batch &b, int64_t id0, int64_t *n_out_total)
{
	static const char ops[] = "MIDNSHP=XBFGUVE";
	const FmtOpt &o = b.o;
	const std::string prefix(o.prefix, (size_t)o.prefix_len);
	std::string s;
	int64_t id = id0;
	for (size_t q = 0; q + 1 < b.hit_off.size(); ++q) {
		const std::string qn = b.qname.substr((size_t)b.qname_off[q], (size_t)(b.qname_off[q + 1] - b.qname_off[q]));
		const int32_t qlen = (int32_t)(b.q_off[q + 1] - b.q_off[q]);
		const int64_t n_reg = b.hit_off[q + 1] - b.hit_off[q];
		const mpa_hit_t *hs = b.hits.data() + b.hit_off[q];
		int32_t best = -1;
		int64_t n_out = 0;
		if (n_reg > 0) best = hs[0].has_aln ? hs[0].dp_max : hs[0].chn_sc;
		auto head = [&]() { if (o.flag & (MPA_MF_GFF | MPA_MF_GTF)) s += "##PAF\t"; P(s, "%s\t%d", qn.c_str(), qlen); };
		for (int64_t j = 0; j < n_reg && j < o.out_n; ++j) {
			const mpa_hit_t &h = hs[j];
			const int64_t hidx = b.hit_off[q] + j;
			const int32_t sc = h.has_aln ? h.dp_max : h.chn_sc;
			if (sc <= 0 || sc < (double)best * o.out_sim) continue;
			if (h.qe - h.qs < (double)qlen * o.out_cov) continue;
			++id, ++n_out;
			const int c = (int)(h.vid >> 1);
			const bool rev = h.vid & 1;
			const std::string cn = b.cname.substr((size_t)b.cname_off[c], (size_t)(b.cname_off[c + 1] - b.cname_off[c]));
			const long long clen = b.clen[c];
			auto paf = [&]() {
				head();
				P(s, "\t%d\t%d\t%c\t%s\t%lld\t%lld\t%lld\t", h.qs, h.qe, "+-"[rev], cn.c_str(), clen, rev ? clen - h.ve : (long long)h.vs, rev ? clen - h.vs : (long long)h.ve);
				if (h.has_aln) {
					P(s, "%d\t%d\t0\tAS:i:%d\tms:i:%d\tnp:i:%d\tfs:i:%d\tst:i:%d\tda:i:%d\tdo:i:%d\tcg:Z:", h.n_iden * 3, h.blen, h.dp_score, h.dp_max, h.n_plus, h.n_fs, h.n_stop, h.dist_start, h.dist_stop);
					for (int k = 0; k < h.n_cigar; ++k) { const uint32_t w = b.cigars[(size_t)(h.cigar_off + k)]; P(s, "%u", w >> 4), s.push_back(ops[w & 0xf]); }
					if (!(o.flag & MPA_MF_NO_CS)) s += "\tcs:Z:", s.append(b.cs_text, (size_t)b.cs[(size_t)hidx].off, (size_t)b.cs[(size_t)hidx].len);
				} else {
					P(s, "%d\t%d\t%d", h.chn_sc, h.chn_sc_ungap, h.cnt);
					if (!(o.flag & MPA_MF_NO_CS)) s.push_back('\t');
				}
				s.push_back('\n');
			};
			auto rows = [&]() {
				if (!h.has_aln) return;
				const FinRowsRef &r = b.rows[(size_t)hidx];
				static const char *const pre[4] = { "##ATN\t", "##ATA\t", "##AAS\t", "##AQA\t" };
				if (o.flag & MPA_MF_SHOW_RESIDUE) for (int k = 0; k < 4; ++k) s += pre[k], s.append(b.rows_text, (size_t)(r.off + (int64_t)k * r.width), (size_t)r.width), s.push_back('\n');
				if (o.flag & MPA_MF_SHOW_TRANS) s += "##STA\t", s.append(b.rows_text, (size_t)(r.off + 4 * (int64_t)r.width), (size_t)r.n_sta), s.push_back('\n');
			};
			const bool has_stop = h.qe == qlen && h.dist_stop == 0;
			const long long ve_mrna = has_stop ? h.ve + 3 : h.ve;
			const mpa_feat_t *ft = b.feats.data() + h.feat_off;
			auto gff = [&]() {
				if (!h.has_aln) return;
				char ids[256];
				if (o.gff_delim >= 33 && o.gff_delim <= 126) snprintf(ids, sizeof ids, "%s%c%d", qn.c_str(), o.gff_delim, (int)j + 1);
				else snprintf(ids, sizeof ids, "%s%.6ld", prefix.c_str(), (long)id);
				P(s, "%s\tminiprot\tmRNA\t%lld\t%lld\t%d\t%c\t.\tID=%s;Rank=%d;Identity=%.4f;Positive=%.4f", cn.c_str(), (rev ? clen - ve_mrna : (long long)h.vs) + 1, rev ? clen - h.vs : ve_mrna, h.dp_max,
				  "+-"[rev], ids, (int)j + 1, (double)h.n_iden * 3 / h.blen, (double)h.n_plus * 3 / h.blen);
				if (h.n_fs > 0) P(s, ";Frameshift=%d", h.n_fs);
				if (h.n_stop > 0) P(s, ";StopCodon=%d", h.n_stop);
				P(s, ";Target=%s %d %d\n", qn.c_str(), h.qs + 1, h.qe);
				for (int k = 0; k < h.n_feat; ++k) {
					const mpa_feat_t &f = ft[k];
					long long fe = f.ve;
					if (has_stop && f.type == 0 && k + 1 < h.n_feat && ft[k + 1].type == 1) fe += 3;
					P(s, "%s\tminiprot\t%s\t%lld\t%lld\t%d\t%c\t%d\tParent=%s;Rank=%d", cn.c_str(), f.type == 1 ? "stop_codon" : "CDS", (rev ? clen - fe : (long long)f.vs) + 1, rev ? clen - f.vs : fe,
					  f.score, "+-"[rev], f.phase, ids, (int)j + 1);
					if (f.type == 0) {
						P(s, ";Identity=%.4f", (double)f.n_iden * 3 / f.blen);
						if (f.acceptor[0] && strncmp(f.acceptor, "AG", 2) != 0) P(s, ";Acceptor=%c%c", f.acceptor[0], f.acceptor[1]);
						if (f.donor[0] && strncmp(f.donor, "GT", 2) != 0) P(s, ";Donor=%c%c", f.donor[0], f.donor[1]);
						if (f.n_fs > 0) P(s, ";Frameshift=%d", f.n_fs);
						if (f.n_stop > 0) P(s, ";StopCodon=%d", f.n_stop);
						P(s, ";Target=%s %d %d", qn.c_str(), f.qs + 1, f.qe);
					}
					s.push_back('\n');
				}
			};
			auto gtf = [&]() {
				if (!h.has_aln) return;
				char gid[128], tid[128];
				snprintf(gid, sizeof gid, "%sG%.6ld", prefix.c_str(), (long)id), snprintf(tid, sizeof tid, "%sT%.6ld", prefix.c_str(), (long)id);
				const long long vs = rev ? clen - ve_mrna : (long long)h.vs, ve = rev ? clen - h.vs : ve_mrna;
				P(s, "%s\tminiprot\tgene\t%lld\t%lld\t%d\t%c\t.\tgene_id \"%s\";\n", cn.c_str(), vs + 1, ve, h.dp_max, "+-"[rev], gid);
				P(s, "%s\tminiprot\ttranscript\t%lld\t%lld\t%d\t%c\t.\ttranscript_id \"%s\"; gene_id \"%s\";\n", cn.c_str(), vs + 1, ve, h.dp_max, "+-"[rev], tid, gid);
				for (int k = 0; k < h.n_feat; ++k) {
					const mpa_feat_t &f = ft[k];
					if (f.type != 0) continue;
					const long long a = rev ? clen - f.ve : (long long)f.vs, e = rev ? clen - f.vs : (long long)f.ve;
					long long a2 = a, e2 = e;
					if (f.ve == h.ve) { if (rev) a2 = clen - ve_mrna; else e2 = ve_mrna; }
					P(s, "%s\tminiprot\texon\t%lld\t%lld\t%d\t%c\t.\ttranscript_id \"%s\"; gene_id \"%s\";\n", cn.c_str(), a2 + 1, e2, f.score, "+-"[rev], tid, gid);
					P(s, "%s\tminiprot\tCDS\t%lld\t%lld\t%d\t%c\t%d\ttranscript_id \"%s\"; gene_id \"%s\";\n", cn.c_str(), a + 1, e, f.score, "+-"[rev], f.phase, tid, gid);
				}
			};
			const bool residues = (o.flag & (MPA_MF_SHOW_RESIDUE | MPA_MF_SHOW_TRANS)) != 0;
			if (o.flag & MPA_MF_GTF) {
				if (residues) paf(), rows();
				gtf();
			} else {
				if (!(o.flag & MPA_MF_NO_PAF)) paf();
				if (residues) rows();
				if (o.flag & MPA_MF_GFF) gff();
			}
		}
		if (n_out == 0 && (o.flag & MPA_MF_SHOW_UNMAP)) head(), s += "\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0\n";
	}
	*n_out_total = id - id0;
	return s;
}

// ---- the core, with either team ------------------------------------------------------------------------------------------------
struct Run { std::vector<FmtAt> at; std::vector<FmtCounts> cnt, off; std::vector<char> text; std::vector<int64_t> id_at; };

template<class C> static void core_size(const Batch &b, const FmtSrc &S, Run &r)
{
	for (size_t q = 0; q + 1 < b.hit_off.size(); ++q) format_size_core<C>(b.o, S, (int32_t)q, r.at.data(), &r.cnt[q]);
}
template<class C> static void core_write(const Batch &b, const FmtSrc &S, Run &r)
{
	for (size_t q = 0; q + 1 < b.hit_off.size(); ++q) {
		const int64_t h0 = fmt_base(S, (int32_t)q), n_reg = fmt_n_reg(S, (int32_t)q);
		for (int64_t j = 0; j < n_reg; ++j) if (r.at[(size_t)(h0 + j)].rank >= 0) format_write_core<C>(b.o, S, (int32_t)q, j, r.at[(size_t)(h0 + j)], r.off[q], r.text.data(), r.id_at.data());
		if (r.off[q + 1].n_out == r.off[q].n_out && (b.o.flag & MPA_MF_SHOW_UNMAP)) format_unmap_core<C>(b.o, S, (int32_t)q, r.off[q], r.text.data());
	}
}
static void core_between(const Batch &b, Run &r)
{
	const size_t nq = b.hit_off.size() - 1;
	format_scan_serial(r.cnt.data(), (int64_t)nq, r.off.data());
	r.text.assign((size_t)r.off[nq].bytes, '?'), r.id_at.assign((size_t)r.off[nq].ids, -1);
}
static void core_run(const Batch &b, bool threads, Run &r, const FmtSrc *other = nullptr)
{
	const FmtSrc S = other ? *other : b.src();
	const size_t nq = b.hit_off.size() - 1;
	r.at.assign(b.hits.size(), FmtAt{ -1, -1, -2 }), r.cnt.assign(nq, FmtCounts{ -1, -1, -1, -1 }), r.off.assign(nq + 1, FmtCounts{ 0, 0, 0, 0 });
	if (!threads) { core_size<FormatSerial>(b, S, r), core_between(b, r), core_write<FormatSerial>(b, S, r); return; }
	std::vector<std::thread> team;
	for (int l = 0; l < 64; ++l)
		team.emplace_back([&, l]() {
			tl_lane = l;
			core_size<FormatThreads>(b, S, r);
			pthread_barrier_wait(&g_bar);
			if (l == 0) core_between(b, r);
			pthread_barrier_wait(&g_bar);
			core_write<FormatThreads>(b, S, r);
		});
	for (auto &t : team) t.join();
}

static void check_batch(const Batch &b, int which)
{
	for (int threads = 0; threads < 2; ++threads) {
		Run r;
		core_run(b, threads != 0, r);
		const FmtCounts tot = r.off.back();
		if (tot.bad) { fail("a batch that should not decline", which, tot.bad); continue; }
		static const int64_t id0s[] = { 0, 7, 999990 };
		for (int64_t id0 : id0s) {
			int64_t n_out = 0;
			const std::string want = plain_format(b, id0, &n_out);
			std::vector<char> text = r.text;
			if (n_out != tot.n_out) fail("n_out", n_out, tot.n_out);
			const bool ok = format_patch_ids(text.data(), r.id_at.data(), tot.ids, tot.n_out, id0);
			if (ok != (tot.ids == 0 || id0 + n_out <= 999999)) fail("the patch's verdict", which, id0);
			if (!ok) continue;
			if (text.size() != want.size() || (!want.empty() && memcmp(text.data(), want.data(), want.size()) != 0)) {
				size_t d = 0;
				while (d < text.size() && d < want.size() && text[d] == want[d]) ++d;
				fail(threads ? "text, team of 64" : "text, team of one", which, (int64_t)d);
				if (g_bad <= 3) printf("  got  %.120s\n  want %.120s\n", std::string(text.data() + (d > 40 ? d - 40 : 0), text.data() + text.size()).c_str(), want.c_str() + (d > 40 ? d - 40 : 0));
			}
		}
		for (int64_t k = 0; k < tot.ids; ++k)                    // every id place lies inside the text, in ascending order, on six digits
			if (r.id_at[(size_t)k] < 0 || r.id_at[(size_t)k] + 6 > tot.bytes || (k && r.id_at[(size_t)k] <= r.id_at[(size_t)k - 1])) { fail("id_at", which, k); break; }
	}
}

// ---- the hits read where the finish step leaves them (FmtSrc::rec) ----------------------------------------------------------------------
// The aligned hits of a batch as FinRec / FinOut / FinCounts -- the records of a query in reverse order, so that `src` is no identity, the
// rows re-laid `stride` apart -- must give the text of the same hits as a flat result
static void check_fin_source(const Batch &b0, int which)
{
	Batch b = b0;
	b.hits.clear(), b.cs.clear(), b.rows.clear();
	for (size_t q = 0; q + 1 < b0.hit_off.size(); ++q) {
		for (int64_t h = b0.hit_off[q]; h < b0.hit_off[q + 1]; ++h) {
			if (!b0.hits[(size_t)h].has_aln) continue;
			b.hits.push_back(b0.hits[(size_t)h]);
			if (!b0.cs.empty()) b.cs.push_back(b0.cs[(size_t)h]);
			if (!b0.rows.empty()) b.rows.push_back(b0.rows[(size_t)h]);
		}
		b.hit_off[q + 1] = (int64_t)b.hits.size();
	}
	Run flat;
	core_run(b, false, flat);
	const size_t nq = b.hit_off.size() - 1, nh = b.hits.size();
	std::vector<FinRec> rec(nh + 1);
	std::vector<FinOut> out(nh + 1);
	std::vector<FinCounts> off(nq + 1);
	std::string rows_text = "@@@";
	for (size_t q = 0; q <= nq; ++q) memset(&off[q], 0, sizeof(FinCounts)), off[q].hit = b.hit_off[q];
	for (size_t q = 0; q < nq; ++q) {
		const int64_t f = b.hit_off[q], n = b.hit_off[q + 1] - f;
		for (int64_t j = 0; j < n; ++j) {
			const mpa_hit_t &h = b.hits[(size_t)(f + j)];
			const int64_t at = f + (n - 1 - j);
			FinRec &x = rec[(size_t)at];
			memset(&x, 0, sizeof x);
			x.vs = h.vs, x.ve = h.ve, x.cig_off = h.cigar_off, x.feat_off = h.feat_off, x.vid = h.vid, x.qs = h.qs, x.qe = h.qe, x.cnt = h.cnt, x.n_exon = h.n_exon, x.chn_sc = h.chn_sc;
			x.chn_sc_ungap = h.chn_sc_ungap, x.dp_score = h.dp_score, x.dp_max = h.dp_max, x.blen = h.blen, x.n_fs = h.n_fs, x.n_stop = h.n_stop, x.dist_stop = h.dist_stop;
			x.dist_start = h.dist_start, x.n_iden = h.n_iden, x.n_plus = h.n_plus, x.n_cigar = h.n_cigar, x.n_feat = h.n_feat, x.cs_len = -1, x.rows_stride = -1;
			if (!b.cs.empty()) x.cs_off = b.cs[(size_t)(f + j)].off, x.cs_len = b.cs[(size_t)(f + j)].len;
			if (!b.rows.empty()) {
				const FinRowsRef &r = b.rows[(size_t)(f + j)];
				x.rows_off = (int64_t)rows_text.size(), x.rows_w = r.width, x.rows_sta = r.n_sta, x.rows_stride = r.width + 1 + (int32_t)rnd(9);
				for (int k = 0; k < 4; ++k) rows_text.append(b.rows_text, (size_t)(r.off + (int64_t)k * r.width), (size_t)r.width), rows_text.append((size_t)(x.rows_stride - r.width), '!');
				rows_text.append(b.rows_text, (size_t)(r.off + 4 * (int64_t)r.width), (size_t)r.n_sta);
			}
			memset(&out[(size_t)(f + j)], 0, sizeof(FinOut));
			out[(size_t)(f + j)].src = (int32_t)(n - 1 - j), out[(size_t)(f + j)].id = (int32_t)j;
		}
	}
	FmtSrc S = b.src();
	S.hits = nullptr, S.hit_off = nullptr, S.cs = nullptr, S.rows = nullptr, S.rows_text = rows_text.data();
	S.rec = rec.data(), S.out = out.data(), S.first = b.hit_off.data(), S.fin_off = off.data();
	for (int threads = 0; threads < 2; ++threads) {
		Run r;
		core_run(b, threads != 0, r, &S);
		if (r.text != flat.text || r.id_at != flat.id_at || r.off.back().n_out != flat.off.back().n_out || r.off.back().bad) fail(threads ? "fin source, team of 64" : "fin source, team of one", which);
	}
}

// ---- rows whose slots are wider than their width ---------------------------------------------------------------------------------
template<class C> static void strided_rows(const FmtOpt &o, const FmtHit &X, char *dst, int64_t *len)
{
	FmtPut w{ dst, 0, nullptr, 0, 0, 0, C::lane() == 0 };
	fmt_rows<C>(w, o, X);
	*len = w.p;
}
static void check_strided_rows()
{
	static const int widths[] = { 1, 63, 64, 65, 4097 };
	for (int wd : widths)
		for (uint32_t flag : { (uint32_t)MPA_MF_SHOW_RESIDUE, (uint32_t)MPA_MF_SHOW_TRANS, (uint32_t)(MPA_MF_SHOW_RESIDUE | MPA_MF_SHOW_TRANS) }) {
			const int64_t stride = wd + 1 + (int64_t)rnd(40);
			const int32_t n_sta = (int32_t)rnd(80);
			const std::string slot = rand_text((size_t)(4 * stride + n_sta), "ACGTacgt~-.|+ 0123456789*X");
			FmtOpt o;
			memset(&o, 0, sizeof o);
			o.flag = flag;
			FmtHit X;
			memset(&X, 0, sizeof X);
			X.h.has_aln = 1, X.rows = slot.data(), X.rows_stride = stride, X.rows_w = wd, X.rows_sta = n_sta, X.cs_len = -1;
			std::string want;
			static const char *const pre[4] = { "##ATN\t", "##ATA\t", "##AAS\t", "##AQA\t" };
			if (flag & MPA_MF_SHOW_RESIDUE) for (int k = 0; k < 4; ++k) want += pre[k], want.append(slot, (size_t)(k * stride), (size_t)wd), want += '\n';
			if (flag & MPA_MF_SHOW_TRANS) want += "##STA\t", want.append(slot, (size_t)(4 * stride), (size_t)n_sta), want += '\n';
			for (int threads = 0; threads < 2; ++threads) {
				std::vector<char> got(want.size(), '?');
				int64_t len = -1;
				if (!threads) strided_rows<FormatSerial>(o, X, got.data(), &len);
				else {
					std::vector<std::thread> team;
					for (int l = 0; l < 64; ++l) team.emplace_back([&, l]() { tl_lane = l; int64_t n; strided_rows<FormatThreads>(o, X, got.data(), &n); if (l == 0) len = n; });
					for (auto &t : team) t.join();
				}
				if (len != (int64_t)want.size() || memcmp(got.data(), want.data(), want.size()) != 0) fail("strided rows", wd, flag);
			}
		}
}

// ---- "%.4f" --------------------------------------------------------------------------------------------------------------------
static int64_t g_ties = 0;
static void check_ratio(int32_t n, int32_t blen)
{
	char got[64], want[64];
	FmtPut w{ got, 0, nullptr, 0, 0, 0, true };
	fmt_ratio(w, n, blen);
	got[w.p] = 0;
	snprintf(want, sizeof want, "%.4f", (double)n * 3 / blen);
	if (w.bad || strcmp(got, want) != 0) { fail("ratio", n, blen); if (g_bad <= 5) printf("  got %s want %s\n", got, want); }
	FmtPut c{ nullptr, 0, nullptr, 0, 0, 0, true };
	fmt_ratio(c, n, blen);
	if (c.p != w.p) fail("ratio, sized", n, blen);
	if (((int64_t)n * 3 * 100000) % blen == 0 && ((int64_t)n * 3 * 100000 / blen) % 10 == 5) ++g_ties;
}

int main()
{
	pthread_barrier_init(&g_bar, nullptr, 64);
	int n_batch = 0;
	for (int which = 0; which < 60; ++which, ++n_batch) {
		const Batch b = random_batch(which % 13 == 12 ? 300 : 1 + (int)rnd(12), which);
		check_batch(b, which);
		if (which % 2 == 0) check_fin_source(b, which);
	}
	check_strided_rows();
	int64_t n_ratio = 0;
	for (int32_t blen = 1; blen <= 3000; ++blen)
		for (int32_t n = 0; n <= blen; ++n, ++n_ratio) check_ratio(n, blen);
	for (int k = 0; k < 300000; ++k, ++n_ratio) check_ratio((int32_t)rnd((uint64_t)1 << 31), 1 + (int32_t)rnd(((uint64_t)1 << 31) - 1));
	for (int32_t n : { 0, 1, -1, 5, -715827882, 715827882 }) for (int32_t blen : { 1, -1, 3, -96, 2147483647 }) check_ratio(n, blen), ++n_ratio;   // signs, and the widest figure
	{	// a blen of 0 declines
		FmtPut w{ nullptr, 0, nullptr, 0, 0, 0, true };
		fmt_ratio(w, 5, 0);
		FmtPut z{ nullptr, 0, nullptr, 0, 0, 0, true };
		fmt_ratio(z, 0, 0);
		if (!w.bad || !z.bad) fail("a blen of 0 does not decline");
	}
	{	// the id patch at its width edge
		char text[] = "x000001y000002z";
		const int64_t at[2] = { 1, 8 };
		if (!format_patch_ids(text, at, 2, 2, 999997) || strcmp(text, "x999998y999999z") != 0) fail("patch up to 999999");
		char text2[] = "x000001y000002z";
		if (format_patch_ids(text2, at, 2, 2, 999998) || strcmp(text2, "x000001y000002z") != 0) fail("patch past 999999 must refuse and leave the text");
		if (!format_patch_ids(text2, at, 2, 2, 0) || !format_patch_ids(text2, at, 0, 2, 999999) || strcmp(text2, "x000001y000002z") != 0) fail("nothing to patch");
		if (format_patch_ids(text2, at, 2, 1000000, 0)) fail("a batch of a million printed hits must refuse");
	}
	printf("%d batches, %lld ratios (%lld on ties), %lld mismatches\n", n_batch, (long long)n_ratio, (long long)g_ties, (long long)g_bad);
	return g_bad ? 1 : 0;
}
