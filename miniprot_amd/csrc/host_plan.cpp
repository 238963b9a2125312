// host_plan.cpp -- stage A of the stage machine (host_map.cpp has the map of the whole): the per-query host steps from the sketch to the
// alignment plans and the round-1 tasks, their device routes and shared-core models, and the phases of a batch made of them
// (sketch -> device seed -> plan), which the stage machine, the stream pipeline and the test hooks call.
#include <algorithm>
#include <atomic>
#include <cassert>
#include <cstring>
#include <mutex>
#include <memory>
#include "host_batch.h"

// the genome as plans_core.h reads it on the host (outside the namespace, where it was: plans_core<>'s exported names carry it)
struct PlansGenomeHost {
	const mpa_idx_s *mi;
	int64_t off(int32_t c) const { return mi->ctg[(size_t)c].off; }
	int64_t len(int32_t c) const { return mi->ctg[(size_t)c].len; }
	auto strand(uint32_t vid) const { return mpa::genome_strand(mi, vid); }
};

namespace mpa {

// ------------------------------------------------------------------------------------------------
// stage A
// ------------------------------------------------------------------------------------------------

// per-substage CPU-time accumulators of stage A (thread CPU time summed over the workers; printed with MPA_TIMING=1)
static std::atomic<int64_t> g_acc[16];
static const char *const kAccName[16] = { "A.sketch+lookup", "A.sort anchors", "A.pre-chain", "A.chain", "A.regions", "A.refine", "A.plan", "A.round-1 plan",
	"  refine: fetch window", "  refine: sketch nt4", "  refine: sketch prot+sort", "  refine: pairs+sort", "  refine: chain", "  refine: n regions", "  anchors (x1000, all queries / threads)", "  pre-chain survivors (x1000)" };
// (thread CPU time, not wall time: under a CPU quota the wall time of a thread says how often it was throttled, not what it cost)
struct AccTimer {
	int k; double t0; bool on;
	AccTimer(int k_) : k(k_), t0(0), on(timing_on()) { if (on) t0 = thread_cpu_ms(); }
	~AccTimer() { if (on) g_acc[k] += (int64_t)((thread_cpu_ms() - t0) * 1e6); }
};

// mp_cal_max_occ (map.c:126-141): boxplot-style cutoff on the occurrence counts of the query's seeds
static int32_t occurrence_cutoff(const mpa_idx_s *mi, const std::vector<uint64_t> &seeds)
{
	const int64_t n = (int64_t)seeds.size(), n_bucket = (int64_t)mi->ki.size();
	std::vector<uint64_t> cnt(n);
	for (int64_t i = 0; i < n; ++i) {
		const int64_t b = (int64_t)(seeds[i] >> 32);
		const int64_t en = b + 1 < n_bucket ? mi->ki[b + 1] : mi->n_kb;
		cnt[i] = (uint64_t)(en - mi->ki[b]);
	}
	sort_u64(cnt.data(), cnt.data() + n);
	const uint64_t q25 = cnt[(int64_t)(n * .25 + .499)], q75 = cnt[(int64_t)(n * .75 + .499)];
	return (int32_t)(q75 + (q75 - q25) * 1.5 + 10.);
}

// The anchors of a region's refinement (map.c:36-79): every (window position, query position) pair of equal k = kmer2 k-mers,
// sorted.  dev_hits != nullptr: the window was scanned on the device (dev_refine_scan); its k-mer hits are (hash << 32 | position).
void refine_region_pairs(const mpa_idx_s *mi, const mpa_mapopt_t &opt, const RefineQuery &rq, const Region &r, int32_t extl, int32_t extr,
                                const uint64_t *dev_hits, int64_t n_dev_hits, std::vector<uint64_t> &a)
{
	const int32_t kmer = opt.kmer2;
	const int64_t ctg_len = mi->ctg[r.vid >> 1].len;
	const int64_t as = r.vs > extl ? r.vs - extl : 0;
	const int64_t ae = r.ve + extr < ctg_len ? r.ve + extr : ctg_len;
	static thread_local std::vector<uint8_t> nt;
	static thread_local std::vector<uint64_t> sd;
	g_acc[13] += 1000000LL * 1;                                // (count of refined regions, printed /1e6/threads)
	if (dev_hits) {                                            // the window was scanned on the device
		AccTimer tm(11);
		sd.assign(dev_hits, dev_hits + n_dev_hits);
		refine_pairs_from_hits(sd, rq.qk, opt.max_ava, a);
		return;
	}
	nt.resize((size_t)(ae - as));
	{ AccTimer tm(8); fetch_nt(mi, (int32_t)r.vid, as, ae, nt.data()); }
	if (rq.filter) {
		AccTimer tm(9);
		refine_seed_pairs(nt.data(), ae - as, mi->opt.min_aa_len, kmer, rq.qk, rq.filter->data(), opt.max_ava, sd, a);
	} else {
		// large k: the reference's own formulation -- sort the window's and the query's (bit 31 set) k-mers together;
		// one sort of the merged list gives the same groups (query entries never equal reference entries)
		AccTimer tm(10);
		sketch_nt4(nt.data(), ae - as, mi->opt.min_aa_len, kmer, 0, 0, 0, sd, false);
		for (uint64_t x : rq.qk) sd.push_back(x | 1ULL << 31);
		sort_u64(sd.data(), sd.data() + sd.size());
		sd.erase(std::unique(sd.begin(), sd.end()), sd.end());
		a.clear();
		const size_t n = sd.size();
		for (size_t k = 0, i = 1; i <= n; ++i) {
			if (i < n && sd[k] >> 32 == sd[i] >> 32) continue;
			size_t j = k;
			while (j < i && !(sd[j] >> 31 & 1)) ++j;
			const int64_t n1 = (int64_t)(j - k), n2 = (int64_t)(i - j);
			if (n1 > 0 && n2 > 0 && (int32_t)n1 * (int32_t)n2 <= opt.max_ava)
				for (size_t i1 = k; i1 < j; ++i1)
					for (size_t i2 = j; i2 < i; ++i2)
						a.push_back((uint64_t)(uint32_t)sd[i1] << 32 | ((uint32_t)sd[i2] << 1 >> 1));
			k = i;
		}
		sort_u64(a.data(), a.data() + a.size());
	}
}

static void refine_region_from_chains(const mpa_idx_s *mi, const mpa_mapopt_t &opt, Region &r, int32_t extl, const uint64_t *u, int64_t n_u, const uint64_t *a);
// The refinement chain of a region over those anchors and what mp_refine_reg() makes of it (map.c:81-111).  f/pred != nullptr:
// the forward pass of the chain ran on the device (dev_chain_forward).
static void refine_region_chain(const mpa_idx_s *mi, const mpa_mapopt_t &opt, Region &r, int32_t extl, std::vector<uint64_t> &a,
                                const int32_t *f = nullptr, const int32_t *pred = nullptr)
{
	const ChainParams cp = refine_chain_params(opt);
	std::vector<uint64_t> u;
	{ AccTimer tm(12); if (f) chain_anchors_after_forward(cp, f, pred, a, u); else chain_anchors(cp, a, u); }
	refine_region_from_chains(mi, opt, r, extl, u.data(), (int64_t)u.size(), a.data());
}

// ... what mp_refine_reg() makes of the window's chains (map.c:89-111): u[n_u] = score << 32 | anchors per chain, a = the chains' anchors
static void refine_region_from_chains(const mpa_idx_s *mi, const mpa_mapopt_t &opt, Region &r, int32_t extl, const uint64_t *u, int64_t n_u, const uint64_t *a)
{
	const int32_t kmer = opt.kmer2;
	const int64_t as = r.vs > extl ? r.vs - extl : 0;
	if (n_u == 0) { r.cnt = 0, r.off = -1, r.a.clear(); return; }
	// the first chain with the highest score
	size_t best = 0, skip = 0;
	for (size_t i = 1; i < (size_t)n_u; ++i) if ((int32_t)(u[best] >> 32) < (int32_t)(u[i] >> 32)) best = i;
	for (size_t i = 0; i < best; ++i) skip += (uint32_t)u[i];
	const size_t n_a = (uint32_t)u[best];
	r.a.assign(a + skip, a + skip + n_a);
	r.chn_sc = (int32_t)(u[best] >> 32);
	r.cnt = (int32_t)n_a, r.off = 0;
	r.qs = (int32_t)(uint32_t)r.a[0] - (kmer - 1);
	r.qe = (int32_t)(uint32_t)r.a[n_a - 1] + 1;
	r.vs = as + (int64_t)(r.a[0] >> 32) + 1 - 3 * kmer;
	r.ve = as + (int64_t)(r.a[n_a - 1] >> 32) + 1;
	for (uint64_t &x : r.a) x = (uint64_t)((int64_t)(x >> 32) + as - r.vs) << 32 | (x << 32 >> 32);
	r.chn_sc_ungap = chain_score_ungapped(r.a.data(), r.cnt, kmer);
}

static void refine_region(const mpa_idx_s *mi, const mpa_mapopt_t &opt, const RefineQuery &rq, Region &r, int32_t extl, int32_t extr,
                          const uint64_t *dev_hits = nullptr, int64_t n_dev_hits = 0)
{
	static thread_local std::vector<uint64_t> a;
	refine_region_pairs(mi, opt, rq, r, extl, extr, dev_hits, n_dev_hits, a);
	refine_region_chain(mi, opt, r, extl, a);
}

// mp_filter_seed (align.c:6-31): mark (bit 31) anchors inside tight, in-frame runs, trimmed at both ends
static void mark_reliable_anchors(std::vector<uint64_t> &a, int32_t max_aa_dist, int32_t min_cnt, int32_t kmer2, int32_t trim)
{
	const int32_t cnt = (int32_t)a.size();
	for (int32_t i = 0; i < cnt; ++i) {
		int32_t j = i + 1;
		for (; j < cnt; ++j) {
			const int32_t dx = (int32_t)(a[j] >> 32) - (int32_t)(a[j - 1] >> 32), dy = (int32_t)a[j] - (int32_t)a[j - 1];
			if (dx % 3 != 0 || dx > max_aa_dist * 3 || dy > max_aa_dist) break;
		}
		if (j - i < min_cnt) continue;
		int32_t k = j - 2, t = (int32_t)a[j - 1];
		while (k >= i && t - (int32_t)a[k] < trim) --k;
		t = (int32_t)a[i] + 1 - kmer2;
		while (i < k && (int32_t)a[i] + 1 - t < trim) ++i;
		for (; i <= k; ++i) a[i] |= 1ULL << 31;
		i = j - 1;
	}
}

// first half of mp_align (align.c:239-301,316-323): window, left/right extension tasks
static bool plan_alignment(const mpa_batch_s *b, QueryState &qs, int32_t ridx, int32_t extl0, int32_t extr0, AlignPlan &pl)
{
	const mpa_mapopt_t &opt = b->opt;
	Region &r = qs.regs[ridx];
	mark_reliable_anchors(r.a, 6, 3, opt.kmer2, opt.kmer2 + 1);
	int32_t i0 = 0;
	while (i0 < r.cnt && !(r.a[i0] >> 31 & 1)) ++i0;
	if (i0 == r.cnt) { r.cnt = 0; return false; }
	int32_t extl = opt.max_ext, extr = opt.max_ext;
	if (r.qs >= 10) extl = opt.max_intron / 2;
	if (qs.qlen - r.qe >= 10) extr = opt.max_intron / 2;
	if (extl0 > 0) extl = std::min(extl, extl0);
	if (extr0 > 0) extr = std::min(extr, extr0);
	const int64_t ctg_len = b->mi->ctg[r.vid >> 1].len;
	pl.reg = ridx, pl.i0 = i0;
	pl.as = r.vs > extl ? r.vs - extl : 0;
	pl.ae = r.ve + extr < ctg_len ? r.ve + extr : ctg_len;
	pl.vs0 = r.vs;
	pl.vs1 = pl.vs0 + (int64_t)(r.a[i0] >> 32) + 1;
	pl.as1 = (int32_t)((uint32_t)r.a[i0] << 1 >> 1) + 1;
	// where the gap-patching loop will leave r->ve / r->qe: the end of the last kept anchor
	int32_t ne = 0, ae = 0;
	for (int32_t i = i0; i < r.cnt; ++i)
		if (r.a[i] >> 31 & 1) ne = (int32_t)(r.a[i] >> 32) + 1, ae = (int32_t)((uint32_t)r.a[i] << 1 >> 1) + 1;
	pl.mid_ve = ne + pl.vs0, pl.mid_qe = ae;
	pl.has_right = pl.mid_qe < qs.qlen && pl.mid_ve < pl.ae;
	return true;
}

static mpa_dp_task_t make_task(const QueryState &qs, const Region &r, int64_t nt_off, int64_t nl, int32_t aa_off, int32_t al, int32_t flag, int32_t io)
{
	mpa_dp_task_t t;
	t.nt_off = nt_off, t.vid = (int32_t)r.vid, t.nl = (int32_t)nl, t.qid = qs.qid, t.aa_off = aa_off, t.al = al, t.flag = flag, t.io = io, t.tag = 0;
	return t;
}

// mp_map() in sub-stages.  (1) the query's seeds that are not too frequent (map.c:152-170)
void stage_seeds(mpa_batch_s *b, QueryState &qs)
{
	const mpa_idx_s *mi = b->mi;
	const mpa_mapopt_t &opt = b->opt;
	const int64_t n_bucket = (int64_t)mi->ki.size();
	static thread_local std::vector<uint64_t> sd;
	AccTimer tm(0);
	sketch_protein(qs.seq, qs.qlen, mi->opt.kmer, mi->opt.mod_bit, sd);
	sort_u64(sd.data(), sd.data() + sd.size());
	int32_t max_occ = opt.max_occ;
	if (sd.size() >= 8) max_occ = std::min(max_occ, occurrence_cutoff(mi, sd));
	// kept in ascending query position so that the anchor sort only has to look at the block ids
	qs.seeds.clear(), qs.n_anchor = 0, qs.max_occ = max_occ, qs.seeds_ready = true;
	for (uint64_t s : sd) {
		const int64_t bkt = (int64_t)(s >> 32), st = mi->ki[bkt], en = bkt + 1 < n_bucket ? mi->ki[bkt + 1] : mi->n_kb;
		if (en - st <= max_occ && en > st) qs.n_anchor += en - st, qs.seeds.push_back((uint64_t)(uint32_t)s << 32 | (uint64_t)bkt);
	}
	std::sort(qs.seeds.begin(), qs.seeds.end());
}

static inline ChainParams prechain_params(const mpa_idx_s *mi, const mpa_mapopt_t &opt)
{
	const int32_t w = 1 << mi->opt.bbit;
	return ChainParams{ w, w, w, opt.max_chn_max_skip, opt.max_chn_iter, 2, 0, opt.chn_coef_log, !(opt.flag & MPA_MF_NO_SPLICE), mi->opt.kmer, mi->opt.bbit };
}
static inline bool prechain_enabled(const mpa_mapopt_t &opt) { return !(opt.flag & MPA_MF_NO_PRE_CHAIN) && !(opt.flag & MPA_MF_NO_SPLICE); }

// (2, host) anchors of the kept seeds (map.c:171-178), sorted; the pre-chain keeps those with a neighbour within one block
void stage_anchors_host(mpa_batch_s *b, QueryState &qs, std::vector<uint64_t> &a)
{
	const mpa_idx_s *mi = b->mi;
	const mpa_mapopt_t &opt = b->opt;
	const int64_t n_bucket = (int64_t)mi->ki.size();
	static thread_local std::vector<uint64_t> u;
	a.clear();
	if (!qs.seeds_ready) stage_seeds(b, qs);                   // (the batch was sketched on the device, and this query comes back to the host)
	{
		AccTimer tm(0);
		a.reserve((size_t)qs.n_anchor);
		for (uint64_t kq : qs.seeds) {
			const int64_t bkt = (int64_t)(uint32_t)kq, st = mi->ki[bkt], en = bkt + 1 < n_bucket ? mi->ki[bkt + 1] : mi->n_kb;
			const uint64_t qpos = kq >> 32;
			for (int64_t j = st; j < en; ++j) a.push_back((uint64_t)mi->kb.at((size_t)j) << 32 | qpos);   // (at(): a mapped .mpi may leave kb misaligned)
		}
	}
	g_acc[14] += (int64_t)a.size() * 1000;
	{ AccTimer tm(1); sort_anchors_by_block(a); }
	if (prechain_enabled(opt)) {
		AccTimer tm(2);
		chain_anchors_set(prechain_params(mi, opt), a);          // (ascending: the sort of map.c:192 is implied)
		g_acc[15] += (int64_t)a.size() * 1000;
	}
}

// (2, GPU) the same from the sparse result of dev_prechain_forward(): extraction only
void stage_anchors_from_device(mpa_batch_s *b, QueryState &qs, const PrechainSparse &ps, std::vector<uint64_t> &a)
{
	if (!ps.on_host.empty() && ps.on_host[(size_t)qs.qid]) { stage_anchors_host(b, qs, a); return; }   // (the device declined this query: degenerate input)
	AccTimer tm(2);
	const int64_t c0 = ps.cfirst[qs.qid], m = ps.cfirst[qs.qid + 1] - c0;
	a.clear();
	g_acc[14] += qs.n_anchor * 1000;
	if (m == 0) return;
	// (the device hands the predecessors over as indices into the query's part of the view)
	const ChainView v{ qs.n_anchor, m, ps.pos + c0, ps.f + c0, ps.pred + c0, ps.a + c0 };
	chain_extract_set(prechain_params(b->mi, b->opt), v, a);      // (ascending already: no sort)
	g_acc[15] += (int64_t)a.size() * 1000;
}

// (3) everything else up to and including the alignment plans (map.c:185-226)
static void stage_windows_from_chains(mpa_batch_s *b, QueryState &qs, const std::vector<uint64_t> &u, const std::vector<uint64_t> &a);

// MPA_GPU_REGIONS: 0 / unset = main chains to refinement windows on the host (host_regions.cpp); 1 = on the device wherever device
// seeding ran both chaining rounds (k_regions, region_kernels.hip): the regions come back instead of the chains; model = the host
// instance of the device's code with a team of one (regions_core.h: the CPU tests), from host or device chains alike
static StepMode regions_mode() { return step_mode("MPA_GPU_REGIONS"); }
static RegionsParams regions_params(const mpa_idx_s *mi, const mpa_mapopt_t &opt)
{
	RegionsParams p;
	p.n_vid = (int32_t)mi->bo.size() - 1, p.bbit = mi->opt.bbit, p.kmer = mi->opt.kmer, p.mask_len = opt.mask_len, p.best_n = opt.best_n;
	p.max_ext = opt.max_ext, p.min_ext = 100, p.min_diff = mi->opt.kmer * 2, p.mask_level = opt.mask_level, p.pri_ratio = opt.pri_ratio * opt.pri_ratio;
	return p;
}
// what the shared core left for a query (on the host or on the device), into its state
static void regions_apply(QueryState &qs, int32_t n_chains, const RegionRec *r, const uint64_t *ext, int32_t n)
{
	qs.n_chains = n_chains;
	qs.regs.clear(), qs.regs.resize((size_t)n);
	for (int32_t i = 0; i < n; ++i) region_from_rec(qs.regs[(size_t)i], r[i]);
	qs.ext_refine.assign(ext, ext + n);
}
// MPA_GPU_REGIONS=model: the shared core with a team of one
static void regions_model(mpa_batch_s *b, QueryState &qs, const uint64_t *u, int32_t n, const uint64_t *a)
{
	static thread_local std::vector<RegionRec> tmp, out;
	static thread_local std::vector<Pair64> key;
	static thread_local std::vector<SortRange> stack;
	static thread_local std::vector<uint32_t> hist;
	static thread_local std::vector<int32_t> prim;
	static thread_local std::vector<uint64_t> cov, ext;
	const size_t N = (size_t)n;
	tmp.resize(N), out.resize(N), key.resize(N), stack.resize(N / 64 + 4), hist.resize(768), prim.resize(N + 2), cov.resize(N), ext.resize(N);
	const RegionsScratch S{ tmp.data(), key.data(), stack.data(), hist.data(), prim.data(), cov.data(), prim.data() + N };
	const int32_t k = regions_core<RegionsSerial>(regions_params(b->mi, b->opt), b->mi->bo.data(), u, n, a, S, out.data(), ext.data());
	regions_apply(qs, n, out.data(), ext.data(), k);
}
static void stage_chain_to_windows(mpa_batch_s *b, QueryState &qs, std::vector<uint64_t> &a)
{
	const mpa_idx_s *mi = b->mi;
	const mpa_mapopt_t &opt = b->opt;
	const int32_t is_splice = !(opt.flag & MPA_MF_NO_SPLICE);
	static thread_local std::vector<uint64_t> u;
	u.clear();
	const ChainParams cp = main_chain_params(mi, opt);
	(void)is_splice;
	{ AccTimer tm(3); chain_anchors(cp, a, u); }
	stage_windows_from_chains(b, qs, u, a);
}

// ... from the main chains (u: score << 32 | anchors per chain; a: their anchors, chain by chain): regions and their windows
static void stage_windows_from_chains(mpa_batch_s *b, QueryState &qs, const std::vector<uint64_t> &u, const std::vector<uint64_t> &a)
{
	const mpa_idx_s *mi = b->mi;
	const mpa_mapopt_t &opt = b->opt;
	std::vector<Region> &regs = qs.regs;
	AccTimer tm(4);
	if (regions_mode() == STEP_MODEL) { regions_model(b, qs, u.data(), (int32_t)u.size(), a.data()); return; }
	qs.n_chains = (int32_t)u.size();
	regions_from_chains(mi, u, a, regs);
	sort_regions(regs);
	assign_parents(opt.mask_level, opt.mask_len, regs, mi->opt.kmer);
	select_secondary(opt.pri_ratio * opt.pri_ratio, mi->opt.kmer * 2, opt.best_n, regs);
	// refinement at base resolution (map.c:205-222): its windows
	extension_limits(nullptr, regs, &a, 100, opt.max_ext, qs.ext_refine);
}

// the window mp_refine_reg() re-seeds (map.c:36-41)
static inline void refine_window(const mpa_idx_s *mi, const Region &r, uint64_t ext, int64_t *as, int64_t *ae)
{
	const int64_t ctg_len = mi->ctg[r.vid >> 1].len;
	const int32_t extl = (int32_t)(ext >> 32), extr = (int32_t)ext;
	*as = r.vs > extl ? r.vs - extl : 0;
	*ae = r.ve + extr < ctg_len ? r.ve + extr : ctg_len;
}

// (4) refinement of every region (with the device's scan results if there are any), then the alignment plans
// rc != nullptr: the whole refinement ran on the device (dev_refine_chains): the chains of refinement window w = qs.win0 + region
static void stage_refine_to_plan(mpa_batch_s *b, QueryState &qs, const RefineHits *rh, const RefineChains *rc = nullptr)
{
	const mpa_idx_s *mi = b->mi;
	const mpa_mapopt_t &opt = b->opt;
	std::vector<Region> &regs = qs.regs;
	std::vector<uint64_t> &ext = qs.ext_refine;
	{
		AccTimer tm(5);
		std::vector<Region> kept;
		if (rc) {
			std::unique_ptr<RefineQuery> rq;                         // (only for a window the device handed back: rc->on_host)
			for (size_t i = 0; i < regs.size(); ++i) {
				const size_t w = (size_t)qs.win0 + i;
				if (!rc->on_host.empty() && rc->on_host[w]) {
					if (!rq) rq.reset(new RefineQuery(qs.seq, qs.qlen, opt.kmer2));
					refine_region(mi, opt, *rq, regs[i], (int32_t)(ext[i] >> 32), (int32_t)ext[i]);
				} else {
					g_acc[13] += 1000000LL;
					refine_region_from_chains(mi, opt, regs[i], (int32_t)(ext[i] >> 32), rc->U + rc->u_first[w], rc->u_first[w + 1] - rc->u_first[w], rc->A + rc->a_first[w]);
				}
				if (regs[i].cnt > 0) kept.push_back(std::move(regs[i]));
			}
		} else {
			RefineQuery rq(qs.seq, qs.qlen, opt.kmer2, rh == nullptr);
			for (size_t i = 0; i < regs.size(); ++i) {
				if (rh) {
					const int64_t w = qs.win0 + (int64_t)i;
					refine_region(mi, opt, rq, regs[i], (int32_t)(ext[i] >> 32), (int32_t)ext[i], rh->hits.data() + rh->first[w], rh->first[w + 1] - rh->first[w]);
				} else refine_region(mi, opt, rq, regs[i], (int32_t)(ext[i] >> 32), (int32_t)ext[i]);
				if (regs[i].cnt > 0) kept.push_back(std::move(regs[i]));
			}
		}
		regs.swap(kept);
	}
	AccTimer tm6(6);
	sort_regions(regs);
	assign_parents(opt.mask_level, opt.mask_len, regs, mi->opt.kmer);
	select_secondary(opt.pri_ratio * opt.pri_ratio, mi->opt.kmer * 2, opt.best_n, regs);
	if (opt.flag & MPA_MF_NO_ALIGN) return;
	// alignment plans (map.c:223-227, align.c:239-267)
	extension_limits(mi, regs, nullptr, 100, opt.max_intron / 2, ext);
	for (size_t i = 0; i < regs.size(); ++i) {
		AlignPlan pl;
		if (plan_alignment(b, qs, (int32_t)i, (int32_t)(ext[i] >> 32), (int32_t)ext[i], pl)) qs.plans.push_back(std::move(pl));
	}
}

// ------------------------------------------------------------------------------------------------
// round-1 tasks
// ------------------------------------------------------------------------------------------------
static int32_t ungapped_score(const mpa_idx_s *mi, const mpa_mapopt_t &opt, const Region &r, int64_t nt_off, int32_t alen, const char *aa)
{
	std::vector<uint8_t> nt((size_t)alen * 3);
	fetch_nt(mi, (int32_t)r.vid, nt_off, nt_off + (int64_t)alen * 3, nt.data());
	const uint8_t *aa20 = tab_aa20();
	int32_t sc = 0;
	// NB: the reference's loop (align.c:36) advances its nucleotide index by 3 but bounds it by the AMINO-ACID
	// length, so only the first ceil(alen/3) codons contribute to AS:i.  Reproduced for byte-identical output.
	for (int32_t i = 0, j = 0; i < alen; i += 3, ++j) sc += opt.mat[codon_aa(&nt[i]) * opt.asize + aa20[(uint8_t)aa[j]]];
	return sc;
}

// one mp_align_seq() call: either the ungapped shortcut (align.c:65-67) or a DP task with traceback
void make_segment(mpa_batch_s *b, const QueryState &qs, const Region &r, const AlignPlan &pl, int32_t ne0, int32_t ne1, int32_t ae0, int32_t ae1,
                  int32_t qi, int32_t pi, std::vector<mpa_dp_task_t> &tasks, Segment &s)
{
	const mpa_mapopt_t &opt = b->opt;
	s.ne0 = ne0, s.ne1 = ne1, s.ae0 = ae0, s.ae1 = ae1;
	const int32_t nlen = ne1 - ne0, alen = ae1 - ae0;
	if (nlen == alen * 3 && alen <= opt.kmer2) {
		s.task = -1;
		s.score = ungapped_score(b->mi, opt, r, pl.vs0 + ne0, alen, qs.seq + ae0);
		s.cigar.assign(1, (uint32_t)alen << 4);
	} else {
		s.task = (int32_t)tasks.size();
		tasks.push_back(make_task(qs, r, pl.vs0 + ne0, nlen, ae0, alen, MPA_F_CIGAR, opt.io));
	}
}

// round-1 tasks of one query: both extensions of every region plus the gaps between kept anchors
// (align.c:305-313, all iterations but the first).  Runs inside the threaded stage A.
// The reference repeats an extension that did not reach the end of the protein with the cheaper intron penalty of a terminal exon
// (io_end) on a window of at most max_ext rows (align.c:290-296, 324-331).  Whether it will is known only after the first call, but
// WHAT it would compute is not: window, protein slice and penalty depend on the plan alone.  So the repeat is issued speculatively
// next to the first call -- at most max_ext (1 000) rows against windows of max_intron / 2, about 4 % more extension rows at
// config 3 -- and a batch needs two DP rounds instead of three: one launch, one host round trip and one tail fewer.
static void plan_round1(mpa_batch_s *b, QueryState &qs)
{
	const mpa_mapopt_t &opt = b->opt;
	const bool retry = opt.io > opt.io_end;
	for (size_t pi = 0; pi < qs.plans.size(); ++pi) {
		AlignPlan &pl = qs.plans[pi];
		const Region &r = qs.regs[pl.reg];
		pl.t_left = (int32_t)qs.local1.size();
		qs.local1.push_back(make_task(qs, r, pl.as, pl.vs1 - pl.as, 0, pl.as1, MPA_F_EXT_LEFT | MPA_F_SS_SKIP0, opt.io));   // starts at the window's first position
		if (retry) {                                          // 5'-end exon: the same with a cheaper intron, on the window's last max_ext rows
			const int64_t as_alt = pl.vs1 - pl.as > opt.max_ext ? pl.vs1 - opt.max_ext : pl.as;
			pl.t_left2 = (int32_t)qs.local1.size();
			qs.local1.push_back(make_task(qs, r, as_alt, pl.vs1 - as_alt, 0, pl.as1, MPA_F_EXT_LEFT | (as_alt == pl.as ? MPA_F_SS_SKIP0 : 0), opt.io_end));
		}
		if (pl.has_right) {
			pl.t_right = (int32_t)qs.local1.size();
			qs.local1.push_back(make_task(qs, r, pl.mid_ve, pl.ae - pl.mid_ve, pl.mid_qe, qs.qlen - pl.mid_qe, MPA_F_EXT_RIGHT, opt.io));
			if (retry) {                                      // 3'-end exon
				const int64_t l_ext = std::min<int64_t>(pl.ae - pl.mid_ve, opt.max_ext);
				pl.t_right2 = (int32_t)qs.local1.size();
				qs.local1.push_back(make_task(qs, r, pl.mid_ve, l_ext, pl.mid_qe, qs.qlen - pl.mid_qe, MPA_F_EXT_RIGHT, opt.io_end));
			}
		}
		int32_t ne0 = (int32_t)(pl.vs1 - pl.vs0), ae0 = pl.as1;
		for (int32_t i = pl.i0 + 1; i < r.cnt; ++i) {
			if (!(r.a[i] >> 31 & 1)) continue;
			const int32_t ne1 = (int32_t)(r.a[i] >> 32) + 1, ae1 = (int32_t)((uint32_t)r.a[i] << 1 >> 1) + 1;
			pl.gaps.emplace_back();
			make_segment(b, qs, r, pl, ne0, ne1, ae0, ae1, qs.qid, (int32_t)pi, qs.local1, pl.gaps.back());
			ne0 = ne1, ae0 = ae1;
		}
	}
}

void emit_round1(mpa_batch_s *b)
{
	int64_t n = 0;
	for (QueryState &qs : b->qs) qs.base1 = n, n += (int64_t)qs.local1.size();
	b->tasks.resize((size_t)n);
	parallel_for(b->n_threads, (int64_t)b->qs.size(), [&](int64_t qi) {
		QueryState &qs = b->qs[qi];
		if (!qs.local1.empty()) memcpy(&b->tasks[qs.base1], qs.local1.data(), qs.local1.size() * sizeof(mpa_dp_task_t));
	});
}

// ------------------------------------------------------------------------------------------------
// the phases of a batch
// ------------------------------------------------------------------------------------------------

// MPA_GPU_SEED: 0 = seeding always on the host, 1 = always on the device, unset = by the size of the batch
static thread_local int tl_seed_mode = -2;          // (the mpa_dbg_* test hooks force a mode for their own call, on their own thread)
static int gpu_seeding_mode()
{
	if (tl_seed_mode != -2) return tl_seed_mode;
	const char *e = getenv("MPA_GPU_SEED");             // (read per call: the tests flip it)
	return e ? (atoi(e) != 0 ? 1 : 0) : -1;
}
SeedModeScope::SeedModeScope(int m) : keep(tl_seed_mode) { tl_seed_mode = m; }
SeedModeScope::~SeedModeScope() { tl_seed_mode = keep; }
// Below this many anchors per mini-batch the host's own sort + forward pass is faster than a round trip to a GPU that is
// busy with DP rounds (measured: 2.7 M anchors at config 2 -> host, 25 M at 600 Mbp and 240 M at config 3 -> device).
static const int64_t kDeviceSeedingMinAnchors = 8000000;

// The on/off knobs of seeding (read per call: the tests flip them):
// MPA_GPU_SKETCH: 1 = the sketch stage runs on the device wherever device seeding does (sketch_exec.hip); 0 / unset = on the host
// MPA_GPU_SEED_NOPRE: 1 = a run without a pre-chain (-S, --no-pre-chain) is seeded and chained on the device too, where MPA_GPU_SEED
// allows device seeding at all (the direct route: dev_seed_direct); 0 / unset = such a run keeps the host stages
static bool knob_on(const char *name)
{
	const char *e = getenv(name);
	return e && atoi(e) != 0;
}
// Which way a batch is seeded, from the options alone (whether the device takes a batch of an eligible route is then a matter of
// MPA_GPU_SEED and its size).  SEED_PRECHAIN: sift -> pre-chain -> main chain (map.c:186 runs the pre-chain).  SEED_DIRECT: sift by
// the main chain's reach -> main chain; its extraction reads a sparse view, which is only valid with min_chn_cnt > 1 (chain_core.h)
// -- a run whose options the extraction would hand back wholesale (chain_ends_sparse_possible) makes no device pass at all.
SeedRoute seed_route(const mpa_mapopt_t &opt, const mpa_idxopt_t &io)
{
	if (io.bbit <= 0) return SEED_ON_HOST;
	if (prechain_enabled(opt)) return SEED_PRECHAIN;
	if (!knob_on("MPA_GPU_SEED_NOPRE")) return SEED_ON_HOST;
	ChainParams p = ChainParams();
	p.min_cnt = opt.min_chn_cnt, p.min_sc = opt.min_chn_sc, p.kmer = io.kmer;
	const ChainView large{ 65, 0, nullptr, nullptr, nullptr, nullptr };      // (a query of 64 anchors or fewer builds the full list whatever the options: it fits)
	return chain_ends_sparse_possible(p, large) ? SEED_DIRECT : SEED_ON_HOST;
}

mpa_batch_s *batch_shell(const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads)
{
	if (mi->kb.empty() && mi->n_kb == 0) { set_error("the index has no k-mer table (genome-only index): cannot map"); return nullptr; }
	mpa_batch_s *b = new mpa_batch_s();
	b->mi = mi, b->opt = *opt, b->q = *q, b->n_threads = n_threads > 1 ? n_threads : 1;
	mpa_dpopt_from_mapopt(opt, &b->dpopt);
	b->qs.resize(q->n_seq);
	for (int32_t i = 0; i < q->n_seq; ++i) {
		b->qs[i].qid = i, b->qs[i].seq = q->seqs + q->q_off[i], b->qs[i].qlen = (int32_t)(q->q_off[i + 1] - q->q_off[i]);
	}
	return b;
}

// Phase 1a of a batch, host only: the seeds of every query (sketch, bucket lookup, occurrence cut-off: map.c:126-177 up to the
// anchor loop) and, if the batch is worth seeding on the device, its seed jobs.  In the stream pipeline this is a stage of its own.
mpa_batch_t *batch_sketch_phase(bool have_device, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads)
{
	mpa_batch_s *b = batch_shell(mi, opt, q, n_threads);
	if (!b) return nullptr;
	// with MPA_GPU_SKETCH the stage runs where its result is consumed: the seeder sketches on the device (batch_device_seed_phase)
	if (have_device && knob_on("MPA_GPU_SKETCH") && gpu_seeding_mode() != 0 && seed_route(*opt, mi->opt) != SEED_ON_HOST && q->n_seq > 0) { b->dev_sketch = true; return b; }
	batch_host_seeds(b, have_device);
	return b;
}

// the host's sketch stage: seeds of every query and, if the batch is worth seeding on the device, its seed jobs
void batch_host_seeds(mpa_batch_s *b, bool have_device)
{
	const mpa_idx_t *mi = b->mi;
	const mpa_mapopt_t *opt = &b->opt;
	const mpa_qbatch_t *q = &b->q;
	const double t0 = now_ms();
	parallel_for(b->n_threads, q->n_seq, [&](int64_t i) { stage_seeds(b, b->qs[i]); });
	timing_note("  A1: seeds of all queries", now_ms() - t0);
	const int mode = gpu_seeding_mode();
	if (!have_device || mode == 0 || seed_route(*opt, mi->opt) == SEED_ON_HOST || q->n_seq == 0) return;
	std::vector<int64_t> &qfirst = b->seed_qfirst;
	std::vector<size_t> jfirst((size_t)q->n_seq + 1, 0);
	qfirst.assign((size_t)q->n_seq + 1, 0);
	for (int32_t i = 0; i < q->n_seq; ++i) qfirst[i + 1] = qfirst[i] + b->qs[i].n_anchor, jfirst[i + 1] = jfirst[i] + b->qs[i].seeds.size();
	if ((mode < 0 && qfirst[q->n_seq] < kDeviceSeedingMinAnchors) || jfirst[q->n_seq] == 0) { qfirst.clear(); return; }
	b->seed_jobs.resize(jfirst[q->n_seq]);
	const int64_t n_bucket = (int64_t)mi->ki.size();
	SeedJob *const jobs_p = b->seed_jobs.data();
	const int64_t *const qfirst_p = qfirst.data();
	const size_t *const jfirst_p = jfirst.data();
	parallel_for(b->n_threads, q->n_seq, [&, jobs_p, qfirst_p, jfirst_p](int64_t i) {
		int64_t dst = qfirst_p[i];
		size_t j = jfirst_p[i];
		for (uint64_t kq : b->qs[i].seeds) {
			const int64_t bkt = (int64_t)(uint32_t)kq, st = mi->ki[bkt], en = bkt + 1 < n_bucket ? mi->ki[bkt + 1] : mi->n_kb;
			jobs_p[j++] = SeedJob{ st, dst, (int32_t)(en - st), (int32_t)(kq >> 32), (int32_t)i };
			dst += en - st;
		}
	});
	timing_note("  A1: seed jobs", now_ms() - t0);
}

// Phase 1b: the anchors of the seed jobs, the pre-chain and the main chain on the device (seed_exec.hip).  false = error.
// sketch_ms: receives the wall time of the sketch stage where it ran in this phase (MPA_GPU_SKETCH), else 0
bool batch_device_seed_phase(mpa_ctx_t *seed_ctx, mpa_batch_s *b, bool want_chains, SeedHold *hold, double *sketch_ms, bool for_planner)
{
	if (sketch_ms) *sketch_ms = 0;
	if (!seed_ctx) return true;
	const mpa_idx_t *mi = b->mi;
	const SeedRoute route = seed_route(b->opt, mi->opt);
	if (route == SEED_DIRECT && !want_chains) {          // (there is no pre-chain whose survivors the device could return: the host stages)
		if (b->dev_sketch) { b->dev_sketch = false; batch_host_seeds(b, false); }
		std::vector<SeedJob>().swap(b->seed_jobs);
		std::vector<int64_t>().swap(b->seed_qfirst);
		return true;
	}
	SketchResult sk;
	bool jobs_on_device = false;
	if (b->dev_sketch) {
		// the sketch stage on the device: its jobs stay in the seeder context's HBM, the prefix arrays and flags come back
		b->dev_sketch = false;
		const double t0 = now_ms();
		const int rc = dev_sketch_jobs(seed_ctx, const_cast<mpa_idx_s*>(mi), b->opt.max_occ, &b->q, sk);
		if (rc == MPA_ERR_UNSUPPORTED) {                // (no device memory for ki, k > 7, a batch beyond 32-bit job indices)
			if (timing_on()) fprintf(stderr, "[mpa-timing]   device sketch declined (%s): sketch on the host\n", mpa_last_error());
			batch_host_seeds(b, true);
		} else if (rc != MPA_OK) return false;
		else {
			timing_note("  sketch on the GPU (sketch + lookup + cut-off + seed jobs)", now_ms() - t0);
			for (int32_t i = 0; i < b->q.n_seq; ++i) b->qs[i].n_anchor = sk.qfirst[i + 1] - sk.qfirst[i];   // (0 for a query handed back: stage_seeds counts it)
			// MPA_GPU_SEED unset keeps its meaning: a batch under the threshold is seeded on the host, from seeds built when asked for
			jobs_on_device = !((gpu_seeding_mode() < 0 && sk.n_anchor < kDeviceSeedingMinAnchors) || sk.n_jobs == 0);
		}
		if (sketch_ms) *sketch_ms = now_ms() - t0;
		if (rc == MPA_OK && !jobs_on_device) return true;
	}
	if (!jobs_on_device && b->seed_jobs.empty()) return true;
	const double t1 = now_ms();
	// (with the main chain's parameters the device carries on through both chaining rounds, unless the caller only wants the pre-chain)
	const ChainParams main_cp = main_chain_params(mi, b->opt);
	// (MPA_GPU_REGIONS=1 and the caller is the planner, which wants windows, not chains: the main round ends in k_regions)
	const RegionsParams reg_p = regions_params(mi, b->opt);
	const RegionsParams *rp = for_planner && want_chains && regions_mode() == STEP_DEVICE ? &reg_p : nullptr;
	const int rc = route == SEED_DIRECT
		? (jobs_on_device ? dev_seed_direct(seed_ctx, const_cast<mpa_idx_s*>(mi), main_cp, b->q.n_seq, sk.qfirst, nullptr, sk.n_jobs, b->sparse, hold, sk.jfirst, nullptr, rp)
		                  : dev_seed_direct(seed_ctx, const_cast<mpa_idx_s*>(mi), main_cp, b->q.n_seq, b->seed_qfirst.data(), b->seed_jobs.data(), (int64_t)b->seed_jobs.size(), b->sparse, hold,
		                                    nullptr, nullptr, rp))
		: jobs_on_device
		? dev_prechain_forward(seed_ctx, const_cast<mpa_idx_s*>(mi), prechain_params(mi, b->opt), b->q.n_seq, sk.qfirst, nullptr, sk.n_jobs, b->sparse,
		                       want_chains ? &main_cp : nullptr, hold, sk.jfirst, rp)
		: dev_prechain_forward(seed_ctx, const_cast<mpa_idx_s*>(mi), prechain_params(mi, b->opt), b->q.n_seq, b->seed_qfirst.data(), b->seed_jobs.data(),
		                       (int64_t)b->seed_jobs.size(), b->sparse, want_chains ? &main_cp : nullptr, hold, nullptr, rp);
	std::vector<SeedJob>().swap(b->seed_jobs);
	std::vector<int64_t>().swap(b->seed_qfirst);
	if (rc == MPA_ERR_UNSUPPORTED) {                    // e.g. the batch does not fit the device: seed on the host
		if (timing_on()) fprintf(stderr, "[mpa-timing]   device seeding declined (%s): seeding on the host\n", mpa_last_error());
		return true;
	}
	if (rc != MPA_OK) return false;
	b->seeded_on_device = true;
	if (jobs_on_device && sk.n_flagged) {               // queries the sketch kernel handed back have no jobs on the device: the host seeds them
		if (b->sparse.on_host.empty()) b->sparse.on_host.assign((size_t)b->q.n_seq, 0);
		for (int32_t i = 0; i < b->q.n_seq; ++i) if (sk.flag[i]) b->sparse.on_host[(size_t)i] = 1;
	}
	timing_note(route == SEED_DIRECT ? "  seeding on the GPU (direct route: sift by the main chain's reach + main chain, no pre-chain)"
	                                 : "  seeding on the GPU (sift + pre-chain + both chaining rounds)", now_ms() - t1);
	return true;
}

// Phase 1 of a batch: seeds of every query; with a device context and a batch that is worth it, also the anchors, the pre-chain
// and the main chain on the device.
mpa_batch_t *batch_seed_phase(mpa_ctx_t *seed_ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads, bool want_chains, SeedHold *hold, bool for_planner)
{
	mpa_batch_t *b = batch_sketch_phase(seed_ctx != nullptr, mi, opt, q, n_threads);
	if (b && !batch_device_seed_phase(seed_ctx, b, want_chains, hold, nullptr, for_planner)) { delete b; return nullptr; }
	return b;
}

// Phase 2: pre-chain (host: anchors, sort, forward pass, extraction; after device seeding: extraction only), chaining,
// regions, refinement, alignment plans.  b->sparse (pinned memory of the seeding context) is not needed afterwards.
static int gpu_refine_mode()
{
	const char *e = getenv("MPA_GPU_REFINE");           // 0 / 1 / unset = by the size of the batch
	return e ? (atoi(e) != 0 ? 1 : 0) : -1;
}
static const int64_t kDeviceRefineMinBases = 100000000;     // below this the host's own scan is as fast as the round trip

// the packed k-mer words of a query (RefineQuery::words without the bitmap)
void query_words(const char *aa, int32_t l_aa, int32_t k, std::vector<uint32_t> &w)
{
	const uint8_t *aa13 = tab_aa13();
	const uint32_t mask = (1U << 4 * k) - 1;
	uint32_t x = 0;
	w.clear();
	for (int32_t i = 0, run = 0; i < l_aa; ++i) {
		const uint32_t c = aa13[(uint8_t)aa[i]];
		if (c >= 14) { run = 0, x = 0; continue; }
		x = (x << 4 | c) & mask;
		if (++run >= k) w.push_back(x);
	}
}

// the k-mer groups of one query (QueryGroups, host_batch.h)
void query_groups(const char *aa, int32_t l_aa, int32_t k, QueryGroups &out)
{
	const uint8_t *aa13 = tab_aa13();
	const uint32_t mask = (1U << 4 * k) - 1;
	static thread_local std::vector<uint64_t> hk;           // hash << 32 | position
	static thread_local std::vector<uint32_t> wd;           // word of the k-mer ending at position i (by position)
	hk.clear(), wd.assign((size_t)l_aa, 0);
	uint32_t x = 0;
	for (int32_t i = 0, run = 0; i < l_aa; ++i) {
		const uint32_t c = aa13[(uint8_t)aa[i]];
		if (c >= 14) { run = 0, x = 0; continue; }
		x = (x << 4 | c) & mask;
		if (++run >= k) hk.push_back((uint64_t)hash32_mask(x, mask) << 32 | (uint32_t)i), wd[(size_t)i] = x;
	}
	sort_u64(hk.data(), hk.data() + hk.size());
	out.gword.clear(), out.gcount.clear(), out.qpos.clear();
	for (size_t i = 0; i < hk.size(); ++i) {
		if (i == 0 || hk[i] >> 32 != hk[i - 1] >> 32) out.gword.push_back(wd[(size_t)(uint32_t)hk[i]]), out.gcount.push_back(0);
		++out.gcount.back();
		out.qpos.push_back((uint32_t)hk[i]);
	}
}

// the groups of all queries of a batch, back to back (what dev_refine_chains takes)
void gather_query_groups(const QueryGroups *per, int64_t n_q, RefineGroupsHost &G)
{
	G.qg_first.assign((size_t)n_q + 1, 0);
	size_t n_kmer = 0;
	for (int64_t i = 0; i < n_q; ++i) G.qg_first[(size_t)i + 1] = G.qg_first[(size_t)i] + (int64_t)per[(size_t)i].gword.size(), n_kmer += per[(size_t)i].qpos.size();
	G.gword.resize((size_t)G.qg_first[(size_t)n_q]), G.gcount.resize(G.gword.size()), G.gfirst.resize(G.gword.size()), G.qpos.resize(n_kmer);
	size_t at = 0;
	for (int64_t i = 0; i < n_q; ++i) {
		const QueryGroups &p = per[(size_t)i];
		const size_t g0 = (size_t)G.qg_first[(size_t)i];
		size_t k0 = at;
		for (size_t g = 0; g < p.gword.size(); ++g) G.gword[g0 + g] = p.gword[g], G.gcount[g0 + g] = p.gcount[g], G.gfirst[g0 + g] = (uint32_t)k0, k0 += p.gcount[g];
		if (!p.qpos.empty()) memcpy(&G.qpos[at], p.qpos.data(), p.qpos.size() * 4);
		at += p.qpos.size();
	}
}

// MPA_REGIONS_DUMP=<file> (diagnostics; the tests' view of the stage): what the first planning step left for every query of the
// batch, appended in query order, whichever path produced it.  Per query: int32 qid, chains before the selection, n; n records of
// 64 bytes (int32 cnt, id, parent, n_sub, subsc, chn_sc, chn_sc_ungap; uint32 vid; int32 qs, qe; int64 vs, ve; int32 split flag,
// int32 0); n refinement limits (uint64: left << 32 | right).  Layout and parser: tests/regionsdump.py
static void regions_dump(const mpa_batch_s *b)
{
	const char *fn = getenv("MPA_REGIONS_DUMP");
	if (!fn || !*fn) return;
	static std::mutex mu;                                // (batches of a stream are planned side by side: one writer at a time)
	std::lock_guard<std::mutex> g(mu);
	FILE *fp = fopen(fn, "ab");
	if (!fp) return;
	for (const QueryState &qs : b->qs) {
		const int32_t head[3] = { qs.qid, qs.n_chains, (int32_t)qs.regs.size() };
		fwrite(head, 4, 3, fp);
		for (const Region &r : qs.regs) {
			const int32_t w[10] = { r.cnt, r.id, r.parent, r.n_sub, r.subsc, r.chn_sc, r.chn_sc_ungap, (int32_t)r.vid, r.qs, r.qe };
			const int64_t v[2] = { r.vs, r.ve };
			const int32_t t[2] = { r.split, 0 };
			fwrite(w, 4, 10, fp), fwrite(v, 8, 2, fp), fwrite(t, 4, 2, fp);
		}
		if (!qs.regs.empty()) fwrite(qs.ext_refine.data(), 8, qs.regs.size(), fp);
	}
	fclose(fp);
}

// MPA_GPU_PLANS: 0 / unset = refinement chains to regions, plans, round-1 tasks and gap segments on the host (stage_refine_to_plan,
// plan_round1); 1 = on the device wherever dev_refine_chains ran (k_plans, plan_kernels.hip): the records come back instead of the
// refinement chains; model = the host instance of the device's code with a team of one (plans_core.h: the CPU tests), from the
// device's chains or the host refinement's alike
static StepMode plans_mode() { return step_mode("MPA_GPU_PLANS"); }
static PlansParams plans_params(const mpa_idx_s *mi, const mpa_mapopt_t &opt)
{
	PlansParams p;
	p.kmer2 = opt.kmer2, p.kmer = mi->opt.kmer, p.mask_len = opt.mask_len, p.best_n = opt.best_n, p.max_ext = opt.max_ext, p.max_intron = opt.max_intron;
	p.io = opt.io, p.io_end = opt.io_end, p.no_align = (opt.flag & MPA_MF_NO_ALIGN) ? 1 : 0, p.asize = opt.asize;
	p.mask_level = opt.mask_level, p.pri_ratio = opt.pri_ratio * opt.pri_ratio;
	return p;
}
static inline PlansWindow plans_window(const mpa_idx_s *mi, const Region &r, uint64_t ext)
{
	int64_t as, ae;
	refine_window(mi, r, ext, &as, &ae);
	return PlansWindow{ as, r.vid, r.n_sub, r.subsc, r.split };
}
// what the shared core left for a query (on the host or on the device), into its state.  Region::a stays empty: nothing reads it
// behind plan_round1
static void plans_apply(QueryState &qs, const PlansCounts &n, const RegionRec *r, const PlanRec *pl, const mpa_dp_task_t *t, const SegRec *sg)
{
	qs.regs.clear(), qs.regs.resize((size_t)n.n_reg);
	for (int32_t i = 0; i < n.n_reg; ++i) region_from_rec(qs.regs[(size_t)i], r[i]);
	qs.plans.clear(), qs.plans.resize((size_t)n.n_plan);
	for (int32_t i = 0; i < n.n_plan; ++i) {
		AlignPlan &x = qs.plans[(size_t)i];
		const PlanRec &y = pl[i];
		x.reg = y.reg, x.as = y.as, x.ae = y.ae, x.vs0 = y.vs0, x.vs1 = y.vs1, x.as1 = y.as1, x.mid_ve = y.mid_ve, x.mid_qe = y.mid_qe, x.has_right = y.has_right != 0;
		x.t_left = y.t_left, x.t_left2 = y.t_left2, x.t_right = y.t_right, x.t_right2 = y.t_right2;
		x.gaps.resize((size_t)y.n_gap);
		for (int32_t g = 0; g < y.n_gap; ++g) segment_from_rec(x.gaps[(size_t)g], sg[y.gap0 + g]);
	}
	qs.local1.assign(t, t + n.n_task);
}
// MPA_GPU_PLANS=model: the chains of every refinement window of the query -- the device's (rc), or the host refinement's own,
// collected instead of consumed region by region -- through the shared core with a team of one
static void plans_model(mpa_batch_s *b, QueryState &qs, const RefineHits *rh, const RefineChains *rc)
{
	const mpa_idx_s *mi = b->mi;
	const mpa_mapopt_t &opt = b->opt;
	static thread_local std::vector<uint64_t> U, A, pa, pu, cov, ext;
	static thread_local std::vector<int64_t> cu, ca, nu, aoff;
	static thread_local std::vector<PlansWindow> win;
	static thread_local std::vector<RegionRec> tmp, reg;
	static thread_local std::vector<PlanRec> plan;
	static thread_local std::vector<mpa_dp_task_t> task;
	static thread_local std::vector<SegRec> seg;
	static thread_local std::vector<Pair64> key;
	static thread_local std::vector<SortRange> stack;
	static thread_local std::vector<uint32_t> hist;
	static thread_local std::vector<int32_t> prim, flag, list;
	const size_t n = qs.regs.size();
	U.clear(), A.clear(), cu.assign(n, 0), ca.assign(n, 0), nu.assign(n, 0), win.resize(n);
	{
		AccTimer tm(5);
		std::unique_ptr<RefineQuery> rq;
		const ChainParams cp = refine_chain_params(opt);
		for (size_t i = 0; i < n; ++i) {
			const size_t w = (size_t)qs.win0 + i;
			win[i] = plans_window(mi, qs.regs[i], qs.ext_refine[i]);
			cu[i] = (int64_t)U.size(), ca[i] = (int64_t)A.size();
			if (rc && !(!rc->on_host.empty() && rc->on_host[w])) {
				g_acc[13] += 1000000LL;
				U.insert(U.end(), rc->U + rc->u_first[w], rc->U + rc->u_first[w + 1]);
				A.insert(A.end(), rc->A + rc->a_first[w], rc->A + rc->a_first[w + 1]);
			} else {
				if (!rq) rq.reset(new RefineQuery(qs.seq, qs.qlen, opt.kmer2, rc != nullptr || rh == nullptr));
				const int32_t extl = (int32_t)(qs.ext_refine[i] >> 32), extr = (int32_t)qs.ext_refine[i];
				if (rh && !rc) refine_region_pairs(mi, opt, *rq, qs.regs[i], extl, extr, rh->hits.data() + rh->first[w], rh->first[w + 1] - rh->first[w], pa);
				else refine_region_pairs(mi, opt, *rq, qs.regs[i], extl, extr, nullptr, 0, pa);
				{ AccTimer tm12(12); chain_anchors(cp, pa, pu); }
				U.insert(U.end(), pu.begin(), pu.end());
				size_t na = 0;
				for (uint64_t x : pu) na += (uint32_t)x;
				A.insert(A.end(), pa.begin(), pa.begin() + na);
			}
			nu[i] = (int64_t)U.size() - cu[i];
		}
	}
	AccTimer tm6(6);
	const size_t m = A.size();
	tmp.resize(n), reg.resize(n), plan.resize(n), task.resize(4 * n + m), seg.resize(m + 1), key.resize(n), stack.resize(n / 64 + 4), hist.resize(768), prim.resize(n + 2);
	cov.resize(n), ext.resize(n), aoff.resize(n), flag.resize(m + 1), list.resize(m + 1);
	uint8_t tab[ALN_TAB_BYTES];
	aln_tables_fill(tab, opt.mat, 484);
	const PlansQuery Q{ (int32_t)n, qs.qid, qs.qlen, win.data(), cu.data(), ca.data(), nu.data(), U.data(), A.data(), (const uint8_t*)qs.seq };
	const PlansScratch S{ tmp.data(), key.data(), stack.data(), hist.data(), prim.data(), cov.data(), ext.data(), aoff.data(), flag.data(), list.data(), prim.data() + n };
	const PlansCounts c = plans_core<PlansSerial>(plans_params(mi, opt), Q, PlansGenomeHost{ mi }, tab, S, reg.data(), plan.data(), task.data(), seg.data());
	plans_apply(qs, c, reg.data(), plan.data(), task.data(), seg.data());
}

// MPA_PLANS_DUMP=<file> (diagnostics; the tests' view of the step): what the step from the refinement chains to the round-1 tasks left
// in every query's state, appended in query order, whichever path produced it.  Per query: int32 qid, regions, plans, tasks, gap
// segments; the regions (64 bytes: as MPA_REGIONS_DUMP, with off where that has 0); the plans (80 bytes: int64 as, ae, vs0, vs1,
// mid_ve; int32 reg, as1, mid_qe, has_right, t_left, t_left2, t_right, t_right2, first gap, gaps); the tasks (mpa_dp_task_t, 40
// bytes); the segments (24 bytes: int32 ne0, ne1, ae0, ae1, task, score).  Layout and parser: tests/plansdump.py
static void plans_dump(const mpa_batch_s *b)
{
	const char *fn = getenv("MPA_PLANS_DUMP");
	if (!fn || !*fn) return;
	static std::mutex mu;                                // (batches of a stream are planned side by side: one writer at a time)
	std::lock_guard<std::mutex> g(mu);
	FILE *fp = fopen(fn, "ab");
	if (!fp) return;
	for (const QueryState &qs : b->qs) {
		int32_t n_seg = 0;
		for (const AlignPlan &pl : qs.plans) n_seg += (int32_t)pl.gaps.size();
		const int32_t head[5] = { qs.qid, (int32_t)qs.regs.size(), (int32_t)qs.plans.size(), (int32_t)qs.local1.size(), n_seg };
		fwrite(head, 4, 5, fp);
		for (const Region &r : qs.regs) {
			const int32_t w[10] = { r.cnt, r.id, r.parent, r.n_sub, r.subsc, r.chn_sc, r.chn_sc_ungap, (int32_t)r.vid, r.qs, r.qe };
			const int64_t v[2] = { r.vs, r.ve };
			const int32_t t[2] = { r.split, r.off };
			fwrite(w, 4, 10, fp), fwrite(v, 8, 2, fp), fwrite(t, 4, 2, fp);
		}
		int32_t gap0 = 0;
		for (const AlignPlan &pl : qs.plans) {
			const int64_t v[5] = { pl.as, pl.ae, pl.vs0, pl.vs1, pl.mid_ve };
			const int32_t w[10] = { pl.reg, pl.as1, pl.mid_qe, pl.has_right ? 1 : 0, pl.t_left, pl.t_left2, pl.t_right, pl.t_right2, gap0, (int32_t)pl.gaps.size() };
			fwrite(v, 8, 5, fp), fwrite(w, 4, 10, fp);
			gap0 += (int32_t)pl.gaps.size();
		}
		if (!qs.local1.empty()) fwrite(qs.local1.data(), sizeof(mpa_dp_task_t), qs.local1.size(), fp);
		for (const AlignPlan &pl : qs.plans)
			for (const Segment &s : pl.gaps) {
				// (a shortcut segment carries its one-word cigar alen << 4 on every path; one that does not shows as the impossible score)
				const bool bare = s.task < 0 && !(s.cigar.size() == 1 && s.cigar[0] == (uint32_t)(s.ae1 - s.ae0) << 4);
				const int32_t w[6] = { s.ne0, s.ne1, s.ae0, s.ae1, s.task, bare ? INT32_MIN : s.score };
				fwrite(w, 4, 6, fp);
			}
	}
	fclose(fp);
}

// Phase 2 in three steps.  (a) anchors (host, or the device's pre-chain / chains / regions) to the refinement windows of every query
static void plan_windows(mpa_batch_s *b)
{
	const double t0 = now_ms();
	const int64_t n_q = (int64_t)b->qs.size();
	parallel_for(b->n_threads, n_q, [&](int64_t i) {
		static thread_local std::vector<uint64_t> a, u;
		const PrechainSparse &ps = b->sparse;
		if (b->seeded_on_device && ps.has_chains && !(!ps.on_host.empty() && ps.on_host[(size_t)i])) {
			// both chaining rounds ran on the device: its chains are what mp_chain() returns for this query (map.c:195)
			g_acc[14] += b->qs[i].n_anchor * 1000;
			if (ps.has_regions) {                              // ... and k_regions has made the windows from them: nothing to do but take them
				AccTimer tm(4);
				const int64_t u0 = ps.u_first[(size_t)i];
				regions_apply(b->qs[i], (int32_t)(ps.u_first[(size_t)i + 1] - u0), ps.R + u0, ps.E + u0, ps.n_reg[i]);
				return;
			}
			u.assign(ps.U + ps.u_first[(size_t)i], ps.U + ps.u_first[(size_t)i + 1]);
			a.assign(ps.A + ps.a_first[(size_t)i], ps.A + ps.a_first[(size_t)i + 1]);
			stage_windows_from_chains(b, b->qs[i], u, a);
			return;
		}
		if (b->seeded_on_device && !ps.has_chains) stage_anchors_from_device(b, b->qs[i], ps, a);
		else stage_anchors_host(b, b->qs[i], a);
		stage_chain_to_windows(b, b->qs[i], a);
	});
	if (timing_on()) {
		const PrechainSparse &ps = b->sparse;
		if (b->seeded_on_device && ps.has_regions) {
			int64_t n_rec = 0;
			for (int64_t i = 0; i < n_q; ++i) n_rec += ps.n_reg[i];
			fprintf(stderr, "[mpa-timing]   regions on the GPU: %lld queries, records downloaded %lld B, anchors downloaded 0 B, anchors and chains not downloaded %lld B\n", (long long)n_q,
			        (long long)(n_rec * (int64_t)(sizeof(RegionRec) + 8) + n_q * 4), (long long)((ps.a_first[(size_t)n_q] + ps.u_first[(size_t)n_q]) * 8));
		}
		if (regions_mode() == STEP_MODEL) timing_note("  regions: shared core", now_ms() - t0);
	}
	b->sparse = PrechainSparse();
	regions_dump(b);
	timing_note("  plan: anchors..windows (wall)", now_ms() - t0);
}

// what the device made of a batch's refinement windows: their chains (with MPA_GPU_PLANS=1 the plans too), or the hits of the scan alone
struct MPA_HOST_LOCAL DeviceRefinement {
	RefineHits rh;
	RefineChains rchains;
	bool on_device = false, chains_on_device = false;
};

// (b) the refinement of all windows on the device, or its scan alone, if the batch is worth the round trip
static void plan_refine_on_device(mpa_batch_s *b, mpa_ctx_t *rctx, StepMode pmode, DeviceRefinement &D)
{
	const double t_a = now_ms();
	const int64_t n_q = (int64_t)b->qs.size();
	RefineHits &rh = D.rh;
	RefineChains &rchains = D.rchains;
	bool &on_device = D.on_device, &chains_on_device = D.chains_on_device;
	const int mode = gpu_refine_mode();
	// (outside the kernels' range -- dev_refine_in_range(): -l above 7, -L above 37 -- the host refines; the device is not asked)
	if (rctx && mode != 0 && dev_refine_in_range(b->opt.kmer2, b->mi->opt.min_aa_len)) {
		static thread_local std::vector<RefineWindow> wins;
		static thread_local std::vector<int64_t> qw_first;
		static thread_local std::vector<uint32_t> qwords;
		wins.clear();
		int64_t n_bases = 0;
		for (int64_t i = 0; i < n_q; ++i) {
			QueryState &qs = b->qs[i];
			qs.win0 = (int64_t)wins.size();
			for (size_t r = 0; r < qs.regs.size(); ++r) {
				int64_t as, ae;
				refine_window(b->mi, qs.regs[r], qs.ext_refine[r], &as, &ae);
				wins.push_back(RefineWindow{ as, (int32_t)i, (int32_t)qs.regs[r].vid, (int32_t)(ae - as) });
				n_bases += ae - as;
			}
		}
		if (!wins.empty() && (mode == 1 || n_bases >= kDeviceRefineMinBases)) {
			// the whole refinement on the device: groups of every query (in parallel), then scan + pairing + sort + chains
			static thread_local std::vector<QueryGroups> per;
			static thread_local RefineGroupsHost G;
			per.resize((size_t)n_q);
			QueryGroups *perp = per.data();
			parallel_for(b->n_threads, n_q, [&, perp](int64_t i) { query_groups(b->qs[i].seq, b->qs[i].qlen, b->opt.kmer2, perp[i]); });
			gather_query_groups(perp, n_q, G);
			// MPA_GPU_PLANS=1: the call carries on to the plans; what it needs of the windows' regions and of the queries
			static thread_local std::vector<PlansWindow> pwin;
			static thread_local std::vector<int64_t> pwin0;
			PlansRequest preq;
			const bool want_plans = pmode == STEP_DEVICE;
			if (want_plans) {
				pwin.clear(), pwin0.assign((size_t)n_q + 1, 0);
				for (int64_t i = 0; i < n_q; ++i) {
					const QueryState &qs = b->qs[i];
					pwin0[(size_t)i] = qs.win0;
					for (size_t r = 0; r < qs.regs.size(); ++r) pwin.push_back(plans_window(b->mi, qs.regs[r], qs.ext_refine[r]));
				}
				pwin0[(size_t)n_q] = (int64_t)wins.size();
				preq = PlansRequest{ plans_params(b->mi, b->opt), pwin.data(), pwin0.data(), b->q.seqs, b->q.q_off, b->opt.mat };
			}
			const double t1 = now_ms();
			const int rc = dev_refine_chains(rctx, const_cast<mpa_idx_s*>(b->mi), b->opt.kmer2, b->mi->opt.min_aa_len, b->opt.max_ava, refine_chain_params(b->opt), (int32_t)n_q, G,
			                                 (int64_t)wins.size(), wins.data(), rchains, want_plans ? &preq : nullptr);
			chains_on_device = rc == MPA_OK;                   // anything else: the scan alone below, or the host
			if (chains_on_device) timing_note("  refinement on the GPU (scan + pairs + chains)", now_ms() - t1);
			else if (timing_on()) fprintf(stderr, "[mpa-timing]   device refinement declined (%s)\n", mpa_last_error());
		}
		if (!chains_on_device && !wins.empty() && (mode == 1 || n_bases >= kDeviceRefineMinBases)) {
			std::vector<uint32_t> w;
			qw_first.assign((size_t)n_q + 1, 0), qwords.clear();
			for (int64_t i = 0; i < n_q; ++i) {
				query_words(b->qs[i].seq, b->qs[i].qlen, b->opt.kmer2, w);
				qwords.insert(qwords.end(), w.begin(), w.end());
				qw_first[i + 1] = (int64_t)qwords.size();
			}
			const double t1 = now_ms();
			const int rc = dev_refine_scan(rctx, const_cast<mpa_idx_s*>(b->mi), b->opt.kmer2, b->mi->opt.min_aa_len, (int32_t)n_q, qw_first.data(), qwords.data(),
			                               (int64_t)wins.size(), wins.data(), rh);
			on_device = rc == MPA_OK;                         // anything else: scan on the host
			if (on_device) timing_note("  refinement scan on the GPU", now_ms() - t1);
			else if (timing_on()) fprintf(stderr, "[mpa-timing]   device refinement scan declined (%s): refinement on the host\n", mpa_last_error());
		}
	}
	timing_note("  plan: windows + scan (wall)", now_ms() - t_a);
}

// (c) refinement (what is left of it for the host) to regions, alignment plans and the round-1 tasks of every query
static void plan_refine_to_tasks(mpa_batch_s *b, StepMode pmode, const DeviceRefinement &D)
{
	const int64_t n_q = (int64_t)b->qs.size();
	const RefineChains &rchains = D.rchains;
	const RefineHits *rhp = D.on_device ? &D.rh : nullptr;
	const double t_b = now_ms();
	const RefineChains *rcp = D.chains_on_device ? &rchains : nullptr;
	const bool plans_on_device = D.chains_on_device && rchains.has_plans;
	parallel_for(b->n_threads, n_q, [&, rhp, rcp](int64_t i) {
		QueryState &qs = b->qs[i];
		if (plans_on_device) {                                 // k_plans has made regions, plans, tasks and segments: nothing to do but take them
			AccTimer tm(6);
			const int64_t w0 = qs.win0, a0 = rcp->a_first[(size_t)w0];
			plans_apply(qs, rcp->PN[i], rcp->PR + w0, rcp->PP + w0, rcp->PT + 4 * w0 + a0, rcp->PS + a0);
			return;
		}
		if (pmode == STEP_MODEL) { plans_model(b, qs, rhp, rcp); return; }
		stage_refine_to_plan(b, qs, rhp, rcp);
		AccTimer tm(7);
		plan_round1(b, qs);
	});
	if (timing_on()) {
		if (plans_on_device) {
			int64_t bytes = n_q * (int64_t)sizeof(PlansCounts);
			for (int64_t i = 0; i < n_q; ++i) {
				const PlansCounts &c = rchains.PN[i];
				bytes += (int64_t)c.n_reg * (int64_t)sizeof(RegionRec) + (int64_t)c.n_plan * (int64_t)sizeof(PlanRec) + (int64_t)c.n_task * (int64_t)sizeof(mpa_dp_task_t) + (int64_t)c.n_seg * (int64_t)sizeof(SegRec);
			}
			fprintf(stderr, "[mpa-timing]   plans on the GPU: %lld queries, records downloaded %lld B, refinement anchors downloaded 0 B, anchors and chains not downloaded %lld B\n",
			        (long long)n_q, (long long)bytes, (long long)((rchains.a_first.back() + rchains.u_first.back()) * 8));
		}
		if (pmode == STEP_MODEL) timing_note("  plans: shared core", now_ms() - t_b);
	}
	plans_dump(b);
	timing_note("  plan: refine..plans (wall)", now_ms() - t_b);
}

void batch_plan_phase(mpa_batch_s *b, mpa_ctx_t *rctx)
{
	const double t0 = now_ms();
	plan_windows(b);
	const StepMode pmode = plans_mode();
	DeviceRefinement D;
	plan_refine_on_device(b, rctx, pmode, D);
	plan_refine_to_tasks(b, pmode, D);
	timing_note("stage A (seed..plan)", now_ms() - t0);
	if (timing_on()) for (int k = 0; k < 16; ++k) { timing_note(kAccName[k], (double)g_acc[k].exchange(0) / 1e6); }   // thread CPU ms summed over the workers (13-15: counts)
	if (b->opt.flag & MPA_MF_NO_ALIGN) { b->round = 4; return; }
	// the round-1 task list is part of planning too: in a stream it is ready before a DP lane picks the batch up
	const double t1 = now_ms();
	emit_round1(b);
	timing_note("emit round 1", now_ms() - t1);
	b->round = 1;
	if (b->tasks.empty()) { (void)take_round3(b, nullptr, nullptr); b->round = 4; }   // nothing to align at all (and no context yet: the host walk)
}

mpa_batch_t *batch_begin_impl(mpa_ctx_t *seed_ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int n_threads)
{
	mpa_batch_t *b = batch_seed_phase(seed_ctx, mi, opt, q, n_threads, true, nullptr, true);
	if (b) batch_plan_phase(b, seed_ctx);
	return b;
}

} // namespace mpa
