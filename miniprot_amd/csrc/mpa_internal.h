// mpa_internal.h -- internal declarations shared by the host pipeline and the device units (dev_ctx.h lists those).
// Not part of the C ABI (that is include/mpamd.h).
#pragma once
#include <cstdint>
#include <cstddef>
#include <string>
#include <new>
#include <exception>
#include <vector>
#include <cstring>
#include <cstdlib>
#include "../../include/mpamd.h"
#include "chain_core.h"
#include "aln_stats_core.h"
#include "aln_cs_core.h"
#include "aln_rows_core.h"
#include "regions_core.h"
#include "plans_core.h"
#include "spans_core.h"
#include "finish_core.h"
#include "format_core.h"

namespace mpa {

// ---- tables (tables.cpp) -------------------------------------------------------------------------
// Alphabets follow the reference so that scores, hashes and output text are identical:
// nt4: A0 C1 G2 T3 N4 (nasw-tab.c:6); aa20: ARNDCQEGHILKMFPSTWYV*X (nasw-tab.c:9); aa13: nasw-tab.c:12.
extern const uint8_t *tab_nt4();     // [256]
extern const uint8_t *tab_aa20();    // [256]
extern const uint8_t *tab_aa13();    // [256]
extern const uint8_t *tab_codon();   // [64]  codon -> aa20 for the active translation table
extern const uint8_t *tab_codon13(); // [64]  codon -> reduced alphabet
extern const int8_t *blosum62();     // [484]
int set_trans_code(int code);        // ns_make_tables (nasw-tab.c:85); returns <0 if undefined
extern const char *const kAA;        // "ARNDCQEGHILKMFPSTWYV*X"
// the tables the shared walks read (ALN_TAB_*, aln_stats_core.h) into dst[ALN_TAB_BYTES]: codon table, aa20 and the first mat_bytes of
// the substitution matrix, zeros behind them.  The host's models pass all 484 bytes of opt.mat, as the host walks index it; the
// device calls pass asize * asize
static inline void aln_tables_fill(uint8_t *dst, const int8_t *mat, size_t mat_bytes)
{
	memcpy(dst + ALN_TAB_CODON, tab_codon(), 64);
	memcpy(dst + ALN_TAB_AA20, tab_aa20(), 256);
	memset(dst + ALN_TAB_MAT, 0, 484);
	memcpy(dst + ALN_TAB_MAT, mat, mat_bytes);
}

void set_error(const std::string &msg);
// no C++ exception may cross the C ABI: the extern "C" entry points run their bodies through this
template<typename R, typename F> static inline R guarded(R on_error, F f)
{
	try { return f(); }
	catch (const std::bad_alloc&) { set_error("out of host memory"); }
	catch (const std::exception &e) { set_error(std::string("internal error: ") + e.what()); }
	return on_error;
}

// MPA_TIMING=1 prints wall-clock stage timings to stderr
double now_ms();
bool timing_on();
void timing_note(const char *what, double ms);
double thread_cpu_ms();                                   // CPU time of the calling thread
void cpu_add(const char *label, double ms);               // accumulate under a label (coarse: per stage call, per parallel region and worker)
void cpu_report_and_reset(const char *header, double wall_ms);
struct CpuSpan {                                          // CPU time of the calling thread over a scope, under a label
	const char *label; double t0; bool on;
	explicit CpuSpan(const char *l) : label(l), t0(0), on(timing_on()) { if (on) t0 = thread_cpu_ms(); }
	~CpuSpan() { if (on) cpu_add(label, thread_cpu_ms() - t0); }
};

// ---- index (index.cpp) ---------------------------------------------------------------------------
struct Contig { int64_t off, len; std::string name; };

struct DeviceIndex;                  // opaque to the host pipeline, owned by the device context (dev_ctx.h, dev_ctx.hip)

// The big arrays of an index (packed genome, bucket offsets, occurrence lists): either owned (an index that was built or read
// into memory) or a VIEW into a read-only mapping of the .mpi file (mpa_idx_restore), so that the processes of a multi-GPU job --
// one per GPU, each restoring the same file -- share ONE copy in the page cache instead of holding 7.6 GB each at 3 Gbp.
// The interface is the subset of std::vector the library uses.  A view may be misaligned for T (the .mpi packs its sections back
// to back): at() reads through memcpy; data() is for byte copies (upload, dump) and for callers of the reference's mp_idx_t.
template<class T> struct IdxArray {
	std::vector<T> own;
	T *p = nullptr;
	size_t n = 0;
	T *data() { return p; }
	const T *data() const { return p; }
	size_t size() const { return n; }
	bool empty() const { return n == 0; }
	T &operator[](size_t i) { return p[i]; }                 // (writes: owned storage only, which is aligned)
	T operator[](size_t i) const { return at(i); }           // (reads go through memcpy: a view may be misaligned for T)
	T at(size_t i) const { T v; memcpy(&v, (const char*)p + i * sizeof(T), sizeof(T)); return v; }
	void resize(size_t k) { adopt(); own.resize(k); sync(); }
	void resize(size_t k, T v) { adopt(); own.resize(k, v); sync(); }
	void assign(size_t k, T v) { own.assign(k, v); sync(); }
	void clear() { own.clear(); sync(); }
	void swap(std::vector<T> &o) { own.swap(o); sync(); }
	void view(T *q, size_t k) { std::vector<T>().swap(own); p = q, n = k; }
private:
	void sync() { p = own.data(), n = own.size(); }
	void adopt() { if (n && p != own.data()) { std::vector<T> c(n); memcpy(c.data(), p, n * sizeof(T)); own.swap(c); sync(); } }
};

} // namespace mpa

struct mpa_idx_s {
	mpa_idxopt_t opt;
	int64_t n_kb = 0;
	int64_t l_seq = 0;
	std::vector<mpa::Contig> ctg;
	mpa::IdxArray<uint8_t> seq;      // 4-bit packed, low nibble = even offset (ntseq.c:64-67)
	std::vector<char> names;         // NUL separated, exactly as stored in the .mpi
	mpa::IdxArray<int64_t> ki;       // bucket offsets, 1<<(4*kmer-mod_bit) entries
	mpa::IdxArray<uint32_t> kb;      // global block ids
	std::vector<uint32_t> bo;        // per (contig,strand) block offset, 2*n_ctg+1 entries (index.c:11-26)
	uint32_t n_block = 0;
	std::vector<uint8_t> spsc;       // splice-score track (--spsc), empty if none: [strand][l_seq], indexed by contig offset + strand-local position
	// genome (and, once seeding has run there, the occurrence lists) resident in the HBM of device d (set by mpa_idx_to_device): one copy
	// per device, so that the pipelines of several GPUs of one process map against the same index (mpa_map_batches_multi)
	static const int kMaxDevices = 16;
	mpa::DeviceIndex *dev[kMaxDevices] = {};
	void *map_base = nullptr;        // the .mpi file mapped by mpa_idx_restore (seq / kb are views into it), or null
	size_t map_len = 0;
};

// the result of a batch (mpa_batch_finish; read through the mpa_result_* accessors of the C ABI, and by the formatter directly)
struct mpa_result_s {
	int32_t n_seq = 0;
	std::vector<mpa_hit_t> hits;
	std::vector<int64_t> hit_off;
	std::vector<uint32_t> cigars;
	std::vector<mpa_feat_t> feats;
	// cs:Z: bodies that came with the hits (MPA_GPU_CS): one entry per hit when any hit carries one, none at all otherwise
	struct CsRef { int64_t off; int32_t len, present; };
	std::vector<CsRef> cs;
	std::string cs_text;
	// residue rows that came with the hits (MPA_GPU_ROWS), the same way: at off the four rows of `width` bytes each (none when the
	// options print no --aln rows), then n_sta STA bytes (none without --trans)
	struct RowsRef { int64_t off; int32_t width, n_sta, present; };
	std::vector<RowsRef> rows;
	std::string rows_text;
	// (MPA_GPU_FORMAT=1, inside the stream pipeline only) the batch's output text as the device wrote it behind the finish step, with ids
	// relative to the batch, where its id fields lie and how many hits it prints (fmt_n_out < 0: none).  The pipeline takes it out before
	// the result reaches the caller (format_take_text); no accessor and no formatter looks at it
	std::string fmt_text;
	std::vector<int64_t> fmt_id_at;
	int64_t fmt_n_out = -1;
};

namespace mpa {

inline uint8_t nt_at(const mpa_idx_s *mi, int64_t p) { return mi->seq[p >> 1] >> ((p & 1) * 4) & 0xf; }
// strand-local window fetch; same contract as mp_ntseq_get_by_v (ntseq.c:108-114)
int64_t fetch_nt(const mpa_idx_s *mi, int32_t vid, int64_t st, int64_t en, uint8_t *out);
// the body of a cs:Z: string as the formatter builds it (host_format.cpp: mp_write_cs, format.c:102-187); aa = the query at qs
void put_cs_body(std::string &s, const mpa_idx_s *mi, const char *aa, int32_t vid, int64_t vs, int64_t ve, const uint32_t *cig, int32_t n_cigar);
int32_t block2vid(const mpa_idx_s *mi, uint32_t blk);        // mp_idx_block2pos (index.c:28-44)
int64_t idx_read_spsc(mpa_idx_s *mi, const char *fn, int32_t max_sc);   // mp_ntseq_read_spsc (ntseq.c:234-296)

// ---- device context and index (dev_ctx.hip, index_run.hip) --------------------------------------
int dev_upload_index(mpa_ctx_t *ctx, mpa_idx_s *mi);
int dev_index_build(mpa_ctx_t *ctx, mpa_idx_s *mi);           // k-mer table of a genome-only index on the device (index.c:52-136)
int32_t idx_plan_passes(const int64_t *hist, int32_t n_bins, int64_t budget_keys, int32_t *first_bin);   // bucket ranges of a multi-pass build (index.cpp; mpa_dbg_idx_plan_passes)
void dev_free_index(mpa_idx_s *mi);
mpa_ctx_t *ctx_sibling(mpa_ctx_t *ctx, int k);   // extra context on the same device (k >= 1), owned by ctx
// the sibling contexts of a stream of batches, created in the order and the priority classes of a stream plan (stream_plan.h) for the
// process's hardware queues and the layout asked for (StreamLayout); siblings made by another plan are destroyed first.  The plan in
// force stays with the root (ctx_stream_plan; nullptr before the first stream).  ctx_hw_queues(): GPU_MAX_HW_QUEUES as the process saw
// it when its first context was created.
struct StreamPlan;
int ctx_apply_stream_plan(mpa_ctx_t *root, int n_lanes, int n_seed, int n_plan, int layout);
const StreamPlan *ctx_stream_plan(const mpa_ctx_t *root);
int32_t ctx_pool_list(const mpa_ctx_t *ctx, int32_t sibling, const char **names, int64_t *caps, int32_t cap);   // the registered device pools of a context or one of its siblings (mpa_dbg_ctx_pools)
int ctx_hw_queues(void);
void ctx_absorb_sibling_stats(mpa_ctx_t *ctx);
void ctx_set_side_offset(mpa_ctx_t *ctx, int off);   // which of its side streams a DP round starts with
void ctx_set_role(mpa_ctx_t *root, mpa_ctx_t *ctx, int role);   // ctx's pools share their high-water marks with the root's other contexts of that role (0 DP lane, 1 seeder, 2 planner)

// ---- GPU seeding, chaining and refinement (drivers: seed_run.hip, refine_run.hip) -----------------
struct SeedJob { int64_t kb_off, dst; int32_t cnt, qpos, qid; };   // one kept seed: its occurrence list and where its anchors go
struct PrechainSparse {              // result for a mini-batch: the chained anchors (with a predecessor, or being one), query by query
	std::vector<int64_t> cfirst;     // [n_query + 1] offsets into the arrays below
	int64_t m = 0;
	const int32_t *pos = nullptr, *f = nullptr, *pred = nullptr;   // pinned buffers owned by the context, valid until its next call; pred = index into the query's part of the view, -1 for none
	const uint64_t *a = nullptr;
	std::vector<uint8_t> on_host;    // [n_query] 1 = the device declined this query (k_seed_sift: too many anchors in one block; k_chain_extract: a degenerate problem): seed and chain it on the host; empty = none
	// has_chains: both chaining rounds ran on the device (pre-chain extraction, main-chain forward pass and extraction): what comes
	// back are the main chains of every query -- u (score << 32 | anchors per chain) and their anchors, chain by chain -- and the
	// arrays above are not filled
	bool has_chains = false;
	std::vector<int64_t> u_first, a_first;   // [n_query + 1]
	const uint64_t *U = nullptr, *A = nullptr;   // pinned buffers of the context, valid until its next call
	// has_regions (MPA_GPU_REGIONS=1, on top of has_chains): the main round ended in k_regions instead of k_chain_pack.  U and A stay
	// null; u_first / a_first still count the chains and anchors of every query (what was NOT downloaded), and the selected regions
	// of query q -- n_reg[q] fixed-size records and their refinement limits -- lie at R / E + u_first[q]
	bool has_regions = false;
	const RegionRec *R = nullptr;
	const uint64_t *E = nullptr;
	const int32_t *n_reg = nullptr;
};
// What the device refinement takes (k_refine_scan, k_refine_scan_map), stated once for the callers' gate (host_plan.cpp) and the
// guards of dev_refine_scan / dev_refine_chains: k-mers of 1..7 residues (4 bits each in a 32-bit word whose all-ones value marks
// an empty slot of the LDS table) and a minimum ORF length that the walk into the chunk's halo can decide -- from a k-mer at the
// chunk's first position the walk sees (halo - 3 k) / 3 whole codons before it: 37 codons in all for every k of 3..7.
static const int32_t kRefineHaloBases = 112;
static const int32_t kRefineMaxKmer = 7;
static inline bool dev_refine_in_range(int32_t kmer, int32_t min_aa_len)
{
	return kmer >= 1 && kmer <= kRefineMaxKmer && min_aa_len <= (kRefineHaloBases - 3 * kmer) / 3 + kmer;
}
struct RefineWindow { int64_t as; int32_t qid, vid, len; };    // strand-local window [as, as + len) on vid, refined for query qid
struct RefineHits { std::vector<int64_t> first; std::vector<uint64_t> hits; };
int dev_refine_scan(mpa_ctx_t *ctx, mpa_idx_s *mi, int32_t kmer, int32_t min_aa_len, int32_t n_query, const int64_t *qw_first, const uint32_t *qwords,
                    int64_t n_win, const RefineWindow *wins, RefineHits &out);
// The whole refinement of a mini-batch on the device (mp_refine_reg, map.c:32-96): window scan, pairing of equal k-mers, the sort
// of every window's pairs, the forward pass and the extraction of its chain.  The query side comes as GROUPS (the distinct k-mers
// of every query: packed word, and the query positions that carry it).  out: the chains of every window as mp_chain() returns them.
struct RefineGroupsHost {
	std::vector<int64_t> qg_first;           // [n_query + 1]
	std::vector<uint32_t> gword, gfirst, gcount, qpos;
};
struct RefineChains {
	std::vector<int64_t> u_first, a_first;   // [n_win + 1]
	const uint64_t *U = nullptr, *A = nullptr;   // pinned buffers of the context, valid until its next call
	std::vector<uint8_t> on_host;            // [n_win] 1 = the device left this window out (2^22 bases or more, or its query has a position >= 2^22): refine it on the host
	// has_plans (MPA_GPU_PLANS=1): the call ended in k_plans instead of k_chain_pack.  U and A stay null; u_first / a_first still count
	// what was NOT downloaded.  Query q with first window w0: counts PN[q]; its regions and plans at PR / PP + w0, its gap segments at
	// PS + a_first[w0], its round-1 tasks at PT + 4 w0 + a_first[w0] (pinned, valid until the context's next call)
	bool has_plans = false;
	const RegionRec *PR = nullptr;
	const PlanRec *PP = nullptr;
	const mpa_dp_task_t *PT = nullptr;
	const SegRec *PS = nullptr;
	const PlansCounts *PN = nullptr;
};
// what dev_refine_chains needs on top of the windows to carry on to the plans (plans_core.h): the step's parameters, what every
// window's region carries over from the first region pass, and the queries themselves
struct PlansRequest {
	PlansParams p;
	const PlansWindow *win;                  // [n_win]
	const int64_t *win0;                     // [n_query + 1] first window of every query
	const char *text;                        // the batch's protein text: query q = text[q_off[q] .. q_off[q + 1])
	const int64_t *q_off;                    // [n_query + 1]
	const int8_t *mat;                       // [484]
};
// plans != nullptr: the call ends in the regions, plans, round-1 tasks and gap segments of every query (out.has_plans) instead of the
// chains, unless a window is the host's or a pool or pinned block cannot grow -- then the chains come back as without it
int dev_refine_chains(mpa_ctx_t *ctx, mpa_idx_s *mi, int32_t kmer, int32_t min_aa_len, int32_t max_ava, const ChainParams &cp, int32_t n_query, const RefineGroupsHost &groups,
                      int64_t n_win, const RefineWindow *wins, RefineChains &out, const PlansRequest *plans = nullptr);
// forward pass of mp_chain (chain.c:181-209) for a batch of problems on the device; see seed_run.hip
struct ChainIO { uint64_t *a = nullptr; int32_t *f = nullptr, *pred = nullptr; };   // pinned buffers of the context, valid until its next chain call
int dev_chain_buffers(mpa_ctx_t *ctx, int64_t n, ChainIO &io);
int dev_chain_forward(mpa_ctx_t *ctx, const ChainParams &p, int32_t n_prob, const int64_t *first, const ChainIO &io);
// main != nullptr: carry on with the main chain on the device (has_chains), if the seeding mode supports it
// hold != nullptr: the pinned result buffers live there (valid until the holder's next use) instead of in the context
struct SeedHold;
SeedHold *ctx_seed_hold(mpa_ctx_t *ctx, int k);   // k-th result holder of a context (created on first use, owned by it)
// regions != nullptr (with main): the main round ends in the regions of every query instead of its chains (out.has_regions), unless a
// pool or pinned block cannot grow -- then the chains come back as without it
int dev_prechain_forward(mpa_ctx_t *ctx, mpa_idx_s *mi, const ChainParams &pre, int32_t n_query, const int64_t *qfirst,
                         const SeedJob *jobs, int64_t n_jobs, PrechainSparse &out, const ChainParams *main = nullptr, SeedHold *hold = nullptr,
                         const int64_t *jfirst_dev = nullptr, const RegionsParams *regions = nullptr);
// Seeding where map.c:186 runs no pre-chain (-S, --no-pre-chain): the sift keeps the anchors that have another one within the main
// chain's reach, and the main chain runs over them directly.  out as from dev_prechain_forward(main != nullptr): has_chains, on_host.
// kept != nullptr (mpa_dbg_sift_kept): stop behind the sift; the kept anchors (block << 32 | query position) of every query in
// sorted order, and the sift's hand-back flags.
static const int32_t kSiftReachMax = 15;   // widest reach the sift filters by; beyond it every anchor is kept
struct SiftKept { std::vector<int64_t> first; std::vector<uint64_t> a; std::vector<uint8_t> flag; };
int dev_seed_direct(mpa_ctx_t *ctx, mpa_idx_s *mi, const ChainParams &mainp, int32_t n_query, const int64_t *qfirst, const SeedJob *jobs, int64_t n_jobs,
                    PrechainSparse &out, SeedHold *hold = nullptr, const int64_t *jfirst_dev = nullptr, SiftKept *kept = nullptr, const RegionsParams *regions = nullptr);
// The sketch stage (map.c:126-170) of a mini-batch on the device, sketch_exec.hip: the kept seeds of every query as the sift's
// jobs, left in the context's device memory -- dev_prechain_forward(jobs = nullptr, jfirst_dev = jfirst) then runs on them.  What
// comes back (pinned memory of the context, valid until its next sketch): first anchor / first job of every query, the cut-off in
// force, and flag[q] = 1 where the device hands the query to the host (no jobs, no anchors counted for it).
struct SketchResult {
	const int64_t *qfirst = nullptr, *jfirst = nullptr;   // [n_query + 1]
	const int32_t *max_occ = nullptr, *flag = nullptr;    // [n_query]
	int64_t n_anchor = 0, n_jobs = 0;
	int32_t n_flagged = 0;
};
int dev_sketch_jobs(mpa_ctx_t *ctx, mpa_idx_s *mi, int32_t max_occ, const mpa_qbatch_t *q, SketchResult &out);
int dev_sketch_fetch(mpa_ctx_t *ctx, int64_t n_jobs, SeedJob *jobs, int32_t *bucket);   // test hook: the jobs the last sketch left, and their buckets

// ---- the walks over the finished alignments on the device: statistics (MPA_GPU_STATS=1; aln_stats_core.h), cs:Z: difference strings
// (MPA_GPU_CS=1; aln_cs_core.h) and --aln / --trans residue rows (MPA_GPU_ROWS=1; aln_rows_core.h).  Driver: stats_run.hip ----
// One call takes any non-empty subset of the three.  Its sizes: n_cigar = the CIGAR words that go up (0 with dev_cig); n_feat = the
// feature slots (< 0: no statistics in this call); slot_bytes = the sum of aln_cs_bound() over the alignments (< 0: no cs strings);
// rows_bytes = the sum of aln_rows_slot() (< 0: no rows).
// dev_aln_walks_stage sizes the context's pinned blocks for the call and hands out where the caller writes its jobs, CIGAR words,
// protein text and, next to the jobs, cs.slot_off[n_jobs + 1] / rows.slot_off[n_jobs + 1]; dev_aln_walks sends them up, launches the
// kernels asked for and waits once.  Afterwards io.out[n_jobs] / io.feat[n_feat] hold the statistics, cs.body + cs.slot_off[j] holds
// cs.out[j].len bytes, and rows.body + rows.slot_off[j] the slot aln_rows_core.h describes with rows.out[j] (all pinned memory of the
// context, valid until its next call).  MPA_ERR_UNSUPPORTED from either: the device declines (a pool or pinned block could not grow)
// and the caller keeps the host's walks.
struct AlnWalkSizes { int64_t n_jobs, n_cigar, text_bytes, n_feat, slot_bytes, rows_bytes; };
struct AlnStatsIO { AlnStatsJob *jobs = nullptr; uint32_t *cigar = nullptr; char *text = nullptr; const AlnStatsOut *out = nullptr; const AlnFeat *feat = nullptr; };
struct AlnCsIO { int64_t *slot_off = nullptr; const AlnCsOut *out = nullptr; const char *body = nullptr; };
struct AlnRowsIO { int64_t *slot_off = nullptr; const AlnRowsOut *out = nullptr; const char *body = nullptr; };
// fin != nullptr (MPA_GPU_FINISH=1, with the statistics in the call; the records staged through dev_finish_stage): the ranking and the
// flat result run behind the walks' kernels on the same stream and in front of the call's one wait, reading the out records, features,
// slots and CIGAR words where they lie; nothing of the walks' own output is downloaded then (io.out, cs.out, rows.out stay null) and
// fin->flat is the result.
struct FinishResident;
struct FormatResident;
int dev_aln_walks_stage(mpa_ctx_t *ctx, const AlnWalkSizes &z, AlnStatsIO &io, AlnCsIO &cs, AlnRowsIO &rows);
int dev_aln_walks(mpa_ctx_t *ctx, mpa_idx_s *mi, const AlnStatsParams &p, const AlnRowsParams &rp, const int8_t *mat, const AlnWalkSizes &z, AlnStatsIO &io, AlnCsIO &cs,
                  AlnRowsIO &rows, bool dev_cig = false, FinishResident *fin = nullptr, FormatResident *fmt = nullptr);

// ---- accepted spans and region CIGARs on the device (MPA_GPU_SPANS=1; driver: stats_run.hip; kernels: span_kernels.hip; code:
// spans_core.h) ----
// Between the rounds: dev_spans_stage sizes the context's pinned block and hands out where the caller writes the batch's plans, gap
// segments, round-1 results and protein text; dev_spans_round1 runs k_spans / k_spans_emit and leaves rec[n_plan], the n_task round-2
// tasks and keeps the round-1 CIGAR pool on the device -- pool1 == nullptr: a device-to-device copy of the n_pool1 words the last
// mpa_dp_run on this context left (before the next one overwrites them); otherwise the caller's words go up.
// Behind round 2: dev_spans_asm_stage hands out where the round-2 results and the slot offsets (slot_off[n_plan + 1], in words) go;
// dev_spans_assemble runs k_assemble on what round 1 left and, for pool2 == nullptr, the pool of the last mpa_dp_run, and leaves
// rec[n_plan] and the slots' words in pinned memory (valid until the context's next call); the words also stay on the device for
// dev_aln_walks (dev_cig).  d_rst2 != nullptr (a resident round 2, MPA_GPU_ROUND2): the round-2 records are read from that device
// pointer and only the slot offsets go up.  MPA_ERR_UNSUPPORTED from any of them: a pool or pinned block could not grow -- the caller
// keeps the host step.
// (r2, with MPA_GPU_ROUND2=1: the round-2 tasks in place on the device and their bounds; d_tasks == nullptr: not asked for)
struct DpResidentIn { const mpa_dp_task_t *d_tasks = nullptr; int64_t prep_bound = 0, max_nl = 0, max_al = 0; };
struct SpansIO { SpansPlan *plan = nullptr; SegRec *seg = nullptr; mpa_dp_rst_t *rst1 = nullptr; char *text = nullptr;
                 const SpanRec *rec = nullptr; const mpa_dp_task_t *task = nullptr; int32_t n_task = 0; DpResidentIn r2; };
int dev_spans_stage(mpa_ctx_t *ctx, int64_t n_plan, int64_t n_seg, int64_t n_rst1, int64_t text_bytes, SpansIO &io);
int dev_spans_round1(mpa_ctx_t *ctx, mpa_idx_s *mi, const SpansParams &p, const int8_t *mat, int64_t n_plan, int64_t n_seg, int64_t n_rst1, int64_t text_bytes,
                     const uint32_t *pool1, int64_t n_pool1, SpansIO &io);
struct SpansAsmIO { mpa_dp_rst_t *rst2 = nullptr; int64_t *slot_off = nullptr; const AsmRec *rec = nullptr; const uint32_t *cigar = nullptr; };
int dev_spans_asm_stage(mpa_ctx_t *ctx, int64_t n_plan, int64_t n_rst2, SpansAsmIO &io);
int dev_spans_assemble(mpa_ctx_t *ctx, int64_t n_plan, int64_t n_rst2, const uint32_t *pool2, int64_t n_pool2, SpansAsmIO &io, const mpa_dp_rst_t *d_rst2 = nullptr);

// ---- ranking and flat result of a batch (MPA_GPU_FINISH; code: finish_core.h; kernels: finish_kernels.hip;
// driver: stats_run.hip; the host side and the model: host_finish.cpp) ----
// The tables of a call: the queries' aligned regions as records (query q: rec[first[q] .. first[q + 1])), and the CIGAR words, features,
// cs text and rows text their offsets point into.  in_*: the sizes of those arrays; out_*: the sums of the records' n_cigar, n_feat,
// cs_len and row bytes (a result that keeps every hit); n_big: queries of more than FINISH_LDS_REGS regions (finish_count_big).
// dev_finish_stage sizes the context's pinned blocks and hands out where the caller writes the tables; dev_finish sends them up, runs
// k_finish_rank, k_finish_scan and k_finish_gather on the context's stream, whose stores put the flat result into a pinned block at its
// real size, and waits once: flat points into that pinned memory of the context, valid until its next call.  (The hook's way; a batch
// takes the step inside dev_aln_walks, where only first[] and the records go up and the rest is read where the walks left it.)  MPA_ERR_UNSUPPORTED from either: a pool or pinned block could
// not grow -- the caller keeps the host's ranking.
struct FinishSizes { int64_t n_query, n_rec, n_big, in_words, in_feat, in_cs, in_rows, out_words, out_feat, out_cs, out_rows; };
struct FinishTables { int64_t *first = nullptr; FinRec *rec = nullptr; uint32_t *words = nullptr; mpa_feat_t *feats = nullptr; char *cs_text = nullptr, *rows_text = nullptr; };
struct FinishFlat { const FinCounts *off = nullptr; const mpa_hit_t *hits = nullptr; const FinCsRef *cs = nullptr; const FinRowsRef *rows = nullptr; const uint32_t *cigars = nullptr;
                    const mpa_feat_t *feats = nullptr; const char *cs_text = nullptr, *rows_text = nullptr; int64_t bytes_down = 0; };
struct FinishResident { FinParams p; FinishSizes z; FinishFlat flat; };   // the step inside dev_aln_walks: in p and z, out flat
static inline int64_t finish_count_big(const int64_t *first, int64_t n_query)
{
	int64_t n = 0;
	for (int64_t q = 0; q < n_query; ++q) n += first[q + 1] - first[q] > FINISH_LDS_REGS;
	return n;
}
int dev_finish_stage(mpa_ctx_t *ctx, const FinishSizes &z, FinishTables &t);
int dev_finish(mpa_ctx_t *ctx, const FinParams &p, const FinishSizes &z, FinishFlat &flat);
int dev_finish_last(const mpa_ctx_t *ctx, int64_t out[6]);
// the same through the shared core on the host with a team of one, into a result (host_finish.cpp); and a device call's flat arrays
// into a result, one copy each
void finish_model(const FinParams &p, const FinishSizes &z, const FinishTables &t, mpa_result_s *res);
void finish_flat_to_result(const FinishFlat &f, int64_t n_query, mpa_result_s *res);
// every index the step follows, checked once for both paths (the test hook; the batch's own tables are made right)
bool finish_tables_ok(const FinishSizes &z, const FinishTables &t);

// ---- the output text of a batch (MPA_GPU_FORMAT; code: format_core.h; kernels: format_kernels.hip; driver:
// stats_run.hip; the host side and the model: host_format.cpp) ----
// The sizes of a call: the flat result's arrays (has_cs / has_rows: it carries cs bodies / rows), the name pools, and the room for the text
// and the id places (bounds: format_bounds).  dev_format_stage sizes the context's pinned blocks and hands out where the caller writes
// the tables; dev_format sends them up, runs k_format_size, k_format_scan and k_format_write on the context's stream, whose stores put
// totals, id places and text into a pinned block, and waits once: out points into that pinned memory of the context, valid until its
// next call.  out.declined: the kernels wrote no text (a blen of 0, something not carried, or more than the room given) -- the caller
// formats on the host.  MPA_ERR_UNSUPPORTED from either: a pool or pinned block could not grow.
struct FormatSizes { int64_t n_query, n_hit, n_words, n_feat, cs_bytes, rows_bytes, qname_bytes, n_ctg, cname_bytes, text_cap, id_cap, n_place; int32_t has_cs, has_rows; };   // n_place: entries of at[] (the hits that may be printed)
struct FormatTables { int64_t *hit_off = nullptr, *q_off = nullptr, *qname_off = nullptr, *cname_off = nullptr, *clen = nullptr; mpa_hit_t *hits = nullptr; FinCsRef *cs = nullptr;
                      FinRowsRef *rows = nullptr; mpa_feat_t *feats = nullptr; uint32_t *cigars = nullptr; char *cs_text = nullptr, *rows_text = nullptr, *qname = nullptr, *cname = nullptr; };
struct FormatOut { const char *text = nullptr; const int64_t *id_at = nullptr; FmtCounts tot = { 0, 0, 0, 0 }; bool declined = false; };
int dev_format_stage(mpa_ctx_t *ctx, const FormatSizes &z, FormatTables &t);
int dev_format(mpa_ctx_t *ctx, const FmtOpt &o, const FormatSizes &z, FormatOut &out);
int dev_format_last(const mpa_ctx_t *ctx, int64_t out[6]);
// The same three kernels inside dev_aln_walks (MPA_GPU_FORMAT=1, behind the finish step of the same call: `fmt` next to `fin`), on the
// call's stream behind k_finish_gather and in front of its one wait.  They read the hits where the finish step left them (FmtSrc::rec):
// nothing of the result goes up again, only the names and lengths staged through dev_format_stage with z.n_hit = 0 and z.n_place = the
// aligned regions.  In: o, z (staged); out: what dev_format gives.  A pool that cannot grow declines the whole call, as for the finish step
struct FormatResident { FmtOpt o; FormatSizes z; FormatOut out; };
// The host side (host_format.cpp).  format_knob: MPA_GPU_FORMAT, read per call -- 0 unset, 2 model.  format_opt_from: the options the
// step reads (false: a gff_prefix longer than FORMAT_PREFIX_MAX).  FormatInput: a result and its names as the tables of a call, owning
// what it had to build (names pools; with `build`, the cs bodies and rows of hits that carry none, by the host's walks).
// format_tables_ok: every index the step follows.  format_bounds: text_cap / id_cap from what the host already has.  format_host:
// the three stages with a team of one; nullptr, or why it declined.  format_finish_text: the patch with id0 into a malloc'ed string.
int format_knob();                                        // 0 unset, 1 the device stage inside a batch's call, 2 model
bool format_opt_from(const mpa_mapopt_t &opt, FmtOpt &o);
struct FormatInput {
	FormatSizes z = {};
	FmtSrc S = {};
	std::vector<int64_t> qname_off, cname_off, clen;
	std::string qname, cname, cs_text, rows_text;
	std::vector<FinCsRef> cs;
	std::vector<FinRowsRef> rows;
};
void format_input(const mpa_idx_s *mi, const mpa_mapopt_t &opt, const mpa_qbatch_t *q, const char *const *names, const mpa_result_s *r, bool build, FormatInput &in);
bool format_tables_ok(const FormatInput &in);
void format_bounds(const FmtOpt &o, FormatInput &in);
struct FormatText { std::string text; std::vector<int64_t> id_at; FmtCounts tot = { 0, 0, 0, 0 }; };
const char *format_host(const FmtOpt &o, const FormatInput &in, FormatText &t);
const char *format_decline_reason(const FmtCounts &tot, int64_t text_cap, int64_t id_cap);
// the pipeline's output stage: the text a batch's device call left in its result (fmt_n_out >= 0) patched with *id_io, which advances, into
// a malloc'ed string; -1: there is none, or ids reach seven digits (said under MPA_TIMING=1) -- the caller formats.  The result never keeps it
int64_t format_take_text(mpa_result_s *r, int32_t n_query, int64_t *id_io, char **out);

// ---- DP round 2 from device-resident tasks (MPA_GPU_ROUND2=1; dp_exec.hip) ----
// What dev_spans_round1 leaves for it: the round-2 tasks where k_spans_emit wrote them (a pool of the context) and the three bounds the
// device planner sizes by (dp_results_core.h), reduced on the device and downloaded next to the task count (DpResidentIn, above).
// ... and what a resident round says about itself: host waits of the planner and of the round behind it, bytes up and down (task records
// among the bytes up, words of the dense CIGAR pool among the bytes down)
// (chained_launches: kernels of the step between the rounds launched inside the round's wait -- MPA_GPU_ROUND1, below; 0 for round 2)
struct DpResidentRec { int64_t plan_waits = 0, round_waits = 0, bytes_up = 0, task_bytes_up = 0, bytes_down = 0, pool_bytes_down = 0, chained_launches = 0; };
// The round of n calls planned from in.d_tasks in place, its result records written on the device and downloaded with the round's one
// wait into rst[n]; *n_pool: words of the dense CIGAR pool, which stays in the context (dp_fetch_pool); *d_rst: the records on the
// device, valid until the context's next round.  MPA_ERR_UNSUPPORTED: declined (the last error says why) -- the caller runs mpa_dp_run.
int dp_run_resident(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q, int64_t n, const DpResidentIn &in, mpa_dp_rst_t *rst, int64_t *n_pool,
                    const mpa_dp_rst_t **d_rst, DpResidentRec *rec);
// the dense pool the context's last round left (n_pool words) into a malloc'ed block: a second wait, for the fallbacks that need the words
int dp_fetch_pool(mpa_ctx_t *ctx, int64_t n_pool, uint32_t **pool);
// MPA_GPU_ROUND2, read per batch
static inline bool round2_knob() { const char *e = getenv("MPA_GPU_ROUND2"); return e && atoi(e) != 0; }
// the bounds of the n tasks at d_tasks, reduced on the device (k_task_bounds, span_kernels.hip): for the hook mpa_dbg_dp_run_resident
int dev_task_bounds(mpa_ctx_t *ctx, const mpa_dp_task_t *d_tasks, int64_t n, DpResidentIn &out);

// ---- DP round 1 and the step behind it in one submission (MPA_GPU_ROUND1=1; dp_exec.hip, stats_run.hip) ----
// The step between the rounds as the round sees it: c says what the caller staged through dev_spans_stage (plans, gap segments, text;
// the record section of the block is left alone -- the round's own kernels write it on the device).
// dev_spans_chain_prepare (before the round is launched; whatever can decline does so here): the block up without its record section,
// sp_pool1 sized at pool_words; dev: where records and dense pool go, and what went up (block_bytes / rst1_bytes: the whole block and its
// record section, for the record).  dev_spans_chain_enqueue (behind the round's results kernels, in front of its one wait): k_spans,
// k_spans_emit and, with MPA_GPU_ROUND2=1, k_task_bounds under the guard of g_err / g_bad (the round's hand-off error word and the bad-call
// word of its results header: either non-zero and the kernels read no record and write a task count of 0), then the step's download; no
// wait.  dev_spans_chain_collect (behind the wait, for a round that passed its checks): what dev_spans_round1 leaves in io.
struct SpansChain { SpansParams p; const int8_t *mat; int64_t n_plan, n_seg, n_rst1, text_bytes; bool want_r2; };   // want_r2: k_task_bounds too (MPA_GPU_ROUND2=1; the hook: always)
struct SpansChainDev { mpa_dp_rst_t *d_rst1 = nullptr; uint32_t *d_pool1 = nullptr; int64_t bytes_up = 0, block_bytes = 0, rst1_bytes = 0; };
int dev_spans_chain_prepare(mpa_ctx_t *ctx, mpa_idx_s *mi, const SpansChain &c, int64_t pool_words, SpansChainDev &dev);
int dev_spans_chain_enqueue(mpa_ctx_t *ctx, mpa_idx_s *mi, const SpansChain &c, const int32_t *g_err, const int64_t *g_bad, int64_t *launches, int64_t *bytes_down);
int dev_spans_chain_collect(mpa_ctx_t *ctx, const SpansChain &c, int64_t n_pool1, SpansIO &io);
// (the hook mpa_dbg_spans_guard) the step alone on a staged block that holds its records, with guard words of the caller's on the device
int dev_spans_round1_guarded(mpa_ctx_t *ctx, mpa_idx_s *mi, const SpansChain &c, int32_t err, int64_t bad, SpansIO &io);
// The round of n calls from the caller's task table, planned on the device (or declined), with the chained step: rst[n] and *n_pool as
// for dp_run_resident, io what dev_spans_round1 would have left (rec, task, n_task, r2), the dense pool in the context's sp_pool1
// (dp_fetch_pool1).  rec->bytes_up holds planner upload + query residues + the staged block without its record section; parts[4]
// (nullable): those three and the bytes of the record section that stayed down.  MPA_ERR_UNSUPPORTED: declined (the last error says why),
// io untouched -- the caller runs mpa_dp_run and the step as always.
int dp_run_round1_chained(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q, int64_t n, const mpa_dp_task_t *tasks, const SpansChain &c,
                          mpa_dp_rst_t *rst, int64_t *n_pool, SpansIO &io, DpResidentRec *rec, int64_t *parts = nullptr);
// the round-1 words a chained round left in the context's sp_pool1 (n_pool words) into a malloc'ed block: a wait of its own
int dp_fetch_pool1(mpa_ctx_t *ctx, int64_t n_pool, uint32_t **pool);
// MPA_GPU_ROUND1, read per batch
static inline bool round1_knob() { const char *e = getenv("MPA_GPU_ROUND1"); return e && atoi(e) != 0; }

} // namespace mpa
