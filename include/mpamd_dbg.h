/* mpamd_dbg.h -- the test hooks of MPA_GPU_SPANS, MPA_GPU_DPPLAN, MPA_GPU_ROUND2, the stream plan, the contexts' pool registry and the chain extraction.  They are not part of the C ABI of libmpamd.so (include/mpamd.h):
 * they are built from miniprot_amd/csrc/spans_dbg.cpp, dpplan_dbg.cpp, round2_dbg.cpp, stream_dbg.cpp, ctx_pools_dbg.cpp and chain_dbg.cpp into a library of its own, libmpamd_dbg.so, next to libmpamd.so
 * and linked against it. */
#ifndef MPAMD_DBG_H
#define MPAMD_DBG_H
#include "mpamd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The two steps of MPA_GPU_SPANS on hand-made inputs: the accepted spans between the DP rounds and the region CIGARs behind them, on
 * the device (k_spans, k_spans_emit, k_assemble) or, with ctx == NULL, through the shared core on the host (spans_core.h).
 * plans: n_plan records of 104 bytes -- int64 as, ae, vs0, vs1, mid_ve; int32 reg, as1, mid_qe, has_right, t_left, t_left2, t_right,
 * t_right2, first gap segment (in segs), gap segments; int64 first residue of the query in q's text; int32 qid, qlen; uint32 vid; int32
 * first round-1 result of the query (the t_* and the gap tasks count from it).  segs: n_seg records of 24 bytes -- int32 ne0, ne1, ae0,
 * ae1, task (-1: the ungapped shortcut), score.  rst1 / pool1 and rst2 / pool2: the results of the two rounds and their CIGAR pools;
 * rst2 is indexed by round-2 task number.  n_rst2 < 0: stop behind the first step.
 * Out: span_rec[n_plan] (80 bytes: int64 vs; int32 qs, l_nt, l_aa, r_nt, r_aa, flags (1 / 2: the left / right span was
 * made, 4 / 8: that side's terminal-exon repeat counted); the left and the right span as segment records),
 * tasks[at most 2 n_plan] and *n_task; asm_rec[n_plan] (40 bytes: int64 ve, first word in cigar; int32 qe, dp_score, n_cigar, n_exon,
 * bad, merged boundaries) and the words in cigar[cigar_cap] (a plan's slot is the sum of its segments' words).  Every index is checked first:
 * MPA_ERR_ARG for inputs that point outside their arrays.
 */
int mpa_dbg_spans(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int32_t n_plan, const void *plans, int32_t n_seg, const void *segs,
                  int64_t n_rst1, const mpa_dp_rst_t *rst1, const uint32_t *pool1, int64_t n_pool1, int64_t n_rst2, const mpa_dp_rst_t *rst2, const uint32_t *pool2,
                  int64_t n_pool2, void *span_rec, mpa_dp_task_t *tasks, int32_t *n_task, void *asm_rec, uint32_t *cigar, int64_t cigar_cap);

/* The planner of a DP round on the device (MPA_GPU_DPPLAN) for a task table: the arguments of mpa_dbg_dp_plan
 * (mpamd.h) behind a context, and the same serialisation, assembled from what the device planner left in the context's pools and in
 * its header.  ctx == NULL: the model -- the planner's stages run on the host with a team of one; no device is needed.  The contig
 * lengths are uploaded by the hook: no index has to be resident.  Returns the bytes of the serialisation (written when they fit cap),
 * a negative MPA_ERR_* code, or MPA_DBG_DP_PLAN_DECLINED (1; no serialisation is that short) when the device planner declines the table
 * and mpa_dp_run would plan it on the host: penalties above 255, the worker pool, the anti-diagonal switch, a repeated round, more than
 * 2^20 calls, a call of class X_HUGE, more than one traceback chunk, unit costs beyond the sort key, a pool that cannot grow, and every
 * table or option the host planner refuses.  mpa_last_error() says which. */
#define MPA_DBG_DP_PLAN_DECLINED 1
int64_t mpa_dbg_dp_plan_device(mpa_ctx_t *ctx, const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, int32_t n_seq, const int64_t *q_off, int64_t n,
                               const mpa_dp_task_t *tasks, const int64_t *knobs, void *buf, int64_t cap);

/* MPA_DP_SPLIT_WIDE (extension calls of 1025..3072 columns on the classes X_SPLIT8 / X_SPLIT12, 8 / 12 workgroups
 * per pair of calls).  mpa_dbg_dp_plan_wide is mpa_dbg_dp_plan (mpamd.h) with knobs[9]: knobs[8] is split_wide, which the hook -- like
 * the executor -- drops with the worker pool (knobs[4]) and in a repeated round (knobs[2]).  Its serialisation is mpa_dbg_dp_plan's,
 * byte for byte, followed by five int64: first descriptor and number of descriptors of X_SPLIT8, the same of X_SPLIT12, and the number of
 * boundaries n_bound (11 per X_SPLIT12 group, 7 per X_SPLIT8, 3 per X_SPLIT4, 1 per X_SPLIT2).  The descriptors of the two classes lie
 * between X_SPLIT4's and X_128's in ExtWave[]; their calls carry DTask::cls 9 and 10.  mpa_dbg_dp_plan_device_wide is
 * mpa_dbg_dp_plan_device with the same ninth knob and the same five words.
 * mpa_dbg_dp_last_classes: the extension calls per DpClass (0 .. 15: X_16, X_32, X_64, X_W2, X_W4, X_SPLIT2, X_SPLIT4, X_HUGE, X_128,
 * X_SPLIT8, X_SPLIT12) in the plan of the context's last mpa_dp_run -- of its repeat, when a hand-off timed out. */
int64_t mpa_dbg_dp_plan_wide(const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, int32_t n_seq, const int64_t *q_off, int64_t n, const mpa_dp_task_t *tasks,
                             const int64_t *knobs, void *buf, int64_t cap);
int64_t mpa_dbg_dp_plan_device_wide(mpa_ctx_t *ctx, const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, int32_t n_seq, const int64_t *q_off, int64_t n,
                                    const mpa_dp_task_t *tasks, const int64_t *knobs, void *buf, int64_t cap);
int mpa_dbg_dp_last_classes(const mpa_ctx_t *ctx, int64_t ext_calls[16]);

/* MPA_DP_HUGE_WG (X_HUGE extension calls swept by k_ext_huge_wg, one wave per 64-column block, W waves in one
 * workgroup).  mpa_dbg_dp_last_huge: of the context's last mpa_dp_run (of its repeat, when a hand-off timed out) out[0] the X_HUGE calls
 * the one-wave kernel swept, out[1] those the workgroup kernel swept, out[2] the column blocks and out[3] the passes of the latter.
 * mpa_dbg_dp_huge_wg_info: the schedule's constants (miniprot_amd/csrc/ext_huge_wg_core.h) -- out[0] W waves per workgroup, out[1] R rows
 * per chunk, out[2] MIN_BLOCKS, the fewest column blocks at which a call takes the workgroup kernel. */
int mpa_dbg_dp_last_huge(const mpa_ctx_t *ctx, int64_t out[4]);
void mpa_dbg_dp_huge_wg_info(int32_t out[3]);

/* MPA_DP_MB_WG (traceback calls of more than 1 024 columns, class T_MB, swept by k_glob_mb_wg on the same schedule,
 * whose constants are mpa_dbg_dp_huge_wg_info's).  mpa_dbg_dp_last_mb: of the context's last mpa_dp_run, over all its traceback chunks,
 * out[0] the T_MB calls swept on one wave (in the round kernel or by k_glob_narrow), out[1] those swept on workgroups, out[2] the column
 * blocks and out[3] the passes of the latter. */
int mpa_dbg_dp_last_mb(const mpa_ctx_t *ctx, int64_t out[4]);

/* MPA_DP_LITE_W8 (traceback calls of 257..512 columns on the checkpointed class T_LITE_W8, DTask::cls 13 -- an
 * eight-wave group per pair of calls swept by k_lite_w8, walked by k_walk_w8).  mpa_dbg_dp_last_w8: of the context's last mpa_dp_run
 * out[0] the calls of the class, out[1] their padded cells ((nl - 2) * 8 * ceil(al / 8) each), out[2] the groups k_lite_w8 was launched
 * over, out[3] the blocks of MPA_TB_BLOCK rows k_walk_w8 recomputed.  mpa_dbg_dp_plan_w8 is mpa_dbg_dp_plan_wide with knobs[10]: knobs[9]
 * is lite_w8, which the hook -- like the executor -- drops with the worker pool (knobs[4]).  Its serialisation is mpa_dbg_dp_plan_wide's,
 * byte for byte, followed by three int64: first descriptor and number of descriptors of T_LITE_W8 in ExtWave[] (behind T_LITE_W4's) and
 * the calls of its walk list, the sixth (behind T_LITE_W4's in the section of walk calls). */
int mpa_dbg_dp_last_w8(const mpa_ctx_t *ctx, int64_t out[4]);
int64_t mpa_dbg_dp_plan_w8(const mpa_dpopt_t *opt, int32_t n_ctg, const int64_t *ctg_len, int32_t n_seq, const int64_t *q_off, int64_t n, const mpa_dp_task_t *tasks,
                           const int64_t *knobs, void *buf, int64_t cap);

/* A DP round from device-resident tasks (MPA_GPU_ROUND2): the arguments of mpa_dp_run.  On a context the hook
 * puts the tasks into a device pool, has their bounds reduced there (k_task_bounds), plans the round from the tasks in place, runs it
 * with the result records and the dense CIGAR pool assembled on the device in front of the round's one wait, and only then fetches the
 * dense pool.  rst[n], *cigar_pool (mpa_free) and *n_pool are what mpa_dp_run returns for the same table.  rec[MPA_DBG_ROUND2_REC] says what
 * the call did: [0] host waits of the planner, [1] host waits of the round behind it, [2] bytes uploaded by planner and round, [3] bytes
 * of task records among them, [4] bytes downloaded by planner and round, [5] bytes of CIGAR pool among them, [6] bytes of the explicit
 * pool fetch behind the round, [7] prep-chunk bound, [8] largest nl, [9] largest al of the tasks as reduced, [10] words of the dense pool.
 * ctx == NULL: no DP runs; made_up holds what the kernels would have left -- ext_out (nt_len, aa_len, score, flags per call), score and
 * n_cigar per call, gids[n_glob] the traceback calls in the planner's order -- and the stages of dp_results_core.h run on it with a
 * team of one: rst[n], *n_pool, rec[7..10]; *cigar_pool stays NULL.  mi, opt and q may be NULL then.
 * Returns MPA_OK, a negative MPA_ERR_* code, or MPA_DBG_ROUND2_DECLINED (1) when the round is one that falls back to mpa_dp_run: whatever the
 * device planner declines (mpa_dbg_dp_plan_device above), a pool or pinned block that cannot grow, a repeated round. */
#define MPA_DBG_ROUND2_DECLINED 1
#define MPA_DBG_ROUND2_REC 12
typedef struct { const int32_t *ext_out, *score, *n_cigar, *gids; int64_t n_glob; } mpa_dbg_dp_outputs_t;
int mpa_dbg_dp_run_resident(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_dpopt_t *opt, const mpa_qbatch_t *q, int64_t n, const mpa_dp_task_t *tasks,
                            const mpa_dbg_dp_outputs_t *made_up, mpa_dp_rst_t *rst, uint32_t **cigar_pool, int64_t *n_pool, int64_t *rec);

/* DP round 1 and the step behind it in one submission (MPA_GPU_ROUND1), on a context: what mpa_dbg_spans takes for
 * its round-1 half -- options, queries, plans[n_plan] (SpansPlan, 104 bytes) and segs[n_seg] (SegRec, 24 bytes) -- and, in place of round-1
 * results, the round-1 task table tasks[n] the plans' task numbers point into (base1 + t_left ...), with the DP options.  The hook stages
 * the step's block and sends it up without its record section, plans the round on the device from the table, runs it with records and
 * dense pool assembled on the device, the records copied into the block's record section, k_spans / k_spans_emit / k_task_bounds chained
 * behind them inside the round's one wait, and only then fetches the dense pool from the spans step's pool.  Out: rst[n] and *cigar_pool
 * (mpa_free) / *n_pool as mpa_dp_run returns them for the table; span_rec[n_plan] (SpanRec, 80 bytes), tasks2[up to 2 n_plan] / *n_task as
 * mpa_dbg_spans returns them for those results; bounds[3] (prep chunks, largest nl, largest al of tasks2).  rec[MPA_DBG_ROUND1_REC]: [0] host
 * waits of the planner, [1] host waits of the round behind it, [2] bytes uploaded by planner, round and step, [3] bytes of task records among
 * them, [4] bytes downloaded, [5] bytes of CIGAR pool among them, [6] kernels of the step launched inside the round's wait, [7] the
 * planner's upload, [8] the queries' residues, [9] the step's block as it went up, [10] bytes of its record section, which did not, [11]
 * bytes of the explicit pool fetch: [2] = [7] + [8] + [9].  Every index the step follows that does not depend on the round's results is
 * checked first (MPA_ERR_ARG; also without a context: the round has no host model).  Returns MPA_OK, a negative MPA_ERR_* code, or
 * MPA_DBG_ROUND1_DECLINED (1) for a round that falls back to mpa_dp_run: whatever the device planner declines, a pool or pinned block
 * that cannot grow, a repeated round; the last error says why. */
#define MPA_DBG_ROUND1_DECLINED 1
#define MPA_DBG_ROUND1_REC 12
int mpa_dbg_round1_chain(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_dpopt_t *dpopt, const mpa_qbatch_t *q, int32_t n_plan, const void *plans,
                         int32_t n_seg, const void *segs, int64_t n, const mpa_dp_task_t *tasks, mpa_dp_rst_t *rst, void *span_rec, mpa_dp_task_t *tasks2, int32_t *n_task,
                         int64_t *bounds, uint32_t **cigar_pool, int64_t *n_pool, int64_t *rec);

/* The device guard of the chained step: k_spans, k_spans_emit and k_task_bounds on a context, on plans, segments
 * and round-1 records as mpa_dbg_spans takes them, with the two words a chained step is guarded by set by the caller on the device -- err,
 * the round's hand-off error word, and bad, the bad-call word of its results header; at least one must be non-zero (MPA_ERR_ARG otherwise:
 * with both zero the step is mpa_dbg_spans).  The kernels then read no record of rst1[] and no genome byte: *n_task and bounds[3] come
 * back 0 whatever rst1[] holds. */
int mpa_dbg_spans_guard(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, int32_t n_plan, const void *plans, int32_t n_seg, const void *segs,
                        int64_t n_rst1, const mpa_dp_rst_t *rst1, int32_t err, int64_t bad, int32_t *n_task, int64_t *bounds);

/* The stream plan (miniprot_amd/csrc/stream_plan.h): which streams mpa_map_batches creates for its DP lanes,
 * seeders and planners, in which priority class (0 normal, 1 high, 2 low) and in which order, for the hardware queues of the process.
 * As int32 words: q, lanes, seeders, planners, layout (0 legacy, 1 A, 2 B, 3 C), streams created up front; per lane class, rank in
 * creation order, side streams it may create, their class; per seeder and then per planner main class, main rank, seeding class, seeding
 * rank (the same stream twice unless the layout is the legacy one).  Both return the words the plan takes, written when they fit cap.
 * mpa_dbg_stream_plan: the plan in force on a context, that is the one its last mpa_map_batches* call created its sibling contexts by
 * (0 words before the first).  mpa_dbg_stream_plan_for: the module's plan for q hardware queues (q <= 0: GPU_MAX_HW_QUEUES as the
 * process saw it when its first context was created, or as it sees it now if there is none yet) and a value of MPA_STREAM_PLAN
 * (NULL: unset). */
int64_t mpa_dbg_stream_plan(const mpa_ctx_t *ctx, int32_t *out, int64_t cap);
int64_t mpa_dbg_stream_plan_for(int32_t q, int32_t n_lanes, int32_t n_seed, int32_t n_plan, const char *layout, int32_t *out, int64_t cap);

/* The device pools of a context (miniprot_amd/csrc/dev_ctx.h): every pool registers with its context under its
 * name when the context is created, in the same order in every context of a process.  sibling 0: ctx itself; k >= 1: the k-th sibling
 * context it owns (the DP lanes, seeders and planners of its last stream of batches).  Returns the number of registered pools and
 * writes the name (a string the library owns) and the capacity in bytes (0: not allocated yet) of the first cap of them; names and
 * caps may be NULL with cap 0.  MPA_ERR_ARG: no context, or no sibling of that number. */
int32_t mpa_dbg_ctx_pools(const mpa_ctx_t *ctx, int32_t sibling, const char **names, int64_t *caps, int32_t cap);

/* The chain extraction (k_chain_extract = chain_extract_core of miniprot_amd/csrc/chain_core.h) on raw anchors: the eleven parameters of
 * mp_chain in the order mpa_dbg_chain takes them, then n_prob chaining problems whose sorted anchors lie back to back in a[]
 * (first[n_prob + 1], first[0] = 0), as for mpa_dbg_chain_forward.  mode says which view of a problem the extraction gets:
 *   MPA_DBG_CHAIN_DENSE          every anchor, set_only 0: the main chain behind the pre-chain, the refinement chains
 *   MPA_DBG_CHAIN_SPARSE_SET     sparse, set_only 1: the pre-chain (a_out: the anchors of the kept chains, ascending; no u)
 *   MPA_DBG_CHAIN_SPARSE_CHAINS  sparse, set_only 0: the direct route (-S, --no-pre-chain)
 * The sparse view is mpa_dbg_prechain_sparse's: the anchors of runs of two or more whose consecutive blocks differ by at most
 * max(max_dist_x, bw) >> bbit, pred re-indexed into the view, n_total the full count.  It is exact when min_cnt rejects one-anchor
 * chains or the view leaves nothing out; the hook does not check that.
 * ctx != NULL: forward pass on the device, views built on the host from its f / pred and uploaded, then the product's own carving of
 * the extraction scratch, status memset and launch (chain_extract_launch for the set, chain_extract_pack for chains), on the context's
 * chaining pool as it is -- never zeroed between calls.  ctx == NULL: the host forward pass and chain_extract_core with a team of one,
 * in work space of the kernel's sizes (room for m + 64 chain ends), so that it declines what the kernel declines.
 * Out, per problem q: u[off_u[q] .. off_u[q + 1]) (score << 32 | anchors per chain) and a_out[off_a[q] .. off_a[q + 1]); u and a_out
 * have room for first[n_prob] words each; status[q] = 1: the extraction declined the problem (it needs the full list of chain ends and
 * n_total > m + 64), nothing written for it; rec[8 q ..]: the path the problem takes, computed on the host from f / pred and the view by
 * the preconditions of chain_core.h -- [0] anchors in the view m, [1] n_total, [2] non-roots (chained anchors) in the view, [3] their
 * largest score max_f, [4] the class, [5] c0 = n_total minus the non-roots scoring 256 or more (the region of level 1's bucket 0),
 * [6] the largest level-1 bucket (non-roots of 256 or more sharing bits 8-15 of their score), [7] why the full list is needed (bits).
 * Classes: FULL_LIST -- sorted_chain_ends_sparse returns -1 and the list fits; ONE_LEVEL -- max_f < 256; TWO_LEVEL; DECLINED. */
#define MPA_DBG_CHAIN_DENSE 0
#define MPA_DBG_CHAIN_SPARSE_SET 1
#define MPA_DBG_CHAIN_SPARSE_CHAINS 2
#define MPA_DBG_CHAIN_REC 8
#define MPA_DBG_CHAIN_FULL_LIST 0
#define MPA_DBG_CHAIN_ONE_LEVEL 1
#define MPA_DBG_CHAIN_TWO_LEVEL 2
#define MPA_DBG_CHAIN_DECLINED 3
#define MPA_DBG_CHAIN_WHY_MIN_CNT 1   /* min_cnt <= 1 */
#define MPA_DBG_CHAIN_WHY_MIN_SC 2    /* min_sc > kmer */
#define MPA_DBG_CHAIN_WHY_SMALL 4     /* n_total <= 64 */
#define MPA_DBG_CHAIN_WHY_MAX_F 8     /* max_f >= 65536, and nothing above */
#define MPA_DBG_CHAIN_WHY_OTHER 16    /* kmer outside 0..255, or a chained anchor that scores no more than a lone one */
int mpa_dbg_chain_extract(mpa_ctx_t *ctx, int32_t max_dist_x, int32_t max_dist_y, int32_t bw, int32_t max_skip, int32_t max_iter, int32_t min_cnt, int32_t min_sc,
                          float coef_log, int32_t is_spliced, int32_t kmer, int32_t bbit, int32_t n_prob, const int64_t *first, const uint64_t *a, int32_t mode,
                          int64_t *off_u, uint64_t *u, int64_t *off_a, uint64_t *a_out, int32_t *status, int64_t *rec);

/* Ranking and flat result of a batch (MPA_GPU_FINISH; miniprot_amd/csrc/finish_core.h) on hand-made tables: the tail
 * of mp_map() behind mp_align() -- mp_sort_reg, mp_select_multi_exon(opt->io), mp_set_parent(opt->mask_level, opt->mask_len, sub_diff = kmer)
 * and mp_select_sub(opt->pri_ratio, 2 kmer, opt->best_n) -- per query, the exclusive prefix of the queries' counts, and the gather of every
 * kept hit into the arrays of a result, laid out as mpa_batch_finish() lays them out.  On a context: k_finish_rank, k_finish_scan and
 * k_finish_gather; ctx == NULL: the shared core on the host with a team of one.
 * Query q's aligned regions are recs[first[q] .. first[q + 1]), first[0] = 0.  A record is 160 bytes: int64 vs, ve, first CIGAR word (in
 * words), first feature (in feats), first byte of its cs body (in cs_text), first byte of its rows slot (in rows_text); uint32 vid, hash;
 * int32 qs, qe, cnt, n_exon, chn_sc, chn_sc_ungap; parent, n_sub, subsc, dp_max2 (carried in); dp_score, dp_max, blen, n_fs, n_stop,
 * dist_stop, dist_start, n_iden, n_plus; n_cigar, n_feat; cs_len (< 0: no cs body carried); rows width, STA bytes, stride (the slot holds
 * four rows of `width` bytes `stride` apart and the STA bytes behind 4 stride; stride < 0: no rows carried); one word the hook ignores.
 * Every index is checked first: MPA_ERR_ARG for records that point outside their arrays.  *out: the result (mpa_result_destroy), hits
 * with qid = q; read its arrays with the accessors of mpamd.h or, as bytes, with mpa_dbg_result_flat.
 * mpa_dbg_finish_last: of the context's last device call, the hook's or a batch's inside its walks' call -- [0] queries, [1] hits in, [2] hits kept, [3] bytes the kernels wrote into pinned host memory (the result at its real size), [4] queries of
 * more than 64 regions (ranked in HBM scratch, not in LDS), [5] host waits of the call (a batch's: walks and finish together).
 * mpa_dbg_result_flat: array `which` of any result as bytes into buf[cap]; returns its size in bytes (written when it fits).  The cs and
 * rows references come field by field -- 16 bytes (int64 off; int32 len, present) and 24 bytes (int64 off; int32 width, n_sta, present,
 * zero) per hit, or none at all when no hit carries one -- every other array as it lies in the result. */
#define MPA_DBG_FINISH_REC 6
#define MPA_DBG_FLAT_HITS 0
#define MPA_DBG_FLAT_HIT_OFF 1
#define MPA_DBG_FLAT_CIGARS 2
#define MPA_DBG_FLAT_FEATS 3
#define MPA_DBG_FLAT_CS 4
#define MPA_DBG_FLAT_CS_TEXT 5
#define MPA_DBG_FLAT_ROWS 6
#define MPA_DBG_FLAT_ROWS_TEXT 7
int mpa_dbg_finish(mpa_ctx_t *ctx, const mpa_mapopt_t *opt, int32_t kmer, int32_t n_query, const int64_t *first, const void *recs, const uint32_t *words, int64_t n_words,
                   const mpa_feat_t *feats, int64_t n_feat, const char *cs_text, int64_t cs_bytes, const char *rows_text, int64_t rows_bytes, mpa_result_t **out);
int mpa_dbg_finish_last(const mpa_ctx_t *ctx, int64_t out[MPA_DBG_FINISH_REC]);
int64_t mpa_dbg_result_flat(const mpa_result_t *r, int32_t which, void *buf, int64_t cap);

/* The output text of a batch (MPA_GPU_FORMAT; miniprot_amd/csrc/format_core.h): what mpa_format_output() prints
 * for result r -- PAF, the carried --aln / --trans rows, GFF3 or GTF according to opt->flag, behind the output filters -- through select
 * and size, scan and write.  On a context: the result's arrays, the query names and the contigs' names and lengths go up and
 * k_format_size, k_format_scan and k_format_write put the text, with ids relative to the batch, and the places of its id fields into
 * pinned memory; ctx == NULL: the shared core on the host with a team of one (which builds the cs bodies and rows of hits that carry
 * none with the host's walks; on a context such a hit declines).  Then the patch with id0: every six-digit id field becomes field + id0.
 * *text (mpa_free): the text, *len its bytes, *n_out the printed hits (= how far the running id advances).  Returns MPA_OK, or
 * MPA_DBG_FORMAT_DECLINED when the step declined -- a blen of 0, something not carried, a gff_prefix longer than 64 bytes, ids reaching
 * seven digits, more text than the block's bound -- and *text is mpa_format_output()'s; negative: an error.  Every index of the result is
 * checked first.
 * mpa_dbg_format_last: of the context's last device call -- [0] queries, [1] hits printed, [2] bytes of text the kernels wrote, [3] id
 * fields, [4] host waits of the call, [5] 1 when it declined.
 * mpa_dbg_result_make: a result (mpa_result_destroy) from flat arrays laid out as mpa_dbg_result_flat gives them; cs / rows: the 16- /
 * 24-byte references of every hit, or NULL when no hit carries one.
 * mpa_dbg_idx_names: an index (mpa_idx_destroy) that holds contig names and lengths and nothing else -- all the formatter reads when
 * every aligned hit carries what the options print.  Contigs longer than any test could hold as sequence. */
#define MPA_DBG_FORMAT_REC 6
#define MPA_DBG_FORMAT_DECLINED 1
int mpa_dbg_format(mpa_ctx_t *ctx, const mpa_idx_t *mi, const mpa_mapopt_t *opt, const mpa_qbatch_t *q, const char *const *names, const mpa_result_t *r, int64_t id0, char **text,
                   int64_t *len, int64_t *n_out);
int mpa_dbg_format_last(const mpa_ctx_t *ctx, int64_t out[MPA_DBG_FORMAT_REC]);
int mpa_dbg_result_make(int32_t n_seq, const int64_t *hit_off, const mpa_hit_t *hits, const uint32_t *cigars, int64_t n_words, const mpa_feat_t *feats, int64_t n_feat, const void *cs,
                        const char *cs_text, int64_t cs_bytes, const void *rows, const char *rows_text, int64_t rows_bytes, mpa_result_t **out);
mpa_idx_t *mpa_dbg_idx_names(int32_t n_ctg, const char *const *names, const int64_t *lens);

#ifdef __cplusplus
}
#endif
#endif
