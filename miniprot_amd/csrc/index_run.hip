// index_run.hip -- host driver of the index build on the device (dev_index_build, in one pass or in passes over bucket ranges) and
// its entry points of the C ABI.  The unit of the index-build kernels (index_kernels.hip).
#include "dev_ctx.h"
#include "index_kernels.hip"

namespace mpa {
// mp_idx_build's k-mer table on the device (index.c:52-136): scan (count, then emit), one radix sort of all keys, unique,
// bucket histogram + scan.  Leaves kb[] resident for the seeding kernels.  MPA_ERR_UNSUPPORTED (the caller builds on the host):
// parameters outside the kernel's range, or not enough device memory for the keys of this genome.
//
// The keys cost 44 bytes each while they are sorted (two key buffers, the sort's scratch, flags, a 64-bit scan, kb).  When that
// exceeds the budget, dev_index_build_passes builds the table in passes: a key is bucket << 32 | block, so the keys of a contiguous
// range of buckets give a contiguous slice of kb[] and that range's part of the bucket counts, and the ranges in ascending order
// concatenate into the bytes of the one-pass build.  A histogram of the keys over the top min(bucket bits, 12) bits of the bucket
// (k_index_scan<INDEX_HIST>) lets the host plan the fewest ranges that fit (idx_plan_passes); every pass counts and emits the keys of its
// range only (the RANGED instantiations), sorts, de-duplicates, adds to the one cnt[] array (indexed by absolute bucket) and hands its
// slice of kb[] to the host; the whole kb[] goes up once at the end, into the exact allocation a one-pass build leaves.
struct IndexPassEnv {
	mpa_ctx_t *ctx; mpa_idx_s *mi; DeviceIndex *d; hipStream_t s;
	IndexScanArgs a; size_t lds; int64_t n_chunk, n_keys; int bucket_bits; int64_t budget;
	DevBuf *b_count, *b_off, *b_tmp;
	double t0;
};

// the total of an exclusive scan of n 32-bit elements into 64-bit offsets: the last offset plus the last element (one wait on s)
static int scan_total(mpa_ctx_t *ctx, hipStream_t s, const uint64_t *off, const uint32_t *elem, int64_t n, int64_t *total)
{
	uint64_t last_off = 0;
	uint32_t last_elem = 0;
	HIP_TRY(hipMemcpyAsync(&last_off, off + (n - 1), 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(&last_elem, elem + (n - 1), 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	*total = (int64_t)(last_off + last_elem);
	return MPA_OK;
}

// the finished kb[] of a build takes the place of the resident one; the old table's bucket offsets go with it (the new table's go up
// with the first device sketch)
static void install_kb(DeviceIndex *d, DevTable<uint32_t> &kb)
{
	d->kb = std::move(kb);
	d->ki.release();
}

static int dev_index_build_passes(const IndexPassEnv &E)
{
	mpa_ctx_t *ctx = E.ctx;
	mpa_idx_s *mi = E.mi;
	hipStream_t s = E.s;
	const int64_t n_chunk = E.n_chunk;
	const size_t n_bucket = (size_t)1 << E.bucket_bits;
	const int hist_bits = std::min(E.bucket_bits, 12), hist_shift = E.bucket_bits - hist_bits, n_bin = 1 << hist_bits;
	const bool timed = timing_on();
	double ms_scan = 0;
	auto scan_clock = [&](double t) -> int { if (timed) { HIP_TRY(hipStreamSynchronize(s)); ms_scan += now_ms() - t; } return MPA_OK; };
	int rc;
	// 1. the histogram
	DevBuf b_hist;
	if ((rc = b_hist.ensure_exact((size_t)n_bin * 8))) return rc;
	HIP_TRY(hipMemsetAsync(b_hist.p, 0, (size_t)n_bin * 8, s));
	double tc = timed ? now_ms() : 0;
	IndexPassArgs r{ n_chunk, b_hist.as<unsigned long long>(), hist_shift, n_bin, 0u, 0u };
	hipLaunchKernelGGL((k_index_scan<INDEX_HIST, false>), dim3((unsigned)std::min<int64_t>(n_chunk, 2048)), dim3(256), E.lds + (size_t)n_bin * 4, s, E.a, (uint32_t*)nullptr,
	                   (const uint64_t*)nullptr, (uint64_t*)nullptr, r);
	HIP_TRY(hipGetLastError());
	if ((rc = scan_clock(tc))) return rc;
	std::vector<int64_t> hist((size_t)n_bin);
	HIP_TRY(hipMemcpyAsync(hist.data(), b_hist.p, (size_t)n_bin * 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	b_hist.release();
	int64_t hist_sum = 0, max_bin = 0;
	int32_t arg_max = 0;
	for (int32_t b = 0; b < n_bin; ++b) { hist_sum += hist[b]; if (hist[b] > max_bin) max_bin = hist[b], arg_max = b; }
	if (hist_sum != E.n_keys) { set_error("index build: the histogram of the keys does not add up to their count"); return MPA_ERR_HIP; }
	// 2. the plan
	const int64_t budget_keys = E.budget / 44;
	std::vector<int32_t> first_bin((size_t)n_bin + 1);
	const int32_t n_pass = idx_plan_passes(hist.data(), n_bin, budget_keys, first_bin.data());
	ctx->idx_stats.hist_bits = hist_bits, ctx->idx_stats.max_bin_keys = max_bin;
	ctx->idx_hist = hist;
	if (n_pass < 0) {
		set_error("index build: bin " + std::to_string(arg_max) + " of the " + std::to_string(n_bin) + "-bin key histogram holds " + std::to_string(max_bin) + " keys and would need " +
		          std::to_string(max_bin * 44) + " bytes of device memory, the budget is " + std::to_string(E.budget));
		return MPA_ERR_UNSUPPORTED;
	}
	int64_t max_pass = 0;
	std::vector<int64_t> pass_keys((size_t)n_pass, 0);
	for (int32_t p = 0; p < n_pass; ++p) {
		for (int32_t b = first_bin[p]; b < first_bin[p + 1]; ++b) pass_keys[p] += hist[b];
		max_pass = std::max(max_pass, pass_keys[p]);
	}
	// 3. the passes, over buffers sized once for the fullest of them
	DevBuf b_keys, b_keys2, b_flag, b_idx, b_kbp, b_cnt, b_ki;
	if ((rc = b_keys.ensure_exact((size_t)max_pass * 8 + 16)) || (rc = b_keys2.ensure_exact((size_t)max_pass * 8 + 16)) || (rc = b_flag.ensure_exact((size_t)max_pass * 4 + 16)) ||
	    (rc = b_idx.ensure_exact((size_t)max_pass * 8 + 16)) || (rc = b_kbp.ensure_exact((size_t)max_pass * 4 + 16)) || (rc = b_cnt.ensure_exact(n_bucket * 8)) ||
	    (rc = b_ki.ensure_exact(n_bucket * 8))) return rc;
	{	// (the sort's scratch for the fullest pass, before the first pass: what does not fit fails here)
		size_t tmp_bytes = 0;
		HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_bytes, b_keys.as<uint64_t>(), b_keys2.as<uint64_t>(), (size_t)max_pass, 0u, 32u + (unsigned)E.bucket_bits, s));
		if ((rc = E.b_tmp->ensure_exact(tmp_bytes + 256))) return rc;
	}
	HIP_TRY(hipMemsetAsync(b_cnt.p, 0, n_bucket * 8, s));
	std::vector<uint32_t> kb_new;
	kb_new.reserve((size_t)E.n_keys);                          // (an upper bound: the distinct keys are fewer)
	int64_t n_kb = 0;
	for (int32_t p = 0; p < n_pass; ++p) {
		const int64_t nk = pass_keys[p];
		if (nk == 0) continue;
		r.hist = nullptr, r.bin_lo = (uint32_t)first_bin[p], r.bin_hi = (uint32_t)first_bin[p + 1];
		tc = timed ? now_ms() : 0;
		hipLaunchKernelGGL((k_index_scan<INDEX_COUNT, true>), dim3((unsigned)n_chunk), dim3(256), E.lds, s, E.a, E.b_count->as<uint32_t>(), (const uint64_t*)nullptr, (uint64_t*)nullptr, r);
		HIP_TRY(hipGetLastError());
		if ((rc = scan_clock(tc))) return rc;
		if ((rc = dev_exclusive_scan(*E.b_tmp, true, rocprim::make_transform_iterator(E.b_count->as<uint32_t>(), U32ToU64()), E.b_off->as<uint64_t>(), (uint64_t)0, (size_t)n_chunk, s))) return rc;
		// (the emit pass writes at these offsets: they must add up to what the buffers were sized for)
		int64_t n_emit = 0;
		if ((rc = scan_total(ctx, s, E.b_off->as<uint64_t>(), E.b_count->as<uint32_t>(), n_chunk, &n_emit))) return rc;
		if (n_emit != nk) { set_error("index build: a pass counts other keys than the histogram gave it"); return MPA_ERR_HIP; }
		tc = timed ? now_ms() : 0;
		hipLaunchKernelGGL((k_index_scan<INDEX_EMIT, true>), dim3((unsigned)n_chunk), dim3(256), E.lds, s, E.a, (uint32_t*)nullptr, E.b_off->as<uint64_t>(), b_keys.as<uint64_t>(), r);
		HIP_TRY(hipGetLastError());
		if ((rc = scan_clock(tc))) return rc;
		if ((rc = dev_sort_keys(*E.b_tmp, true, b_keys.as<uint64_t>(), b_keys2.as<uint64_t>(), (size_t)nk, 0u, 32u + (unsigned)E.bucket_bits, s))) return rc;
		const uint64_t *sorted = b_keys2.as<uint64_t>();
		const unsigned nblk = (unsigned)((nk + 255) / 256);
		hipLaunchKernelGGL(k_index_flag, dim3(nblk), dim3(256), 0, s, sorted, nk, b_flag.as<uint32_t>());
		if ((rc = dev_exclusive_scan(*E.b_tmp, true, rocprim::make_transform_iterator(b_flag.as<uint32_t>(), U32ToU64()), b_idx.as<uint64_t>(), (uint64_t)0, (size_t)nk, s))) return rc;
		int64_t n_kb_pass = 0;
		if ((rc = scan_total(ctx, s, b_idx.as<uint64_t>(), b_flag.as<uint32_t>(), nk, &n_kb_pass))) return rc;
		if (n_kb_pass < 1 || n_kb_pass > nk) { set_error("index build: a pass has more distinct keys than keys"); return MPA_ERR_HIP; }
		hipLaunchKernelGGL(k_index_compact, dim3(nblk), dim3(256), 0, s, sorted, nk, b_flag.as<uint32_t>(), b_idx.as<uint64_t>(), b_kbp.as<uint32_t>(), b_cnt.as<unsigned long long>());
		HIP_TRY(hipGetLastError());
		kb_new.resize((size_t)(n_kb + n_kb_pass));
		HIP_TRY(hipMemcpyAsync(kb_new.data() + n_kb, b_kbp.p, (size_t)n_kb_pass * 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(wait_stream(ctx, s));
		n_kb += n_kb_pass;
	}
	// 4. bucket boundaries from the counts of all passes; the pass buffers go before the whole kb[] comes up
	if ((rc = dev_exclusive_scan(*E.b_tmp, true, b_cnt.as<uint64_t>(), b_ki.as<uint64_t>(), (uint64_t)0, n_bucket, s))) return rc;
	std::vector<int64_t> ki_new(n_bucket);
	HIP_TRY(hipMemcpyAsync(ki_new.data(), b_ki.p, n_bucket * 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	b_keys.release(), b_keys2.release(), b_flag.release(), b_idx.release(), b_kbp.release(), b_cnt.release(), b_ki.release();
	DevTable<uint32_t> d_kb;
	HIP_TRY(d_kb.take((size_t)n_kb * 4 + 16));
	HIP_TRY(hipMemcpyAsync(d_kb, kb_new.data(), (size_t)n_kb * 4, hipMemcpyHostToDevice, s));
	HIP_TRY(wait_stream(ctx, s));
	mi->ki.swap(ki_new), mi->kb.swap(kb_new), mi->n_kb = n_kb;
	install_kb(E.d, d_kb);
	ctx->idx_stats.n_pass = n_pass, ctx->idx_stats.max_pass_keys = max_pass;
	if (timed) {
		char note[64];
		snprintf(note, sizeof note, "index build on the GPU (%d passes)", (int)n_pass);
		timing_note("    index scans of all passes", ms_scan);
		timing_note(note, now_ms() - E.t0);
	}
	return MPA_OK;
}

int dev_index_build(mpa_ctx_t *ctx, mpa_idx_s *mi)
{
	const int32_t n_strand = (int32_t)mi->ctg.size() * 2;
	const mpa_idxopt_t &io = mi->opt;
	const int bucket_bits = io.kmer * 4 - io.mod_bit;
	if (n_strand == 0 || io.kmer < 1 || io.kmer > 7 || io.mod_bit < 0 || bucket_bits < 1 || bucket_bits > 28 || io.bbit < 0 || io.bbit > 20 || io.min_aa_len < io.kmer ||
	    io.min_aa_len > 1000) { set_error("index build: parameters outside the device kernel's range"); return MPA_ERR_UNSUPPORTED; }
	HIP_TRY(hipSetDevice(ctx->device));
	if (dev_upload_index(ctx, mi) != MPA_OK) return MPA_ERR_HIP;
	DeviceIndex *d = mi->dev[ctx->device];
	hipStream_t s = ctx->stream;
	std::vector<int64_t> chunk_first((size_t)n_strand + 1, 0);
	for (int32_t j = 0; j < n_strand; ++j) chunk_first[j + 1] = chunk_first[j] + (mi->ctg[j >> 1].len + REFINE_CHUNK - 1) / REFINE_CHUNK;
	const int64_t n_chunk = chunk_first[n_strand];
	if (n_chunk == 0 || n_chunk > 0x7fffffff) { set_error("index build: genome too small or too large for one launch"); return MPA_ERR_UNSUPPORTED; }
	const size_t n_bucket = (size_t)1 << bucket_bits;
	DevBuf b_first, b_bo, b_count, b_off, b_keys, b_keys2, b_flag, b_idx, b_tmp, b_cnt, b_ki;   // (gone with the call, however it ends)
	int rc;
	if ((rc = b_first.ensure(((size_t)n_strand + 1) * 8)) || (rc = b_bo.ensure((size_t)n_strand * 4 + 4)) || (rc = b_count.ensure((size_t)n_chunk * 4 + 4)) ||
	    (rc = b_off.ensure(((size_t)n_chunk + 1) * 8))) return rc;
	HIP_TRY(hipMemcpyAsync(b_first.p, chunk_first.data(), ((size_t)n_strand + 1) * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(hipMemcpyAsync(b_bo.p, mi->bo.data(), (size_t)n_strand * 4, hipMemcpyHostToDevice, s));
	IndexScanArgs a;
	a.g = DevGenome{ d->seq, d->ctg_off, d->ctg_len, nullptr, mi->l_seq };
	a.chunk_first = b_first.as<int64_t>(), a.bo = b_bo.as<uint32_t>();
	a.n_strand = n_strand, a.kmer = io.kmer, a.mod_bit = io.mod_bit, a.bbit = io.bbit, a.min_aa_len = io.min_aa_len, a.halo = (3 * io.min_aa_len + 2 + 15) & ~15;
	for (int c = 0; c < 64; ++c) a.rt.t[c] = tab_codon()[c] >= 20 ? 0xff : tab_codon13()[c];
	const size_t lds = (size_t)REFINE_CHUNK + 2 * (size_t)a.halo;
	const double t0 = now_ms();
	ctx->idx_stats = mpa_idx_build_stats_t{}, ctx->idx_stats.n_pass = 1;
	ctx->idx_hist.clear();
	hipLaunchKernelGGL((k_index_scan<INDEX_COUNT, false>), dim3((unsigned)n_chunk), dim3(256), lds, s, a, b_count.as<uint32_t>(), (const uint64_t*)nullptr, (uint64_t*)nullptr, IndexPassArgs{});
	HIP_TRY(hipGetLastError());
	// exclusive scan of the per-chunk counts (as 64-bit offsets)
	if ((rc = dev_exclusive_scan(b_tmp, false, rocprim::make_transform_iterator(b_count.as<uint32_t>(), U32ToU64()), b_off.as<uint64_t>(), (uint64_t)0, (size_t)n_chunk, s))) return rc;
	int64_t n_keys = 0;
	if ((rc = scan_total(ctx, s, b_off.as<uint64_t>(), b_count.as<uint32_t>(), n_chunk, &n_keys))) return rc;
	if (n_keys == 0) { mi->ki.assign(n_bucket, 0), mi->kb.clear(), mi->n_kb = 0; return MPA_OK; }
	{	// two key buffers, flags, scan, kb: ~40 bytes per key.  The budget for them is 7/8 of the free memory less the two bucket
		// tables, which every build needs; MPA_IDX_BUILD_MB (read on every call: for users who share a device) and the tests' hook cap it
		size_t free_b = 0, total_b = 0;
		int64_t budget = INT64_MAX;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
			if (n_bucket * 16 > free_b - (free_b >> 3)) { set_error("index build: not enough device memory for the bucket tables of this index"); return MPA_ERR_UNSUPPORTED; }
			budget = (int64_t)(free_b - (free_b >> 3) - n_bucket * 16);
		}
		const char *e = getenv("MPA_IDX_BUILD_MB");
		if (e && atoll(e) > 0) budget = std::min<int64_t>(budget, atoll(e) << 20);
		if (ctx->idx_budget_dbg > 0) budget = std::min(budget, ctx->idx_budget_dbg);
		ctx->idx_stats.n_keys = n_keys, ctx->idx_stats.max_pass_keys = n_keys, ctx->idx_stats.budget_bytes = budget;
		if (n_keys > budget / 44) {
			ctx->idx_stats.n_pass = 0, ctx->idx_stats.max_pass_keys = 0;
			return dev_index_build_passes(IndexPassEnv{ ctx, mi, d, s, a, lds, n_chunk, n_keys, bucket_bits, budget, &b_count, &b_off, &b_tmp, t0 });
		}
	}
	if ((rc = b_keys.ensure((size_t)n_keys * 8)) || (rc = b_keys2.ensure((size_t)n_keys * 8))) return rc;
	hipLaunchKernelGGL((k_index_scan<INDEX_EMIT, false>), dim3((unsigned)n_chunk), dim3(256), lds, s, a, (uint32_t*)nullptr, b_off.as<uint64_t>(), b_keys.as<uint64_t>(), IndexPassArgs{});
	HIP_TRY(hipGetLastError());
	if ((rc = dev_sort_keys(b_tmp, false, b_keys.as<uint64_t>(), b_keys2.as<uint64_t>(), (size_t)n_keys, 0u, 32u + (unsigned)bucket_bits, s))) return rc;
	b_keys.release();
	const uint64_t *sorted = b_keys2.as<uint64_t>();
	if ((rc = b_flag.ensure((size_t)n_keys * 4)) || (rc = b_idx.ensure((size_t)n_keys * 8)) || (rc = b_cnt.ensure(n_bucket * 8)) || (rc = b_ki.ensure(n_bucket * 8))) return rc;
	const unsigned nblk = (unsigned)((n_keys + 255) / 256);
	hipLaunchKernelGGL(k_index_flag, dim3(nblk), dim3(256), 0, s, sorted, n_keys, b_flag.as<uint32_t>());
	if ((rc = dev_exclusive_scan(b_tmp, false, rocprim::make_transform_iterator(b_flag.as<uint32_t>(), U32ToU64()), b_idx.as<uint64_t>(), (uint64_t)0, (size_t)n_keys, s))) return rc;
	int64_t n_kb = 0;
	if ((rc = scan_total(ctx, s, b_idx.as<uint64_t>(), b_flag.as<uint32_t>(), n_keys, &n_kb))) return rc;
	DevTable<uint32_t> d_kb;                               // (a local until the table is whole: an error below gives it back)
	HIP_TRY(d_kb.take((size_t)n_kb * 4 + 16));
	HIP_TRY(hipMemsetAsync(b_cnt.p, 0, n_bucket * 8, s));
	hipLaunchKernelGGL(k_index_compact, dim3(nblk), dim3(256), 0, s, sorted, n_keys, b_flag.as<uint32_t>(), b_idx.as<uint64_t>(), (uint32_t*)d_kb, b_cnt.as<unsigned long long>());
	if ((rc = dev_exclusive_scan(b_tmp, false, b_cnt.as<uint64_t>(), b_ki.as<uint64_t>(), (uint64_t)0, n_bucket, s))) return rc;
	HIP_TRY(hipGetLastError());
	// (into temporaries: a copy that fails must not leave the index with a half-filled table)
	std::vector<int64_t> ki_new(n_bucket);
	std::vector<uint32_t> kb_new((size_t)n_kb);
	HIP_TRY(hipMemcpyAsync(ki_new.data(), b_ki.p, n_bucket * 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(kb_new.data(), (const uint32_t*)d_kb, (size_t)n_kb * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(wait_stream(ctx, s));
	mi->ki.swap(ki_new), mi->kb.swap(kb_new), mi->n_kb = n_kb;
	install_kb(d, d_kb);                                   // stays resident for the seeding kernels
	timing_note("index build on the GPU", now_ms() - t0);
	return MPA_OK;
}
} // namespace mpa

extern "C" {

int mpa_idx_build_kmers_device(mpa_ctx_t *ctx, mpa_idx_t *mi)
{
	if (!ctx) { set_error("no device context"); return MPA_ERR_NO_DEVICE; }
	return mpa::guarded<int>(MPA_ERR_HIP, [&] { return dev_index_build(ctx, mi); });
}

void mpa_idx_build_last_stats(const mpa_ctx_t *ctx, mpa_idx_build_stats_t *st) { if (st) *st = ctx ? ctx->idx_stats : mpa_idx_build_stats_t{}; }
void mpa_dbg_idx_build_budget(mpa_ctx_t *ctx, int64_t bytes) { if (ctx) ctx->idx_budget_dbg = bytes > 0 ? bytes : 0; }
int32_t mpa_dbg_idx_build_hist(const mpa_ctx_t *ctx, int64_t *hist, int32_t cap)
{
	if (!ctx) return 0;
	const int32_t n = (int32_t)ctx->idx_hist.size();
	if (hist && cap > 0) memcpy(hist, ctx->idx_hist.data(), (size_t)std::min(n, cap) * 8);
	return n;
}

} // extern "C"
