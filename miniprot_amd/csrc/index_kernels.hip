// index_kernels.hip -- the kernels of the index build on the device (k_index_scan, k_index_flag, k_index_compact), included by
// index_run.hip (which includes dev_common.h first: strand_base, d_hash32_mask, RefineTab, REFINE_CHUNK).

namespace mpa {

// ------------------------------------------------------------------------------------------------
// Index build on the device (mp_idx_build: build_worker + build_bidx, index.c:52-136; mp_sketch_nt4 + mp_sketch_clean_orf,
// sketch.c:40-100): every selected k-mer of every reading frame of both strands of every contig as (bucket << 32 | global
// block id); sorted and de-duplicated these keys ARE the index -- kb[] is their low words (inside a bucket ascending global
// block id = contig/strand order, then position, which is the reference's layout) and ki[] the bucket boundaries.
// k_index_scan: one workgroup per 2 048 positions of a strand (bases + halo in LDS); a thread forms the k-mer that ends at
// its position from `kmer` codons, hashes it, applies the modimizer test, and checks that the open reading frame around it
// has at least min_aa_len codons by walking its frame both ways (an ORF ends at a stop codon, an ambiguous base or the
// contig end).  Two passes over the genome: count per chunk, exclusive scan, then emit at exact offsets.
// ------------------------------------------------------------------------------------------------
struct IndexScanArgs {
	DevGenome g;
	const int64_t *chunk_first;     // [2 n_ctg + 1] first chunk of every strand
	const uint32_t *bo;             // [2 n_ctg] block offset of every strand
	int32_t n_strand, kmer, mod_bit, bbit, min_aa_len, halo;
	RefineTab rt;
};

// One kernel, three modes.  INDEX_COUNT / INDEX_EMIT are the two passes above; INDEX_HIST adds the keys to a coarse histogram of
// their buckets (bin = bucket >> hist_shift, n_bin = at most 4 096 counters in LDS behind the chunk's bases) -- what the multi-pass
// build plans its bucket ranges from: a workgroup walks its share of the chunks (chunk, chunk + gridDim.x, ...) with its counters
// in LDS and adds its non-zero bins to the global histogram once, one 64-bit atomic each: integers, so the sums are exact in any
// order.  RANGED: a key whose bin lies outside [bin_lo, bin_hi) is neither counted nor written, so that a pass builds the slice of
// the table that belongs to a contiguous range of buckets.  The one-pass build launches <INDEX_COUNT, false> and <INDEX_EMIT, false>,
// which use nothing of IndexPassArgs.
enum { INDEX_COUNT = 0, INDEX_EMIT = 1, INDEX_HIST = 2 };
struct IndexPassArgs {
	int64_t n_chunk;                // INDEX_HIST: chunks of the genome
	unsigned long long *hist;       // INDEX_HIST: [n_bin] global histogram
	int32_t hist_shift, n_bin;
	uint32_t bin_lo, bin_hi;        // RANGED
};

template<int MODE, bool RANGED>
__global__ __launch_bounds__(256) void k_index_scan(IndexScanArgs a, uint32_t *count, const uint64_t *offset, uint64_t *keys, IndexPassArgs r)
{
	extern __shared__ uint32_t lds_index[];
	uint8_t *base = (uint8_t*)lds_index;                            // [REFINE_CHUNK + 2 halo] nt4 codes, 15 = outside the contig
	__shared__ uint8_t tab[64];
	__shared__ uint32_t n_here;
	int64_t chunk = blockIdx.x;
	if (MODE == INDEX_HIST)
		for (int b = threadIdx.x; b < r.n_bin; b += 256) lds_index[(REFINE_CHUNK + 2 * a.halo) / 4 + b] = 0;   // (the halo is a multiple of 16 bases)
	do {
		int32_t lo = 0, hi = a.n_strand - 1;
		while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (a.chunk_first[mid] <= chunk) lo = mid; else hi = mid - 1; }
		const int32_t strand = lo, cid = strand >> 1, rev = strand & 1;
		const int64_t off = a.g.ctg_off[cid], clen = a.g.ctg_len[cid];
		const int64_t start = (chunk - a.chunk_first[strand]) * REFINE_CHUNK;
		const int32_t halo = a.halo, span = REFINE_CHUNK + 2 * halo;
		if (threadIdx.x < 64) tab[threadIdx.x] = a.rt.t[threadIdx.x];
		if (threadIdx.x == 0) n_here = 0;
		for (int k = threadIdx.x; k < span; k += 256) {
			const int64_t p = start - halo + k;
			base[k] = (p < 0 || p >= clen) ? 15 : (uint8_t)strand_base(a.g.seq, off, clen, rev, p);
		}
		__syncthreads();
		const uint32_t mask = (1u << (4 * a.kmer)) - 1, mask_mod = (1u << a.mod_bit) - 1;
		auto codon_at = [&](int e) -> uint32_t {                      // reduced residue of the codon whose last base is LDS index e; 0xff if none
			const uint32_t b0 = base[e - 2], b1 = base[e - 1], b2 = base[e];
			if ((b0 | b1 | b2) > 3) return 0xffu;
			return tab[b0 << 4 | b1 << 2 | b2];
		};
		const uint64_t out0 = MODE == INDEX_EMIT ? offset[chunk] : 0;
		for (int t = 0; t < REFINE_CHUNK / 256; ++t) {
			const int64_t pos = start + t * 256 + (int64_t)threadIdx.x; // strand-local position of the k-mer's last base
			if (pos >= clen) continue;
			const int e = (int)(pos - start) + halo;
			uint32_t word = 0;
			bool ok = true;
			for (int c = a.kmer - 1; c >= 0; --c) {
				const uint32_t r1 = codon_at(e - 3 * c);
				if (r1 == 0xffu) { ok = false; break; }
				word = word << 4 | r1;
			}
			if (!ok) continue;
			const uint32_t h = d_hash32_mask(word & mask, mask);
			if (h & mask_mod) continue;
			if (RANGED) { const uint32_t bin = (h >> a.mod_bit) >> r.hist_shift; if (bin < r.bin_lo || bin >= r.bin_hi) continue; }
			int32_t n = a.kmer;
			for (int q = e - 3 * a.kmer; n < a.min_aa_len && q >= 2 && codon_at(q) != 0xffu; q -= 3) ++n;
			for (int q = e + 3; n < a.min_aa_len && q < span && codon_at(q) != 0xffu; q += 3) ++n;
			if (n < a.min_aa_len) continue;
			if (MODE == INDEX_HIST) { atomicAdd(&lds_index[span / 4 + ((h >> a.mod_bit) >> r.hist_shift)], 1u); continue; }
			const uint32_t slot = atomicAdd(&n_here, 1u);
			if (MODE == INDEX_EMIT) keys[out0 + slot] = (uint64_t)(h >> a.mod_bit) << 32 | (uint64_t)((uint32_t)(pos >> a.bbit) + a.bo[strand]);
		}
		if (MODE != INDEX_HIST) break;
		__syncthreads();                                            // (the next chunk's bases overwrite this one's)
		chunk += gridDim.x;
	} while (chunk < r.n_chunk);
	if (MODE == INDEX_COUNT) {
		__syncthreads();
		if (threadIdx.x == 0) count[chunk] = n_here;
	}
	if (MODE == INDEX_HIST)
		for (int b = threadIdx.x; b < r.n_bin; b += 256) {
			const uint32_t v = lds_index[(REFINE_CHUNK + 2 * a.halo) / 4 + b];
			if (v) atomicAdd(&r.hist[b], (unsigned long long)v);
		}
}

// flag[i] = 1 where sorted key i differs from key i - 1
__global__ __launch_bounds__(256) void k_index_flag(const uint64_t *keys, int64_t n, uint32_t *flag)
{
	MPA_SHORT_KERNEL();
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}
// the distinct keys: kb[] = their block ids, cnt[bucket] = how many per bucket
__global__ __launch_bounds__(256) void k_index_compact(const uint64_t *keys, int64_t n, const uint32_t *flag, const uint64_t *idx, uint32_t *kb, unsigned long long *cnt)
{
	MPA_SHORT_KERNEL();
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n || !flag[i]) return;
	kb[idx[i]] = (uint32_t)keys[i];
	atomicAdd(&cnt[keys[i] >> 32], 1ULL);
}

} // namespace mpa
