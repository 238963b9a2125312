// refine_kernels.hip -- the kernels of the refinement stage (mp_refine_reg, map.c:32-111), included by refine_run.hip (which includes
// dev_common.h first: strand_base, packed_window16, d_hash32_mask, RefineTab, REFINE_CHUNK): the window scans k_refine_scan /
// k_refine_scan_gset (hits for the host to pair) and k_refine_scan_map / k_refine_scan_gmap (hits counted per group), the k-mer
// tables of long queries in device memory (k_refine_gmap_build) and the pairing kernels k_refine_pair_count / _emit / _decode.
// The chains of the pairs are the seeding stage's (seed_run.hip: chain_fwd_launch, chain_extract_pack).

namespace mpa {

// ------------------------------------------------------------------------------------------------
// Refinement scan (map.c:97-111 = mp_sketch_nt4 + mp_sketch_clean_orf at k = kmer2, every k-mer, base resolution): which
// positions of a region's window end a k-mer that the query also has?  One workgroup per 2048-position chunk of a window;
// the query's k-mer words sit in an LDS hash set, the chunk's bases (with a halo wide enough to decide the minimum ORF
// length) in LDS as well.  A thread forms the k-mer that ENDS at its position directly from five codons -- no rolling
// state, so chunks are independent.  Hits go to one global list (window, position, hash); the host groups and pairs them.
// ------------------------------------------------------------------------------------------------
struct RefineWindowDev { int64_t as; int32_t qid, vid, len, pad; };
struct RefineChunk { int32_t win, start; };
#define REFINE_HALO 112
#define REFINE_LCAP 384                                     /* hits a workgroup of k_refine_scan_map collects in LDS per chunk before it asks for room in the global list */
#define REFINE_SUPER 4                                      /* chunks of one window a workgroup of k_refine_scan_map sweeps (round 5, one atomic per hit: 8 chunks measured 10.9 ms against 9.0 alone; round 6, hits collected per workgroup: see profiles/r06_experiments.txt) */


// The k-mer maps of LONG queries live in device memory instead of LDS (past 4 096 LDS slots a workgroup's map would take the CU's
// LDS from the DP): one open-addressing table per long query in a pool, 8 bytes per slot = (k-mer word, group), so that ONE load
// answers a probe; same hash as the LDS maps, slots = the power of two >= 2 x entries (at least 1 024), empty = all ones.  The
// tables of a batch are built once per batch (k_refine_gmap_build, behind one memset of the pool) and stay in L2 for the scan:
// 1 MB for a 36 000-residue protein against 4 MiB of L2 per XCD.
struct RefineGmap {
	const uint2 *slots;          // the pool
	const int64_t *desc;         // [n_query] first slot << 8 | log2(slots) of the query's table (meaningless for a query that has none)
};
__device__ __forceinline__ uint32_t gmap_probe(const uint2 *tab, int32_t log2, uint32_t word)     // the group of `word`, 0xffffffff = not in the table
{
	const uint32_t m = (1u << log2) - 1;
	for (uint32_t slot = (word * 2654435761u) >> (32 - log2);; slot = (slot + 1) & m) {
		const uint2 kv = tab[slot];
		if (kv.x == word) return kv.y;
		if (kv.x == 0xffffffffu) return 0xffffffffu;              // (at most half of the slots are taken: the walk ends)
	}
}
// one workgroup column per long query (blockIdx.y); words[first[q] .. first[q + 1]) are its entries, equal words share a slot
__global__ __launch_bounds__(256) void k_refine_gmap_build(const int64_t *first, const uint32_t *words, const int32_t *long_q, const int64_t *desc, uint32_t *pool)
{
	MPA_SHORT_KERNEL();
	const int32_t q = long_q[blockIdx.y];
	const int64_t d = desc[q], k0 = first[q], k1 = first[q + 1];
	const int32_t log2 = (int32_t)(d & 255);
	const uint32_t m = (1u << log2) - 1;
	uint32_t *tab = pool + 2 * (d >> 8);                          // slot s = tab[2 s] (word), tab[2 s + 1] (entry)
	for (int64_t k = k0 + (int64_t)blockIdx.x * 256 + threadIdx.x; k < k1; k += (int64_t)gridDim.x * 256) {
		const uint32_t word = words[k];
		uint32_t slot = (word * 2654435761u) >> (32 - log2);
		for (;;) {
			const uint32_t old = atomicCAS(&tab[2 * slot], 0xffffffffu, word);
			if (old == 0xffffffffu) { tab[2 * slot + 1] = (uint32_t)(k - k0); break; }
			if (old == word) break;
			slot = (slot + 1) & m;
		}
	}
}

// GSET: the query's k-mer set is its table in device memory (RefineGmap), not an LDS set filled by the workgroup
template <bool GSET>
__device__ __forceinline__ void refine_scan_body(DevGenome g, const RefineWindowDev *wins, const RefineChunk *chunks, const int64_t *qw_first, const uint32_t *qwords,
                                                 const RefineTab &rt, int32_t kmer, int32_t min_aa_len, int32_t hs_log2, uint4 *hits, unsigned long long *n_hits, unsigned long long cap,
                                                 const RefineGmap gm)
{
	MPA_SHORT_KERNEL();
	extern __shared__ uint32_t lds_refine[];
	const int32_t HS = GSET ? 0 : 1 << hs_log2;
	uint32_t *table = lds_refine;                                   // [HS] open addressing, 0xffffffff = empty
	uint8_t *base = (uint8_t*)(table + HS);                         // [REFINE_CHUNK + 2 * REFINE_HALO] nt4 codes, 15 = outside the window
	__shared__ uint8_t tab[64];                                    // codon -> reduced residue, 0xff = stop
	const RefineChunk ch = chunks[blockIdx.x];
	const RefineWindowDev w = wins[ch.win];
	const int cid = w.vid >> 1, rev = w.vid & 1;
	const int64_t off = g.ctg_off[cid], clen = g.ctg_len[cid];
	if (threadIdx.x < 64) tab[threadIdx.x] = rt.t[threadIdx.x];
	for (int k = threadIdx.x; k < HS; k += 256) table[k] = 0xffffffffu;
	for (int k = threadIdx.x; k < REFINE_CHUNK + 2 * REFINE_HALO; k += 256) {
		const int64_t p = (int64_t)ch.start - REFINE_HALO + k;        // window-local
		base[k] = (p < 0 || p >= w.len) ? 15 : (uint8_t)strand_base(g.seq, off, clen, rev, w.as + p);
	}
	__syncthreads();
	if (!GSET) for (int64_t k = qw_first[w.qid] + threadIdx.x; k < qw_first[w.qid + 1]; k += 256) {
		const uint32_t word = qwords[k];
		uint32_t slot = (word * 2654435761u) >> (32 - hs_log2);
		for (;;) {
			const uint32_t old = atomicCAS(&table[slot], 0xffffffffu, word);
			if (old == 0xffffffffu || old == word) break;
			slot = (slot + 1) & (HS - 1);
		}
	}
	__syncthreads();
	const int64_t gd = GSET ? gm.desc[w.qid] : 0;
	const uint2 *gtab = GSET ? gm.slots + (gd >> 8) : nullptr;
	const uint32_t mask = (1u << (4 * kmer)) - 1;
	auto codon_at = [&](int e) -> uint32_t {                          // reduced residue of the codon whose last base is LDS index e; 0xff if none
		const uint32_t b0 = base[e - 2], b1 = base[e - 1], b2 = base[e];
		if ((b0 | b1 | b2) > 3) return 0xffu;
		return tab[b0 << 4 | b1 << 2 | b2];
	};
	for (int t = 0; t < REFINE_CHUNK / 256; ++t) {
		const int32_t pos = ch.start + t * 256 + (int32_t)threadIdx.x;   // window-local position of the k-mer's last base
		if (pos >= w.len) continue;
		const int e = pos - ch.start + REFINE_HALO;
		uint32_t word = 0;
		bool ok = true;
		for (int c = kmer - 1; c >= 0; --c) {
			const uint32_t r = codon_at(e - 3 * c);
			if (r == 0xffu) { ok = false; break; }
			word = word << 4 | r;
		}
		if (!ok) continue;
		word &= mask;
		bool found = false;
		if (GSET) found = gmap_probe(gtab, (int32_t)(gd & 255), word) != 0xffffffffu;
		else for (uint32_t slot = (word * 2654435761u) >> (32 - hs_log2);; slot = (slot + 1) & (HS - 1)) {
			const uint32_t v = table[slot];
			if (v == word) { found = true; break; }
			if (v == 0xffffffffu) break;
		}
		if (!found) continue;
		// the open reading frame around the k-mer must be at least min_aa_len codons long (sketch.c:64-100)
		int32_t n = kmer;
		for (int q = e - 3 * kmer; n < min_aa_len && q >= 2 && codon_at(q) != 0xffu; q -= 3) ++n;
		for (int q = e + 3; n < min_aa_len && q < REFINE_CHUNK + 2 * REFINE_HALO && codon_at(q) != 0xffu; q += 3) ++n;
		if (n < min_aa_len) continue;
		const unsigned long long at = atomicAdd(n_hits, 1ULL);
		if (at < cap) hits[at] = make_uint4((uint32_t)ch.win, (uint32_t)pos, d_hash32_mask(word, mask), 0u);
	}
}
__global__ __launch_bounds__(256) void k_refine_scan(DevGenome g, const RefineWindowDev *wins, const RefineChunk *chunks, const int64_t *qw_first, const uint32_t *qwords,
                                                     RefineTab rt, int32_t kmer, int32_t min_aa_len, int32_t hs_log2, uint4 *hits, unsigned long long *n_hits, unsigned long long cap)
{
	refine_scan_body<false>(g, wins, chunks, qw_first, qwords, rt, kmer, min_aa_len, hs_log2, hits, n_hits, cap, RefineGmap{ nullptr, nullptr });
}
// the same scan for the windows of long queries: the k-mer set is the query's table in device memory; LDS holds the bases only
__global__ __launch_bounds__(256) void k_refine_scan_gset(DevGenome g, const RefineWindowDev *wins, const RefineChunk *chunks, RefineTab rt, int32_t kmer, int32_t min_aa_len,
                                                          uint4 *hits, unsigned long long *n_hits, unsigned long long cap, RefineGmap gm)
{
	refine_scan_body<true>(g, wins, chunks, nullptr, nullptr, rt, kmer, min_aa_len, 0, hits, n_hits, cap, gm);
}

// ------------------------------------------------------------------------------------------------
// Refinement pairing on the device (mp_refine_reg, map.c:53-79): the window positions and the query positions that carry the
// same k-mer, all pairs per k-mer unless there are too many.
//   k_refine_scan_map   the refinement scan again, but the query's DISTINCT k-mers ("groups") sit in an LDS map word -> group, and
//                       every hit also counts itself in wcnt[window][group]: n1 of map.c:66 needs no sort
//   k_refine_pair_count n2 = the group's query positions; the pairs of a hit are n2 if n1 * n2 <= max_ava (32-bit product, as the
//                       reference computes it), else none
//   (exclusive scan)    where each hit's pairs go
//   k_refine_pair_emit  window << 44 | window position << 22 | query position -- one radix sort of these keys is the reference's
//                       sort of every window's pair list (map.c:80), and the window boundaries fall out of per-window counts
//   k_refine_pair_decode  position << 32 | query position: the anchors mp_chain() takes (bbit = 0)
// ------------------------------------------------------------------------------------------------
struct RefineGroups {
	const int64_t *qg_first;     // [n_query + 1] first group of every query
	const uint32_t *gword;       // [n_group] the packed k-mer word of the group
	const uint32_t *gfirst;      // [n_group] its first entry in qpos
	const uint32_t *gcount;      // [n_group] how many query positions carry it
	const uint32_t *qpos;        // query positions (index of the k-mer's last residue), group by group, ascending inside a group
};

// GMAP: the map word -> group is the query's table in device memory (RefineGmap, built by k_refine_gmap_build), not an LDS map that
// the workgroup fills; LDS then holds bases, codons and the hit buffer only
template <bool GMAP>
__device__ __forceinline__ void refine_scan_map_body(DevGenome g, const RefineWindowDev *wins, const RefineChunk *chunks, RefineGroups gr, const int64_t *wg_first, const RefineTab &rt,
                                                     int32_t kmer, int32_t min_aa_len, int32_t hs_log2, uint4 *hits, unsigned long long *n_hits, unsigned long long cap, uint32_t *wcnt,
                                                     const int32_t n_super, const RefineGmap gm)
{
	MPA_SHORT_KERNEL();
	extern __shared__ uint32_t lds_refine[];
	const int32_t HS = GMAP ? 0 : 1 << hs_log2;
	uint32_t *tkey = lds_refine, *tval = tkey + HS;               // open addressing: word -> group (0xffffffff = empty)
	uint8_t *base = (uint8_t*)(tval + HS);                          // [REFINE_CHUNK + 2 * REFINE_HALO] nt4 codes, 15 = outside the window
	uint8_t *cod = base + REFINE_CHUNK + 2 * REFINE_HALO;           // [same] reduced-alphabet code of the codon ENDING at each position, 0xff = none
	__shared__ uint8_t tab[64];
	// The hits of a chunk are collected in LDS and get their places in the global list with ONE returning atomic per workgroup and
	// chunk that has any (round 5: one per hit -- 3.5 M returning atomics on one address per launch, which IS the 8 ms the kernel
	// took: profiles/r05_pmc_summary.json, 72 % of the wave cycles waiting).  A hit beyond REFINE_LCAP takes its place directly, as
	// before.  The order of the list means nothing: its consumers index it (k_refine_pair_count / _emit) and sort what they emit.
	__shared__ uint4 l_hit[REFINE_LCAP];
	__shared__ uint32_t l_n;
	__shared__ unsigned long long l_base;
	if (threadIdx.x == 0) l_n = 0;
	const RefineChunk ch = chunks[blockIdx.x];
	const RefineWindowDev w = wins[ch.win];
	const int cid = w.vid >> 1, rev = w.vid & 1;
	const int64_t off = g.ctg_off[cid], clen = g.ctg_len[cid];
	if (threadIdx.x < 64) tab[threadIdx.x] = rt.t[threadIdx.x];
	for (int k = threadIdx.x; k < HS; k += 256) tkey[k] = 0xffffffffu;
	__syncthreads();
	// the query's k-mer map, once per workgroup; a workgroup sweeps REFINE_SUPER consecutive chunks of its window
	const int64_t G0 = gr.qg_first[w.qid], G1 = gr.qg_first[w.qid + 1];
	const int64_t gd = GMAP ? gm.desc[w.qid] : 0;
	const uint2 *gtab = GMAP ? gm.slots + (gd >> 8) : nullptr;
	if (!GMAP) for (int64_t k = G0 + threadIdx.x; k < G1; k += 256) {
		const uint32_t word = gr.gword[k];
		uint32_t slot = (word * 2654435761u) >> (32 - hs_log2);
		for (;;) {
			const uint32_t old = atomicCAS(&tkey[slot], 0xffffffffu, word);
			if (old == 0xffffffffu) { tval[slot] = (uint32_t)(k - G0); break; }     // (the groups' words are distinct)
			slot = (slot + 1) & (HS - 1);
		}
	}
	__syncthreads();
	const uint32_t mask = (1u << (4 * kmer)) - 1;
	auto codon_at = [&](int e) -> uint32_t { return cod[e]; };
	const int64_t wc0 = wg_first[ch.win];
	for (int32_t cstart = ch.start; cstart < w.len && cstart < ch.start + n_super * REFINE_CHUNK; cstart += REFINE_CHUNK) {
	if (cstart != ch.start) __syncthreads();                    // (the scan of the chunk before has finished with base[] and cod[])
	// the chunk's bases and its halo, sixteen per thread from three aligned words of the packed genome (a byte load per base before)
	static_assert((REFINE_CHUNK + 2 * REFINE_HALO) % 16 == 0, "chunk + halo must be a multiple of 16");
	for (int k = threadIdx.x * 16; k < REFINE_CHUNK + 2 * REFINE_HALO; k += 256 * 16) {
		const int64_t p = (int64_t)cstart - REFINE_HALO + k;         // window position of base[k]
		const int64_t x = w.as + p;                                    // strand position
		const uint64_t nib = packed_window16(g.seq, g.l_seq, rev ? off + clen - 1 - x : off + x, rev ? -1 : 1, rev);
		uint32_t o[4];
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			uint32_t v = 0;
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const int64_t pj = p + 4 * q + j;
				const uint32_t bb = (pj < 0 || pj >= w.len) ? 15u : (uint32_t)(nib >> (4 * (4 * q + j))) & 15u;
				v |= bb << (8 * j);
			}
			o[q] = v;
		}
		uint32_t *dst = (uint32_t*)(base + k);                       // (k is a multiple of 16, base of 4)
		dst[0] = o[0], dst[1] = o[1], dst[2] = o[2], dst[3] = o[3];
	}
	__syncthreads();
	// the codon ending at every position, once (every k-mer and every reading-frame walk below reads these instead of three bases
	// and the table per codon)
	for (int e = threadIdx.x; e < REFINE_CHUNK + 2 * REFINE_HALO; e += 256) {
		uint32_t c = 0xffu;
		if (e >= 2) {
			const uint32_t b0 = base[e - 2], b1 = base[e - 1], b2 = base[e];
			if ((b0 | b1 | b2) <= 3) c = tab[b0 << 4 | b1 << 2 | b2];
		}
		cod[e] = (uint8_t)c;
	}
	__syncthreads();
	// Who scans what: thread 3q + r (q < 85) takes the PER positions 3 PER q + r, + 3, + 6, ... -- one reading frame of a stretch of 3 PER
	// bases -- so that the k-mer word ROLLS: one codon read per position instead of kmer (round 5: thread t took positions t, t + 256,
	// ...: five LDS byte reads per k-mer).  Thread 255 takes the chunk's last PER positions the old way.  `run` = valid codons in a row.
	constexpr int PER = REFINE_CHUNK / 256;
	auto try_hit = [&](const int32_t pos, const int e, const uint32_t word) {
		uint32_t grp = 0xffffffffu;
		if (GMAP) grp = gmap_probe(gtab, (int32_t)(gd & 255), word);
		else for (uint32_t slot = (word * 2654435761u) >> (32 - hs_log2);; slot = (slot + 1) & (HS - 1)) {
			const uint32_t v = tkey[slot];
			if (v == word) { grp = tval[slot]; break; }
			if (v == 0xffffffffu) break;
		}
		if (grp == 0xffffffffu) return;
		int32_t n = kmer;
		for (int q = e - 3 * kmer; n < min_aa_len && q >= 2 && codon_at(q) != 0xffu; q -= 3) ++n;
		for (int q = e + 3; n < min_aa_len && q < REFINE_CHUNK + 2 * REFINE_HALO && codon_at(q) != 0xffu; q += 3) ++n;
		if (n < min_aa_len) return;
		const uint4 hit = make_uint4((uint32_t)ch.win, (uint32_t)pos, (uint32_t)(G0 + grp), grp);
		const uint32_t li = atomicAdd(&l_n, 1u);
		if (li < REFINE_LCAP) l_hit[li] = hit;
		else {
			const unsigned long long at = atomicAdd(n_hits, 1ULL);
			if (at < cap) hits[at] = hit;
		}
		atomicAdd(&wcnt[wc0 + grp], 1u);
	};
	if (threadIdx.x < 255) {
		const int q3 = (int)threadIdx.x / 3, fr = (int)threadIdx.x - 3 * q3;
		const int e0 = REFINE_HALO + 3 * PER * q3 + fr;              // LDS index of the last base of the thread's first k-mer
		uint32_t word = 0;
		int run = 0;
		for (int c = kmer - 1; c >= 1; --c) {                         // the kmer - 1 codons before it
			const uint32_t r = codon_at(e0 - 3 * c);
			if (r == 0xffu) run = 0, word = 0; else word = word << 4 | r, ++run;
		}
#pragma unroll
		for (int j = 0; j < PER; ++j) {
			const int e = e0 + 3 * j;
			const uint32_t r = codon_at(e);
			if (r == 0xffu) { run = 0, word = 0; continue; }
			word = (word << 4 | r) & mask, ++run;
			const int32_t pos = cstart + e - REFINE_HALO;
			if (run >= kmer && pos < w.len) try_hit(pos, e, word);
		}
	} else {
		for (int j = 0; j < PER; ++j) {
			const int e = REFINE_HALO + 3 * PER * 85 + j;
			const int32_t pos = cstart + e - REFINE_HALO;
			if (pos >= w.len) continue;
			uint32_t word = 0;
			bool ok = true;
			for (int c = kmer - 1; c >= 0; --c) {
				const uint32_t r = codon_at(e - 3 * c);
				if (r == 0xffu) { ok = false; break; }
				word = word << 4 | r;
			}
			if (ok) try_hit(pos, e, word & mask);
		}
	}
	__syncthreads();
	// (the buffer is emptied when a chunk leaves it more than half full, and behind the workgroup's last chunk)
	const bool last_chunk = cstart + REFINE_CHUNK >= w.len || cstart + REFINE_CHUNK >= ch.start + n_super * REFINE_CHUNK;
	const uint32_t ln = (l_n >= REFINE_LCAP / 2 || last_chunk) ? (l_n < REFINE_LCAP ? l_n : REFINE_LCAP) : 0u;
	if (ln) {                                                   // (uniform: every thread sees the same count behind the barrier)
		if (threadIdx.x == 0) l_base = atomicAdd(n_hits, (unsigned long long)ln);
		__syncthreads();
		for (uint32_t k = threadIdx.x; k < ln; k += 256) { const unsigned long long at = l_base + k; if (at < cap) hits[at] = l_hit[k]; }
		__syncthreads();
		if (threadIdx.x == 0) l_n = 0;
	}
	}
}
__global__ __launch_bounds__(256) void k_refine_scan_map(DevGenome g, const RefineWindowDev *wins, const RefineChunk *chunks, RefineGroups gr, const int64_t *wg_first, RefineTab rt,
                                                         int32_t kmer, int32_t min_aa_len, int32_t hs_log2, uint4 *hits, unsigned long long *n_hits, unsigned long long cap, uint32_t *wcnt,
                                                         const int32_t n_super)
{
	refine_scan_map_body<false>(g, wins, chunks, gr, wg_first, rt, kmer, min_aa_len, hs_log2, hits, n_hits, cap, wcnt, n_super, RefineGmap{ nullptr, nullptr });
}
// the fourth size class ("long": more groups than the largest LDS map takes)
__global__ __launch_bounds__(256) void k_refine_scan_gmap(DevGenome g, const RefineWindowDev *wins, const RefineChunk *chunks, RefineGroups gr, const int64_t *wg_first, RefineTab rt,
                                                          int32_t kmer, int32_t min_aa_len, uint4 *hits, unsigned long long *n_hits, unsigned long long cap, uint32_t *wcnt,
                                                          const int32_t n_super, RefineGmap gm)
{
	refine_scan_map_body<true>(g, wins, chunks, gr, wg_first, rt, kmer, min_aa_len, 0, hits, n_hits, cap, wcnt, n_super, gm);
}

__global__ __launch_bounds__(256) void k_refine_pair_count(const uint4 *hits, int64_t n_hits, const int64_t *wg_first, const uint32_t *wcnt, const uint32_t *gcount, int32_t max_ava,
                                                           uint32_t *pc, uint32_t *wpairs)
{
	MPA_SHORT_KERNEL();
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_hits) return;
	const uint4 h = hits[i];
	const int32_t n1 = (int32_t)wcnt[wg_first[h.x] + h.w], n2 = (int32_t)gcount[h.z];
	const uint32_t c = (n2 > 0 && (int32_t)((uint32_t)n1 * (uint32_t)n2) <= max_ava) ? (uint32_t)n2 : 0u;   // (the reference's 32-bit product, wrap-around and all)
	pc[i] = c;
	if (c) atomicAdd(&wpairs[h.x], c);
}

__global__ __launch_bounds__(256) void k_refine_pair_emit(const uint4 *hits, int64_t n_hits, const uint32_t *pc, const uint64_t *po, RefineGroups gr, uint64_t *keys)
{
	MPA_SHORT_KERNEL();
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_hits) return;
	const uint32_t c = pc[i];
	if (!c) return;
	const uint4 h = hits[i];
	const uint64_t hi = (uint64_t)h.x << 44 | (uint64_t)h.y << 22;
	const uint32_t *qp = gr.qpos + gr.gfirst[h.z];
	uint64_t *dst = keys + po[i];
	for (uint32_t j = 0; j < c; ++j) dst[j] = hi | qp[j];
}

__global__ __launch_bounds__(256) void k_refine_pair_decode(const uint64_t *keys, int64_t n, uint64_t *a)
{
	MPA_SHORT_KERNEL();
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) { const uint64_t k = keys[i]; a[i] = ((k >> 22) & 0x3fffffULL) << 32 | (k & 0x3fffffULL); }
}

} // namespace mpa
