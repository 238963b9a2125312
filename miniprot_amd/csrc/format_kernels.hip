// format_kernels.hip -- the output text of a batch on the device (MPA_GPU_FORMAT), included by stats_run.hip,
// whose dev_format() launches them.  The code itself is format_core.h, the one source the host model runs too; this file is its device
// team and the kernels around it.
//   k_format_size    one wavefront per query: which of its hits are printed, the exact bytes and id fields of each, the query's sums
//   k_format_scan    the exclusive prefix of the sums over the batch: one workgroup, FORMAT_SCAN queries per step and a carry; the
//                    totals go to the head of the pinned block
//   k_format_write   one workgroup per query, one wavefront per printed hit at a time: the hit's text at its offset and the places of
//                    its id fields, into the pinned block.  A batch that was declined while sizing (a blen of 0, a cs string or rows
//                    that a hit does not carry) or whose text or id fields exceed the room the host gave writes nothing
// Plain vector stores only.  Wave64, latency-bound kernels of small problems, like the finish kernels.

namespace mpa {

#define FORMAT_SCAN 256                                   /* queries per step of k_format_scan (its workgroup) */
#define FORMAT_WRITE_WAVES 4                              /* hits a workgroup of k_format_write writes side by side */

struct FormatWave : CoopWave {                            // the team of format_core.h on the device: one wavefront
	static __device__ __forceinline__ int64_t sum64(int64_t v)
	{
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
		return v;
	}
};

__global__ __launch_bounds__(64) void k_format_size(FmtOpt o, FmtSrc S, int32_t n_query, FmtAt *at, FmtCounts *cnt)
{
	MPA_SHORT_KERNEL();
	const int32_t q = (int32_t)blockIdx.x;
	if (q >= n_query) return;
	format_size_core<FormatWave>(o, S, q, at, cnt + q);
}

__global__ __launch_bounds__(FORMAT_SCAN) void k_format_scan(const FmtCounts *cnt, int32_t n_query, FmtCounts *off, FmtCounts *head)
{
	MPA_SHORT_KERNEL();
	__shared__ int64_t s_tot[FORMAT_SCAN / 64][4];
	const int t = (int)threadIdx.x, wave = t >> 6;
	int64_t carry[4] = { 0, 0, 0, 0 };
	for (int32_t base = 0; base < n_query; base += FORMAT_SCAN) {
		const int32_t q = base + t;
		const bool have = q < n_query;
		const FmtCounts c = have ? cnt[q] : FmtCounts{ 0, 0, 0, 0 };
		const int64_t v[4] = { c.bytes, c.ids, c.n_out, c.bad };
		int64_t e[4];
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			int64_t total;
			e[k] = CoopWave::scan_excl(v[k], &total);
			if ((t & 63) == 0) s_tot[wave][k] = total;
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			int64_t below = 0, all = 0;
#pragma unroll
			for (int w = 0; w < FORMAT_SCAN / 64; ++w) { const int64_t s = s_tot[w][k]; below += w < wave ? s : 0, all += s; }
			e[k] += carry[k] + below, carry[k] += all;
		}
		if (have) off[q] = FmtCounts{ e[0], e[1], e[2], e[3] };
		__syncthreads();
	}
	if (t == 0) off[n_query] = *head = FmtCounts{ carry[0], carry[1], carry[2], carry[3] };
}

__global__ __launch_bounds__(64 * FORMAT_WRITE_WAVES) void k_format_write(FmtOpt o, FmtSrc S, int32_t n_query, const FmtAt *at, const FmtCounts *off, char *text, int64_t text_cap,
                                                                          int64_t *id_at, int64_t id_cap)
{
	MPA_SHORT_KERNEL();
	const int32_t q = (int32_t)blockIdx.x;
	if (q >= n_query) return;
	const FmtCounts tot = off[n_query];
	if (tot.bad != 0 || tot.bytes > text_cap || tot.ids > id_cap) return;   // (the host reads the same totals and formats the batch itself)
	const FmtCounts mine = off[q];
	const int64_t h0 = fmt_base(S, q), n_reg = fmt_n_reg(S, q);
	const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
	for (int64_t j = wave; j < n_reg; j += FORMAT_WRITE_WAVES) {
		const FmtAt a = at[h0 + j];
		if (a.rank >= 0) format_write_core<FormatWave>(o, S, q, j, a, mine, text, id_at);
	}
	if (wave == 0 && off[q + 1].n_out == mine.n_out && (o.flag & MPA_MF_SHOW_UNMAP)) format_unmap_core<FormatWave>(o, S, q, mine, text);
}

} // namespace mpa
