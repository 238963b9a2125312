/* finish_ref_shim.c -- the reference's own ranking of aligned regions for the tests of MPA_GPU_FINISH: mp_sort_reg,
 * mp_select_multi_exon, mp_set_parent and mp_select_sub of the compiled reference (hit.o), called in the order of the tail of mp_map()
 * on hand-made regions.  Compiled by tests/finishref.py against include/miniprot.h (whose layouts tests/test_compat.py pins) and linked
 * against the reference library; the four prototypes are declared here because that header does not export them. */
#include <stdlib.h>
#include <string.h>
#include "miniprot.h"

void mp_sort_reg(void *km, int *n_regs, mp_reg1_t *r);
void mp_select_multi_exon(int32_t n, mp_reg1_t *r, int32_t single_penalty);
void mp_set_parent(void *km, float mask_level, int mask_len, int n, mp_reg1_t *r, int sub_diff, int hard_mask_level);
void mp_select_sub(void *km, float pri_ratio, int min_diff, int best_n, int *n_, mp_reg1_t *r);

#define FIN_IN 16  /* int64 per region in: vs, ve, vid, hash, qs, qe, cnt, n_exon, chn_sc, chn_sc_ungap, parent, n_sub, subsc, dp_max2, dp_max, spare */
#define FIN_OUT 8  /* int64 per kept region out: which input it is, id, parent, n_sub, subsc, dp_max2, two spares */

/* does the reference accept the table?  (mp_sort_reg asserts that the regions it keeps are aligned: two or more regions need one with cnt > 0) */
int finish_ref_accepts(int n, const int64_t *in)
{
	int i, live = 0;
	for (i = 0; i < n; ++i) live += in[i * FIN_IN + 6] > 0;
	return n <= 1 || live > 0;
}

/* returns how many regions are left, or -1 for a table the reference does not accept */
int finish_ref(int n, const int64_t *in, float mask_level, int mask_len, int kmer, float pri_ratio, int best_n, int io, int64_t *out)
{
	int i, k = n;
	mp_reg1_t *r;
	if (!finish_ref_accepts(n, in)) return -1;
	if (n <= 0) return 0;
	r = (mp_reg1_t*)calloc((size_t)n, sizeof(mp_reg1_t));
	for (i = 0; i < n; ++i) {
		const int64_t *x = in + (size_t)i * FIN_IN;
		mp_reg1_t *t = &r[i];
		t->vs = x[0], t->ve = x[1], t->vid = (uint32_t)x[2], t->hash = (uint32_t)x[3], t->qs = (int32_t)x[4], t->qe = (int32_t)x[5], t->cnt = (int32_t)x[6], t->n_exon = (int32_t)x[7];
		t->chn_sc = (int32_t)x[8], t->chn_sc_ungap = (int32_t)x[9], t->parent = (int32_t)x[10], t->n_sub = (int32_t)x[11], t->subsc = (int32_t)x[12];
		t->off = i;                                          /* (none of the four functions reads or writes it) */
		t->p = (mp_extra_t*)calloc(1, sizeof(mp_extra_t) + 4);   /* (mp_select_sub frees the ones it drops) */
		t->feat = (mp_feat_t*)calloc(1, sizeof(mp_feat_t));
		t->p->dp_max2 = (int32_t)x[13], t->p->dp_max = (int32_t)x[14];
	}
	mp_sort_reg(0, &k, r);
	mp_select_multi_exon(k, r, io);
	mp_set_parent(0, mask_level, mask_len, k, r, kmer, 0);
	mp_select_sub(0, pri_ratio, kmer * 2, best_n, &k, r);
	for (i = 0; i < k; ++i) {
		int64_t *o = out + (size_t)i * FIN_OUT;
		o[0] = r[i].off, o[1] = r[i].id, o[2] = r[i].parent, o[3] = r[i].n_sub, o[4] = r[i].subsc, o[5] = r[i].p ? r[i].p->dp_max2 : 0, o[6] = o[7] = 0;
		free(r[i].p), free(r[i].feat);
	}
	free(r);
	return k;
}
