"""Hand-made results and options for the tests of MPA_GPU_FORMAT (miniprot_amd/csrc/format_core.h), seeded: flat
results as mpa_dbg_result_make takes them, name-only indexes (mpa_dbg_idx_names) and the map options that decide what is printed.

A table is a dict: name, ctg (names, lengths), qnames, qlens, opt (flag, out_n, out_sim, out_cov, delim, prefix) and the flat arrays
hit_off, hits, cigars, feats, cs, cs_text, rows, rows_text.  Every aligned hit carries what the table's options print (a cs body unless
--no-cs, rows with --aln / --trans), so that no formatter has to read a genome; what is absent is absent because the options do not
print it or because the hit has no alignment.  The expected text is always mpa_format_output()'s, the host formatter's."""
import functools
import numpy as np
import miniprot_amd as mpa
from finishcases import HIT, CS_REF, ROWS_REF

FEAT = np.dtype([("vs", "<i8"), ("ve", "<i8"), ("qs", "<i4"), ("qe", "<i4"), ("type", "<i2"), ("phase", "<i2"), ("n_fs", "<i4"), ("n_stop", "<i4"), ("score", "<i4"),
                 ("n_iden", "<i4"), ("blen", "<i4"), ("donor", "S2"), ("acceptor", "S2"), ("pad", "<i4")])
assert FEAT.itemsize == 56

UNMAP, GFF, NO_PAF, GTF, ALN, TRANS, NO_CS = 0x4, 0x8, 0x10, 0x20, 0x80, 0x100, 0x200
# the output flags of golden.SYNTH_CASES, plus the delimiter form of the GFF3 id and a custom prefix
FLAGSETS = [("paf", dict(flag=0)), ("paf_u", dict(flag=UNMAP)), ("gff_u", dict(flag=UNMAP | GFF)), ("gtf", dict(flag=GTF)),
            ("gffonly_delim_nocs", dict(flag=GFF | NO_PAF | NO_CS, delim=ord("#"))), ("aln_u", dict(flag=UNMAP | ALN)), ("trans_gff", dict(flag=TRANS | GFF)),
            ("aln_trans_gtf", dict(flag=ALN | TRANS | GTF)), ("gff_delim", dict(flag=GFF, delim=ord("|"))), ("gff_prefix", dict(flag=GFF | UNMAP, prefix=b"Prot_x.")),
            ("gtf_prefix64", dict(flag=GTF, prefix=b"p" * 64))]
DEFAULT_OPT = dict(flag=0, out_n=1000, out_sim=0.99, out_cov=0.1, delim=-1, prefix=None)
CTG = (["chr1", "c2_with_a_longer_name", "big"], [5000000, 1234567, (1 << 31) + 123456789])   # the last one: positions past 2^31
CS_ALPHABET = np.frombuffer(b":*+-~acgtnACDEFGHIKLMNPQRSTVWY0123456789", np.uint8)
ROW_ALPHABET = np.frombuffer(b"ACGTacgt~-.|+ 0123456789*XARNDCQEGHILKMFPSTWYV!$", np.uint8)


def hit(qs, qe, dp_max, vid=0, vs=1000, ve=2000, has_aln=1, n_cigar=3, cig_digits=None, feats=None, n_feat=None, cs_len=12, width=30, n_sta=10, **kw):
    """a hit as a dict: record fields, and what hangs off it -- n_cigar words (cig_digits: the digits of every length, default mixed), its
    features (a list of feat() dicts, or n_feat generated ones), the length of its cs body, the width of its rows and its STA bytes"""
    d = dict(qs=qs, qe=qe, dp_max=dp_max, vid=vid, vs=vs, ve=ve, has_aln=has_aln, chn_sc=max(dp_max // 2, 1), chn_sc_ungap=max(dp_max // 3, 1), cnt=5, n_exon=2, dp_score=dp_max,
             blen=3 * (qe - qs) + 9, n_iden=qe - qs - 1, n_plus=qe - qs, n_fs=0, n_stop=0, dist_stop=-1, dist_start=3)
    d.update(kw)
    d["_"] = dict(n_cigar=n_cigar, cig_digits=cig_digits, feats=feats, n_feat=2 if feats is None and n_feat is None else n_feat, cs_len=cs_len, width=width, n_sta=n_sta)
    return d


def feat(vs, ve, qs, qe, type=0, phase=0, score=50, n_iden=10, blen=33, n_fs=0, n_stop=0, donor=b"GT", acceptor=b"AG"):
    return dict(vs=vs, ve=ve, qs=qs, qe=qe, type=type, phase=phase, score=score, n_iden=n_iden, blen=blen, n_fs=n_fs, n_stop=n_stop, donor=donor, acceptor=acceptor)


def gen_feats(rng, h, n):
    """n features along the hit: CDS with every kind of attribute, a stop_codon at the end of every third hit's list"""
    out = []
    span = max((h["ve"] - h["vs"]) // max(n, 1), 3)
    for j in range(n):
        vs = h["vs"] + j * span
        ve = h["ve"] if j == n - 1 else vs + span - 1
        out.append(feat(vs, ve, h["qs"] + j, h["qs"] + j + 1 + int(rng.integers(0, 50)), phase=int(rng.integers(0, 3)), score=int(rng.integers(-20, 5000)),
                        n_iden=int(rng.integers(0, 400)), blen=int(rng.integers(1, 1300)), n_fs=int(rng.integers(0, 3)) * int(rng.random() < 0.3),
                        n_stop=int(rng.integers(0, 3)) * int(rng.random() < 0.3), donor=[b"GT", b"GC", b"AT", b"\0\0", b"G\0"][int(rng.integers(0, 5))],
                        acceptor=[b"AG", b"AC", b"TG", b"\0\0", b"A\0"][int(rng.integers(0, 5))]))
    if n >= 2 and rng.random() < 0.5:                     # the stop codon's feature behind the last CDS (which then ends three bases early)
        out[-1].update(type=1, vs=out[-1]["ve"] - 3, phase=0)
        out[-2]["ve"] = h["ve"]
    return out


def build(name, queries, opt=None, rng=None, ctg=CTG, qlens=None):
    """queries: a list of lists of hit() dicts.  Query i is called q<i> (every seventh has a long name) and has qlens[i] residues
    (default: its largest qe, so that a hit can end at the query's end)"""
    rng = rng or np.random.default_rng(7)
    o = dict(DEFAULT_OPT)
    o.update(opt or {})
    flag = o["flag"]
    residues = bool(flag & (ALN | TRANS))
    paf = residues if flag & GTF else not flag & NO_PAF
    want_cs, want_rows = paf and not flag & NO_CS, residues
    n = sum(len(q) for q in queries)
    hits = np.zeros(n, HIT)
    cs, rows = np.zeros(n, CS_REF), np.zeros(n, ROWS_REF)
    hit_off = np.zeros(len(queries) + 1, np.int64)
    # (slack in front of every array: offsets that are not zero-based catch an emitter that forgets them)
    words, feats, cs_parts, rows_parts = [np.array([0x11, 0x22, 0x33], np.uint32)], [np.zeros(1, FEAT)], [b"#" * 5], [b"%" * 7]
    n_words, n_feats, n_cs, n_rows = 3, 1, 5, 7
    k = 0
    for qi, q in enumerate(queries):
        for h in q:
            x = h["_"]
            for f, v in h.items():
                if f != "_":
                    hits[k][f] = v
            hits[k]["qid"], hits[k]["id"], hits[k]["parent"] = qi, k - hit_off[qi], 0
            if h["has_aln"]:
                nc = x["n_cigar"]
                dg = x["cig_digits"] if x["cig_digits"] is not None else rng.integers(1, 9, nc)
                lens = np.array([int(rng.integers(10 ** (d - 1), min(10 ** d, 1 << 28))) for d in np.broadcast_to(dg, nc)], np.uint32)
                words.append(lens << 4 | rng.integers(0, 15, nc).astype(np.uint32))
                hits[k]["n_cigar"], hits[k]["cigar_off"] = nc, n_words
                n_words += nc
                fl = x["feats"] if x["feats"] is not None else gen_feats(rng, h, x["n_feat"])
                fa = np.zeros(len(fl), FEAT)
                for j, fd in enumerate(fl):
                    for f, v in fd.items():
                        fa[j][f] = v
                fa["pad"] = 0
                feats.append(fa)
                hits[k]["n_feat"], hits[k]["feat_off"] = len(fl), n_feats
                n_feats += len(fl)
                if want_cs:
                    body = CS_ALPHABET[rng.integers(0, len(CS_ALPHABET), x["cs_len"])].tobytes()
                    cs[k] = (n_cs, len(body), 1)
                    cs_parts.append(body)
                    n_cs += len(body)
                if want_rows:
                    w, ns = x["width"], x["n_sta"]
                    body = ROW_ALPHABET[rng.integers(0, len(ROW_ALPHABET), 4 * w + ns)].tobytes()
                    rows[k] = (n_rows, w, ns, 1, 0)
                    rows_parts.append(body)
                    n_rows += len(body)
            k += 1
        hit_off[qi + 1] = k
    if qlens is None:
        qlens = [max([h["qe"] for h in q] + [5]) for q in queries]
    qnames = ["q%d" % i if i % 7 != 3 else "sp|Q%05d|A_LONGER_NAME_%d" % (i, i) for i in range(len(queries))]
    return dict(name=name, ctg=ctg, qnames=qnames, qlens=list(qlens), opt=o, hit_off=hit_off, hits=hits, cigars=np.concatenate(words), feats=np.concatenate(feats),
                cs=cs if want_cs else None, cs_text=b"".join(cs_parts) if want_cs else b"", rows=rows if want_rows else None, rows_text=b"".join(rows_parts) if want_rows else b"")


def random_queries(rng, n_query, max_hits=4, big=True):
    out = []
    for _ in range(n_query):
        q = []
        qlen = int(rng.integers(30, 3000))
        for j in range(int(rng.integers(0, max_hits + 1))):
            qs = int(rng.integers(0, qlen - 20))
            qe = int(rng.integers(qs + 10, qlen + 1)) if rng.random() < 0.7 else qlen
            c = int(rng.integers(0, 3 if big else 2))
            clen = CTG[1][c]
            vs = int(rng.integers(0, clen - 40000))
            ve = vs + int(rng.integers(30, 30000))
            q.append(hit(qs, qe, int(rng.integers(-50, 3000)) if j else int(rng.integers(100, 3000)), vid=2 * c + int(rng.integers(0, 2)), vs=vs, ve=ve,
                         has_aln=int(rng.random() < 0.85), n_cigar=int(rng.integers(1, 12)), n_feat=int(rng.integers(0, 6)), cs_len=int(rng.integers(1, 80)),
                         width=int(rng.integers(1, 200)), n_sta=int(rng.integers(0, 70)), n_fs=int(rng.integers(0, 3)), n_stop=int(rng.integers(0, 2)),
                         dist_stop=int(rng.integers(-1, 2)), dist_start=int(rng.integers(-1, 100)), chn_sc=int(rng.integers(-5, 900))))
        q.sort(key=lambda h: -(h["dp_max"] if h["has_aln"] else h["chn_sc"]))
        out.append(q)
    return out


def _digits(d, neg=False):
    v = min(10 ** d - 1, 2 ** 31 - 1) if d else 0
    return -v if neg else v


@functools.lru_cache(maxsize=None)
def tables():
    rng = np.random.default_rng(20240614)
    T = []
    for name, o in FLAGSETS:                              # every flag combination on the same mixed batch
        T.append(build("mixed_" + name, random_queries(np.random.default_rng(11), 14), o, rng))
    # integers of 1 .. 10 digits in every field that prints one, negative scores, both strands, the contig past 2^31
    q = []
    for d in range(1, 11):
        big = _digits(d)
        q.append([hit(min(big, 10 ** 6), min(big, 10 ** 6) + 7, max(big, 1), vid=4 + (d & 1), vs=_digits(d) * (10 if d > 9 else 1), ve=CTG[1][2] - d, dp_score=_digits(d, d & 1),
                      n_iden=big // 3, blen=max(big, 1), n_plus=big, n_fs=big, n_stop=big, dist_start=_digits(d, True), dist_stop=_digits(d, d & 1), n_feat=3),
                  hit(0, 5, 1, vid=d & 1, vs=d, ve=10 ** min(d, 6), has_aln=0, chn_sc=max(big, 1), chn_sc_ungap=_digits(d, True), cnt=big)])
    for name, o in (("paf", dict(flag=UNMAP, out_sim=0.0, out_cov=0.0)), ("gff", dict(flag=GFF, out_sim=0.0, out_cov=0.0)), ("gtf", dict(flag=GTF, out_sim=0.0, out_cov=0.0))):
        T.append(build("integers_" + name, q, o, rng))
    # the filters: hits exactly on, one below and one above each threshold; out_n of 0, 1 and beyond the hits; with and without -u
    for sim in (0.0, 0.5, 0.97, 0.99, 1.0):
        for cov in (0.0, 0.1, 1.0):
            q = []
            for best in (100, 200, 1000, 33):
                t = int(best * sim)
                qlen = 200
                c = int(qlen * cov)
                hs = [hit(0, qlen, best)] + [hit(10, 10 + max(c + dc, 1) if c + dc <= qlen - 10 else qlen, max(t + ds, -3), has_aln=(ds + dc) & 1, chn_sc=max(t + ds, -3))
                                             for ds in (-1, 0, 1) for dc in (-1, 0, 1)]
                hs += [hit(0, qlen - 1, best - 1), hit(1, qlen, best), hit(0, 20, 0), hit(0, max(c, 1), -7, has_aln=0, chn_sc=t)]
                q.append(hs)
            q.append([])                                  # no hit at all
            q.append([hit(0, 3, 5, has_aln=0, chn_sc=-2)])   # hits, none printed
            for out_n, fl in ((1000, UNMAP | GFF), (1, GTF), (0, UNMAP)) if (sim, cov) in ((0.99, 0.1), (0.5, 1.0)) else ((1000, UNMAP | GFF),):
                T.append(build("filter_s%g_c%g_n%d" % (sim, cov, out_n), q, dict(flag=fl, out_n=out_n, out_sim=sim, out_cov=cov), rng, qlens=[200] * len(q)))
    T.append(build("unmapped_silent", [[], [hit(0, 3, -1)], []], dict(flag=GFF), rng))
    # CIGARs of 1, 63, 64, 65 and 1 000 words with lengths of 1 .. 9 digits
    q = [[hit(0, 50, 100, n_cigar=n, cig_digits=None if n > 9 else d) for d in ((1, 5, 9) if n < 1000 else (None,))] for n in (1, 63, 64, 65, 1000)]
    q.append([hit(0, 50, 100, n_cigar=9, cig_digits=np.arange(1, 10))])
    T.append(build("cigars", q, dict(flag=0, out_sim=0.0), rng))
    # 0, 1, 64 and 65 features; has_stop on and off (qe == qlen and dist_stop == 0), both strands
    q = [[hit(0, 90, 500, vid=v, vs=7000, ve=90000, n_feat=n, dist_stop=ds, n_fs=n & 1, n_stop=v)] for n in (0, 1, 2, 64, 65, 130) for v in (0, 1, 5) for ds in (0, 1)]
    for name, o in (("gff", dict(flag=GFF)), ("gtf", dict(flag=GTF)), ("delim", dict(flag=GFF | NO_PAF, delim=ord("#"))), ("prefix", dict(flag=GFF | NO_CS, prefix=b"gene:"))):
        T.append(build("feats_" + name, q, o, rng, qlens=[90 if i % 4 else 91 for i in range(len(q))]))
    # cs bodies of 1 .. 5 000 bytes, present and (--no-cs; has_aln == 0) absent
    q = [[hit(0, 50, 100, cs_len=n), hit(0, 50, 100, has_aln=0, chn_sc=100)] for n in (1, 2, 63, 64, 65, 255, 256, 5000)]
    T.append(build("cs_present", q, dict(flag=UNMAP), rng))
    T.append(build("cs_absent", q, dict(flag=UNMAP | NO_CS), rng))
    # rows of width 1, 63, 64, 65 and 4 097 with --aln, --trans and both
    q = [[hit(0, 50, 100, width=w, n_sta=s), hit(0, 50, 100, has_aln=0, chn_sc=100)] for w, s in ((1, 1), (63, 21), (64, 0), (65, 22), (4097, 1366))]
    for name, fl in (("aln", ALN), ("trans", TRANS), ("both", ALN | TRANS), ("both_gtf", ALN | TRANS | GTF), ("aln_gff", ALN | GFF)):
        T.append(build("rows_" + name, q, dict(flag=fl), rng))
    # ratios on exact ties: n * 3 / blen with a decimal expansion that ends in a 5 at the fifth place (3/96 = 0.03125, ...)
    q = []
    for blen in (32, 96, 160, 480, 800, 1600, 6400):
        ns = [n for n in range(1, blen // 3 + 1) if (n * 3 * 100000) % blen == 0 and (n * 3 * 100000 // blen) % 10 == 5][:12]
        assert ns, blen
        q.append([hit(0, 50, 100, n_iden=n, n_plus=ns[-1 - i], blen=blen, feats=[feat(1000, 2000, 0, 50, n_iden=n, blen=blen), feat(2100, 2200, 0, 50, n_iden=0, blen=1),
                                                                                     feat(2300, 2400, 0, 50, n_iden=blen // 3, blen=blen)]) for i, n in enumerate(ns)])
    T.append(build("ratio_ties", q, dict(flag=GFF | NO_PAF, out_sim=0.0), rng))
    # 257 and 3 000 queries: the scan's carry; ids across many queries
    T.append(build("queries_257", random_queries(np.random.default_rng(12), 257, 2), dict(flag=GFF | UNMAP), rng))
    T.append(build("queries_3000", random_queries(np.random.default_rng(13), 3000, 2, big=False), dict(flag=GTF | ALN), rng))
    T.append(build("queries_1", [[hit(0, 50, 100)]], dict(flag=GFF), rng))
    names = [t["name"] for t in T]
    assert len(set(names)) == len(names)
    return T


def objects(t):
    """(Index, MapOpt, Queries, Result) of a table; close the index and the result when done"""
    idx = mpa.dbg_idx_names(t["ctg"][0], t["ctg"][1])
    mo = mpa.default_mapopt()
    o = t["opt"]
    mo.flag, mo.out_n, mo.out_sim, mo.out_cov, mo.gff_delim = o["flag"], o["out_n"], o["out_sim"], o["out_cov"], o["delim"]
    if o["prefix"] is not None:
        mo.gff_prefix = o["prefix"]
    q = mpa.Queries(["A" * n for n in t["qlens"]], t["qnames"])
    res = mpa.dbg_result_make(t["hit_off"], t["hits"], t["cigars"], t["feats"].view(np.uint8), t["cs"], t["cs_text"], t["rows"], t["rows_text"])
    return idx, mo, q, res


ID0S = (0, 7, 999990)


def n_printed_expected(t):
    """the printed hits of a table by the filters' plain restatement (numpy fp64, the expressions of map.c:298-306)"""
    o, hits, off = t["opt"], t["hits"], t["hit_off"]
    sim, cov = np.float64(np.float32(o["out_sim"])), np.float64(np.float32(o["out_cov"]))
    n = 0
    for i in range(len(off) - 1):
        h = hits[off[i]:off[i + 1]]
        if not len(h):
            continue
        sc = np.where(h["has_aln"] != 0, h["dp_max"], h["chn_sc"]).astype(np.float64)
        keep = (sc > 0) & ~(sc < sc[0] * sim) & ~((h["qe"] - h["qs"]).astype(np.float64) < np.float64(t["qlens"][i]) * cov)
        keep[o["out_n"]:] = False
        n += int(keep.sum())
    return n
