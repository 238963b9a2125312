"""Hand-made tables for the tests of MPA_GPU_FINISH (miniprot_amd/csrc/finish_core.h), seeded: the aligned
regions of a batch as mpa_dbg_finish takes them, the reference's own ranking of them through tests/finish_ref_shim.c, and a plain
restatement of the layout stage in numpy.

A table is a dict: name, first (int64, n_query + 1), recs (REC records), words (uint32), feats (uint8, 56 bytes each), cs_text,
rows_text (bytes) and opt (mask_level, mask_len, pri_ratio, best_n, io, kmer).  Every record's dp_score is its number in the table, so
that a hit of the result names the record it came from."""
import ctypes as C
import functools
import os
import subprocess
import numpy as np
import miniprot_amd as mpa
import refbind

REC = np.dtype([("vs", "<i8"), ("ve", "<i8"), ("cig_off", "<i8"), ("feat_off", "<i8"), ("cs_off", "<i8"), ("rows_off", "<i8"), ("vid", "<u4"), ("hash", "<u4"),
                ("qs", "<i4"), ("qe", "<i4"), ("cnt", "<i4"), ("n_exon", "<i4"), ("chn_sc", "<i4"), ("chn_sc_ungap", "<i4"), ("parent", "<i4"), ("n_sub", "<i4"),
                ("subsc", "<i4"), ("dp_max2", "<i4"), ("dp_score", "<i4"), ("dp_max", "<i4"), ("blen", "<i4"), ("n_fs", "<i4"), ("n_stop", "<i4"), ("dist_stop", "<i4"),
                ("dist_start", "<i4"), ("n_iden", "<i4"), ("n_plus", "<i4"), ("n_cigar", "<i4"), ("n_feat", "<i4"), ("cs_len", "<i4"), ("rows_w", "<i4"),
                ("rows_sta", "<i4"), ("rows_stride", "<i4"), ("job", "<i4")])
HIT = np.dtype([("qid", "<i4"), ("id", "<i4"), ("parent", "<i4"), ("n_sub", "<i4"), ("subsc", "<i4"), ("cnt", "<i4"), ("n_exon", "<i4"), ("chn_sc", "<i4"),
                ("chn_sc_ungap", "<i4"), ("vid", "<u4"), ("qs", "<i4"), ("qe", "<i4"), ("vs", "<i8"), ("ve", "<i8"), ("has_aln", "<i4"), ("dp_score", "<i4"),
                ("dp_max", "<i4"), ("dp_max2", "<i4"), ("blen", "<i4"), ("n_fs", "<i4"), ("n_stop", "<i4"), ("dist_stop", "<i4"), ("dist_start", "<i4"), ("n_iden", "<i4"),
                ("n_plus", "<i4"), ("n_cigar", "<i4"), ("n_feat", "<i4"), ("pad", "<i4"), ("cigar_off", "<i8"), ("feat_off", "<i8")])
CS_REF = np.dtype([("off", "<i8"), ("len", "<i4"), ("present", "<i4")])
ROWS_REF = np.dtype([("off", "<i8"), ("width", "<i4"), ("n_sta", "<i4"), ("present", "<i4"), ("pad", "<i4")])
assert REC.itemsize == 160 and HIT.itemsize == 136 and CS_REF.itemsize == 16 and ROWS_REF.itemsize == 24

DEFAULT_OPT = dict(mask_level=0.5, mask_len=2147483647, pri_ratio=0.7, best_n=30, io=29, kmer=6)


def reg(qs, qe, dp_max, vid=0, vs=None, ve=None, n_exon=2, cnt=5, hash=None, chn_sc=None, **kw):
    """one region as a dict of record fields; vs / ve default to a place of its own that follows the query span"""
    d = dict(qs=qs, qe=qe, dp_max=dp_max, vid=vid, vs=3 * qs + 1000 if vs is None else vs, ve=3 * qe + 1000 if ve is None else ve, n_exon=n_exon, cnt=cnt,
             hash=hash, chn_sc=dp_max // 2 if chn_sc is None else chn_sc)
    d.update(kw)
    return d


def random_query(rng, n, span=300, scores=None, ties=False):
    """n regions with overlapping query spans and few distinct scores, so that parents, secondaries and ties all occur"""
    out = []
    for _ in range(n):
        qs = int(rng.integers(0, span - 10))
        qe = qs + int(rng.integers(5, min(120, span - qs) + 1))
        sc = int(rng.choice(scores)) if scores is not None else int(rng.integers(20, 400))
        r = reg(qs, qe, sc, vid=int(rng.integers(0, 4)), n_exon=int(rng.integers(1, 4)), cnt=int(rng.integers(1, 9)), chn_sc=int(rng.integers(10, 300)),
                n_sub=int(rng.integers(0, 3)), subsc=int(rng.integers(0, 50)), parent=int(rng.integers(0, 5)), dp_max2=int(rng.integers(0, 30)))
        if ties and rng.random() < 0.5:
            r["hash"] = 7
        if out and rng.random() < 0.15:                   # the same place as an earlier region, with its span or a shifted one
            o = out[int(rng.integers(0, len(out)))]
            r.update(vid=o["vid"], vs=o["vs"], ve=o["ve"])
            if rng.random() < 0.6:
                r.update(qs=o["qs"], qe=o["qe"])
        out.append(r)
    return out


# what hangs off a region: CIGAR words, features, a cs body, a rows slot -- the lengths the gather's loops distinguish
CIGAR_LENGTHS = (1, 63, 64, 65, 1000)
CS_LENGTHS = (1, 255, 256, 5000)


def build(name, queries, opt=None, rng=None, payload="small", cs="all", rows="all"):
    """queries: a list of lists of reg() dicts.  payload: "small" (1-3 words, 1-2 features, short text) or "edges" (the lengths above in
    turn).  cs / rows: "all", "none" or "mixed" regions carry a cs body / a rows slot."""
    rng = rng or np.random.default_rng(1)
    o = dict(DEFAULT_OPT)
    o.update(opt or {})
    n = sum(len(q) for q in queries)
    recs = np.zeros(n, REC)
    first = np.zeros(len(queries) + 1, np.int64)
    words, feats, cs_parts, rows_parts = [], [], [], []
    # (slack in front of every array: offsets that are not zero-based catch a gather that forgets them)
    n_words, n_feats, n_cs, n_rows = 3, 1, 5, 7
    words.append(rng.integers(0, 2 ** 32, 3, dtype=np.uint64).astype(np.uint32))
    feats.append(rng.integers(0, 256, 56, dtype=np.uint8))
    cs_parts.append(b"#" * 5)
    rows_parts.append(b"%" * 7)
    i = 0
    for qi, q in enumerate(queries):
        first[qi] = i
        for r in q:
            x = recs[i]
            for k, v in r.items():
                if v is not None:
                    x[k] = v
            x["hash"] = r["hash"] if r.get("hash") is not None else int(rng.integers(0, 2 ** 32))
            x["dp_score"] = i
            x["chn_sc_ungap"] = int(rng.integers(0, 500))
            for k in ("blen", "n_fs", "n_stop", "dist_stop", "dist_start", "n_iden", "n_plus"):
                x[k] = int(rng.integers(-1, 1000))
            if payload == "edges":
                nc, nf = CIGAR_LENGTHS[i % 5], 1 + (7 * i) % 40
                ncs, w, sta = CS_LENGTHS[i % 4], (0, 1, 63, 64, 65, 300)[i % 6], (0, 5, 70)[i % 3]
            else:
                nc, nf = int(rng.integers(1, 4)), int(rng.integers(1, 3))
                ncs, w, sta = int(rng.integers(0, 12)), int(rng.integers(0, 9)), int(rng.integers(0, 4))
            x["n_cigar"], x["cig_off"] = nc, n_words
            words.append(rng.integers(0, 2 ** 32, nc, dtype=np.uint64).astype(np.uint32))
            n_words += nc
            x["n_feat"], x["feat_off"] = nf, n_feats
            feats.append(rng.integers(0, 256, 56 * nf, dtype=np.uint8))      # (the padding word too: the gather has to zero it)
            n_feats += nf
            x["cs_len"], x["rows_stride"] = -1, -1
            if cs == "all" or (cs == "mixed" and rng.random() < 0.5):
                x["cs_len"], x["cs_off"] = ncs, n_cs
                cs_parts.append(rng.integers(33, 127, ncs, dtype=np.uint8).tobytes() + b"!")     # (a byte of slack behind every body)
                n_cs += ncs + 1
            if rows == "all" or (rows == "mixed" and rng.random() < 0.5):
                stride = w + int(rng.integers(0, 4))
                x["rows_w"], x["rows_sta"], x["rows_stride"], x["rows_off"] = w, sta, stride, n_rows
                rows_parts.append(rng.integers(33, 127, 4 * stride + sta, dtype=np.uint8).tobytes())
                n_rows += 4 * stride + sta
            i += 1
    first[len(queries)] = i
    return dict(name=name, first=first, recs=recs, words=np.concatenate(words), feats=np.concatenate(feats), cs_text=b"".join(cs_parts), rows_text=b"".join(rows_parts), opt=o)


@functools.lru_cache(maxsize=1)
def tables():
    rng = np.random.default_rng(20240613)
    T = []
    # sizes: 64 / 65 is the radix sort's insertion threshold and the device's LDS capacity, 257 and up takes several digit passes
    T.append(build("sizes", [random_query(rng, n) for n in (0, 1, 2, 3, 63, 64, 65, 257, 300)], rng=rng))
    T.append(build("one_query", [random_query(rng, 9)], rng=rng))
    # sort keys
    keys = [[reg(10 * i, 10 * i + 8, 50) for i in range(70)],                                   # all dp_max equal, distinct hashes
            [reg(int(rng.integers(0, 280)), 300, 50) for _ in range(300)],
            [reg(5 * i, 5 * i + 4, 77, hash=9) for i in range(5)],                              # equal full keys
            [reg(4 * i, 4 * i + 30, 77, hash=9) for i in range(66)],
            [reg(int(rng.integers(0, 200)), 290, 31, hash=3) for _ in range(260)],
            [reg(20 * i, 20 * i + 30, int(v)) for i, v in enumerate((-5, 12, -200, 0, 7, -1, -5, 300, -10 ** 9, 10 ** 9))],   # negative dp_max (no difference of two overflows an int)
            random_query(rng, 130, scores=(40, 41, 42), ties=True), random_query(rng, 280, scores=(-3, 0, 3), ties=True)]
    T.append(build("keys", keys, rng=rng))
    # the multi-exon swap: a single-exon top hit and the first multi-exon hit at dp_max + io equal to, one below and one above the top
    io = DEFAULT_OPT["io"]
    T.append(build("multi_exon", [[reg(0, 50, 100, n_exon=1), reg(60, 90, 90, n_exon=1), reg(100, 150, 100 - io + d, n_exon=2), reg(160, 200, 100 - io + d + 1, n_exon=3)]
                                  for d in (0, -1, 1)] + [[reg(0, 50, 100, n_exon=1), reg(10, 60, 99, n_exon=2)]], rng=rng))
    # parents: a region secondary to the second of two overlapping primaries; uncovered at mask_len and one above; the identical hit after DP
    par = [[reg(0, 100, 500), reg(60, 160, 400), reg(70, 150, 300), reg(65, 155, 299), reg(0, 160, 200)],
           [reg(300, 500, 500), reg(310, 510, 300)], [reg(300, 500, 500), reg(310, 511, 300)],
           [reg(0, 100, 500, vs=1000, ve=1300), reg(0, 100, 400, vs=1000, ve=1300), reg(10, 100, 399, vs=1000, ve=1300), reg(0, 100, 398, vs=1000, ve=1300, vid=1),
            reg(0, 100, 300, vs=1003, ve=1300)]]
    T.append(build("parents", par, opt=dict(mask_len=10), rng=rng))
    # selection
    sel = [[reg(0, 100, 1000, cnt=9), reg(0, 99, 994), reg(1, 100, 993), reg(2, 100, 500), reg(3, 100, 299), reg(4, 100, 300)],      # gaps at sub_diff and one above; pri_ratio's edge
           [reg(0, 100, 17), reg(0, 99, 5), reg(1, 100, 4), reg(2, 100, 6)],                                                       # min_diff's edge
           [reg(0, 100, 100)] + [reg(i, 100, 90 - i) for i in range(1, 6)],
           [reg(0, 100, 100, vs=50, ve=350), reg(0, 100, 90, vs=50, ve=350), reg(0, 100, 80)],                                      # two regions at one place
           [reg(0, 100, 100), reg(0, 100, 999, cnt=0), reg(5, 100, 90), reg(200, 250, 10, cnt=-1)],                                 # soft-deleted entries
           [reg(0, 10, 5, cnt=0)]]                                                                                                  # (alone, it stays: mp_sort_reg returns early)
    for best_n in (0, 1, 2, 30):
        T.append(build("select_n%d" % best_n, sel, opt=dict(pri_ratio=0.3, best_n=best_n), rng=rng))
    T.append(build("select_off", sel + [random_query(rng, 40)], opt=dict(pri_ratio=0.0), rng=rng))
    # gather lengths, rows and cs present, absent and mixed
    T.append(build("gather_edges", [[reg(40 * i, 40 * i + 30, 100 + i) for i in range(12)], random_query(rng, 20)], rng=rng, payload="edges"))
    T.append(build("gather_none", [random_query(rng, 6), random_query(rng, 3)], rng=rng, payload="edges", cs="none", rows="none"))
    T.append(build("gather_mixed", [random_query(rng, 30) for _ in range(4)], rng=rng, payload="edges", cs="mixed", rows="mixed"))
    # batch shapes
    T.append(build("q257", [random_query(rng, int(rng.integers(0, 6))) for _ in range(257)], rng=rng, cs="mixed"))
    many = [random_query(rng, int(rng.integers(0, 4))) for _ in range(3000)]
    for q in (0, 1, 2, 255, 256, 257, 1500, 1501, 2998, 2999):         # no kept hit at the front, around a scan step's edge, in the middle and at the end
        many[q] = []
    T.append(build("q3000", many, rng=rng, rows="none"))
    # random options over random queries
    for k in range(6):
        opt = dict(mask_level=float(rng.choice((0.1, 0.5, 0.9))), mask_len=int(rng.choice((0, 20, 2147483647))), pri_ratio=float(rng.choice((0.0, 0.3, 0.7, 1.0))),
                   best_n=int(rng.choice((0, 1, 3, 30))), io=int(rng.choice((0, 29))), kmer=int(rng.choice((5, 6))))
        T.append(build("fuzz%d" % k, [random_query(rng, int(rng.integers(0, 40)), scores=(50, 55, 56, 62, 100) if k % 2 else None, ties=bool(k % 3 == 0)) for _ in range(25)],
                       opt=opt, rng=rng, cs="mixed", rows="mixed"))
    return T


def mapopt(t):
    mo = mpa.default_mapopt()
    o = t["opt"]
    mo.mask_level, mo.mask_len, mo.pri_ratio, mo.best_n, mo.io = o["mask_level"], o["mask_len"], o["pri_ratio"], o["best_n"], o["io"]
    return mo


def run(ctx, t):
    """the table through mpa_dbg_finish on a context (None: the shared core on the host): the flat arrays as a dict of bytes"""
    return mpa.dbg_finish(ctx, mapopt(t), t["opt"]["kmer"], t["first"], t["recs"].view(np.uint8), t["words"], t["feats"], t["cs_text"], t["rows_text"])


# ---- the reference's ranking
HERE = os.path.dirname(os.path.abspath(__file__))
_shim = None


def shim(build_dir):
    """tests/finish_ref_shim.c compiled against include/miniprot.h and the reference library (oracle/_ref/)"""
    global _shim
    if _shim is None:
        so = os.path.join(str(build_dir), "finish_ref_shim.so")
        ref_dir = os.path.dirname(refbind.REF_SO)
        subprocess.run(["gcc", "-O1", "-g", "-shared", "-fPIC", "-I" + os.path.join(os.path.dirname(HERE), "include"), os.path.join(HERE, "finish_ref_shim.c"), "-o", so,
                        "-L" + ref_dir, "-lminiprot_ref", "-Wl,-rpath," + ref_dir], check=True)
        refbind.ref()
        _shim = C.CDLL(so)
        _shim.finish_ref.restype = C.c_int
        _shim.finish_ref.argtypes = [C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p]
        _shim.finish_ref_accepts.restype = C.c_int
        _shim.finish_ref_accepts.argtypes = [C.c_int, C.c_void_p]
    return _shim


IN_FIELDS = ("vs", "ve", "vid", "hash", "qs", "qe", "cnt", "n_exon", "chn_sc", "chn_sc_ungap", "parent", "n_sub", "subsc", "dp_max2", "dp_max")


def reference_ranks(t, build_dir):
    """per query an int64 array [kept, 6]: record number in the query, id, parent, n_sub, subsc, dp_max2 -- by the reference itself.
    Raises when the reference does not accept a query's table."""
    S = shim(build_dir)
    o = t["opt"]
    out = []
    for q in range(len(t["first"]) - 1):
        r = t["recs"][t["first"][q]:t["first"][q + 1]]
        n = len(r)
        a = np.zeros((n, 16), np.int64)
        for k, f in enumerate(IN_FIELDS):
            a[:, k] = r[f]
        res = np.zeros((n + 1, 8), np.int64)
        assert S.finish_ref_accepts(n, a.ctypes.data), "%s: the reference does not accept query %d" % (t["name"], q)
        k = S.finish_ref(n, a.ctypes.data, o["mask_level"], o["mask_len"], o["kmer"], o["pri_ratio"], o["best_n"], o["io"], res.ctypes.data)
        assert 0 <= k <= n
        out.append(res[:k, :6].copy())
    return out


# ---- the layout stage, restated: what mpa_batch_finish() would lay out for those ranks
def expected_flat(t, ranks):
    recs, first = t["recs"], t["first"]
    n_hit = sum(len(r) for r in ranks)
    hits = np.zeros(n_hit, HIT)
    hit_off = np.zeros(len(ranks) + 1, np.int64)
    cs, rows = np.zeros(n_hit, CS_REF), np.zeros(n_hit, ROWS_REF)
    cig, feat, cs_text, rows_text = [], [], [], []
    n_cig = n_feat = n_cs = n_rows = 0
    feats_in = t["feats"].reshape(-1, 56)
    h = 0
    for q, rk in enumerate(ranks):
        hit_off[q] = h
        for src, id_, parent, n_sub, subsc, dp_max2 in rk:
            x = recs[first[q] + src]
            y = hits[h]
            for f in ("cnt", "n_exon", "chn_sc", "chn_sc_ungap", "vid", "qs", "qe", "vs", "ve", "dp_score", "dp_max", "blen", "n_fs", "n_stop", "dist_stop", "dist_start", "n_iden",
                      "n_plus", "n_cigar", "n_feat"):
                y[f] = x[f]
            y["qid"], y["id"], y["parent"], y["n_sub"], y["subsc"], y["dp_max2"], y["has_aln"], y["cigar_off"], y["feat_off"] = q, id_, parent, n_sub, subsc, dp_max2, 1, n_cig, n_feat
            cig.append(t["words"][x["cig_off"]:x["cig_off"] + x["n_cigar"]])
            n_cig += int(x["n_cigar"])
            f = feats_in[x["feat_off"]:x["feat_off"] + x["n_feat"]].copy()
            f[:, 52:] = 0
            feat.append(f.reshape(-1))
            n_feat += int(x["n_feat"])
            if x["cs_len"] >= 0:
                cs[h] = (n_cs, x["cs_len"], 1)
                cs_text.append(t["cs_text"][x["cs_off"]:x["cs_off"] + x["cs_len"]])
                n_cs += int(x["cs_len"])
            if x["rows_stride"] >= 0:
                rows[h] = (n_rows, x["rows_w"], x["rows_sta"], 1, 0)
                o, w, s = int(x["rows_off"]), int(x["rows_w"]), int(x["rows_stride"])
                body = b"".join(t["rows_text"][o + k * s:o + k * s + w] for k in range(4)) + t["rows_text"][o + 4 * s:o + 4 * s + int(x["rows_sta"])]
                rows_text.append(body)
                n_rows += len(body)
            h += 1
    hit_off[len(ranks)] = h
    any_cs, any_rows = bool(cs["present"].any()), bool(rows["present"].any())
    return dict(hits=hits.tobytes(), hit_off=hit_off.tobytes(), cigars=np.concatenate(cig + [np.zeros(0, np.uint32)]).astype(np.uint32).tobytes(),
                feats=np.concatenate(feat + [np.zeros(0, np.uint8)]).astype(np.uint8).tobytes(), cs=cs.tobytes() if any_cs else b"", cs_text=b"".join(cs_text) if any_cs else b"",
                rows=rows.tobytes() if any_rows else b"", rows_text=b"".join(rows_text) if any_rows else b"")


def first_difference(got, want):
    """None, or a sentence about the first array that differs"""
    for name in mpa.FLAT_ARRAYS:
        a, b = got[name], want[name]
        if a != b:
            k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
            return "%s differs at byte %d (%d bytes against %d)" % (name, k, len(a), len(b))
    return None
