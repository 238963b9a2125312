"""Task tables and the parser for the plan of a DP round (mpa_dbg_dp_plan; tests/test_dp_plan_cpu.py).  Sequence content never reaches
the planner: a table is contig lengths, query lengths, calls, scoring options and the executor's knobs."""
import json
import os
import numpy as np
import miniprot_amd as mpa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dp_plan_digests.json")

CTG_LEN = [6000, 9000, 4000]
Q_LEN = [1200, 700, 300, 1150]
KNOBS = dict(lite_min=384, lite_wide=0, no_split=0, antidiag=0, pool=0, ext_dual=1, unit_prio=1, tb_budget=8 << 30)
EXT, GLOB = "ext", "glob"


def _table(rng, spec):
    """spec: (mode, al, nl) per call; query, slice, contig, strand, window start and io are drawn"""
    t = np.zeros(len(spec), dtype=mpa.DP_TASK)
    for k, (mode, al, nl) in enumerate(spec):
        qid = int(rng.choice([q for q, l in enumerate(Q_LEN) if l >= al]))
        cid = int(rng.integers(0, len(CTG_LEN)))
        t[k] = (int(rng.integers(0, CTG_LEN[cid] - nl + 1)), 2 * cid + int(rng.integers(0, 2)), nl, qid, int(rng.integers(0, Q_LEN[qid] - al + 1)), al,
                mpa.F_CIGAR if mode == GLOB else (mpa.F_EXT_LEFT, mpa.F_EXT_RIGHT)[int(rng.integers(0, 2))], int(rng.integers(10, 41)), k)
    return t


EDGES = [1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1100]


def _spread(rng, mode, n, al_max=1100, nls=None):
    """every column-class edge, then n more calls with columns drawn evenly over the classes"""
    out = []
    for al in [a for a in EDGES if a <= al_max]:
        out.append((mode, al, int(rng.integers(3, 2501)) if nls is None else int(rng.choice(nls))))
    for _ in range(n):
        hi = int(rng.choice([16, 32, 64, 128, 256, 512, 1024, 1100]))
        al = int(rng.integers(1, min(hi, al_max) + 1))
        out.append((mode, al, int(rng.integers(3, 2501)) if nls is None else int(rng.choice(nls))))
    return out


def cases():
    """name -> (tasks, option overrides, knobs)"""
    c = {}
    r = np.random.default_rng(9001)
    c["a_ext"] = (_table(r, _spread(r, EXT, 200)), {}, {})
    r = np.random.default_rng(9002)
    c["b_glob"] = (_table(r, _spread(r, GLOB, 150, nls=[3, 50, 383, 384, 385, 700, 2500])), {}, {})
    r = np.random.default_rng(9003)
    nls = [3, 4, 98, 99, 100, 195, 1025]
    spec = [(GLOB, int(r.integers(129, 257)), nl) for nl in nls + nls + [99]]                     # 15 calls of 129..256 columns: seven pairs and an odd one
    spec += [(GLOB, int(r.integers(1, 129)), int(r.choice(nls))) for _ in range(40)] + [(GLOB, 300, 500), (EXT, 40, 300), (EXT, 100, 1025)]
    c["c_wide"] = (_table(r, spec), {}, dict(lite_min=3, lite_wide=1))
    r = np.random.default_rng(9004)
    spec = [(GLOB, int(r.integers(1, 300)), int(r.integers(3, 1200))) for _ in range(80)] + [(GLOB, 512, 2500), (GLOB, 1100, 2000), (EXT, 30, 100)]
    c["d_budget"] = (_table(r, spec), {}, dict(tb_budget=1 << 20))
    r = np.random.default_rng(9005)
    c["e_wide_ge"] = (_table(r, _spread(r, EXT, 10, nls=[3, 100, 600]) + _spread(r, GLOB, 10, nls=[3, 100, 400, 600])), dict(ge=300), {})
    r = np.random.default_rng(9006)
    spec = [(m, al, int(r.choice([3, 200, 384, 900]))) for m in (EXT, GLOB) for al in (1, 16, 30, 40, 41, 47, 48, 49, 64, 100, 130, 200, 300)]
    c["f_saturate"] = (_table(r, spec), dict(go=20000, ge=255), {})
    r = np.random.default_rng(9007)
    c["g_no_split"] = (_table(r, _spread(r, EXT, 40) + [(GLOB, 50, 400)]), {}, dict(no_split=1))
    r = np.random.default_rng(9008)
    c["h_pool"] = (_table(r, _spread(r, EXT, 60, al_max=1024) + _spread(r, GLOB, 60, al_max=300, nls=[3, 50, 99, 400])), {}, dict(pool=1, lite_min=3, lite_wide=1))
    r = np.random.default_rng(9009)
    c["i_antidiag"] = (_table(r, _spread(r, EXT, 80, al_max=300) + [(GLOB, 20, 500)]), {}, dict(antidiag=1))
    r = np.random.default_rng(9010)
    c["k_no_dual_no_prio"] = (_table(r, _spread(r, EXT, 60, al_max=300) + _spread(r, GLOB, 20, al_max=300)), {}, dict(ext_dual=0, unit_prio=0))
    return c


def refusals():
    """name -> (tasks, option overrides): tables the planner must refuse, the offending call second of three"""
    def three(mode, n_col, n_row, **field):
        t = _table(np.random.default_rng(9100), [(EXT, 30, 100), (mode, n_col, n_row), (GLOB, 30, 100)])
        for k, v in field.items():
            t[1][k] = v
        return t
    return {
        "malformed": (three(EXT, 30, 100, al=0), {}),
        "window_past_contig": (three(EXT, 30, 100, vid=4, nt_off=CTG_LEN[2] - 99), {}),
        "slice_past_query": (three(GLOB, 30, 100, qid=2, aa_off=Q_LEN[2] - 29), {}),
        "ext_columns_x_ge": (three(EXT, 1100, 100), dict(ge=500)),
        "glob_columns_x_ge": (three(GLOB, 1100, 100), dict(ge=500)),
        "global_without_cigar": (three(GLOB, 30, 100, flag=0), {}),
        "option_out_of_range": (three(EXT, 30, 100), dict(xdrop=-1)),
    }


def dpopt(**over):
    o = mpa.dpopt_from(mpa.default_mapopt())
    for k, v in over.items():
        setattr(o, k, v)
    return o


def q_off():
    return np.concatenate([[0], np.cumsum(Q_LEN)]).astype(np.int64)


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return "%016x" % h


# ---- the serialised plan: int64 header (HEADER fields, then offset and bytes of every section), then the sections in upload order
HEADER = ("n n_ext n_glob n_reg_glob n_lite n_prep_chunks n_ewaves n_tb_chunks n_units n_group_units n_huge wide_ge round_has_glob "
          "max_nl max_nl_ext rec_total rec_pad prof_total cig_total bnd_total hkey_total lite_total ck_total tb_max key_stride n_wide_groups n_split n_bound "
          "xg_bytes xg_tail q_bytes "
          + " ".join("ewave_first%d" % k for k in range(7)) + " " + " ".join("ewave_cnt%d" % k for k in range(7)) + " dwave_first dwave_cnt "
          + " ".join("lwave_first%d" % k for k in range(4)) + " " + " ".join("lwave_cnt%d" % k for k in range(4)) + " l12_first l12_cnt "
          "sz_tasks sz_chunks sz_qseq sz_rec sz_prof sz_waves sz_extout sz_tb sz_cig sz_ncig sz_lite sz_ckpt sz_wlist sz_score sz_rowkey sz_bnd sz_hkey sz_list sz_xg sz_units "
          "up_tasks up_chunks up_q up_waves up_list up_gw up_units up_off up_ids up_args up_wl up_end dn_eo dn_sc dn_nc dn_err dn_wb dn_end "
          "st_n_ext st_n_glob st_cells_ext st_cells_glob st_alg_bytes_ext st_alg_bytes_glob st_rows_prep st_n_ckpt st_cells_ckpt st_n_ckpt_wide st_cells_ckpt_wide "
          "st_cells_ext_round st_cells_glob_round").split()
SECTIONS = "tasks chunks ewaves pen chunk_tab glist gwaves units wlist walk_launches huge_waves huge_list".split()

DTASK = np.dtype([("nt_off", "<i8"), ("q_off", "<i8"), ("rec_off", "<i8"), ("prof_off", "<i8"), ("tb_off", "<i8"), ("cig_off", "<i8"), ("bnd_off", "<i8"),
                  ("vid", "<i4"), ("nl", "<i4"), ("al", "<i4"), ("flag", "<i4"), ("io", "<i4"), ("ncol", "<i4"), ("pw", "<i4"), ("cig_cap", "<i4"),
                  ("out_idx", "<i4"), ("cls", "<i4")])
PREPCHUNK = np.dtype([("task", "<i4"), ("row0", "<i4")])
EXTWAVE = np.dtype([("task", "<i4", 8), ("max_nl", "<i4"), ("pad_", "<i4", 3), ("rec_base", "<i8"), ("lite_off", "<i8"), ("ck_off", "<i8")])
GLOBWAVE = np.dtype([("task", "<i4", 4), ("max_nl", "<i4"), ("pad_", "<i4", 3)])
DPUNIT = np.dtype([("kind", "<i4"), ("first", "<i4"), ("count", "<i4"), ("blk", "<i4"), ("n_blk", "<i4"), ("sgroup", "<i4"), ("xg_first", "<i4"), ("prio", "<i4")])
CHUNK_TAB = np.dtype([("first", "<i8"), ("last", "<i8"), ("tb_words", "<i8"), ("n_gw", "<i8"), ("cls_first", "<i8", 8), ("cls_cnt", "<i8", 8)])
SECTION_DTYPE = dict(tasks=DTASK, chunks=PREPCHUNK, ewaves=EXTWAVE, pen=np.dtype("<i4"), chunk_tab=CHUNK_TAB, glist=np.dtype("<i4"), gwaves=GLOBWAVE, units=DPUNIT,
                     wlist=np.dtype("<i4"), walk_launches=np.dtype("<i4"), huge_waves=GLOBWAVE, huge_list=np.dtype("<i4"))


class Plan:
    def __init__(self, buf):
        nh = len(HEADER)
        head = np.frombuffer(buf, dtype="<i8", count=nh + 2 * len(SECTIONS))
        self.header = {k: int(v) for k, v in zip(HEADER, head[:nh])}
        self.raw, self.sec = {}, {}
        for k, name in enumerate(SECTIONS):
            off, size = int(head[nh + 2 * k]), int(head[nh + 2 * k + 1])
            self.raw[name] = bytes(buf[off:off + size])
            self.sec[name] = np.frombuffer(self.raw[name], dtype=SECTION_DTYPE[name])

    def digests(self):
        d = {name: fnv1a64(self.raw[name]) for name in SECTIONS}
        d["header"] = fnv1a64(np.array([self.header[k] for k in HEADER], dtype="<i8").tobytes())
        return d


def plan(tasks, opt_over=None, knobs=None, ctg_len=CTG_LEN, qoff=None):
    """-> Plan, or (code, message) of a refusal"""
    kn = dict(KNOBS)
    kn.update(knobs or {})
    r = mpa.dbg_dp_plan(dpopt(**(opt_over or {})), ctg_len, q_off() if qoff is None else qoff, tasks, kn)
    return r if isinstance(r, tuple) else Plan(r)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
