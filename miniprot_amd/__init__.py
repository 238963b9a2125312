"""miniprot_amd -- Python view of libmpamd.so, the MI355X-native drop-in for miniprot's hot path.

This module is plumbing only: it loads the C-ABI library (include/mpamd.h) with ctypes and offers thin
helpers for the tests and bench.py.  All compute lives in miniprot_amd/csrc (hand-written HIP for
gfx950 + host C++).  There is no Python or CPU fallback: if the shared library is missing this import
fails, and if no GPU is usable Context() raises.
"""
import ctypes as C
import os
import subprocess
import numpy as np

# one HIP stream per kernel class: give the runtime enough hardware queues (must be set before HIP initialises)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPA_LIB_PATH") or os.path.join(_HERE, "libmpamd.so")   # (override: experiment builds)

F_CIGAR, F_EXT_LEFT, F_EXT_RIGHT = 1, 2, 4

DP_TASK = np.dtype([("nt_off", "<i8"), ("vid", "<i4"), ("nl", "<i4"), ("qid", "<i4"), ("aa_off", "<i4"),
                    ("al", "<i4"), ("flag", "<i4"), ("io", "<i4"), ("tag", "<i4")], align=True)
DP_RST = np.dtype([("nt_len", "<i4"), ("aa_len", "<i4"), ("score", "<i4"), ("n_cigar", "<i4"),
                   ("cigar_off", "<i8")], align=True)
HIT = np.dtype([("qid", "<i4"), ("id", "<i4"), ("parent", "<i4"), ("n_sub", "<i4"), ("subsc", "<i4"), ("cnt", "<i4"),
                ("n_exon", "<i4"), ("chn_sc", "<i4"), ("chn_sc_ungap", "<i4"), ("vid", "<u4"), ("qs", "<i4"),
                ("qe", "<i4"), ("vs", "<i8"), ("ve", "<i8"), ("has_aln", "<i4"), ("dp_score", "<i4"),
                ("dp_max", "<i4"), ("dp_max2", "<i4"), ("blen", "<i4"), ("n_fs", "<i4"), ("n_stop", "<i4"),
                ("dist_stop", "<i4"), ("dist_start", "<i4"), ("n_iden", "<i4"), ("n_plus", "<i4"),
                ("n_cigar", "<i4"), ("n_feat", "<i4"), ("cigar_off", "<i8"), ("feat_off", "<i8")], align=True)


class MapOpt(C.Structure):
    _fields_ = [("flag", C.c_uint32), ("mini_batch_size", C.c_int64), ("max_occ", C.c_int32), ("max_gap", C.c_int32),
                ("max_intron", C.c_int32), ("min_max_intron", C.c_int32), ("max_max_intron", C.c_int32),
                ("bw", C.c_int32), ("max_ext", C.c_int32), ("max_ava", C.c_int32), ("min_chn_cnt", C.c_int32),
                ("max_chn_max_skip", C.c_int32), ("max_chn_iter", C.c_int32), ("min_chn_sc", C.c_int32),
                ("chn_coef_log", C.c_float), ("mask_level", C.c_float), ("mask_len", C.c_int32),
                ("pri_ratio", C.c_float), ("out_sim", C.c_float), ("out_cov", C.c_float), ("best_n", C.c_int32),
                ("out_n", C.c_int32), ("kmer2", C.c_int32), ("go", C.c_int32), ("ge", C.c_int32), ("io", C.c_int32),
                ("fs", C.c_int32), ("io_end", C.c_int32), ("ie_coef", C.c_float), ("sp_model", C.c_int32),
                ("sp_null_bonus", C.c_int32), ("sp_max_bonus", C.c_int32), ("sp_scale", C.c_float),
                ("xdrop", C.c_int32), ("end_bonus", C.c_int32), ("asize", C.c_int32), ("gff_delim", C.c_int32),
                ("max_intron_flank", C.c_int32), ("gff_prefix", C.c_char_p), ("mat", C.c_int8 * 484)]


class DpOpt(C.Structure):
    _fields_ = [("go", C.c_int32), ("ge", C.c_int32), ("fs", C.c_int32), ("xdrop", C.c_int32),
                ("end_bonus", C.c_int32), ("sp", C.c_int32 * 6), ("ie_coef", C.c_float), ("mat", C.c_int8 * 484),
                ("sp_null_bonus", C.c_int32)]


class QBatch(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("seqs", C.c_char_p), ("q_off", C.POINTER(C.c_int64))]


class DpStats(C.Structure):
    _fields_ = [("n_ext", C.c_int64), ("n_glob", C.c_int64), ("cells_ext", C.c_int64), ("cells_glob", C.c_int64),
                ("rows_prep", C.c_int64), ("alg_bytes_ext", C.c_int64), ("alg_bytes_glob", C.c_int64),
                ("ms_prep", C.c_double), ("ms_ext", C.c_double), ("ms_glob", C.c_double),
                ("ms_backtrack", C.c_double), ("ms_total", C.c_double), ("launches_ext", C.c_int32),
                ("launches_glob", C.c_int32), ("cells_ext_round", C.c_int64), ("cells_glob_round", C.c_int64),
                ("ms_round", C.c_double), ("launches_round", C.c_int32), ("pad_", C.c_int32), ("ms_round_union", C.c_double),
                ("n_ckpt", C.c_int64), ("cells_ckpt", C.c_int64), ("walk_blocks", C.c_int64),
                ("n_ckpt_wide", C.c_int64), ("cells_ckpt_wide", C.c_int64)]


class IdxBuildStats(C.Structure):
    _fields_ = [("n_pass", C.c_int32), ("hist_bits", C.c_int32), ("n_keys", C.c_int64), ("max_pass_keys", C.c_int64),
                ("max_bin_keys", C.c_int64), ("budget_bytes", C.c_int64)]


def build(verbose=False):
    """Compile libmpamd.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libmpamd.so failed:\n" + (r.stdout or "") + (r.stderr or ""))


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no Python/CPU fallback for the HIP kernels)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.mpa_last_error.restype = C.c_char_p
        L.mpa_version.restype = C.c_char_p
        L.mpa_ctx_create.restype = C.c_void_p
        L.mpa_ctx_create.argtypes = [C.c_int]
        L.mpa_ctx_destroy.argtypes = [C.c_void_p]
        L.mpa_idx_restore.restype = C.c_void_p
        L.mpa_idx_restore.argtypes = [C.c_char_p]
        L.mpa_idx_from_nt4.restype = C.c_void_p
        L.mpa_idx_from_nt4.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p]
        L.mpa_idx_dump.argtypes = [C.c_char_p, C.c_void_p]
        L.mpa_idx_build_kmers.argtypes = [C.c_void_p, C.c_int]
        L.mpa_idx_build_kmers_device.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "mpa_idx_build_last_stats"):                    # (absent from older builds loaded through MPA_LIB_PATH)
            L.mpa_idx_build_last_stats.argtypes = [C.c_void_p, C.POINTER(IdxBuildStats)]
            L.mpa_idx_build_last_stats.restype = None
            L.mpa_dbg_idx_build_budget.argtypes = [C.c_void_p, C.c_int64]
            L.mpa_dbg_idx_build_budget.restype = None
            L.mpa_dbg_idx_plan_passes.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]
            L.mpa_dbg_idx_plan_passes.restype = C.c_int32
            L.mpa_dbg_idx_build_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
            L.mpa_dbg_idx_build_hist.restype = C.c_int32
        L.mpa_idx_read_fasta.restype = C.c_void_p
        L.mpa_idx_read_fasta.argtypes = [C.c_char_p, C.c_void_p]
        L.mpa_idx_destroy.argtypes = [C.c_void_p]
        L.mpa_idx_n_ctg.argtypes = [C.c_void_p]
        L.mpa_idx_ctg_len.restype = C.c_int64
        L.mpa_idx_ctg_len.argtypes = [C.c_void_p, C.c_int32]
        L.mpa_idx_ctg_name.restype = C.c_char_p
        L.mpa_idx_ctg_name.argtypes = [C.c_void_p, C.c_int32]
        L.mpa_idx_genome_len.restype = C.c_int64
        L.mpa_idx_genome_len.argtypes = [C.c_void_p]
        L.mpa_idx_get_nt.restype = C.c_int64
        L.mpa_idx_get_nt.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]
        L.mpa_idx_to_device.argtypes = [C.c_void_p, C.c_void_p]
        L.mpa_mapopt_init.argtypes = [C.POINTER(MapOpt)]
        L.mpa_mapopt_set_fs.argtypes = [C.POINTER(MapOpt), C.c_int32]
        L.mpa_mapopt_set_max_intron.argtypes = [C.POINTER(MapOpt), C.c_int64]
        L.mpa_dpopt_from_mapopt.argtypes = [C.POINTER(MapOpt), C.POINTER(DpOpt)]
        L.mpa_dp_run.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DpOpt), C.POINTER(QBatch), C.c_int64, C.c_void_p,
                                 C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_int64)]
        L.mpa_dp_last_stats.argtypes = [C.c_void_p, C.POINTER(DpStats)]
        L.mpa_dp_total_stats.argtypes = [C.c_void_p, C.POINTER(DpStats), C.c_int]
        if hasattr(L, "mpa_dp_handoff_retries"):                      # (absent from older builds loaded through MPA_LIB_PATH)
            L.mpa_dp_handoff_retries.argtypes = [C.c_void_p]
            L.mpa_dp_handoff_retries.restype = C.c_int64
        # (an older build loaded through MPA_LIB_PATH may lack the diagnostics below: the accessors then return 0 / empty)
        if hasattr(L, "mpa_device_bytes"):
            L.mpa_device_bytes.restype = C.c_int64
        if hasattr(L, "mpa_pool_growths"):
            L.mpa_pool_growths.restype = C.c_int64
        if hasattr(L, "mpa_stage_clocks"):
            L.mpa_stage_clocks.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.mpa_free.argtypes = [C.c_void_p]
        for name, res, args in [
            ("mpa_batch_begin", C.c_void_p, [C.c_void_p, C.POINTER(MapOpt), C.POINTER(QBatch), C.c_int]),
            ("mpa_batch_dp_tasks", C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(DpOpt)]),
            ("mpa_batch_dp_results", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
            ("mpa_batch_finish", C.c_void_p, [C.c_void_p]),
            ("mpa_map_batch", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(MapOpt), C.POINTER(QBatch), C.c_int,
                                        C.POINTER(C.c_void_p)]),
            ("mpa_result_n_hit", C.c_int64, [C.c_void_p]),
            ("mpa_result_hits", C.c_void_p, [C.c_void_p]),
            ("mpa_result_hit_off", C.POINTER(C.c_int64), [C.c_void_p]),
            ("mpa_result_cigars", C.POINTER(C.c_uint32), [C.c_void_p]),
            ("mpa_result_destroy", None, [C.c_void_p]),
            ("mpa_idx_set_spsc", C.c_int64, [C.c_void_p, C.c_char_p, C.POINTER(MapOpt), C.c_int]),
            ("mpa_idx_get_spsc", C.c_int64, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]),
            ("mpa_map_batches", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(MapOpt), C.c_int32, C.POINTER(QBatch),
                                          C.POINTER(C.POINTER(C.c_char_p)), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
            ("mpa_format_output", C.c_int64, [C.c_void_p, C.POINTER(MapOpt), C.POINTER(QBatch), C.POINTER(C.c_char_p),
                                              C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]),
            ("mpa_result_n_output", C.c_int64, [C.POINTER(MapOpt), C.POINTER(QBatch), C.c_void_p]),
            ("mpa_format_paf", C.c_int64, [C.c_void_p, C.POINTER(MapOpt), C.POINTER(QBatch), C.POINTER(C.c_char_p),
                                           C.c_void_p, C.POINTER(C.c_void_p)]),
            ("mpa_dbg_refine_chains", C.c_int64, [C.c_void_p, C.c_void_p, C.POINTER(MapOpt), C.POINTER(QBatch), C.c_int32, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
        ]:
            if hasattr(L, name):
                f = getattr(L, name)
                f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def last_error():
    return lib().mpa_last_error().decode()


class MpaError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise MpaError("libmpamd error %d: %s" % (rc, last_error()))


class Context:
    """A HIP device context (one per GPU / per process rank)."""

    def __init__(self, device=0):
        self.h = lib().mpa_ctx_create(device)
        if not self.h:
            raise MpaError("cannot create a device context: " + last_error())

    def close(self):
        if self.h:
            lib().mpa_ctx_destroy(self.h)
            self.h = None

    def dp_stats(self, total=False, reset=False):
        st = DpStats()
        if total:
            lib().mpa_dp_total_stats(self.h, C.byref(st), 1 if reset else 0)
        else:
            lib().mpa_dp_last_stats(self.h, C.byref(st))
        return {k: getattr(st, k) for k, _ in DpStats._fields_}

    def idx_build_stats(self):
        """what the last device index build on this context did (mpa_idx_build_last_stats): passes, histogram bits, keys in all /
        in the fullest pass / in the fullest bin, and the budget in bytes"""
        st = IdxBuildStats()
        lib().mpa_idx_build_last_stats(self.h, C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in IdxBuildStats._fields_}

    def idx_build_budget(self, nbytes):
        """(tests) an exact budget in bytes for the keys of the device index build; 0 restores the default"""
        lib().mpa_dbg_idx_build_budget(self.h, int(nbytes))

    def idx_build_hist(self):
        """the key histogram the last multi-pass index build planned from (int64 array; empty after a one-pass build)"""
        n = lib().mpa_dbg_idx_build_hist(self.h, None, 0)
        hist = np.zeros(n, dtype=np.int64)
        if n:
            lib().mpa_dbg_idx_build_hist(self.h, hist.ctypes.data, n)
        return hist

    def handoff_retries(self):
        """DP rounds repeated because a workgroup hand-off of a split extension call timed out (mpa_dp_handoff_retries)."""
        return int(lib().mpa_dp_handoff_retries(self.h)) if hasattr(lib(), "mpa_dp_handoff_retries") else 0

    @staticmethod
    def device_bytes():
        """bytes of HBM held through the library: resident index + every pool of every context (mpa_device_bytes)"""
        return int(lib().mpa_device_bytes()) if hasattr(lib(), "mpa_device_bytes") else 0

    @staticmethod
    def stage_clocks(reset=False):
        """{stage: (wall ms, calls)} of mpa_map_batches' stages since the last reset (mpa_stage_clocks)"""
        ms, n = (C.c_double * 5)(), (C.c_int64 * 5)()
        if hasattr(lib(), "mpa_stage_clocks"):
            lib().mpa_stage_clocks(ms, n, 1 if reset else 0)
        return {k: (ms[i], int(n[i])) for i, k in enumerate(("seeding", "planning", "dp", "output", "sketch"))}

    @staticmethod
    def pool_growths():
        """how often a device pool had to be re-allocated so far (mpa_pool_growths)"""
        return int(lib().mpa_pool_growths()) if hasattr(lib(), "mpa_pool_growths") else 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Index:
    def __init__(self, handle):
        if not handle:
            raise MpaError("cannot open the index: " + last_error())
        self.h = handle

    @classmethod
    def restore(cls, path):
        return cls(lib().mpa_idx_restore(os.fsencode(path)))

    @classmethod
    def from_nt4(cls, contigs, names=None):
        """contigs: list of uint8 arrays of nt4 codes."""
        n = len(contigs)
        names = names or ["ctg%d" % i for i in range(n)]
        arr = (C.c_char_p * n)(*[s.encode() for s in names])
        lens = np.array([len(c) for c in contigs], dtype=np.int64)
        cat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint8) for c in contigs]))
        return cls(lib().mpa_idx_from_nt4(n, arr, lens.ctypes.data, cat.ctypes.data))

    @classmethod
    def from_fasta(cls, path, n_threads=4):
        """Read a (possibly gzipped) FASTA, pack it and build the k-mer table on the host (index.c:97-136)."""
        import gzip
        op = gzip.open if path.endswith(".gz") else open
        names, parts, cur = [], [], []
        lut = np.full(256, 4, dtype=np.uint8)
        for i, ch in enumerate(b"ACGT"):
            lut[ch] = lut[ch | 0x20] = i
        with op(path, "rb") as f:
            for line in f:
                if line.startswith(b">"):
                    if names:
                        parts.append(np.concatenate(cur) if cur else np.zeros(0, np.uint8))
                    names.append(line[1:].split()[0].decode())
                    cur = []
                else:
                    cur.append(lut[np.frombuffer(line.rstrip(), dtype=np.uint8)])
        if names:
            parts.append(np.concatenate(cur) if cur else np.zeros(0, np.uint8))
        idx = cls.from_nt4(parts, names)
        _check(lib().mpa_idx_build_kmers(idx.h, n_threads))
        return idx

    @classmethod
    def read_fasta(cls, path, idxopt=None):
        """Genome-only index of a FASTA file (mpa_idx_read_fasta); idxopt: (bbit, min_aa_len, kmer, mod_bit, trans_code) or None"""
        io = (C.c_int32 * 5)()
        lib().mpa_idxopt_init(io)
        if idxopt is not None:
            for k, v in enumerate(idxopt):
                io[k] = v
        return cls(lib().mpa_idx_read_fasta(os.fsencode(path), io))

    def build_kmers(self, n_threads=4, ctx=None):
        """The k-mer table (mp_idx_build): on the GPU when a context is given and the device path takes the job, else on the host.
        Returns "gpu" or "host"."""
        if ctx is not None:
            rc = lib().mpa_idx_build_kmers_device(ctx.h, self.h)
            if rc == 0:
                return "gpu"
            if rc != -3:                                      # MPA_ERR_UNSUPPORTED: parameters / memory -> host
                _check(rc)
        _check(lib().mpa_idx_build_kmers(self.h, n_threads))
        return "host"

    def to_device(self, ctx):
        _check(lib().mpa_idx_to_device(ctx.h, self.h))

    def n_ctg(self):
        return lib().mpa_idx_n_ctg(self.h)

    def ctg_len(self, cid):
        return lib().mpa_idx_ctg_len(self.h, cid)

    def ctg_name(self, cid):
        return lib().mpa_idx_ctg_name(self.h, cid).decode()

    def genome_len(self):
        return lib().mpa_idx_genome_len(self.h)

    has_spsc = False

    def set_spsc(self, path, mo, keep_io=False):
        """--spsc: load a splice-score file (mp_set_spsc); adjusts mo.io / mo.io_end unless keep_io.  Before to_device()."""
        n = lib().mpa_idx_set_spsc(self.h, path.encode(), C.byref(mo), 1 if keep_io else 0)
        if n < 0:
            raise MpaError(last_error())
        self.has_spsc = True
        return n

    def get_spsc(self, vid, st, en):
        """the ss[] bytes the reference hands the DP for the window [st,en) of vid, or None without a track"""
        out = np.zeros(max(en - st, 1), dtype=np.uint8)
        n = lib().mpa_idx_get_spsc(self.h, vid, st, en, out.ctypes.data)
        return None if n < 0 else out[:n]

    def get_nt(self, vid, st, en):
        buf = np.zeros(max(en - st, 0), dtype=np.uint8)
        n = lib().mpa_idx_get_nt(self.h, vid, st, en, buf.ctypes.data)
        return buf[:max(n, 0)]

    def dump(self, path):
        _check(lib().mpa_idx_dump(os.fsencode(path), self.h))

    def close(self):
        if self.h:
            lib().mpa_idx_destroy(self.h)
            self.h = None


class Queries:
    """A batch of protein sequences as the C ABI wants them (one concatenated buffer + offsets)."""

    def __init__(self, seqs, names=None):
        self.seqs = [s if isinstance(s, bytes) else s.encode() for s in seqs]
        self.names = names or ["q%d" % i for i in range(len(self.seqs))]
        self.buf = b"".join(self.seqs)
        self.off = np.zeros(len(self.seqs) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in self.seqs], out=self.off[1:])
        self.c = QBatch(len(self.seqs), self.buf, self.off.ctypes.data_as(C.POINTER(C.c_int64)))


def idx_plan_passes(hist, budget_keys):
    """The pass planner of the device index build (mpa_dbg_idx_plan_passes; no device needed): hist = keys per bin, at most
    budget_keys keys per pass.  Returns the list first_bin[0 .. n_pass] (pass p = bins [first_bin[p], first_bin[p + 1])), or -1
    when a bin alone exceeds the budget."""
    hist = np.ascontiguousarray(hist, dtype=np.int64)
    first = np.zeros(len(hist) + 1, dtype=np.int32)
    n = lib().mpa_dbg_idx_plan_passes(hist.ctypes.data, len(hist), int(budget_keys), first.ctypes.data)
    return -1 if n < 0 else [int(x) for x in first[:n + 1]]


def dbg_dp_plan(dpopt, ctg_len, q_off, tasks, knobs):
    """The plan of one mpa_dp_run() call (mpa_dbg_dp_plan; no device needed) for a task table: contig lengths, query offsets (n_seq + 1),
    DP_TASK array, and the executor's knobs as a dict (lite_min, lite_wide, no_split, antidiag, pool, ext_dual, unit_prio, tb_budget).
    Returns the serialised plan as bytes (layout: mpamd.h), or (code, message) when the planner refuses the table."""
    tasks = np.ascontiguousarray(tasks, dtype=DP_TASK)
    ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int64)
    q_off = np.ascontiguousarray(q_off, dtype=np.int64)
    kn = np.array([knobs[k] for k in ("lite_min", "lite_wide", "no_split", "antidiag", "pool", "ext_dual", "unit_prio", "tb_budget")], dtype=np.int64)
    f = lib().mpa_dbg_dp_plan
    f.restype = C.c_int64
    f.argtypes = [C.POINTER(DpOpt), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    args = (C.byref(dpopt), len(ctg_len), ctg_len.ctypes.data, len(q_off) - 1, q_off.ctypes.data, len(tasks), tasks.ctypes.data, kn.ctypes.data)
    need = f(*args, None, 0)
    if need < 0:
        return int(need), last_error()
    buf = np.zeros(need, dtype=np.uint8)
    assert f(*args, buf.ctypes.data, need) == need
    return buf.tobytes()


def default_mapopt():
    mo = MapOpt()
    lib().mpa_mapopt_init(C.byref(mo))
    return mo


def dpopt_from(mo):
    dp = DpOpt()
    lib().mpa_dpopt_from_mapopt(C.byref(mo), C.byref(dp))
    return dp


class Result:
    """Owner of an mpa_result_t (the structured hits of one batch)."""

    def __init__(self, handle):
        self.h = handle

    def n_hit(self):
        return lib().mpa_result_n_hit(self.h)

    def n_output(self, mo, queries):
        """ids the output of this batch consumes (mpa_result_n_output)"""
        return lib().mpa_result_n_output(C.byref(mo), C.byref(queries.c), self.h)

    def close(self):
        if self.h:
            lib().mpa_result_destroy(C.c_void_p(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_output(idx, mo, queries, result, id0=0):
    """mpa_format_output(): the text of one batch whose first printed hit gets id0 + 1.  Returns (text, id after the batch)."""
    names = (C.c_char_p * len(queries.names))(*[n.encode() for n in queries.names])
    out = C.c_void_p()
    idc = C.c_int64(id0)
    n = lib().mpa_format_output(idx.h, C.byref(mo), C.byref(queries.c), names, result.h, C.byref(idc), C.byref(out))
    if n < 0:
        raise MpaError(last_error())
    txt = C.string_at(out.value, n)
    lib().mpa_free(out)
    return txt, idc.value


def map_batch(ctx, idx, mo, queries, n_threads=1):
    """mpa_map_batch(): one blocking batch; returns its Result."""
    res = C.c_void_p()
    _check(lib().mpa_map_batch(ctx.h, idx.h, C.byref(mo), C.byref(queries.c), n_threads, C.byref(res)))
    return Result(res.value)


def refine_chains(ctx, idx, mo, queries, wins):
    """mpa_dbg_refine_chains(): the refinement chains of the windows `wins` = [(query, vid, start, length), ...] -- from the device
    refinement (ctx) or from the host stage (ctx = None).  Returns (off_u, u, off_a, a, host_flag): u = score << 32 | anchors of each
    chain and a = the chains' anchors, window k's in [off[k], off[k + 1]); host_flag[k] = 1 where the device handed the window back."""
    n = len(wins)
    qid = np.array([w[0] for w in wins], np.int32)
    vid = np.array([w[1] for w in wins], np.int32)
    as_ = np.array([w[2] for w in wins], np.int64)
    ln_ = np.array([w[3] for w in wins], np.int32)
    off_u, off_a, flag = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64), np.zeros(max(n, 1), np.uint8)
    pu, pa = C.c_void_p(), C.c_void_p()
    rc = lib().mpa_dbg_refine_chains(ctx.h if ctx else None, idx.h, C.byref(mo), C.byref(queries.c), n, qid.ctypes.data, vid.ctypes.data, as_.ctypes.data,
                                     ln_.ctypes.data, off_u.ctypes.data, C.byref(pu), off_a.ctypes.data, C.byref(pa), flag.ctypes.data)
    if rc < 0:
        raise MpaError("libmpamd error %d: %s" % (rc, last_error()))
    u = np.ctypeslib.as_array(C.cast(pu, C.POINTER(C.c_uint64)), (max(int(off_u[n]), 1),))[:int(off_u[n])].copy()
    a = np.ctypeslib.as_array(C.cast(pa, C.POINTER(C.c_uint64)), (max(int(off_a[n]), 1),))[:int(off_a[n])].copy()
    lib().mpa_free(pu), lib().mpa_free(pa)
    return off_u, u, off_a, a, flag[:n]


CLAIM_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p)


DBG_LIB_PATH = os.path.join(_HERE, "libmpamd_dbg.so")   # the test hooks of the device steps: a library of its own, linked against libmpamd.so
_dbg_lib = None


def dbg_lib():
    """libmpamd_dbg.so (mpa_dbg_spans), loaded behind libmpamd.so"""
    global _dbg_lib
    if _dbg_lib is None:
        lib()
        if not os.path.exists(DBG_LIB_PATH):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % DBG_LIB_PATH)
        _dbg_lib = C.CDLL(DBG_LIB_PATH)
    return _dbg_lib


def dbg_spans(ctx, idx, mo, queries, plans, segs, rst1, pool1, rst2=None, pool2=None):
    """mpa_dbg_spans(): the two steps of MPA_GPU_SPANS on hand-made inputs -- the accepted spans between the DP rounds and the region
    CIGARs behind them -- on the device (ctx) or through the shared core on the host (ctx None).  plans (104-byte records), segs (24),
    rst1 / rst2 (mpa_dp_rst_t) and the pools (uint32) are numpy arrays laid out as include/mpamd_dbg.h says.  Returns (span records as
    bytes, round-2 tasks as bytes) for rst2 None, else (span records, tasks, assemble records, cigar words as a uint32 array)."""
    import numpy as np
    fn = dbg_lib().mpa_dbg_spans
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MapOpt), C.POINTER(QBatch), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                   C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int64]
    n = len(plans)
    rec, tasks, arec, n_task = np.zeros(80 * n, np.uint8), np.zeros(80 * n + 8, np.uint8), np.zeros(40 * n, np.uint8), C.c_int32(0)
    cap = 2 * n + len(segs) + len(pool1) + (len(pool2) if pool2 is not None else 0) + 16
    cig = np.zeros(cap, np.uint32)
    keep = [np.ascontiguousarray(x) if x is not None else None for x in (plans, segs, rst1, pool1, rst2, pool2)]
    ptr = [x.ctypes.data if x is not None and len(x) else None for x in keep]
    _check(fn(ctx.h if ctx else None, idx.h, C.byref(mo), C.byref(queries.c), n, ptr[0], len(segs), ptr[1], len(rst1), ptr[2], ptr[3], len(pool1),
              -1 if rst2 is None else len(rst2), ptr[4], ptr[5], 0 if pool2 is None else len(pool2), rec.ctypes.data, tasks.ctypes.data, C.byref(n_task), arec.ctypes.data,
              cig.ctypes.data, cap))
    tasks = tasks[:40 * n_task.value].tobytes()
    if rst2 is None:
        return rec.tobytes(), tasks
    return rec.tobytes(), tasks, arec.tobytes(), cig


FLAT_ARRAYS = ("hits", "hit_off", "cigars", "feats", "cs", "cs_text", "rows", "rows_text")   # MPA_DBG_FLAT_* (include/mpamd_dbg.h), in order


def result_flat(handle):
    """mpa_dbg_result_flat(): the flat arrays of a result (a Result or a raw mpa_result_t handle) as a dict of bytes, keyed by FLAT_ARRAYS."""
    f = dbg_lib().mpa_dbg_result_flat
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    h = getattr(handle, "h", handle)
    out = {}
    for which, name in enumerate(FLAT_ARRAYS):
        n = f(h, which, None, 0)
        if n < 0:
            raise MpaError("mpa_dbg_result_flat: %d: %s" % (n, last_error()))
        buf = C.create_string_buffer(max(int(n), 1))
        f(h, which, buf, n)
        out[name] = buf.raw[:n]
    return out


def dbg_finish(ctx, mo, kmer, first, recs, words, feats, cs_text, rows_text):
    """mpa_dbg_finish(): ranking and flat result (MPA_GPU_FINISH) of hand-made tables, on the device (ctx) or through the shared core on
    the host (ctx None).  first (int64, n_query + 1), recs (160-byte records as a uint8 array), words (uint32), feats (56-byte records
    as a uint8 array) are numpy arrays, cs_text / rows_text bytes, laid out as include/mpamd_dbg.h says.  Returns result_flat()'s dict."""
    import numpy as np
    f = dbg_lib().mpa_dbg_finish
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(MapOpt), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_char_p, C.c_int64,
                  C.c_char_p, C.c_int64, C.POINTER(C.c_void_p)]
    first = np.ascontiguousarray(first, np.int64)
    recs, words, feats = np.ascontiguousarray(recs, np.uint8), np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(feats, np.uint8)
    assert len(recs) == 160 * int(first[-1]) and len(feats) % 56 == 0
    out = C.c_void_p(None)
    _check(f(ctx.h if ctx else None, C.byref(mo), int(kmer), len(first) - 1, first.ctypes.data, recs.ctypes.data if len(recs) else None, words.ctypes.data if len(words) else None,
             len(words), feats.ctypes.data if len(feats) else None, len(feats) // 56, cs_text if cs_text else None, len(cs_text), rows_text if rows_text else None, len(rows_text),
             C.byref(out)))
    try:
        return result_flat(out.value)
    finally:
        lib().mpa_result_destroy(C.c_void_p(out.value))


def dbg_finish_last(ctx):
    """mpa_dbg_finish_last(): of the context's last device finish call, (queries, hits in, hits kept, bytes down, queries ranked in HBM
    scratch, host waits)."""
    f = dbg_lib().mpa_dbg_finish_last
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int64 * 6)]
    out = (C.c_int64 * 6)()
    _check(f(ctx.h, C.byref(out)))
    return tuple(int(x) for x in out)


FORMAT_DECLINED = 1   # MPA_DBG_FORMAT_DECLINED (include/mpamd_dbg.h)


def dbg_idx_names(names, lens):
    """mpa_dbg_idx_names(): an Index of contig names and lengths alone (no sequence): what the formatter reads of an index when every
    aligned hit carries what the options print."""
    f = dbg_lib().mpa_dbg_idx_names
    f.restype = C.c_void_p
    f.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
    arr = (C.c_char_p * len(names))(*[s.encode() for s in names])
    ln = np.ascontiguousarray(lens, np.int64)
    return Index(f(len(names), arr, ln.ctypes.data))


def dbg_result_make(hit_off, hits, cigars, feats, cs=None, cs_text=b"", rows=None, rows_text=b""):
    """mpa_dbg_result_make(): a Result from flat arrays -- hit_off (int64, n_seq + 1), hits (HIT records), cigars (uint32), feats (56-byte
    records as a uint8 array), and the cs / rows references of every hit (16- / 24-byte records as uint8 arrays, or None) with their texts."""
    f = dbg_lib().mpa_dbg_result_make
    f.restype = C.c_int
    f.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_char_p, C.c_int64,
                  C.POINTER(C.c_void_p)]
    hit_off = np.ascontiguousarray(hit_off, np.int64)
    hits = np.ascontiguousarray(hits)
    cigars, feats = np.ascontiguousarray(cigars, np.uint32), np.ascontiguousarray(feats, np.uint8)
    assert hits.nbytes == 136 * int(hit_off[-1]) and len(feats) % 56 == 0
    cs = None if cs is None else np.ascontiguousarray(cs).view(np.uint8)
    rows = None if rows is None else np.ascontiguousarray(rows).view(np.uint8)
    assert cs is None or len(cs) == 16 * int(hit_off[-1])
    assert rows is None or len(rows) == 24 * int(hit_off[-1])
    out = C.c_void_p(None)
    _check(f(len(hit_off) - 1, hit_off.ctypes.data, hits.ctypes.data if hits.nbytes else None, cigars.ctypes.data if len(cigars) else None, len(cigars),
             feats.ctypes.data if len(feats) else None, len(feats) // 56, None if cs is None else cs.ctypes.data, cs_text, len(cs_text),
             None if rows is None else rows.ctypes.data, rows_text, len(rows_text), C.byref(out)))
    return Result(out.value)


def dbg_format(ctx, idx, mo, queries, result, id0=0):
    """mpa_dbg_format(): the output text of a result through the three stages of MPA_GPU_FORMAT, on the device (ctx) or through the shared
    core on the host (ctx None), patched with id0.  Returns (text, printed hits, declined): declined = the step declined and the text is
    mpa_format_output()'s."""
    f = dbg_lib().mpa_dbg_format
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MapOpt), C.POINTER(QBatch), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    names = (C.c_char_p * len(queries.names))(*[n.encode() for n in queries.names])
    out, n, n_out = C.c_void_p(None), C.c_int64(0), C.c_int64(0)
    rc = f(ctx.h if ctx else None, idx.h, C.byref(mo), C.byref(queries.c), names, result.h, int(id0), C.byref(out), C.byref(n), C.byref(n_out))
    if rc < 0:
        _check(rc)
    txt = C.string_at(out.value, n.value)
    lib().mpa_free(out)
    return txt, int(n_out.value), rc == FORMAT_DECLINED


def dbg_format_last(ctx):
    """mpa_dbg_format_last(): of the context's last device format call, (queries, hits printed, text bytes, id fields, host waits, declined)."""
    f = dbg_lib().mpa_dbg_format_last
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int64 * 6)]
    out = (C.c_int64 * 6)()
    _check(f(ctx.h, C.byref(out)))
    return tuple(int(x) for x in out)


DP_PLAN_DECLINED = 1   # MPA_DBG_DP_PLAN_DECLINED (include/mpamd_dbg.h)


def dbg_dp_plan_device(ctx, dpopt, ctg_len, q_off, tasks, knobs):
    """mpa_dbg_dp_plan_device(): the plan of dbg_dp_plan() from the device planner of MPA_GPU_DPPLAN on a context, or (ctx None) from its
    model, the planner's stages on the host with a team of one.  Returns the serialised plan as bytes, (DP_PLAN_DECLINED, reason) when
    the device planner leaves the table to the host planner, or (code, message) of an error."""
    import numpy as np
    tasks = np.ascontiguousarray(tasks, dtype=DP_TASK)
    ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int64)
    q_off = np.ascontiguousarray(q_off, dtype=np.int64)
    kn = np.array([knobs[k] for k in ("lite_min", "lite_wide", "no_split", "antidiag", "pool", "ext_dual", "unit_prio", "tb_budget")], dtype=np.int64)
    f = dbg_lib().mpa_dbg_dp_plan_device
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.POINTER(DpOpt), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    args = (ctx.h if ctx else None, C.byref(dpopt), len(ctg_len), ctg_len.ctypes.data, len(q_off) - 1, q_off.ctypes.data, len(tasks), tasks.ctypes.data, kn.ctypes.data)
    need = f(*args, None, 0)
    if need < 0 or need == DP_PLAN_DECLINED:
        return int(need), last_error()
    buf = np.zeros(need, dtype=np.uint8)
    got = f(*args, buf.ctypes.data, need)
    if got != need:
        return int(got), last_error()
    return buf.tobytes()


DP_PLAN_KNOBS_WIDE = ("lite_min", "lite_wide", "no_split", "antidiag", "pool", "ext_dual", "unit_prio", "tb_budget", "split_wide")
DP_PLAN_WIDE_TAIL = 40   # bytes the *_wide serialisations add: int64 first, count of X_SPLIT8; first, count of X_SPLIT12; n_bound
X_HUGE, X_SPLIT8, X_SPLIT12, X_NONE = 7, 9, 10, 11   # DpClass numbers (dp_device.h) in dbg_dp_last_classes(); X_NONE: extension calls of fewer than three rows, swept by nobody


def _dp_plan_wide(f, head, dpopt, ctg_len, q_off, tasks, knobs, declines):
    import numpy as np
    tasks = np.ascontiguousarray(tasks, dtype=DP_TASK)
    ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int64)
    q_off = np.ascontiguousarray(q_off, dtype=np.int64)
    kn = np.array([knobs.get(k, 0) for k in DP_PLAN_KNOBS_WIDE], dtype=np.int64)
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p] * len(head) + [C.POINTER(DpOpt), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    args = tuple(head) + (C.byref(dpopt), len(ctg_len), ctg_len.ctypes.data, len(q_off) - 1, q_off.ctypes.data, len(tasks), tasks.ctypes.data, kn.ctypes.data)
    need = f(*args, None, 0)
    if need < 0 or (declines and need == DP_PLAN_DECLINED):
        return int(need), last_error()
    buf = np.zeros(need, dtype=np.uint8)
    got = f(*args, buf.ctypes.data, need)
    if got != need:
        return int(got), last_error()
    return buf.tobytes()


def dbg_dp_plan_wide(dpopt, ctg_len, q_off, tasks, knobs):
    """mpa_dbg_dp_plan_wide(): dbg_dp_plan() with a ninth knob, split_wide (MPA_DP_SPLIT_WIDE; missing: 0).  The bytes are dbg_dp_plan()'s
    followed by DP_PLAN_WIDE_TAIL more (include/mpamd_dbg.h); (code, message) when the planner refuses the table."""
    return _dp_plan_wide(dbg_lib().mpa_dbg_dp_plan_wide, (), dpopt, ctg_len, q_off, tasks, knobs, False)


def dbg_dp_plan_device_wide(ctx, dpopt, ctg_len, q_off, tasks, knobs):
    """mpa_dbg_dp_plan_device_wide(): dbg_dp_plan_device() with the ninth knob and the tail of dbg_dp_plan_wide()."""
    return _dp_plan_wide(dbg_lib().mpa_dbg_dp_plan_device_wide, (ctx.h if ctx else None,), dpopt, ctg_len, q_off, tasks, knobs, True)


def dbg_dp_last_classes(ctx):
    """mpa_dbg_dp_last_classes(): extension calls per DpClass (a list of 16) in the plan of the context's last dp_run()."""
    import numpy as np
    out = np.zeros(16, np.int64)
    f = dbg_lib().mpa_dbg_dp_last_classes
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p]
    _check(f(ctx.h, out.ctypes.data))
    return [int(x) for x in out]


def dbg_dp_last_huge(ctx):
    """mpa_dbg_dp_last_huge(): of the context's last dp_run(), (X_HUGE calls swept by the one-wave kernel, X_HUGE calls swept by the
    workgroup kernel of MPA_DP_HUGE_WG, column blocks of the latter, passes of the latter)."""
    import numpy as np
    out = np.zeros(4, np.int64)
    f = dbg_lib().mpa_dbg_dp_last_huge
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p]
    _check(f(ctx.h, out.ctypes.data))
    return tuple(int(x) for x in out)


def dbg_dp_last_mb(ctx):
    """mpa_dbg_dp_last_mb(): of the context's last dp_run(), (T_MB traceback calls swept on one wave, T_MB calls swept by the workgroup
    kernel of MPA_DP_MB_WG, column blocks of the latter, passes of the latter)."""
    import numpy as np
    out = np.zeros(4, np.int64)
    f = dbg_lib().mpa_dbg_dp_last_mb
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p]
    _check(f(ctx.h, out.ctypes.data))
    return tuple(int(x) for x in out)


DP_PLAN_KNOBS_W8 = DP_PLAN_KNOBS_WIDE + ("lite_w8",)
DP_PLAN_W8_TAIL = 24   # bytes dbg_dp_plan_w8() adds behind the *_wide tail: int64 first, count of T_LITE_W8's descriptors; calls of its walk list
T_LITE_W8 = 13         # DpClass number (dp_device.h) of the 257..512-column checkpointed traceback class


def dbg_dp_plan_w8(dpopt, ctg_len, q_off, tasks, knobs):
    """mpa_dbg_dp_plan_w8(): dbg_dp_plan_wide() with a tenth knob, lite_w8 (MPA_DP_LITE_W8; missing: 0).  The bytes are dbg_dp_plan_wide()'s
    followed by DP_PLAN_W8_TAIL more (include/mpamd_dbg.h); (code, message) when the planner refuses the table."""
    import numpy as np
    tasks = np.ascontiguousarray(tasks, dtype=DP_TASK)
    ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int64)
    q_off = np.ascontiguousarray(q_off, dtype=np.int64)
    kn = np.array([knobs.get(k, 0) for k in DP_PLAN_KNOBS_W8], dtype=np.int64)
    f = dbg_lib().mpa_dbg_dp_plan_w8
    f.restype = C.c_int64
    f.argtypes = [C.POINTER(DpOpt), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    args = (C.byref(dpopt), len(ctg_len), ctg_len.ctypes.data, len(q_off) - 1, q_off.ctypes.data, len(tasks), tasks.ctypes.data, kn.ctypes.data)
    need = f(*args, None, 0)
    if need < 0:
        return int(need), last_error()
    buf = np.zeros(need, dtype=np.uint8)
    got = f(*args, buf.ctypes.data, need)
    if got != need:
        return int(got), last_error()
    return buf.tobytes()


def dbg_dp_last_w8(ctx):
    """mpa_dbg_dp_last_w8(): of the context's last dp_run(), (traceback calls of the class T_LITE_W8 -- 257..512 columns, MPA_DP_LITE_W8 --,
    their padded cells, the eight-wave groups k_lite_w8 swept, the blocks of 96 rows k_walk_w8 recomputed)."""
    import numpy as np
    out = np.zeros(4, np.int64)
    f = dbg_lib().mpa_dbg_dp_last_w8
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p]
    _check(f(ctx.h, out.ctypes.data))
    return tuple(int(x) for x in out)


def dbg_dp_huge_wg_info():
    """mpa_dbg_dp_huge_wg_info(): (W waves per workgroup, R rows per chunk, MIN_BLOCKS) of the workgroup kernel's schedule."""
    import numpy as np
    out = np.zeros(3, np.int32)
    f = dbg_lib().mpa_dbg_dp_huge_wg_info
    f.restype = None
    f.argtypes = [C.c_void_p]
    f(out.ctypes.data)
    return tuple(int(x) for x in out)


STREAM_CLASSES = ("normal", "high", "low")
STREAM_LAYOUTS = ("legacy", "A", "B", "C")


def _stream_plan_of(words):
    w = [int(x) for x in words]
    q, lanes, seeders, planners, layout, n_streams = w[:6]
    at = 6
    plan = {"q": q, "layout": STREAM_LAYOUTS[layout], "n_streams": n_streams, "lanes": [], "seeders": [], "planners": []}
    for _ in range(lanes):
        plan["lanes"].append({"cls": STREAM_CLASSES[w[at]], "rank": w[at + 1], "side_cap": w[at + 2], "side_cls": STREAM_CLASSES[w[at + 3]]})
        at += 4
    for role, n in (("seeders", seeders), ("planners", planners)):
        for _ in range(n):
            plan[role].append({"cls": STREAM_CLASSES[w[at]], "rank": w[at + 1], "seed_cls": STREAM_CLASSES[w[at + 2]], "seed_rank": w[at + 3]})
            at += 4
    assert at == len(w)
    return plan


def dbg_stream_plan(ctx):
    """mpa_dbg_stream_plan(): the stream plan in force on a context -- the one its last map_batches() created its sibling contexts by --
    as a dict (q, layout, n_streams, lanes / seeders / planners: class and rank in creation order of every stream, a lane's side-stream
    cap and class); None before the first stream of batches."""
    import numpy as np
    out = np.zeros(6 + 4 * 18, np.int32)
    f = dbg_lib().mpa_dbg_stream_plan
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    n = f(ctx.h, out.ctypes.data, len(out))
    _check(min(n, 0))
    return _stream_plan_of(out[:n]) if n else None


def dbg_stream_plan_for(q, lanes=5, seeders=3, planners=4, layout=None):
    """mpa_dbg_stream_plan_for(): the plan of the module (stream_plan.cpp; no device needed) for q hardware queues (0: GPU_MAX_HW_QUEUES
    as the process sees it) and a value of MPA_STREAM_PLAN (None: unset)."""
    import numpy as np
    out = np.zeros(6 + 4 * 18, np.int32)
    f = dbg_lib().mpa_dbg_stream_plan_for
    f.restype = C.c_int64
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_void_p, C.c_int64]
    n = f(q, lanes, seeders, planners, None if layout is None else str(layout).encode(), out.ctypes.data, len(out))
    return _stream_plan_of(out[:n])


def dbg_ctx_pools(ctx, sibling=0):
    """mpa_dbg_ctx_pools(): the device pools a context (sibling 0) or its sibling number `sibling` has registered, in registration
    order, as a list of (name, capacity in bytes); None when the context has no sibling of that number."""
    f = dbg_lib().mpa_dbg_ctx_pools
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    n = f(ctx.h, sibling, None, None, 0)
    if n < 0:
        return None
    names = (C.c_char_p * n)()
    caps = (C.c_int64 * n)()
    _check(min(f(ctx.h, sibling, names, caps, n), 0))
    return [(names[k].decode(), int(caps[k])) for k in range(n)]


ROUND2_DECLINED = 1  # MPA_DBG_ROUND2_DECLINED (include/mpamd_dbg.h)
ROUND2_REC = ("plan_waits", "round_waits", "bytes_up", "task_bytes_up", "bytes_down", "pool_bytes_down", "pool_bytes_fetched", "prep_bound", "max_nl", "max_al", "n_pool", "reserved")


class _DpOutputs(C.Structure):
    _fields_ = [("ext_out", C.c_void_p), ("score", C.c_void_p), ("n_cigar", C.c_void_p), ("gids", C.c_void_p), ("n_glob", C.c_int64)]


def dbg_dp_run_resident(ctx, idx, dpopt, queries, tasks, made_up=None):
    """mpa_dbg_dp_run_resident(): a DP round from device-resident tasks (MPA_GPU_ROUND2) -- the arguments of dp_run().  On a context the
    round is planned from the tasks in a device pool and its result records and dense CIGAR pool are assembled on the device; returns
    (results, cigar_pool, record) with the record a dict of ROUND2_REC, (ROUND2_DECLINED, reason) for a round that falls back to
    mpa_dp_run, or (code, message) of an error.  ctx None: no DP runs -- made_up = (ext_out int32 [n, 4], score int32 [n], n_cigar int32
    [n], gids int32 [n_glob]) goes through the result stages with a team of one; idx, dpopt and queries may be None; the pool is empty."""
    tasks = np.ascontiguousarray(tasks, dtype=DP_TASK)
    rst = np.zeros(len(tasks), dtype=DP_RST)
    pool = C.POINTER(C.c_uint32)()
    n_pool = C.c_int64(0)
    rec = np.zeros(len(ROUND2_REC), dtype=np.int64)
    f = dbg_lib().mpa_dbg_dp_run_resident
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    mu, keep = None, None
    if made_up is not None:
        keep = [np.ascontiguousarray(x, dtype=np.int32) for x in made_up]
        mu = _DpOutputs(keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data if len(keep[3]) else None, len(keep[3]))
    rc = f(ctx.h if ctx else None, idx.h if idx else None, C.byref(dpopt) if dpopt is not None else None, C.byref(queries.c) if queries is not None else None,
           len(tasks), tasks.ctypes.data, C.byref(mu) if mu is not None else None, rst.ctypes.data, C.byref(pool), C.byref(n_pool), rec.ctypes.data)
    if rc != 0:
        return int(rc), last_error()
    words = n_pool.value if pool else 0
    cig = np.ctypeslib.as_array(pool, (max(words, 1),))[:words].copy() if words else np.zeros(0, np.uint32)
    if pool:
        lib().mpa_free(pool)
    return rst, cig, dict(zip(ROUND2_REC, (int(x) for x in rec)))


ROUND1_DECLINED = 1  # MPA_DBG_ROUND1_DECLINED (include/mpamd_dbg.h)
ROUND1_REC = ("plan_waits", "round_waits", "bytes_up", "task_bytes_up", "bytes_down", "pool_bytes_down", "chained_launches", "plan_bytes_up", "residue_bytes", "spans_bytes_up",
              "rst1_bytes_skipped", "pool_bytes_fetched")


def dbg_round1_chain(ctx, idx, mo, dpopt, queries, plans, segs, tasks):
    """mpa_dbg_round1_chain(): DP round 1 and the step behind it in one submission (MPA_GPU_ROUND1) -- plans (104-byte records) and segs (24)
    as dbg_spans() takes them and the round-1 task table they point into.  Returns (results, cigar_pool, span records as bytes, round-2
    tasks as bytes, (prep_bound, max_nl, max_al), record) with the record a dict of ROUND1_REC, (ROUND1_DECLINED, reason) for a round that
    falls back to mpa_dp_run, or (code, message) of an error (ctx None: the argument error)."""
    tasks = np.ascontiguousarray(tasks, dtype=DP_TASK)
    n, n_plan = len(tasks), len(plans)
    rst = np.zeros(n, dtype=DP_RST)
    srec, tasks2, n_task = np.zeros(80 * n_plan + 8, np.uint8), np.zeros(80 * n_plan + 8, np.uint8), C.c_int32(0)
    bounds, rec = np.zeros(3, np.int64), np.zeros(len(ROUND1_REC), dtype=np.int64)
    pool, n_pool = C.POINTER(C.c_uint32)(), C.c_int64(0)
    f = dbg_lib().mpa_dbg_round1_chain
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MapOpt), C.c_void_p, C.POINTER(QBatch), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    keep = [np.ascontiguousarray(x) for x in (plans, segs)]
    ptr = [x.ctypes.data if len(x) else None for x in keep]
    rc = f(ctx.h if ctx else None, idx.h, C.byref(mo), C.addressof(dpopt), C.byref(queries.c), n_plan, ptr[0], len(segs), ptr[1], n, tasks.ctypes.data, rst.ctypes.data,
           srec.ctypes.data, tasks2.ctypes.data, C.byref(n_task), bounds.ctypes.data, C.addressof(pool), C.addressof(n_pool), rec.ctypes.data)
    if rc != 0:
        return int(rc), last_error()
    words = n_pool.value if pool else 0
    cig = np.ctypeslib.as_array(pool, (max(words, 1),))[:words].copy() if words else np.zeros(0, np.uint32)
    if pool:
        lib().mpa_free(pool)
    return rst, cig, srec[:80 * n_plan].tobytes(), tasks2[:40 * n_task.value].tobytes(), tuple(int(x) for x in bounds), dict(zip(ROUND1_REC, (int(x) for x in rec)))


def dbg_spans_guard(ctx, idx, mo, queries, plans, segs, rst1, err, bad):
    """mpa_dbg_spans_guard(): the step between the rounds on the device under the guard words of a round that failed (err, bad; one of
    them non-zero).  Returns (n_task, (prep_bound, max_nl, max_al)) -- zeros, whatever rst1 holds -- or (code, message) of an error."""
    f = dbg_lib().mpa_dbg_spans_guard
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MapOpt), C.POINTER(QBatch), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64,
                  C.POINTER(C.c_int32), C.c_void_p]
    keep = [np.ascontiguousarray(x) for x in (plans, segs, rst1)]
    ptr = [x.ctypes.data if len(x) else None for x in keep]
    n_task, bounds = C.c_int32(-1), np.full(3, -1, np.int64)
    rc = f(ctx.h if ctx else None, idx.h, C.byref(mo), C.byref(queries.c), len(plans), ptr[0], len(segs), ptr[1], len(rst1), ptr[2], int(err), int(bad), C.byref(n_task),
           bounds.ctypes.data)
    if rc != 0:
        return int(rc), last_error()
    return n_task.value, tuple(int(x) for x in bounds)


# mpa_dbg_chain_extract (include/mpamd_dbg.h): modes, the columns of a path record, path classes and the reasons for the full list
CHAIN_DENSE, CHAIN_SPARSE_SET, CHAIN_SPARSE_CHAINS = 0, 1, 2
CHAIN_REC = ("m", "n_total", "non_roots", "max_f", "path", "c0", "big_bucket", "why")
CHAIN_FULL_LIST, CHAIN_ONE_LEVEL, CHAIN_TWO_LEVEL, CHAIN_DECLINED = 0, 1, 2, 3
CHAIN_WHY_MIN_CNT, CHAIN_WHY_MIN_SC, CHAIN_WHY_SMALL, CHAIN_WHY_MAX_F, CHAIN_WHY_OTHER = 1, 2, 4, 8, 16


def dbg_chain_extract(ctx, args, probs, mode):
    """mpa_dbg_chain_extract(): the chain extraction on raw anchors.  args: the eleven parameters of mp_chain (max_dist_x, max_dist_y, bw,
    max_skip, max_iter, min_cnt, min_sc, coef_log, is_spliced, kmer, bbit); probs: a list of sorted uint64 anchor arrays, the problems of
    ONE launch; mode: CHAIN_DENSE / CHAIN_SPARSE_SET / CHAIN_SPARSE_CHAINS.  On a context the forward pass and k_chain_extract run on the
    device, through the chaining routes' own carving and launch; ctx None: chain_extract_core with a team of one in work space of the
    kernel's sizes.  Returns (u, a, status, rec): per problem the chains (score << 32 | anchors) and their anchors as lists of arrays,
    status int32 [n_prob] (1: declined), rec int64 [n_prob, 8] with the columns CHAIN_REC."""
    n_prob = len(probs)
    first = np.zeros(n_prob + 1, np.int64)
    np.cumsum([len(p) for p in probs], out=first[1:])
    a = np.ascontiguousarray(np.concatenate(list(probs) + [np.zeros(0, np.uint64)]), dtype=np.uint64)
    n = len(a)
    off_u, off_a = np.zeros(n_prob + 1, np.int64), np.zeros(n_prob + 1, np.int64)
    u, ao = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    status, rec = np.zeros(n_prob + 1, np.int32), np.zeros((n_prob + 1, len(CHAIN_REC)), np.int64)
    f = dbg_lib().mpa_dbg_chain_extract
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] + [C.c_int32] * 7 + [C.c_float] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 6
    rc = f(ctx.h if ctx else None, *args, n_prob, first.ctypes.data, a.ctypes.data, int(mode), off_u.ctypes.data, u.ctypes.data, off_a.ctypes.data, ao.ctypes.data,
           status.ctypes.data, rec.ctypes.data)
    if rc != 0:
        raise MpaError("mpa_dbg_chain_extract: %d: %s" % (rc, last_error()))
    us = [u[off_u[q]:off_u[q + 1]].copy() for q in range(n_prob)]
    as_ = [ao[off_a[q]:off_a[q + 1]].copy() for q in range(n_prob)]
    return us, as_, status[:n_prob].copy(), rec[:n_prob].copy()


def map_batches(ctx, idx, mo, batches, n_threads=1, keep_results=False, want_text=True, claim=None, id0=0):
    """mpa_map_batches(): a stream of Queries batches through the pipelined mapper.  Returns the list of output texts
    (bytes, one per batch; the hit-id counter runs across the batches as in one output file, its first printed hit
    getting id0 + 1); with keep_results the pair
    (texts, [Result]); with want_text=False no text is produced (texts are None).
    claim: mpa_map_batches_claim() -- `batches` is a whole job shared with other processes and claim() returns the index of
    the next batch this process should map (-1: none left); the return value is then (order, texts[, results]) for the
    batches this call mapped, in the order it claimed them."""
    n = len(batches)
    if n == 0:
        return (([], [], []) if keep_results else ([], [])) if claim else (([], []) if keep_results else [])
    qb = (QBatch * n)(*[b.c for b in batches])
    res = (C.c_void_p * n)()
    idc = C.c_int64(int(id0))
    names = text = tlen = None
    if want_text:
        name_arrays = [(C.c_char_p * len(b.names))(*[x.encode() for x in b.names]) for b in batches]
        names = (C.POINTER(C.c_char_p) * n)(*[C.cast(a, C.POINTER(C.c_char_p)) for a in name_arrays])
        text = (C.c_void_p * n)()
        tlen = (C.c_int64 * n)()
    order = None
    if claim is not None:
        err = []
        def _claim(_user):
            try:
                return int(claim())
            except BaseException as e:                          # (an exception must not unwind through the C pipeline)
                err.append(e)
                return -1
        cb = CLAIM_FN(_claim)
        n_mapped = C.c_int32(0)
        order_c = (C.c_int32 * n)()
        f = lib().mpa_map_batches_claim
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                      CLAIM_FN, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f(ctx.h, idx.h, C.byref(mo), n, qb, names, n_threads, res, C.byref(idc) if want_text else None, text, tlen, cb, None, C.byref(n_mapped), order_c))
        if err:
            raise err[0]
        n = n_mapped.value
        order = [int(order_c[k]) for k in range(n)]
    elif want_text:
        _check(lib().mpa_map_batches(ctx.h, idx.h, C.byref(mo), n, qb, names, n_threads, res, C.byref(idc), text, tlen))
    else:
        _check(lib().mpa_map_batches(ctx.h, idx.h, C.byref(mo), n, qb, None, n_threads, res, None, None, None))
    out, results = [], []
    for k in range(n):
        if want_text:
            out.append(C.string_at(text[k], tlen[k]))
            lib().mpa_free(C.c_void_p(text[k]))
        else:
            out.append(None)
        if keep_results:
            results.append(Result(res[k]))
        else:
            lib().mpa_result_destroy(C.c_void_p(res[k]))
    if order is not None:
        return (order, out, results) if keep_results else (order, out)
    return (out, results) if keep_results else out


def map_batches_multi(ctxs, idx, mo, batches, n_threads=1):
    """mpa_map_batches_multi(): one job over several device contexts of THIS process (one pipeline per context, batches claimed
    from a shared counter).  Returns the output texts in input order -- the bytes a single pipeline produces."""
    n = len(batches)
    if n == 0:
        return []
    qb = (QBatch * n)(*[b.c for b in batches])
    res = (C.c_void_p * n)()
    idc = C.c_int64(0)
    name_arrays = [(C.c_char_p * len(b.names))(*[x.encode() for x in b.names]) for b in batches]
    names = (C.POINTER(C.c_char_p) * n)(*[C.cast(a, C.POINTER(C.c_char_p)) for a in name_arrays])
    text = (C.c_void_p * n)()
    tlen = (C.c_int64 * n)()
    hs = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    f = lib().mpa_map_batches_multi
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(len(ctxs), hs, idx.h, C.byref(mo), n, qb, names, n_threads, res, C.byref(idc), text, tlen))
    out = []
    for k in range(n):
        out.append(C.string_at(text[k], tlen[k]))
        lib().mpa_free(C.c_void_p(text[k]))
        lib().mpa_result_destroy(C.c_void_p(res[k]))
    return out


def dp_run(ctx, idx, dpopt, queries, tasks, wide32=False):
    """Run a batch of DP calls on the GPU.  tasks: numpy array of DP_TASK.  Returns (results, cigar_pool).
    wide32: the 32-bit operator (mpa_dp_run32 = ns_global_gs32b per call) instead of the int16 one."""
    tasks = np.ascontiguousarray(tasks, dtype=DP_TASK)
    rst = np.zeros(len(tasks), dtype=DP_RST)
    pool = C.POINTER(C.c_uint32)()
    n_pool = C.c_int64(0)
    fn = lib().mpa_dp_run32 if wide32 else lib().mpa_dp_run
    fn.argtypes = lib().mpa_dp_run.argtypes
    _check(fn(ctx.h, idx.h, C.byref(dpopt), C.byref(queries.c), len(tasks), tasks.ctypes.data,
              rst.ctypes.data, C.byref(pool), C.byref(n_pool)))
    cig = np.ctypeslib.as_array(pool, (max(n_pool.value, 1),))[:n_pool.value].copy() if n_pool.value else np.zeros(0, np.uint32)
    lib().mpa_free(pool)
    return rst, cig
