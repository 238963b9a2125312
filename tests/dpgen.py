"""Deterministic random DP tasks (protein vs. genomic window) exercising every state of the
spliced/frameshift DP: introns in all three phases with canonical and non-canonical signals,
substitutions, amino-acid indels, frameshifts, in-frame stops, N runs, al<8, al%8==0, long flanks."""
import numpy as np

AA = b"ARNDCQEGHILKMFPSTWYV"
# standard genetic code, codon index = n1<<4|n2<<2|n3 with A0 C1 G2 T3
_CODE = {}
_first = "TTTTTTTTTTTTTTTTCCCCCCCCCCCCCCCCAAAAAAAAAAAAAAAAGGGGGGGGGGGGGGGG"
_second = "TTTTCCCCAAAAGGGGTTTTCCCCAAAAGGGGTTTTCCCCAAAAGGGGTTTTCCCCAAAAGGGG"
_third = "TCAGTCAGTCAGTCAGTCAGTCAGTCAGTCAGTCAGTCAGTCAGTCAGTCAGTCAGTCAGTCAG"
_amino = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
_N = {"A": 0, "C": 1, "G": 2, "T": 3}
for a, b, c, m in zip(_first, _second, _third, _amino):
    _CODE.setdefault(m, []).append((_N[a], _N[b], _N[c]))


def back_translate(prot, rng):
    out = []
    for ch in prot:
        cods = _CODE[chr(ch)]
        out.extend(cods[rng.integers(len(cods))])
    return out


def make_task(rng, al=None, max_intron=400, flank=60, p_intron=0.08, p_sub=0.12, p_indel=0.02, p_fs=0.01, p_n=0.002):
    if al is None:
        al = int(rng.choice([rng.integers(1, 9), rng.integers(8, 41), rng.integers(8, 41), rng.integers(40, 130)]))
    prot = bytes(AA[i] for i in rng.integers(0, 20, al))
    nt = []
    for k in range(al):
        cod = list(back_translate(prot[k:k + 1], rng))
        if rng.random() < p_intron:  # intron inside/after this codon at phase ph
            ph = int(rng.integers(0, 3))
            ilen = int(rng.integers(20, max_intron))
            body = list(rng.integers(0, 4, ilen))
            r = rng.random()
            if r < 0.7:
                body[0:2] = [2, 3]
                body[2] = int(rng.choice([0, 2]))
                body[-2:] = [0, 2]
                body[-3] = int(rng.choice([1, 3]))
            elif r < 0.8:
                body[0:2] = [2, 1]
                body[-2:] = [0, 2]
            elif r < 0.9:
                body[0:2] = [0, 3]
                body[-2:] = [0, 1]
            cod = cod[:ph] + body + cod[ph:]
        if rng.random() < p_fs:
            if rng.random() < 0.5:
                cod = cod[:-1]
            else:
                cod = cod + [int(rng.integers(0, 4))]
        nt.extend(cod)
    # the query diverges from the planted protein
    q = bytearray()
    for ch in prot:
        r = rng.random()
        if r < p_sub:
            q.append(AA[rng.integers(0, 20)])
        elif r < p_sub + p_indel:
            continue
        elif r < p_sub + 2 * p_indel:
            q.append(ch)
            q.append(AA[rng.integers(0, 20)])
        else:
            q.append(ch)
    if len(q) == 0:
        q.append(AA[0])
    if rng.random() < 0.05:
        q[int(rng.integers(0, len(q)))] = ord("*")
    if rng.random() < 0.05:
        q[int(rng.integers(0, len(q)))] = ord("X")
    lf = int(rng.integers(0, flank))
    rf = int(rng.integers(0, flank))
    nt = list(rng.integers(0, 4, lf)) + nt + list(rng.integers(0, 4, rf))
    nt = np.array(nt, dtype=np.uint8)
    if len(nt) < 3:
        nt = np.concatenate([nt, rng.integers(0, 4, 3).astype(np.uint8)])
    mask = rng.random(len(nt)) < p_n
    nt[mask] = 4
    return bytes(nt), bytes(q)


def make_ss(rng, nl, density=0.02):
    """A synthetic splice-score track in the reference's encoding (ntseq.c:234-296): 0xff = unset,
    else score+64 << 1 | is_acceptor."""
    ss = np.full(nl, 0xff, dtype=np.uint8)
    idx = np.nonzero(rng.random(nl) < density)[0]
    sc = rng.integers(-10, 15, len(idx))
    acc = rng.integers(0, 2, len(idx))
    ss[idx] = ((sc + 64) << 1 | acc).astype(np.uint8)
    return bytes(ss)


# Scoring points between miniprot's defaults and the limits mpa_dp_run() accepts (dp_plan.cpp: go, io, xdrop <= 32000, ge, fs <= 16000,
# end_bonus <= 1000; the reference's command line takes any -O/-E/-J/-B/--xdrop, main.c:132-150): one parameter at a time, then
# combinations.  Keyword arguments of refbind.DpParams; a point with fs also needs refbind.mapping_matrix(min(fs, 127)).
PENALTY_POINTS = [
    dict(ge=4), dict(ge=40), dict(ge=120), dict(ge=200), dict(ge=255),
    dict(go=200), dict(go=2000), dict(go=20000), dict(go=32000),
    dict(io=200), dict(io=5000), dict(io=32000),
    dict(xdrop=0), dict(xdrop=1), dict(xdrop=2000), dict(xdrop=32000),
    dict(end_bonus=100), dict(end_bonus=1000),
    dict(fs=60), dict(fs=255),
    dict(sp=(40, 60, 80, 100, 12, 12), ie_coef=1.0),
    dict(go=20000, ge=100), dict(ge=250, io=5000, xdrop=32000, end_bonus=1000), dict(io=32000, ge=200),
]

# al on both sides of every lane-class boundary of the DP kernels (extension: 16 / 32 / 64 lanes, 65..128 in one wave, 2 / 4 / 8 / 16
# blocks of 64 columns, then k_ext_huge)
CLASS_EDGES = (8, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)

# Calls at the int16 bound of the packed kernels (dp_plan.cpp, may_saturate: al * max_mat + ncol * ge + max(0, end_bonus) > 32000 or
# go + ncol * ge > 32000, with ncol = 8 * ceil(al / 8)).  (al, parameters, the parameter to raise by one): with BLOSUM62 (max_mat 11)
# the larger of the two sums is exactly 32000 for a call of al columns, and 32001 once `key` is raised by one.  The score sum decides
# the first five, go + ncol * ge the others; the al cover every extension class and every lane class of the checkpointed sweep, with
# and without padded lanes.
BOUND_CASES = [
    (128, dict(ge=239, end_bonus=0), "end_bonus"),
    (136, dict(ge=224, end_bonus=40), "end_bonus"),
    (256, dict(ge=114, end_bonus=0), "end_bonus"),
    (512, dict(ge=51, end_bonus=256), "end_bonus"),
    (1024, dict(ge=20, end_bonus=256), "end_bonus"),
    (16, dict(go=31952, ge=3), "go"),
    (24, dict(go=29600, ge=100), "go"),
    (40, dict(go=31800, ge=5), "go"),
    (64, dict(go=31360, ge=10), "go"),
    (72, dict(go=31424, ge=8), "go"),
    (128, dict(go=31744, ge=2), "go"),
    (300, dict(go=31392, ge=2), "go"),
    (520, dict(go=16400, ge=30), "go"),
    (1024, dict(go=30976, ge=1), "go"),
]


# The same bound for the 2 048- / 3 072-column extension classes (MPA_DP_SPLIT_WIDE, tests/splitwide.py): (al, parameters, the parameter
# to raise by one, cap on the matrix entries or None).  With max_mat 11, or the cap where one is given (splitwide.capped_matrix), the
# larger sum is exactly 32000.  The score sum decides the first six, go + ncol * ge the others.  al 1 032..2 048 is X_SPLIT8's, beyond it
# X_SPLIT12's; with the uncapped matrix and ge = 1 the guard ends at 2 665 residues, so the last column block (2 816..3 071) is live in
# the cases with a cap only: 2 904 reaches into it, 3 072 fills all twelve.  (al * 11 + ncol * ge = 32000 - end_bonus has no solution
# with end_bonus <= 1000 at al = 2 048 or 3 072: 2 000, 2 128 and 2 904 stand in.)
WIDE_BOUND_CASES = [
    (1032, dict(ge=20, end_bonus=8), "end_bonus", None),
    (1600, dict(ge=9, end_bonus=0), "end_bonus", None),
    (2000, dict(ge=5, end_bonus=0), "end_bonus", None),
    (2128, dict(ge=4, end_bonus=80), "end_bonus", None),
    (2664, dict(ge=1, end_bonus=32), "end_bonus", None),
    (2904, dict(ge=1, end_bonus=56), "end_bonus", 10),
    (1032, dict(go=30968, ge=1), "go", None),
    (2048, dict(go=29952, ge=1), "go", None),
    (2600, dict(go=29400, ge=1), "go", None),
    (3072, dict(go=28928, ge=1), "go", 4),
]


def bound_params(case, over):
    """keyword arguments of BOUND_CASES[k] / WIDE_BOUND_CASES[k] with the decisive sum at 32000 + over"""
    al, kw, key = case[:3]
    kw = dict(kw)
    kw[key] += over
    return kw


def long_window(rng, al, p_indel=0.02):
    """a traceback-shaped call of al residues whose window has at least 384 rows (introns and flanks)"""
    while True:
        nt, aa = make_task(rng, al=al, max_intron=1000, flank=400, p_intron=0.05, p_indel=p_indel)
        if len(nt) >= 384:
            return nt, aa
