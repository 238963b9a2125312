"""Guards of the long-protein fixture (tests/longprot.py, tests/golden/long_u.ref.paf): the case has the group counts the device
refinement's size classes are tested at, the reference maps every long query over its full length, and the host stage -- the
yardstick of the operator tests in test_refine_long_gpu.py -- finds a chain at every planted locus.  No GPU."""
import numpy as np
import miniprot_amd as mpa
import golden
import longprot


def test_group_and_kmer_counts_of_the_case():
    c = longprot.case()
    tab = longprot.aa13()
    n_grp = {name: longprot.groups(c["prots"][i], longprot.KMER2, tab) for name, i in c["long"].items()}
    n_kmer = {name: len(longprot.kmer_words(c["prots"][i], longprot.KMER2, tab)) for name, i in c["long"].items()}
    assert n_grp["g2048"] == 2048 and n_grp["g2049"] == 2049              # last LDS class / first of the global map
    assert n_kmer["k4096"] == 4096 and n_kmer["k4097"] == 4097            # the scan-only fallback's LDS set / past it
    assert n_grp["g3000"] == 3000 and n_grp["g9000"] == 9000 and n_grp["g20000"] == 20000
    assert 2049 < n_grp["k4096"] <= 4096 and 2049 < n_grp["k4097"] <= 4097
    assert n_grp["dup300"] > 2049 and n_grp["xstar"] > 2049
    # the duplication: about 300 k-mers occur twice; X and *: every one of the five takes the k-mers that contain it
    assert n_kmer["dup300"] - n_grp["dup300"] >= 200
    xs = c["prots"][c["long"]["xstar"]]
    assert xs.count(b"X") == 3 and xs.count(b"*") == 2 and n_kmer["xstar"] == len(xs) - 4 - (6 + 5 + 5 + 5)
    # ordinary queries of the two small classes, in between the long ones
    og = [longprot.groups(c["prots"][i], longprot.KMER2, tab) for i in c["ordinary"]]
    assert len(og) == 24 and min(og) <= 512 and any(512 < x <= 1024 for x in og) and max(og) <= 1024
    pos = sorted(c["long"].values())
    assert all(b - a == 3 for a, b in zip(pos[:-1], pos[1:]))              # interleaved
    assert len(c["contigs"]) == 1 and len(c["contigs"][0]) == longprot.GENOME


def test_groups_restatement_against_brute_force():
    """kmer_words() / groups() against a set() of k-mer strings over the reduced alphabet, with X, * and lower case inside"""
    tab = longprot.aa13()
    rng = np.random.default_rng(9)
    letters = np.frombuffer(b"ARNDCQEGHILKMFPSTWYVX*arndc", np.uint8)
    for k in (4, 5, 7):
        for n in (0, 3, k, 40, 3000):
            p = bytes(letters[rng.integers(0, len(letters), n)])
            red = [int(tab[ch]) for ch in p]
            brute = {tuple(red[i:i + k]) for i in range(len(red) - k + 1) if max(red[i:i + k]) < 14}
            assert longprot.groups(p, k, tab) == len(brute), (k, n)
            assert len(longprot.kmer_words(p, k, tab)) == sum(1 for i in range(len(red) - k + 1) if max(red[i:i + k]) < 14)


def test_reference_maps_every_long_query_over_its_length():
    c = longprot.case()
    best = {}
    for line in open(golden.path("long_u.ref.paf"), "rb").read().split(b"\n"):
        f = line.split(b"\t")
        if len(f) > 5 and f[5] != b"*":
            best[f[0].decode()] = max(best.get(f[0].decode(), 0.0), (int(f[3]) - int(f[2])) / int(f[1]))
    for name, i in c["long"].items():
        assert len(c["prots"][i]) > 2049
        assert best.get(c["names"][i], 0.0) >= 0.95, (name, best.get(c["names"][i]))


def test_host_leg_chains_every_long_locus():
    """mpa_dbg_refine_chains with ctx = NULL: refine_region_pairs + chain_anchors of the host on the planted locus of every long query"""
    c = longprot.case()
    idx = mpa.Index.from_nt4(c["contigs"], ["chr1"])
    q = mpa.Queries(c["prots"], c["names"])
    names = [n for n, _, _ in longprot.LONG]
    wins = [(c["long"][n],) + c["loci"][n] for n in names] + [(c["long"]["g2048"], 0, 100, 0)]
    off_u, u, off_a, a, flag = mpa.refine_chains(None, idx, longprot.mapopt(), q, wins)
    assert not flag.any() and off_u[-1] == off_u[-2]                       # (an empty window: no chains)
    for k, n in enumerate(names):
        cnt = u[off_u[k]:off_u[k + 1]] & 0xffffffff
        assert len(cnt) > 0 and int(cnt.sum()) == off_a[k + 1] - off_a[k], n
        # the best chain spans most of the query: its anchors' query positions
        qpos = a[off_a[k]:off_a[k + 1]] & 0xffffffff
        assert int(qpos.max()) - int(qpos.min()) > 0.9 * len(c["prots"][c["long"][n]]), n
    idx.close()


def test_model_of_the_global_map():
    """CPU model of the long queries' k-mer table (k_refine_gmap_build / gmap_probe, refine_kernels.hip): open addressing with the hash
    (word * 2654435761) >> (32 - log2 slots), slots = the power of two >= 2 x groups (at least 1 024), linear probing -- in ANY insertion
    order (the kernel's is not defined) every group is found with its own index, a word the query does not have ends at an empty slot,
    and with the table at most half full the walks stay short"""
    c = longprot.case()
    tab = longprot.aa13()
    rng = np.random.default_rng(4)
    for name in ("g2049", "g20000", "dup300"):
        words = sorted(set(longprot.kmer_words(c["prots"][c["long"][name]], longprot.KMER2, tab)))
        lg = 10
        while (1 << lg) < 2 * len(words):
            lg += 1
        assert (1 << lg) >= 2 * len(words) and ((1 << lg) < 4 * len(words) or lg == 10)
        key, val, m = np.full(1 << lg, 0xffffffff, np.uint64), np.zeros(1 << lg, np.int64), (1 << lg) - 1
        for g in rng.permutation(len(words)):
            s = ((words[g] * 2654435761) & 0xffffffff) >> (32 - lg)
            while key[s] != 0xffffffff:
                s = (s + 1) & m
            key[s], val[s] = words[g], g

        def probe(w):
            s, n = ((w * 2654435761) & 0xffffffff) >> (32 - lg), 1
            while key[s] != w and key[s] != 0xffffffff:
                s, n = (s + 1) & m, n + 1
            return (int(val[s]) if key[s] == w else -1), n

        walks = []
        for g, w in enumerate(words):
            got, n = probe(w)
            assert got == g
            walks.append(n)
        have = set(words)
        for w in rng.integers(0, 1 << 20, 2000):
            if int(w) not in have:
                assert probe(int(w))[0] == -1
        assert max(walks) < 64 and sum(walks) / len(walks) < 2.0, (name, max(walks))
