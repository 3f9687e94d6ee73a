"""tests/taxscreen_model.py against itself: `literal` (dictionaries, one getLowestCommonAncestor
per holder, taxdb.hpp:158-190) equals `closed` (the arrays the GPU computes) on random forests,
in any holder order; the parsers on the edges of the NCBI dump format; one report worked by hand
from taxdb.hpp:192-236."""
import numpy as np

import taxscreen_model as T


def nodes_dmp(rows):
    return "".join("%d\t|\t%d\t|\t%s\t|\tXX\t|\t0\t|\n" % r for r in rows).encode()


def names_dmp(rows):
    return "".join("%d\t|\t%s\t|\t%s\t|\t%s\t|\n" % r for r in rows).encode()


def random_forest(rng):
    """-> (nodes, ref_taxids, holders, counts).  TaxID 1, when the dump has it, is a root; some
    trees have another root; some parents have no line; references carry taxID 0 and IDs the
    dump lacks, two of them the same one."""
    n = int(rng.integers(1, 13))
    ids = [int(x) for x in rng.choice(np.arange(2, 60), size=n, replace=False)]
    with_one = rng.random() < 0.6
    if with_one:
        ids[0] = 1
    nodes = {}
    for i, t in enumerate(ids):
        roll = rng.random()
        if i == 0 or roll < 0.15:
            par = t                                   # its own parent: a root
        elif roll < 0.22:
            par = 777                                 # a parent without a line: a root
        else:
            par = ids[int(rng.integers(0, i))]
        nodes[t] = (par, "rank%d" % (i % 3))
    n_ref = int(rng.integers(1, 9))
    pool = ids + ids + [0, 900, 900, 901]
    ref_taxids = [int(rng.choice(pool)) for _ in range(n_ref)]
    holders = []
    for _ in range(int(rng.integers(1, 11))):
        m = int(rng.integers(1, min(n_ref, 5) + 1))
        holders.append([int(x) for x in rng.choice(n_ref, size=m, replace=False)])
    counts = [int(x) for x in rng.integers(0, 3, size=len(holders))]
    return nodes, ref_taxids, holders, counts


def test_literal_equals_closed_on_random_forests():
    rng = np.random.default_rng(2024)
    seen = dict(no_one=0, other_root=0, tax0=0, unknown=0, same_unknown=0, topped=0, forest=0)
    for _ in range(400):
        nodes, ref_taxids, holders, counts = random_forest(rng)
        tax = T.Tax(nodes)
        ref_node = [tax.node_of(t) for t in ref_taxids]
        lit = T.literal(nodes, ref_taxids, holders, counts)
        a = T.literal_as_arrays(tax, lit)
        b = T.closed(tax, ref_node, holders, counts)
        assert T.same(a, b), (nodes, ref_taxids, holders, counts, a, b)
        shuffled = T.literal(nodes, ref_taxids, holders, counts,
                             visit=lambda h: [h[i] for i in rng.permutation(len(h))])
        assert T.same(T.literal_as_arrays(tax, shuffled), a)
        seen["no_one"] += 1 not in nodes
        seen["other_root"] += any(p == t and t != 1 for t, (p, _) in nodes.items())
        seen["forest"] += int((tax.parent == T.ROOT).sum() >= 2)
        seen["tax0"] += any(ref_taxids[k] == 0 for h in holders for k in h)
        seen["unknown"] += any(ref_taxids[k] >= 900 for h in holders for k in h)
        seen["same_unknown"] += any(sum(ref_taxids[k] == 900 for k in h) >= 2 for h in holders)
        seen["topped"] += any(len(h) >= 2 and x == tax.top for h, x in zip(holders, b["lca"]))
    assert all(v >= 10 for v in seen.values()), seen


def test_closed_corners():
    """the `return 1` branches, one by one"""
    nodes = {1: (1, "no rank"), 5: (1, "a"), 6: (5, "b"), 7: (5, "b"), 8: (8, "no rank"), 9: (8, "a")}
    tax = T.Tax(nodes)
    n = tax.index
    lca = lambda ids: T.closed_lca(tax, [tax.node_of(t) for t in ids])     # noqa: E731
    assert lca([]) == T.NONE and lca([0, 0]) == T.NONE
    assert lca([0, 6, 0]) == n[6] and lca([900]) == T.UNKNOWN and lca([8]) == n[8]
    assert lca([6, 7]) == n[5] and lca([6, 5]) == n[5] and lca([6, 6]) == n[6]
    assert lca([5, 9]) == tax.top                 # no common ancestor
    assert lca([8, 8]) == tax.top == n[1]         # the common ancestor is a root
    assert lca([5, 5]) == n[5] and lca([5, 1]) == tax.top        # ... is taxID 1
    assert lca([900, 900]) == tax.top and lca([6, 901]) == tax.top
    for ids in ([6, 7], [5, 9], [8, 8], [9, 9], [900, 900], [6, 901], [5, 1], [8], [900]):
        got, _, _, _ = T.literal(nodes, ids, [list(range(len(ids)))], [1])
        assert tax.node_of(got[0]) == lca(ids), ids
    del nodes[1]                                  # a dump without taxID 1
    tax = T.Tax(nodes)
    assert tax.top == T.UNKNOWN
    assert T.closed_lca(tax, [tax.node_of(5), tax.node_of(9)]) == T.UNKNOWN
    got, counts_of, total, total_hashes = T.literal(nodes, [5, 9], [[0, 1]], [1])
    assert got == [1] and (total, total_hashes) == (1, 1) and counts_of[1][2:] == [0, 0]


HAND_NODES = [(1, 1, "no rank"), (2, 1, "superkingdom"), (10, 2, "family"), (21, 10, "genus"),
              (20, 10, "genus"), (30, 20, "species"), (31, 21, "species"), (40, 2, "species"),
              (50, 2, "species")]
HAND_NAMES = [(1, "root", "", "scientific name"), (2, "Bacteria", "Bacteria <bacteria>",
                                                   "scientific name"),
              (10, "Fam", "", "scientific name"), (20, "GenA", "", "scientific name"),
              (21, "GenB", "", "scientific name"), (30, "SpA1", "", "scientific name"),
              (31, "SpB1", "", "scientific name"), (40, "Other", "", "scientific name"),
              (50, "Lone", "", "scientific name")]
HAND_REFS = [30, 20, 31, 40, 999, 50]
# (holders, count in the pool) per distinct hash
HAND_ENTRIES = [([0], 3), ([0, 1], 1), ([0, 2], 2), ([2], 0), ([2], 5), ([3], 1), ([4], 4),
                ([5], 0), ([0, 3], 1), ([3, 4], 0), ([1], 2), ([2], 1), ([2], 1)]
# Worked by hand.  LCAs: 30, 20, 10, 31, 31, 40, 999, 50, 2, 1, 20, 31, 31.  Ten entries were seen
# in the pool (the denominator), one of them lost to the unknown 999.  Clade sums (hashes,
# hashesDB): 30 (1, 1); 20 (3, 3); 31 and 21 (3, 4); 10 (7, 8); 40 (1, 1); 50 (0, 1): not printed;
# 2 (9, 11); 1 (9, 12).  20 and 21 tie at 3: ascending taxID, though 21 comes first in the dump.
HAND_REPORT = (
    "%\thashes\ttaxHashes\thashesDB\ttaxHashesDB\ttaxID\trank\tname\n"
    "90.0000\t9\t0\t12\t1\tno rank\t1\troot\n"
    "90.0000\t9\t1\t11\t1\tsuperkingdom\t2\t  Bacteria\n"
    "70.0000\t7\t1\t8\t1\tfamily\t10\t    Fam\n"
    "30.0000\t3\t2\t3\t2\tgenus\t20\t      GenA\n"
    "10.0000\t1\t1\t1\t1\tspecies\t30\t        SpA1\n"
    "30.0000\t3\t0\t4\t0\tgenus\t21\t      GenB\n"
    "30.0000\t3\t3\t4\t4\tspecies\t31\t        SpB1\n"
    "10.0000\t1\t1\t1\t1\tspecies\t40\t    Other\n")


def test_hand_made_report():
    nodes = T.parse_nodes(nodes_dmp(HAND_NODES))
    tax = T.Tax(nodes, T.parse_names(names_dmp(HAND_NAMES), nodes))
    holders = [h for h, _ in HAND_ENTRIES]
    counts = [c for _, c in HAND_ENTRIES]
    lit = T.literal(nodes, HAND_REFS, holders, counts)
    assert lit[0] == [30, 20, 10, 31, 31, 40, 999, 50, 2, 1, 20, 31, 31]
    assert (lit[2], lit[3]) == (10, 13)
    r = T.closed(tax, [tax.node_of(t) for t in HAND_REFS], holders, counts)
    assert T.same(T.literal_as_arrays(tax, lit), r)
    assert T.report(tax, r) == HAND_REPORT
    assert r["clade_hashes"][tax.index[50]] == 1 and r["clade_count"][tax.index[50]] == 0


def test_report_without_taxid_1_is_the_header():
    nodes = {5: (5, "a"), 6: (5, "b")}
    tax = T.Tax(nodes)
    r = T.closed(tax, [tax.node_of(6)], [[0]], [2])
    assert r["clade_count"].tolist() == [1, 1] and T.report(tax, r) == T.HEADER


# ---- parsers ----------------------------------------------------------------------------------
def test_nodes_duplicate_line_first_wins():
    nodes = T.parse_nodes(nodes_dmp([(1, 1, "no rank"), (7, 1, "genus"), (7, 9, "species"),
                                     (9, 1, "family")]))
    assert nodes == {1: (1, "no rank"), 7: (1, "genus"), 9: (1, "family")}
    assert list(nodes) == [1, 7, 9]


def test_nodes_missing_parent_is_a_root_and_cycles_raise():
    tax = T.Tax(T.parse_nodes(nodes_dmp([(1, 1, "no rank"), (7, 1234, "genus"), (8, 7, "species")])))
    assert tax.parent.tolist() == [T.ROOT, T.ROOT, 1] and tax.depth.tolist() == [0, 0, 1]
    import pytest
    with pytest.raises(ValueError):
        T.Tax(T.parse_nodes(nodes_dmp([(1, 1, "no rank"), (7, 8, "a"), (8, 7, "b")])))


def test_names_classes_last_scientific_name_and_missing():
    nodes = T.parse_nodes(nodes_dmp([(1, 1, "no rank"), (7, 1, "genus"), (9, 1, "family")]))
    names = T.parse_names(names_dmp([
        (1, "all", "", "synonym"), (1, "root", "", "scientific name"),
        (7, "Old name", "", "scientific name"), (7, "Bacillus", "Bacillus <firmicutes>",
                                                 "scientific name"),
        (7, "bacilli", "", "common name"), (9, "only a synonym", "", "synonym"),
        (55, "nobody", "", "scientific name")]), nodes)
    assert names == {1: "root", 7: "Bacillus", 9: ""}


def test_comment_taxids():
    assert T.comment_taxid("") == 0 and T.comment_taxid("no number here") == 0
    assert T.comment_taxid("[1 seqs] taxid 562 Escherichia coli") == 562
    assert T.comment_taxid("taxid 562 then taxid 1280") == 1280      # the last one wins
    assert T.comment_taxid("Escherichia taxid") == 0                 # a comment ending in taxid
    assert T.comment_taxid("taxid 562 more taxid") == 0              # ... ends the scan with 0
    assert T.comment_taxid("taxid abc taxid 7") == 0                 # a failed read ends it
    assert T.comment_taxid("taxid 562, strain K12") == 562
    assert T.comment_taxid("taxid=562 Taxid 3") == 0                 # whole words only


def test_mapping_names_with_spaces_and_first_line_wins():
    m = T.parse_mapping(b"562\tg0.fa\n1280 my genome v2.fa\n\n9\tg0.fa\n7\tlast")
    assert m == {"g0.fa": 562, "my genome v2.fa": 1280, "last": 7}
    assert T.parse_mapping(b"12\tok\nnot a number\n5\tnever read\n") == {"ok": 12}
    ids = T.reference_taxids(["g0.fa", "other", "my genome v2.fa", "none"],
                             ["taxid 5", "x taxid 77", "", "nothing"], m)
    assert ids == [562, 77, 1280, 0]
