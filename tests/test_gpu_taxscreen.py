"""`taxscreen` on the GPU (fpm_screen_tax: one LCA fold per entry of U, the tallies and the clade
sums) against tests/taxscreen_model.py: `closed` everywhere, `literal` (one
getLowestCommonAncestor per holder, taxdb.hpp:158-190) on every case here as well, since all of
them are small.  out_lca, the four per-node arrays and the totals are integers: bit-exact.

Every database is built from a list of posting lists (the references that hold entry j); the
counters are set through Screen.add_hashes, without sequence.  References 0..69 have taxID 0
(FPM_TAX_NONE), 70..72 the taxIDs UNK_A, UNK_A and UNK_B, which no dump here has
(FPM_TAX_UNKNOWN), 73..299 a taxon of the tree."""
import numpy as np
import pytest

import screen_model as SM
import taxscreen_model as T

pytestmark = pytest.mark.gpu

N_REF, N_NONE, N_UNK = 300, 70, 3
REAL = list(range(N_NONE + N_UNK, N_REF))
UNK_A, UNK_B = 9000001, 9000002


def hash_of(j):
    return (j + 1) * (2 ** 33) + 7


def database(entries):
    """rows of N_REF references for posting lists `entries`; entry j of U is list j"""
    rows = [[] for _ in range(N_REF)]
    for j, hold in enumerate(entries):
        assert len(set(hold)) == len(hold)
        for i in hold:
            rows[i].append(hash_of(j))
    return [np.array(r, np.uint64) for r in rows]


def run_case(ctx, nodes, ref_taxids, entries, counts, kernel=None, literal=True, rows=None):
    """fpm_screen_tax over the case -> its result, checked against closed (and literal)"""
    import fpmash
    tax = T.Tax(nodes)
    ref_node = np.array([tax.node_of(t) for t in ref_taxids], np.uint32)
    rows = database(entries) if rows is None else rows
    keys = np.repeat(np.array([hash_of(j) for j in range(len(entries))], np.uint64),
                     np.asarray(counts, np.int64))
    sc = fpmash.Screen.from_lists(ctx, rows, 1000)
    try:
        sc.add_hashes(keys)
        U, cnt = sc.counts()
        eU, holders = T.holders_of(rows)
        assert np.array_equal(U, eU) and [sorted(h) for h in entries] == holders
        assert cnt.tolist() == list(counts)
        before = [x.tolist() for x in sc.rows()]
        got = sc.tax(tax.parent, tax.top, ref_node)
        exp = T.closed(tax, ref_node, holders, cnt)
        for k in ("lca", "tax_hashes", "tax_count", "clade_hashes", "clade_count"):
            assert np.array_equal(got[k], exp[k]), (k, np.nonzero(got[k] != exp[k])[0][:10])
        assert (got["total_count"], got["total_hashes"]) == (exp["total_count"], len(entries))
        if literal:
            lit = T.literal_as_arrays(tax, T.literal(nodes, ref_taxids, holders, cnt))
            assert T.same(lit, exp)
        if kernel is not None:
            assert ctx.last_tax_kernel() == kernel
        # the counters are left as they were
        assert [x.tolist() for x in sc.rows()] == before
        assert np.array_equal(sc.counts()[1], cnt)
        got["tax"] = tax
        return got
    finally:
        sc.free()


# ---- trees --------------------------------------------------------------------------------------
def tree_single_root():
    return {1: (1, "no rank")}


def tree_depth_1():
    nodes = {1: (1, "no rank")}
    nodes.update({t: (1, "species") for t in range(2, 12)})
    return nodes


def tree_chain(n=4096):
    nodes = {1: (1, "no rank")}
    nodes.update({t: (t - 1, "clade") for t in range(2, n + 1)})
    return nodes


def tree_forest():
    """three trees: under taxID 1, under 100 (its own parent) and under 200 (its parent has no
    line); genera and species below each"""
    nodes = {1: (1, "no rank"), 100: (100, "no rank"), 200: (5555, "no rank")}
    t = 2
    for root in (1, 100, 200):
        for _ in range(3):
            genus = root * 1000 + t
            nodes[genus] = (root, "genus")
            for _ in range(3):
                t += 1
                nodes[root * 1000 + 500 + t] = (genus, "species")
            t += 1
    return nodes


def ref_taxids_over(nodes, rng, pick=None):
    ids = list(nodes)
    real = [int(x) for x in (pick if pick is not None else rng.choice(ids, size=len(REAL)))]
    return [0] * N_NONE + [UNK_A, UNK_A, UNK_B] + real


def shaped_entries(rng, cut):
    """posting lists of 1, 2, 63, 64, 65 holders and of the cut - 1, the cut and the cut + 1,
    over references with a taxon; lists over every kind of reference; only NONE holders; one
    and two UNKNOWN holders among NONE ones; one hash held by all 300 references"""
    e = []
    for n in sorted({1, 2, 63, 64, 65, cut - 1, cut, cut + 1, 200}):
        for _ in range(3):
            e.append([int(x) for x in rng.choice(REAL, size=n, replace=False)])
        e.append([int(x) for x in rng.choice(N_REF, size=n, replace=False)])
    for n in (1, 2, cut + 6):
        e.append(list(range(n)))                                  # only NONE
        e.append(list(range(n - 1)) + [N_NONE])                   # one UNKNOWN
        e.append(list(range(n - 1)) + [N_NONE + 2])
    for n in (2, cut + 6):
        e.append(list(range(n - 2)) + [N_NONE, N_NONE + 1])       # the same unknown ID twice
        e.append(list(range(n - 2)) + [N_NONE, N_NONE + 2])       # two unknown IDs
        e.append(list(range(n - 2)) + [N_NONE, REAL[0]])          # an unknown and a known one
    e.append(list(range(N_REF)))
    return e


def counts_for(rng, n):
    c = rng.integers(0, 4, size=n)
    c[:3] = [1, 0, 3]
    return [int(x) for x in c]


@pytest.mark.parametrize("shape", ["single_root", "depth_1", "chain", "forest"])
def test_tree_shapes(ctx, shape):
    import fpmash
    rng = np.random.default_rng(len(shape))
    nodes = {"single_root": tree_single_root, "depth_1": tree_depth_1, "chain": tree_chain,
             "forest": tree_forest}[shape]()
    pick = None
    if shape == "chain":
        # holders at both ends and in the middle of the 4,096 nodes
        pick = rng.choice([1, 2, 3, 2047, 2048, 2049, 4094, 4095, 4096], size=len(REAL))
    ref_taxids = ref_taxids_over(nodes, rng, pick)
    entries = shaped_entries(rng, ctx.tax_wave_cut())
    if shape == "forest":
        # two species of one genus, and a species with its own genus
        sp = [i for i in REAL if ref_taxids[i] in (1504, 1505)]
        a, b = [i for i in sp if ref_taxids[i] == 1504], [i for i in sp if ref_taxids[i] == 1505]
        g = [i for i in REAL if ref_taxids[i] == 1002]
        assert a and b and g
        entries += [[a[0], b[0]], [a[0], g[0]]]
    if shape == "chain":
        ends = [REAL[i] for i in range(len(REAL)) if ref_taxids[REAL[i]] in (4096, 4095)]
        mid = [REAL[i] for i in range(len(REAL)) if ref_taxids[REAL[i]] in (2047, 2048, 2049)]
        assert len(ends) >= 2 and len(mid) >= 2
        entries += [ends[:1], ends[:2], ends[:1] + mid[:1], mid[:2]]
    got = run_case(ctx, nodes, ref_taxids, entries, counts_for(rng, len(entries)),
                   kernel=fpmash.TK_WAVE)
    tax = got["tax"]
    lca = got["lca"]
    assert T.NONE in lca and T.UNKNOWN in lca and tax.top in lca
    if shape == "chain":
        assert int(tax.depth[lca[-4]]) >= 4094 and 2000 < int(tax.depth[lca[-1]]) < 2100
    if shape == "forest":
        assert lca[-2] == lca[-1] == tax.index[1002] and tax.depth[lca[-1]] == 1
        assert int((tax.parent == T.ROOT).sum()) == 3


def test_wave_cut_both_sides(ctx):
    """the longest list one short of the cut: every list by one lane; at the cut: by a wave.
    Both give the model's result, and the same one for the lists they share."""
    import fpmash
    cut = ctx.tax_wave_cut()
    rng = np.random.default_rng(cut)
    nodes = tree_forest()
    genus = [1002, 1503, 1504, 1505]                       # one genus and its three species
    pick = [int(x) for x in rng.choice(genus, size=cut + 8)] + \
        [int(x) for x in rng.choice(list(nodes), size=len(REAL) - cut - 8)]
    ref_taxids = ref_taxids_over(nodes, rng, pick)
    under_one = REAL[:cut + 8]
    assert len({ref_taxids[i] for i in under_one[:cut - 1]}) > 1
    short = [[int(x) for x in rng.choice(REAL, size=n, replace=False)]
             for n in (1, 2, cut - 2, cut - 1, cut - 1)] + [under_one[:cut - 1]]
    counts = counts_for(rng, len(short))
    a = run_case(ctx, nodes, ref_taxids, short, counts, kernel=fpmash.TK_THREAD)
    long_ = short + [under_one[:cut], under_one[:cut + 1],
                     [int(x) for x in rng.choice(REAL, size=cut, replace=False)]]
    b = run_case(ctx, nodes, ref_taxids, long_, counts + [2, 0, 1], kernel=fpmash.TK_WAVE)
    assert np.array_equal(a["lca"], b["lca"][:len(short)])
    # a long list inside one tree keeps a real ancestor: the wave's answer is not just `top`
    tax = b["tax"]
    assert b["lca"][len(short)] == b["lca"][len(short) + 1] == tax.index[1002]


def test_one_hash_held_by_300_references_of_one_genus(ctx):
    import fpmash
    nodes = {1: (1, "no rank"), 2: (1, "family"), 3: (2, "genus"), 4: (2, "genus")}
    nodes.update({t: (3, "species") for t in range(10, 40)})
    rng = np.random.default_rng(300)
    ref_taxids = [int(x) for x in rng.integers(10, 40, size=N_REF)]
    got = run_case(ctx, nodes, ref_taxids, [list(range(N_REF)), [0], [5, 9]], [1, 1, 0],
                   kernel=fpmash.TK_WAVE)
    tax = got["tax"]
    assert got["lca"][0] == tax.index[3] and got["tax_count"][tax.index[3]] == 1
    assert got["clade_count"][tax.index[2]] == 2 and got["clade_hashes"][tax.index[1]] == 3


def test_top_absent(ctx):
    """a dump without taxID 1: what the reference's `return 1` names is no taxon; such entries
    only count in the totals"""
    rng = np.random.default_rng(8)
    nodes = {t: p for t, p in tree_forest().items() if t != 1}
    ref_taxids = ref_taxids_over(nodes, rng)
    entries = shaped_entries(rng, ctx.tax_wave_cut())
    got = run_case(ctx, nodes, ref_taxids, entries, counts_for(rng, len(entries)))
    assert got["tax"].top == T.UNKNOWN
    assert got["total_hashes"] > int(got["tax_hashes"].sum())


def test_counters_zero_and_one(ctx):
    nodes = tree_depth_1()
    rng = np.random.default_rng(4)
    ref_taxids = ref_taxids_over(nodes, rng)
    entries = [[REAL[0]], [REAL[1], REAL[2]], [REAL[3]]]
    got = run_case(ctx, nodes, ref_taxids, entries, [0, 0, 0])
    assert got["total_count"] == 0 and not got["tax_count"].any() and not got["clade_count"].any()
    assert got["tax_hashes"].sum() == 3 and got["clade_hashes"][0] == 3
    got = run_case(ctx, nodes, ref_taxids, entries, [0, 1, 0])
    assert got["total_count"] == 1 and got["tax_count"].sum() == 1 and got["clade_count"][0] == 1


@pytest.mark.parametrize("taxid", [1, 7])
def test_one_node(ctx, taxid):
    """n_nodes == 1, as taxID 1 (top is the node) and as another taxID (top absent)"""
    nodes = {taxid: (taxid, "no rank")}
    ref_taxids = [0] * N_NONE + [UNK_A, UNK_A, UNK_B] + [taxid] * len(REAL)
    entries = [[REAL[0]], [REAL[0], REAL[1]], [0], [N_NONE], list(range(N_REF))]
    got = run_case(ctx, nodes, ref_taxids, entries, [1, 1, 1, 1, 1])
    top = 0 if taxid == 1 else T.UNKNOWN
    assert got["lca"].tolist() == [0, top, T.NONE, T.UNKNOWN, top]
    assert got["tax_hashes"].tolist() == ([3] if taxid == 1 else [1]) and got["total_count"] == 5


def test_no_references(ctx):
    import fpmash
    sc = fpmash.Screen.from_lists(ctx, [], 1000)
    try:
        got = sc.tax(np.array([T.ROOT, 0], np.uint32), 0, np.zeros(0, np.uint32))
        assert len(got["lca"]) == 0 and (got["total_count"], got["total_hashes"]) == (0, 0)
        assert not got["tax_hashes"].any() and not got["clade_hashes"].any()
        assert ctx.last_tax_kernel() == fpmash.TK_NONE
    finally:
        sc.free()


def test_invalid_taxonomies_launch_nothing(ctx):
    import fpmash
    rows = [np.array([5, 9], np.uint64), np.array([9], np.uint64)]
    sc = fpmash.Screen.from_lists(ctx, rows, 1000)
    ctx.set_timing(True)
    try:
        ok = sc.tax([T.ROOT, 0, 1], 0, [1, 2])
        assert ok["lca"].tolist() == [1, 1] and ctx.last_tax_kernel() == fpmash.TK_THREAD
        ctx.reset_timing()
        for parent, top, ref_node in (
                ([1, 0], T.UNKNOWN, [0, 1]),                  # a two-node cycle
                ([T.ROOT, 2, 3, 3], 0, [1, 1]),               # a chain that ends in a self-reference
                ([T.ROOT, 0], 0, [2, 0]),                     # a ref_node out of range
                ([T.ROOT, 0], 0, [0, 0xFFFFFFFD]),
                ([T.ROOT, 2], 0, [0, 0]),                     # a parent index out of range
                ([T.ROOT, 0], 2, [0, 0])):                    # a top that is no node
            with pytest.raises(fpmash.FpmError) as e:
                sc.tax(parent, top, ref_node)
            assert e.value.code == fpmash.FPM_EINVAL
        assert ctx.kernel_time(fpmash.K_COMPARE)[1] == 0 and ctx.kernel_time(fpmash.K_FINALIZE)[1] == 0
        assert ctx.last_tax_kernel() == fpmash.TK_THREAD
        assert sc.tax([T.ROOT, 0, 1], 0, [1, 2])["lca"].tolist() == [1, 1]
        assert ctx.kernel_time(fpmash.K_COMPARE)[1] == 1
    finally:
        ctx.set_timing(False)
        sc.free()


def test_context_taxscreen(ctx, oracle):
    """Context.taxscreen end to end: the pool pass, then the fold"""
    import fpmash
    import reads_model as RM
    reads = RM.base_reads()[:60]
    keys = RM.window_hashes(oracle, reads, 21)
    distinct = np.unique(np.asarray(keys, np.uint64))
    db = [distinct[:300], distinct[100:500:2], distinct[250:320], np.array([5, 6], np.uint64)]
    nodes = {1: (1, "no rank"), 2: (1, "genus"), 3: (2, "species"), 4: (2, "species"),
             5: (1, "species")}
    tax = T.Tax(nodes)
    ref_taxids = [3, 4, 5, 0]
    ref_node = [tax.node_of(t) for t in ref_taxids]
    got = ctx.taxscreen(fpmash.make_params(k=21, s=1000), db, reads, tax.parent, tax.top,
                        ref_node, slices=2)
    U, cnt = SM.closed_counts(db, keys)
    exp = T.closed(tax, ref_node, T.holders_of(db)[1], cnt)
    got_r = {k: got[k] for k in exp}
    assert T.same(got_r, exp) and got["set_size"] == SM.set_size(keys, 1000)
    assert {tax.index[2], tax.top, T.NONE} <= set(exp["lca"].tolist())
