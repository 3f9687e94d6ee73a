"""`taxscreen` checker: what CommandTaxScreen.cpp:107-441 and taxdb.hpp:26-236 do after the pool
pass, restated on the CPU.  The pool pass itself is screen's (tests/screen_model.py).

The contract is coded twice: `literal` keeps dictionaries of taxon objects and calls one
getLowestCommonAncestor per holder, line by line, `return 1` branches included; `closed` is the
form the GPU computes, over dense node arrays.  tests/test_taxscreen_model.py compares the two.

Rules that replace undefined behaviour in the reference:
  * the clade loop (:408-437) inserts into the map it iterates; here every taxon with a direct
    tally is visited exactly once;
  * std::sort of a taxon's children (taxdb.hpp:227) is unstable; ties in cladeCount keep ascending
    taxID;
  * a node whose parent has no line in nodes.dmp keeps an uninitialised pointer (taxdb.hpp:37,
    :92-94); here it is a root;
  * the fold visits an unordered set; the closed form does not depend on the order.  (The
    reference's own result does when a node of taxID 0 or 1 has a parent, since only the path
    of `a` stops there, :176 against :183; no NCBI dump has such a node, the closed form holds
    there too, and the random forests of the tests keep taxIDs 0 and 1 at roots.)
"""
import numpy as np

ROOT = 0xFFFFFFFF
NONE = 0xFFFFFFFF
UNKNOWN = 0xFFFFFFFE
_WS = b" \t\n\v\f\r"
HEADER = "%\thashes\ttaxHashes\thashesDB\ttaxHashesDB\ttaxID\trank\tname\n"     # taxdb.hpp:206


# ---- a byte cursor with the istream calls the parsers use -------------------------------------
class _In:
    def __init__(self, data):
        self.b, self.at = bytes(data), 0

    def uint(self):
        """operator>>(uint64_t&): skips white space; None when no digits follow (the stream
        fails) or the value does not fit"""
        b, n = self.b, len(self.b)
        while self.at < n and b[self.at] in _WS:
            self.at += 1
        at = self.at
        if at < n and b[at] == ord("+"):
            at += 1
        end = at
        while end < n and 48 <= b[end] <= 57:
            end += 1
        if end == at:
            return None
        self.at = end
        v = int(b[at:end])
        return v if v < 2 ** 64 else None

    def char(self):
        """operator>>(char&)"""
        while self.at < len(self.b) and self.b[self.at] in _WS:
            self.at += 1
        if self.at >= len(self.b):
            return None
        self.at += 1
        return self.b[self.at - 1]

    def ignore(self, n=1, delim=None):
        end = min(len(self.b), self.at + n)
        if delim is not None:
            i = self.b.find(delim, self.at, end)
            if i >= 0:
                end = i + 1
        self.at = end

    def upto(self, delim):
        """getline(in, s, delim)"""
        i = self.b.find(delim, self.at)
        if i < 0:
            s, self.at = self.b[self.at:], len(self.b)
        else:
            s, self.at = self.b[self.at:i], i + 1
        return s


# ---- parsers ----------------------------------------------------------------------------------
def parse_nodes(data):
    """parseNodesDump, taxdb.hpp:105-127 -> {taxID: (parent taxID, rank)} in file order; the
    first line of a taxID wins (emplace)"""
    f, out = _In(data), {}
    while True:
        tid = f.uint()
        if tid is None or f.char() is None:
            break
        par = f.uint()
        if par is None or f.char() is None:
            break
        f.ignore(1)
        rank = f.upto(b"\t")
        out.setdefault(tid, (par, rank.decode()))
        f.ignore(2560, b"\n")
    return out


def parse_names(data, nodes):
    """parseNamesDump, taxdb.hpp:129-156 -> {taxID: name}: only `scientific name` lines, the
    last one wins; taxa without one have the empty name"""
    f, out = _In(data), {t: "" for t in nodes}
    while True:
        tid = f.uint()
        if tid is None:
            break
        f.ignore(3)
        name = f.upto(b"\t")
        f.ignore(3)
        f.ignore(256, b"|")
        f.ignore(1)
        kind = f.upto(b"\t")
        if kind == b"scientific name" and tid in out:
            out[tid] = name.decode()
        f.ignore(2560, b"\n")
    return out


def parse_mapping(data):
    """CommandTaxScreen.cpp:137-142 -> {reference name: taxID}, the first line of a name wins"""
    f, out = _In(data), {}
    while True:
        tid = f.uint()
        if tid is None:
            break
        f.ignore(1)
        out.setdefault(f.upto(b"\n").decode(), tid)
    return out


def comment_taxid(comment):
    """:163-170: the number after each word `taxid`, the last one wins; a failed read stores 0
    and ends the scan"""
    f = _In(comment.encode() if isinstance(comment, str) else comment)
    tid = 0
    while True:
        while f.at < len(f.b) and f.b[f.at] in _WS:
            f.at += 1
        at = f.at
        while f.at < len(f.b) and f.b[f.at] not in _WS:
            f.at += 1
        if f.at == at:
            return tid
        if f.b[at:f.at] == b"taxid":
            v = f.uint()
            if v is None:
                return 0
            tid = v


def reference_taxids(names, comments, mapping=None):
    """:127-180 -> one taxID per reference (0: none found)"""
    out = []
    for name, comment in zip(names, comments):
        tid = (mapping or {}).get(name, 0)
        if tid == 0:
            tid = comment_taxid(comment)
        out.append(tid)
    return out


# ---- the taxonomy as dense arrays -------------------------------------------------------------
class Tax:
    """nodes in nodes.dmp order: ids, rank, name, parent (index or ROOT), depth, top (the node
    of taxID 1 or UNKNOWN).  A cycle in the parent links raises ValueError."""

    def __init__(self, nodes, names=None):
        self.ids = list(nodes)
        self.index = {t: i for i, t in enumerate(self.ids)}
        self.rank = [nodes[t][1] for t in self.ids]
        self.name = [(names or {}).get(t, "") for t in self.ids]
        self.parent = np.array([ROOT if nodes[t][0] == t or nodes[t][0] not in self.index
                                else self.index[nodes[t][0]] for t in self.ids], np.uint32)
        self.depth = depths(self.parent)
        self.top = self.index.get(1, UNKNOWN)

    def node_of(self, taxid):
        return NONE if taxid == 0 else self.index.get(taxid, UNKNOWN)


def depths(parent):
    n = len(parent)
    depth = np.full(n, -1, np.int64)
    for v in range(n):
        if depth[v] >= 0:
            continue
        path, x = [], v
        while True:
            if len(path) > n:
                raise ValueError("the parent links hold a cycle")
            path.append(x)
            p = int(parent[x])
            if p == ROOT:
                base = 0
                break
            if depth[p] >= 0:
                base = int(depth[p]) + 1
                break
            x = p
        for i, y in enumerate(reversed(path)):
            depth[y] = base + i
    return depth.astype(np.uint32)


# ---- literal: dictionaries and one getLowestCommonAncestor per holder ---------------------------
class _Entry:
    def __init__(self, taxid):
        self.taxID, self.parent = taxid, None


def literal_entries(nodes):
    """TaxDB::TaxDB, taxdb.hpp:85-100 (a missing parent: a root)"""
    entries = {t: _Entry(t) for t in nodes}
    for t, (par, _) in nodes.items():
        if t != par and par in entries:
            entries[t].parent = entries[par]
    return entries


def literal_lca(entries, a, b):
    """getLowestCommonAncestor, taxdb.hpp:158-190"""
    if b == 0:
        return a
    if a == 0:
        return b
    if a not in entries:
        return 1
    if b not in entries:
        return 1
    a_path = set()
    pta = entries[a]
    while pta is not None and pta.taxID > 1 and pta.parent is not None:
        if pta.taxID == b:
            return b
        a_path.add(pta)
        pta = pta.parent
    ptb = entries[b]
    while ptb.taxID > 0 and ptb.parent is not None:
        if ptb in a_path:
            return ptb.taxID
        ptb = ptb.parent
    return 1


def literal(nodes, ref_taxids, holders, counts, visit=None):
    """CommandTaxScreen.cpp:386-437 -> (lca taxID per entry, {taxID: [taxCount, taxHashCount,
    cladeCount, cladeHashCount]}, totalCount, totalHashCount).  holders[u]: the references that
    hold entry u; visit reorders a holder list (the reference's unordered set)."""
    entries = literal_entries(nodes)
    lca, counts_of = [], {}
    for u, hold in enumerate(holders):
        tid = 0
        for k in (visit(list(hold)) if visit else hold):
            tid = literal_lca(entries, ref_taxids[k], tid)
        lca.append(tid)
        c = counts_of.setdefault(tid, [0, 0, 0, 0])
        c[1] += 1
        if counts[u] >= 1:
            c[0] += 1
    total = total_hashes = 0
    for tid, c in list(counts_of.items()):        # each directly tallied taxon once
        total_hashes += c[1]
        total += c[0]
        taxon = entries.get(tid)                    # getEntry: None for 0 and unknown IDs
        while taxon is not None:
            d = counts_of.setdefault(taxon.taxID, [0, 0, 0, 0])
            d[2] += c[0]
            d[3] += c[1]
            taxon = taxon.parent
    return lca, counts_of, total, total_hashes


# ---- closed form: dense arrays ----------------------------------------------------------------
def _common(tax, a, b):
    """the deepest common ancestor of nodes a and b, None in different trees"""
    da, db = int(tax.depth[a]), int(tax.depth[b])
    while da > db:
        a, da = int(tax.parent[a]), da - 1
    while db > da:
        b, db = int(tax.parent[b]), db - 1
    while a != b and da > 0:
        a, b, da = int(tax.parent[a]), int(tax.parent[b]), da - 1
    return a if a == b else None


def closed_lca(tax, nodes_of_holders):
    t = [x for x in nodes_of_holders if x != NONE]
    if not t:
        return NONE
    if len(t) == 1:
        return t[0]
    if UNKNOWN in t:
        return tax.top
    cur = t[0]
    for x in t[1:]:
        cur = _common(tax, cur, x)
        if cur is None:
            return tax.top
    return tax.top if tax.depth[cur] == 0 else cur


def closed(tax, ref_node, holders, counts):
    """-> dict like fpmash.Screen.tax's"""
    n = len(tax.ids)
    lca = np.array([closed_lca(tax, [int(ref_node[k]) for k in hold]) for hold in holders] or [],
                   np.uint32).reshape(-1)
    counts = np.asarray(counts, np.uint32)
    seen = counts >= 1
    hit = lca < n
    th = np.bincount(lca[hit], minlength=n).astype(np.uint32)[:max(n, 0)]
    tc = np.bincount(lca[hit & seen], minlength=n).astype(np.uint32)[:max(n, 0)]
    ch, cc = th.astype(np.int64), tc.astype(np.int64)
    for v in sorted(range(n), key=lambda v: -int(tax.depth[v])):       # deepest first
        p = int(tax.parent[v])
        if p != ROOT:
            ch[p] += ch[v]
            cc[p] += cc[v]
    return {"lca": lca, "tax_hashes": th, "tax_count": tc, "clade_hashes": ch.astype(np.uint32),
            "clade_count": cc.astype(np.uint32), "total_count": int(seen.sum()),
            "total_hashes": len(holders)}


def literal_as_arrays(tax, lit):
    """literal's result in closed's form"""
    lca, counts_of, total, total_hashes = lit
    n = len(tax.ids)
    arr = np.zeros((4, n), np.uint32)
    for tid, c in counts_of.items():
        if tid in tax.index:
            arr[:, tax.index[tid]] = c
    return {"lca": np.array([tax.node_of(t) for t in lca], np.uint32).reshape(-1),
            "tax_count": arr[0], "tax_hashes": arr[1], "clade_count": arr[2],
            "clade_hashes": arr[3], "total_count": total, "total_hashes": total_hashes}


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("lca", "tax_hashes", "tax_count",
                                                    "clade_hashes", "clade_count")) and \
        (a["total_count"], a["total_hashes"]) == (b["total_count"], b["total_hashes"])


# ---- writeReport, taxdb.hpp:192-236 -----------------------------------------------------------
def report(tax, r):
    """stdout of taxscreen from the per-node arrays and total_count"""
    out = [HEADER]
    kids = {}
    for v in range(len(tax.ids)):
        if tax.parent[v] != ROOT and r["clade_hashes"][v] > 0:
            kids.setdefault(int(tax.parent[v]), []).append(v)
    stack = [(tax.top, 0)] if tax.top != UNKNOWN else []
    while stack:
        v, depth = stack.pop()
        if r["clade_count"][v] == 0:
            continue
        out.append("%.4f\t%d\t%d\t%d\t%d\t%s\t%d\t%s%s\n" % (
            100 * int(r["clade_count"][v]) / float(r["total_count"]), r["clade_count"][v],
            r["tax_count"][v], r["clade_hashes"][v], r["tax_hashes"][v], tax.rank[v], tax.ids[v],
            " " * (2 * depth), tax.name[v]))
        order = sorted(kids.get(v, []), key=lambda w: (-int(r["clade_count"][w]), tax.ids[w]))
        stack.extend((w, depth + 1) for w in reversed(order))
    return "".join(out)


def holders_of(rows):
    """-> (U, holders per entry of U) for database rows of ascending distinct hashes"""
    rows = [np.asarray(x, np.uint64) for x in rows]
    U = np.unique(np.concatenate(rows + [np.zeros(0, np.uint64)]))
    holders = [[] for _ in U]
    for i, row in enumerate(rows):
        for u in np.searchsorted(U, row):
            holders[u].append(i)
    return U, holders
