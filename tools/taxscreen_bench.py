#!/usr/bin/env python3
"""taxscreen timing: the LCA fold (tax_lca_kernel) and the clade sums (tax_clade_kernel) of
fpm_screen_tax on one synthetic table, beside the -w pass (screen_winner_kernel) on the same
table, the nearest kernel of the same shape (one unit of work per entry of U over its postings).

Table: --entries (1e6) distinct hashes over 20,000 references, two per species, five species per
genus, ten genera per family, 200 families under order / class / phylum / kingdom / root (depth 7).
70 % of the hashes are held by one reference, 20 % by both references of a species, 8 % by about
six references of one genus, 1.9 % by about fifty of one family, and 0.1 % by 10-25 % of all
references (2,000-5,000 holders: the conserved k-mers a wave folds).  40 % of the hashes are seen
in the pool.

Times of the two tax kernels are the library's HIP events (FPM_K_COMPARE around the fold,
FPM_K_FINALIZE around the clade sums), best of --repeat after one warm-up call.  The -w pass has
no event bracket of its own: run the tool under `rocprofv3 --kernel-trace --stats` to read all
three kernels' durations side by side.  One JSON line.

    python tools/taxscreen_bench.py [--entries 1000000] [--repeat 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fp-mash_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

N_REF, PER_SPECIES, PER_GENUS, PER_FAMILY = 20000, 2, 5, 10
UPPER = [1, 1, 10, 40, 100]          # root, kingdom, phyla, classes, orders


def taxonomy():
    """-> (parent per node, node of each reference's species)"""
    n_species = N_REF // PER_SPECIES
    n_genus = n_species // PER_GENUS
    n_family = n_genus // PER_FAMILY
    parent, level = [0xFFFFFFFF], [0]
    for n in UPPER[1:] + [n_family, n_genus, n_species]:
        first, above = len(parent), level[-1]
        n_above = first - above
        parent += [above + (i * n_above) // n for i in range(n)]
        level.append(first)
    return np.array(parent, np.uint32), level[-1] + np.arange(N_REF) // PER_SPECIES


def holders(rng, n):
    """-> (entry, reference) pairs of n entries by the shares of the module text"""
    kind = rng.choice(5, size=n, p=[0.70, 0.20, 0.08, 0.019, 0.001])
    e_all, r_all = [], []
    for k, group in ((0, 1), (1, PER_SPECIES), (2, PER_SPECIES * PER_GENUS),
                     (3, PER_SPECIES * PER_GENUS * PER_FAMILY), (4, N_REF)):
        e = np.nonzero(kind == k)[0]
        base = rng.integers(0, N_REF // group, size=len(e)) * group
        if k == 0:
            mask = np.ones((len(e), 1), bool)
        elif k == 1:
            mask = np.ones((len(e), group), bool)
        else:
            p = {2: 0.6, 3: 0.5}.get(k)
            p = rng.uniform(0.10, 0.25, size=(len(e), 1)) if p is None else p
            mask = rng.random((len(e), group)) < p
            mask[:, :2] = True
        ei, gi = np.nonzero(mask)
        e_all.append(e[ei])
        r_all.append(base[ei] + gi)
    return np.concatenate(e_all), np.concatenate(r_all)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import fpmash

    rng = np.random.default_rng(a.seed)
    parent, ref_node = taxonomy()
    U = np.unique(rng.integers(1, 2 ** 63, size=a.entries + a.entries // 100, dtype=np.uint64))
    U = U[:a.entries]
    e, r = holders(rng, len(U))
    order = np.lexsort((e, r))
    e, r = e[order], r[order]
    lens = np.bincount(r, minlength=N_REF).astype(np.uint32)
    start = np.cumsum(lens, dtype=np.int64) - lens
    R = np.zeros((N_REF, int(lens.max())), np.uint64)
    R[r, np.arange(len(r)) - start[r]] = U[e]
    post_len = np.bincount(e, minlength=len(U))
    seen = np.nonzero(rng.random(len(U)) < 0.4)[0]
    keys = np.repeat(U[seen], rng.integers(1, 4, size=len(seen)))

    out = {"entries": int(len(U)), "references": N_REF, "cells": int(len(e)),
           "nodes": int(len(parent)), "longest_list": int(post_len.max()),
           "lists_at_or_over_cut": None, "seen": int(len(seen))}
    with fpmash.Context(0) as ctx:
        out["lists_at_or_over_cut"] = int((post_len >= ctx.tax_wave_cut()).sum())
        sc = fpmash.Screen(ctx, R, lens, 1000)
        try:
            sc.add_hashes(keys)
            shared, _ = sc.rows()
            scores = [fpmash.estimate_identity(int(c), int(d), 21) for c, d in zip(shared, lens)]
            sc.rows_winner(scores, np.full(N_REF, 1000, np.uint64))      # the -w pass, once
            ctx.set_timing(True)
            best = {}
            for it in range(a.repeat + 1):
                ctx.reset_timing()
                res = sc.tax(parent, 0, ref_node, lca=False)
                t = {"tax_lca_ms": ctx.kernel_time(fpmash.K_COMPARE)[0],
                     "tax_clade_ms": ctx.kernel_time(fpmash.K_FINALIZE)[0]}
                if it:
                    best = {k: min(v, best.get(k, v)) for k, v in t.items()}
            out.update(best)
            out["kernel"] = fpmash.TAX_KERNELS[ctx.last_tax_kernel()]
            out["tallied_taxa"] = int((res["tax_hashes"] > 0).sum())
            out["root_clade"] = [int(res["clade_count"][0]), int(res["clade_hashes"][0])]
            assert res["total_hashes"] == len(U) and res["total_count"] == len(seen)
            assert int(res["clade_hashes"][0]) == len(U)
        finally:
            sc.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
