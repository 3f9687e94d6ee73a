#!/usr/bin/env python3
"""Reads-mode timing: a synthetic read set (a random genome, fixed-length reads at a given
coverage with substitutions) through fpm_sketch_reads_run at min-copies 1, 2 and 3.

Per min-copies value it prints the widening rounds, the HIP-event time of the kernels (the
library's per-launch events: sketch + count passes, merges / selections), the wall time of
stage / run / fetch, and whether the hashes equal the oracle's: the oracle's counted
bottom-S sketch (S >> s) holds every distinct hash below its maximum with its full count, so
the first s of its entries seen >= m times are the expected sketch.  One JSON line per value.

    python tools/reads_bench.py [--genome 5000000] [--read-len 100] [--coverage 20]
                                [--sub-rate 0.01] [--sketch-size 1000] [--no-check]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fp-mash_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_reads(genome_len, read_len, coverage, sub_rate, seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, genome_len)]
    n = genome_len * coverage // read_len
    out = []
    for c0 in range(0, n, 100_000):                  # in pieces: the index arrays are 8x the reads
        at = rng.integers(0, genome_len - read_len + 1, min(100_000, n - c0))
        reads = genome[at[:, None] + np.arange(read_len)[None, :]]
        m = rng.random(reads.shape) < sub_rate
        reads[m] = acgt[rng.integers(0, 4, int(m.sum()))]
        out.extend(r.tobytes() for r in reads)
    return out


def expected(oracle, reads, k, s, m, wide):
    """first s hashes seen >= m times, from the oracle's counted bottom-`wide` sketch"""
    while True:
        h, c = oracle.sketch_batch(oracle.params(k=k, s=wide), reads, groups=[0] * len(reads),
                                   n_groups=1, counts=True)
        h, c = h[0], c[0]
        full = len(h) == wide
        keep = c >= m
        if full:
            keep[-1] = False          # the maximum of a full sketch: its count is partial
        if keep.sum() >= s or not full:
            return h[keep][:s]
        wide *= 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--coverage", type=int, default=20)
    ap.add_argument("--sub-rate", type=float, default=0.01)
    ap.add_argument("--sketch-size", type=int, default=1000)
    ap.add_argument("--kmer", type=int, default=21)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()

    import fpmash
    reads = make_reads(a.genome, a.read_len, a.coverage, a.sub_rate, a.seed)
    groups = np.zeros(len(reads), np.uint32)
    P = fpmash.make_params(k=a.kmer, s=a.sketch_size)
    exp = {}
    if not a.no_check:
        from oracle import oracle as O
        t0 = time.perf_counter()
        for m in (1, 2, 3):
            exp[m] = expected(O, reads, a.kmer, a.sketch_size, m, 64 * a.sketch_size)
        print(f"# oracle: {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    with fpmash.Context(0) as ctx:
        warm = ctx.sketch_reads(P, reads[:1000], groups=groups[:1000], n_groups=1, min_copies=2)
        del warm
        ctx.set_timing(True)
        for m in (1, 2, 3):
            t0 = time.perf_counter()
            job = ctx.sketch_job(P, reads, groups=groups, n_groups=1, min_copies=m)
            ctx.synchronize()
            t1 = time.perf_counter()
            ctx.reset_timing()
            job.run_reads()
            ctx.synchronize()
            t2 = time.perf_counter()
            rows, cnt, mult, est = job.fetch_reads()
            t3 = time.perf_counter()
            rounds, _ = job.reads_rounds()
            ev = {n: ctx.kernel_time(kid)[0] for n, kid in (("sketch_ms", fpmash.K_SKETCH),
                                                             ("merge_ms", fpmash.K_MERGE))}
            job.free()
            got = rows[0, :cnt[0]]
            res = {"min_copies": m, "reads": len(reads), "bases": len(reads) * a.read_len,
                   "sketch_size": a.sketch_size, "rounds": rounds,
                   "event_ms": round(ev["sketch_ms"] + ev["merge_ms"], 3), **
                   {k: round(v, 3) for k, v in ev.items()},
                   "stage_wall_ms": round((t1 - t0) * 1e3, 1),
                   "run_wall_ms": round((t2 - t1) * 1e3, 1),
                   "fetch_wall_ms": round((t3 - t2) * 1e3, 1),
                   "hashes": int(cnt[0]), "estimate": int(est[0]),
                   "coverage": round(float(mult[0, :cnt[0]].sum()) / max(int(cnt[0]), 1), 3),
                   "hashes_match_oracle": (bool(np.array_equal(got, exp[m])) if m in exp
                                           else None)}
            print(json.dumps(res), flush=True)
            if m in exp and not res["hashes_match_oracle"]:
                sys.exit(1)


if __name__ == "__main__":
    main()
