#!/usr/bin/env python3
"""Screen timing: the pool count pass (screen_count_kernel) against the sketch tile launches of
the same staged job.

Pool: --bases (2e8) of 150-base reads drawn with 1 % substitutions from 100 genomes of config
C2's set (10,000 x 2 kb in 100 families, k = 21), staged as one group of one sketch job.
Databases: the set's 10,000 sketches of 1,000 hashes, and the 100 sketches of the genomes the
reads come from (plus two that find nothing, to split the pass's time: see main).  Per database, fpm_screen_add_job is run on the staged job: it runs the job's
own sketch launches (the yardstick: hash + sort of every window, FPM_K_SKETCH) and then the
count pass over the same tiles (hash + table lookup, FPM_K_SCREEN).  Times are the library's HIP
events around those launches, best of --repeat after one warm-up call; merges and the
selection of the long group are not in either.  One JSON line.

    python tools/screen_bench.py [--bases 200000000] [--read-len 150] [--repeat 2]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fp-mash_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_pool(genomes, n_reads, read_len, seed):
    """n_reads x read_len bytes: windows of the genomes with 1 % substitutions"""
    rng = np.random.default_rng(seed)
    G = np.stack([np.frombuffer(g, np.uint8) for g in genomes])
    out = np.empty((n_reads, read_len), np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    step = 100_000
    for at in range(0, n_reads, step):
        n = min(step, n_reads - at)
        src = rng.integers(0, len(genomes), size=n)
        start = rng.integers(0, G.shape[1] - read_len + 1, size=n)
        block = G[src[:, None], start[:, None] + np.arange(read_len)[None, :]]
        m = rng.random(block.shape) < 0.01
        block[m] = acgt[rng.integers(0, 4, size=int(m.sum()))]
        out[at:at + n] = block
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=200_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--n-seqs", type=int, default=10000)
    ap.add_argument("--families", type=int, default=100)
    ap.add_argument("--seq-len", type=int, default=2000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--s", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()

    import fpmash
    from fpmash import datagen
    per = max(1, a.n_seqs // a.families)
    seqs = datagen.family_dna(a.families, per, a.seq_len, sub_rate=(0.01, 0.10),
                              seed=1000)[: a.n_seqs]
    sources = list(range(0, len(seqs), per))[:100]           # one genome per family
    n_reads = a.bases // a.read_len
    pool = make_pool([seqs[i] for i in sources], n_reads, a.read_len, seed=2000)
    data = pool.tobytes()
    off = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(a.read_len)
    groups = np.zeros(n_reads, np.uint32)
    P = fpmash.make_params(k=a.k, s=a.s)

    res = {"reads": n_reads, "read_len": a.read_len, "bases": n_reads * a.read_len, "k": a.k,
           "s": a.s}
    with fpmash.Context(0) as ctx:
        db = ctx.sketch(P, seqs)
        h = fpmash.vp()
        fpmash._check(fpmash.lib().fpm_sketch_stage(
            ctx.h, C.byref(P), data, fpmash._p(off, fpmash.u64p), n_reads,
            fpmash._p(groups, fpmash.u32p), 1, C.byref(h)))
        job = fpmash.SketchJob.__new__(fpmash.SketchJob)
        job.ctx, job.params, job.n_groups, job.h, job._keep = ctx, P, 1, h.value, (data, off)
        info, plan = job.info(), job.plan()
        res.update(tiles=info["n_tiles"], windows=info["n_kmers"], tile_classes=plan["tiles"],
                   sampled_groups=plan["n_slots"])
        # two more databases split the count pass's time: 100 sketches of unrelated genomes
        # (about as many keys pass the compare with U's maximum, none is found: the lookups
        # without the atomics), and the 10 smallest hashes of each of those (nearly every key
        # fails the compare: staging + hashing alone)
        other = ctx.sketch(P, datagen.random_dna(100, a.seq_len, seed=3000))
        for name, lists in (("db10000", db), ("db100", [db[i] for i in sources]),
                            ("db100_unrelated", other), ("db100_unrelated_cut10", [r[:10] for r in other])):
            t0 = time.perf_counter()
            sc = fpmash.Screen.from_lists(ctx, lists, a.s)
            build_ms = (time.perf_counter() - t0) * 1e3
            sc.add_job(job)                                   # code objects, first-use buffers
            ctx.synchronize()
            ctx.set_timing(True)
            best = None
            for _ in range(a.repeat):
                ctx.reset_timing()
                sc.add_job(job)
                ctx.synchronize()
                sk, n_sk = ctx.kernel_time(fpmash.K_SKETCH)
                co, n_co = ctx.kernel_time(fpmash.K_SCREEN)
                best = (sk, co, n_sk, n_co) if best is None else \
                    (min(best[0], sk), min(best[1], co), n_sk, n_co)
            ctx.set_timing(False)
            U, cnt = sc.counts()
            shared, median = sc.rows()
            res[name] = {"sketch_tiles_ms": round(best[0], 3), "count_pass_ms": round(best[1], 3),
                         "ratio": round(best[1] / best[0], 3), "sketch_launches": best[2],
                         "count_launches": best[3], "distinct_hashes": len(U),
                         "counted_windows_per_pass": int(cnt.sum(dtype=np.uint64)) // (a.repeat + 1),
                         "references_hit": int((shared > 0).sum()),
                         "table_build_wall_ms": round(build_ms, 1),
                         "set_size": sc.set_size()}
            sc.free()
        job.free()
    res["build"] = fpmash.lib().fpm_build_id().decode()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
