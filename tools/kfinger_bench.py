#!/usr/bin/env python3
"""k-finger timing at config C3's shape (5,000 x 2 kb, window 100: 10 M lines).

Kernel times: both passes of fpm_kfinger_* over the whole set in one job, from the library's
HIP events (FPM_K_KFINGER: factorization + line hash; FPM_K_KFINGER_OUT: sizes, scan and the
text lines), best of --repeat after one warm-up call, every repeat listed beside it.  With
--factorization ICFL or CFL_ICFL-<T> the CFL passes over the same records are timed in the same
process, as the yardstick; with a combined form (CFL_COMB, ICFL_COMB, CFL_ICFL_COMB-<T>) also the
passes of the form it combines (plain_*).  --period P replaces the random records by text of period P broken
once per window length (ICFL's longest scans and border chains); --no-wall leaves the wall times
out.
Wall times, best of --repeat: `fpmash kfinger -S` on the FASTA, against the route to the same
.msh without the verb: bin/cflgen writing the k-finger text to a file, then `fpmash sketch -fp`
of that file (which reads its first 1,000,000 lines); and `fpmash kfinger` writing the whole
text, against cflgen writing it.  The two .msh files are compared.  One JSON line.

    python tools/kfinger_bench.py [--n-seqs 5000] [--seq-len 2000] [--window 100] [--repeat 3]
                                  [--factorization CFL] [--period 0] [--threads 16] [--no-wall]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fp-mash_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def best(fn, repeat):
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seqs", type=int, default=5000)
    ap.add_argument("--seq-len", type=int, default=2000)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--factorization", default="CFL")
    ap.add_argument("--period", type=int, default=0)
    ap.add_argument("--threads", type=int, default=16, help="cflgen's threads")
    ap.add_argument("--no-wall", action="store_true")
    a = ap.parse_args()
    import fpmash
    from fpmash import datagen

    rng = np.random.default_rng(3)
    seqs = [bytes(rng.choice(list(b"ACGT"), a.seq_len).astype(np.uint8)) for _ in range(a.n_seqs)]
    if a.period:
        # blocks of TTG.. text of that period, window - 1 bytes, then a byte above its letters:
        # every window holds one break, behind a periodic run of up to window - 1 bytes
        unit = (b"TTG" * a.period)[-a.period:]
        block = (unit * a.window)[:max(a.window - 1, 1)] + b"Z"
        seqs = [(block * (a.seq_len // len(block) + 1))[:a.seq_len] for _ in seqs]
    ids = datagen.lyn2vec_ids(a.n_seqs)
    full = [("G00000" + i + "_0").encode() for i in ids]
    fact = a.factorization
    kind, thr = fpmash.parse_factorization(fact)
    # the form a combined one combines: CFL_COMB -> CFL, CFL_ICFL_COMB-T -> CFL_ICFL-T
    plain = None
    if kind.endswith("_COMB"):
        plain = kind[:-5] + ("-%d" % thr if thr else "")
    res = {"n_seqs": a.n_seqs, "seq_len": a.seq_len, "window": a.window, "factorization": fact,
           "period": a.period, "build": fpmash.build_id()}

    with fpmash.Context(0) as ctx:
        ctx.set_timing(True)

        def passes(f):
            k1, k2 = [], []
            for it in range(a.repeat + 1):
                ctx.reset_timing()
                r = ctx.kfinger(seqs, window=a.window, ids=full, text=True, factorization=f)
                if it:
                    k1.append(round(ctx.kernel_time(fpmash.K_KFINGER)[0], 3))
                    k2.append(round(ctx.kernel_time(fpmash.K_KFINGER_OUT)[0], 3))
            return r, k1, k2

        if fact != "CFL":
            _, k1, k2 = passes("CFL")
            res.update(cfl_pass1_ms=min(k1), cfl_pass2_text_ms=min(k2), cfl_pass1_all_ms=k1,
                       cfl_pass2_text_all_ms=k2)
        if plain and plain != "CFL":
            _, k1, k2 = passes(plain)
            res.update(plain=plain, plain_pass1_ms=min(k1), plain_pass2_text_ms=min(k2),
                       plain_pass1_all_ms=k1, plain_pass2_text_all_ms=k2)
        r, k1, k2 = passes(fact)
        res.update(lines=int(r["n_lines"]), text_bytes=len(r["text"]), pass1_ms=min(k1),
                   pass2_text_ms=min(k2), pass1_all_ms=k1, pass2_text_all_ms=k2)
        text = r["text"]
        del r
    if a.no_wall:
        print(json.dumps(res))
        return

    exe = fpmash.BIN_PATH
    cflgen = os.path.join(os.path.dirname(exe), "cflgen")
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "c3.fa")
        with open(fa, "wb") as f:
            f.write(datagen.fasta_bytes(seqs, ids))
        tsv = os.path.join(d, "c3.tsv")
        with open(tsv, "wb") as f:
            f.write(b"".join(i.encode() + b"\t" + s + b"\n" for s, i in zip(seqs, ids)))
        quiet = dict(stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, cwd=d)

        def verb_sketch():
            subprocess.run([exe, "kfinger", "-S", "-w", str(a.window), "-F", fact, "-o", "new", fa], **quiet)

        def verb_text():
            subprocess.run([exe, "kfinger", "-w", str(a.window), "-F", fact, "-o", "new", fa], **quiet)

        def gen():
            with open(tsv, "rb") as i, open(os.path.join(d, "old.txt"), "wb") as o:
                subprocess.run([cflgen, str(a.window), str(a.threads), fact], stdin=i, stdout=o,
                               check=True)

        def old_sketch():
            subprocess.run([exe, "sketch", "-fp", "-o", "old", "old.txt"], **quiet)

        res["kfinger_S_wall_s"] = round(best(verb_sketch, a.repeat), 3)
        res["kfinger_text_wall_s"] = round(best(verb_text, a.repeat), 3)
        res["cflgen_wall_s"] = round(best(gen, a.repeat), 3)
        res["sketch_fp_wall_s"] = round(best(old_sketch, a.repeat), 3)
        res["cflgen_then_sketch_fp_wall_s"] = round(res["cflgen_wall_s"] + res["sketch_fp_wall_s"], 3)
        same = lambda x, y: open(os.path.join(d, x), "rb").read() == open(os.path.join(d, y), "rb").read()
        res["msh_equal"] = same("new.msh", "old.msh")
        res["text_equal"] = same("new.txt", "old.txt") and open(os.path.join(d, "new.txt"), "rb").read() == text
    print(json.dumps(res))


if __name__ == "__main__":
    main()
