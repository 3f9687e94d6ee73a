#!/usr/bin/env python3
"""k-finger timing at config C3's shape (5,000 x 2 kb, window 100: 10 M lines).

Kernel times: both passes of fpm_kfinger_* over the whole set in one job, from the library's
HIP events (FPM_K_KFINGER: Duval + line hash; FPM_K_KFINGER_OUT: sizes, scan and the text
lines), best of --repeat after one warm-up call.
Wall times, best of --repeat: `fpmash kfinger -S` on the FASTA, against the route to the same
.msh without the verb: bin/cflgen writing the k-finger text to a file, then `fpmash sketch -fp`
of that file (which reads its first 1,000,000 lines); and `fpmash kfinger` writing the whole
text, against cflgen writing it.  The two .msh files are compared.  One JSON line.

    python tools/kfinger_bench.py [--n-seqs 5000] [--seq-len 2000] [--window 100] [--repeat 3]
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
    a = ap.parse_args()
    import fpmash
    from fpmash import datagen

    rng = np.random.default_rng(3)
    seqs = [bytes(rng.choice(list(b"ACGT"), a.seq_len).astype(np.uint8)) for _ in range(a.n_seqs)]
    ids = datagen.lyn2vec_ids(a.n_seqs)
    full = [("G00000" + i + "_0").encode() for i in ids]
    res = {"n_seqs": a.n_seqs, "seq_len": a.seq_len, "window": a.window,
           "build": fpmash.build_id()}

    with fpmash.Context(0) as ctx:
        ctx.set_timing(True)
        k1 = k2 = None
        for it in range(a.repeat + 1):
            ctx.reset_timing()
            r = ctx.kfinger(seqs, window=a.window, ids=full, text=True)
            t1, _ = ctx.kernel_time(fpmash.K_KFINGER)
            t2, _ = ctx.kernel_time(fpmash.K_KFINGER_OUT)
            if it:
                k1 = t1 if k1 is None else min(k1, t1)
                k2 = t2 if k2 is None else min(k2, t2)
        res.update(lines=int(r["n_lines"]), text_bytes=len(r["text"]),
                   pass1_ms=round(k1, 3), pass2_text_ms=round(k2, 3))
        text = r["text"]
        del r

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
            subprocess.run([exe, "kfinger", "-S", "-w", str(a.window), "-o", "new", fa], **quiet)

        def verb_text():
            subprocess.run([exe, "kfinger", "-w", str(a.window), "-o", "new", fa], **quiet)

        def gen():
            with open(tsv, "rb") as i, open(os.path.join(d, "old.txt"), "wb") as o:
                subprocess.run([cflgen, str(a.window)], stdin=i, stdout=o, check=True)

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
